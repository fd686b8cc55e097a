"""hmmsort_correlograms / hmmsort_plan_correlograms against the numpy model tests/correlogram_model.py:
ccg, viol, coinc and n are integers and must come out equal, entry for entry, from the host form, the plan form (single
and batched), api.correlograms and sort_data."""
import ctypes as C

import numpy as np
import pytest

import correlogram_model as CM
import fit_adaptive_model as FA
from conftest import to_oracle_sm

pytestmark = pytest.mark.gpu

NAMES = ("ccg", "viol", "coinc", "n")


def parts(cg):
    return cg.counts, cg.isi_violations, cg.coincidence, cg.n


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == np.int64 and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, bad[:4].tolist(), g[tuple(bad[:4].T)], w[tuple(bad[:4].T)])


def run(H, lists, b, Hb, r, c):
    cg = H.correlograms(lists, bin=b, half_bins=Hb, refractory=r, coincidence=c)
    assert np.array_equal(cg.lags, (np.arange(2 * Hb) - Hb) * b)
    return parts(cg)


def gaps(rng, n, lo=1, hi=40, start=1):
    return (start + np.cumsum(rng.integers(lo, hi + 1, n))).astype(np.int64)


# ---- 1, 2: the smallest lists, the window's edges ---------------------------------------------------------------
def test_degenerate_lists(H):
    lists = [np.zeros(0, dtype=np.int64), np.array([1], dtype=np.int64), np.array([5, 6], dtype=np.int64)]
    ccg, viol, coinc, n = got = run(H, lists, 1, 1, 2, 0)
    same(got, CM.brute(lists, 1, 1, 2, 0), "degenerate")
    want = np.zeros((3, 3, 2), dtype=np.int64)
    want[2, 2] = [1, 0]                        # 6 -> 5 is d = -1: bin 0; 5 -> 6 is d = +1, outside [-1, 1)
    assert np.array_equal(ccg, want) and viol.tolist() == [0, 0, 1] and n.tolist() == [0, 1, 2]
    assert not coinc.any()                     # c = 0 and no two spikes share a sample


@pytest.mark.parametrize("b", [1, 3, 30])
@pytest.mark.parametrize("Hb", [1, 5])
def test_window_edges(H, b, Hb):
    W = Hb * b
    u = np.array([1000], dtype=np.int64)
    v = np.array([1000 - W - 1, 1000 - W, 999, 1000, 1001, 1000 + W - 1, 1000 + W], dtype=np.int64)
    v = np.unique(v)                           # b = H = 1: 1000 - W is 999 and 1000 + W - 1 is 1000
    ccg, viol, coinc, n = got = run(H, [u, v], b, Hb, 0, 1)
    same(got, CM.brute([u, v], b, Hb, 0, 1), "edges")
    want = np.zeros(2 * Hb, dtype=np.int64)    # written out: u -> v, lag d = t_v - 1000
    for d in sorted({-W, -1, 0, 1, W - 1}):    # the lags of v, without -W - 1 and +W: they are outside
        if -W <= d < W:                        # (W = 1: the lag +1 is +W)
            want[(d + W) // b] += 1
    assert np.array_equal(ccg[0, 1], want) and ccg[0, 1].sum() == len(v) - 2
    assert ccg[0, 1, Hb] >= 1 and ccg[0, 1, Hb - 1] >= 1          # d = 0 in bin H, d = -1 in bin H - 1
    if b == 1:
        assert ccg[0, 1, Hb] == 1 and ccg[0, 1, Hb - 1] == 1 and ccg[0, 1, 0] == 1 and ccg[0, 1, 2 * Hb - 1] == 1
    assert not ccg[0, 0].any() and coinc[0, 1] == 1 and coinc[1, 0] == 3 and coinc[0, 0] == 0


# ---- 3, 5: tile seams, large times ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seams():
    rng = np.random.default_rng(31)
    return [gaps(rng, n, start=int(rng.integers(1, 200))) for n in (255, 256, 257, 513)]


def test_tile_seams(H, seams):
    got = run(H, seams, 5, 20, 12, 2)
    same(got, CM.brute(seams, 5, 20, 12, 2), "seams")
    assert got[0].sum() > 10_000 and got[1].min() > 20


def test_large_times(H, seams):
    far = [t + (1 << 39) for t in seams]
    assert max(int(t[-1]) for t in far) < (1 << 40)
    got = run(H, far, 7, 14, 12, 2)
    same(got, CM.fast(far, 7, 14, 12, 2), "shifted")
    same(got, run(H, seams, 7, 14, 12, 2), "shift invariance")


# ---- 4: a burst -------------------------------------------------------------------------------------------------
def test_burst(H):
    n, Hb = 3000, 2048
    burst = np.arange(500, 500 + n, dtype=np.int64)
    few = np.array([501, 1000, 1001, 2500, 3499], dtype=np.int64)
    ccg, viol, coinc, cnt = got = run(H, [burst, few], 1, Hb, 2, 0)
    same(got, CM.fast([burst, few], 1, Hb, 2, 0), "burst")
    m = np.arange(1, Hb)
    assert np.array_equal(ccg[0, 0, Hb + m], n - m) and np.array_equal(ccg[0, 0, Hb - m], n - m)
    assert ccg[0, 0, Hb] == 0 and ccg[0, 0, 0] == n - Hb
    assert viol.tolist() == [n - 1, 1] and coinc[1, 0] == 5 and coinc[0, 1] == 5 and coinc[0, 0] == 0


# ---- 6: a window wider than the recording -----------------------------------------------------------------------
def test_window_wider_than_the_recording(H):
    rng = np.random.default_rng(6)
    lists = [np.sort(rng.choice(3_000_000, 7, replace=False)).astype(np.int64) + 1,
             np.sort(rng.choice(3_000_000, 5, replace=False)).astype(np.int64) + 1]
    b, Hb = 1 << 19, 2048
    assert Hb * b == 1 << 30
    got = run(H, lists, b, Hb, 1 << 20, 1 << 19)
    same(got, CM.brute(lists, b, Hb, 1 << 20, 1 << 19), "wide")
    assert got[0][0, 1].sum() == 35 and got[0][0, 0].sum() == 42      # every pair is inside


# ---- 7: many units ----------------------------------------------------------------------------------------------
def test_many_units(H):
    rng = np.random.default_rng(7)
    lists = CM.random_lists(rng, 40, 300, 50_000)
    lists[3] = lists[3][:0]
    got = run(H, lists, 5, 20, 30, 2)
    same(got, CM.fast(lists, 5, 20, 30, 2), "many units")
    again = run(H, lists, 5, 20, 30, 2)
    assert all(g.tobytes() == a.tobytes() for g, a in zip(got, again))
    assert got[3].tolist() == [len(t) for t in lists] and got[0].sum() > 50_000 and got[2].sum() > 1000


# ---- 8: refusals ------------------------------------------------------------------------------------------------
def raw(H, lists, b=5, Hb=4, r=0, c=0, U=None, n=True, opt=True):
    """hmmsort_correlograms with a token n -> rc (a call that refuses must not have written)"""
    L = H._lib
    lists = [np.ascontiguousarray(t, dtype=np.int64) for t in lists]
    U = len(lists) if U is None else U
    ptrs = (C.c_void_p * max(len(lists), 1))(*[t.ctypes.data if len(t) else None for t in lists])
    cnt = np.array([len(t) for t in lists] + [0], dtype=np.int64)
    tok = np.zeros(8, dtype=np.int64)
    o = L.CcgOpt(b, Hb, r, c)
    out = L.CcgOut(None, None, None, tok.ctypes.data if n else None)
    rc = L.lib().hmmsort_correlograms(U, ptrs, L.ptr(cnt), C.byref(o) if opt else None, C.byref(out))
    assert rc == 0 or not tok.any()
    return rc


def test_refusals(H):
    L = H._lib
    ok = [np.array([3, 9, 10]), np.array([4])]

    def refused(code, *words, **kw):
        rc = raw(H, kw.pop("lists", ok), **kw)
        assert rc == code and all(w in L.last_error() for w in words), (rc, L.last_error())

    refused(L.EINVAL, "unit 1", "position 2", "ascending", lists=[ok[0], np.array([4, 7, 7])])
    refused(L.EINVAL, "unit 0", "position 1", "ascending", lists=[np.array([4, 3]), ok[1]])
    refused(L.EINVAL, "unit 1", "position 0", "time 0", lists=[ok[0], np.array([0, 7])])
    refused(L.EINVAL, "unit 0", "position 2", "2^40", lists=[np.array([1, 2, (1 << 40) + 1]), ok[1]])
    refused(L.EINVAL, "bin = 0", b=0)
    refused(L.EINVAL, "half_bins = 0", Hb=0)
    refused(L.EINVAL, "half_bins = 2049", Hb=2049)
    refused(L.EINVAL, "2^31", b=1 << 20, Hb=2048)
    refused(L.EINVAL, "refractory = -1", r=-1)
    refused(L.EINVAL, "coincidence = -2", c=-2)
    refused(L.EINVAL, "U = 0", U=0)
    refused(L.EINVAL, "U = 4097", lists=[ok[1]] * 4097)
    refused(L.EINVAL, "null", n=False)
    refused(L.EINVAL, "null", opt=False)
    rc = L.lib().hmmsort_correlograms(2, None, None, None, None)
    assert rc == L.EINVAL and "null" in L.last_error()
    refused(L.EUNSUP, str(4096 * 4096 * 4096), "entries", lists=[ok[1]] * 4096, Hb=2048)
    with pytest.raises(H.HmmsortError) as e:
        H.correlograms([ok[0], [5, 5]])
    assert e.value.code == L.EINVAL and "unit 1" in str(e.value)
    assert raw(H, ok) == 0                                 # and the lists the refusals varied are taken


# ---- 9: the plan form on a batched plan, a neuron seen on two channels -------------------------------------------
def test_batched_plan_finds_the_duplicated_units(H):
    import torch
    # the wave engine takes rings of at least 8 states: K = 9 is the shortest template a batched plan accepts
    N, K, nC, T = 2, 9, 3, 12_000
    pp, sg = (0.01, 0.008), 0.3
    base = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                       H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    mus = [base, np.asfortranarray(base[:, ::-1] * 1.1), base]
    ys = [H.create_signal(T, sg, pp, mus[0], seed=90), H.create_signal(T, sg, pp, mus[1], seed=91)]
    ys.append(ys[0])                                       # channel 2 carries channel 0's signal and model
    opts = dict(bin=5, half_bins=20, refractory=30, coincidence=0)
    H.set_option("engine", H.ENGINE_WAVE)
    try:
        plan = H.Plan.batched(T, [sm] * nC, mus, [sg] * nC)
        dx = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
        dll = torch.zeros(nC, dtype=torch.float64, device="cuda")
        plan.viterbi(torch.from_numpy(np.stack(ys)).cuda(), dx, dll)
        cg = plan.correlograms(dx, **opts)
        cg2 = plan.correlograms(dx, stream=torch.cuda.current_stream().cuda_stream, **opts)
        plan.close()
        lists = []
        for c in range(nC):
            one = H.Plan(T, sm, mus[c], sg)
            lists += one.extract_spiketimes(dx[c])
            one.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    assert len(lists) == nC * N and all(len(t) > 40 for t in lists)
    same(parts(cg), parts(H.correlograms(lists, **opts)), "plan form vs host form")
    same(parts(cg), CM.fast(lists, 5, 20, 30, 0), "plan form vs model")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts(cg), parts(cg2)))
    for u in range(N):
        assert cg.coincidence[u, u + 2 * N] == cg.n[u] == cg.n[u + 2 * N] == cg.coincidence[u + 2 * N, u]
    assert H.duplicate_units(cg) == [(0, 4, 1.0), (1, 5, 1.0), (4, 0, 1.0), (5, 1, 1.0)]


# ---- 10: the plan form on an overlap model: two troughs on one sample ---------------------------------------------
def test_blocked_plan_overlap_model(H, O):
    import torch
    pp, sigma, T = (0.03, 0.02), 0.5, 4100
    mu = np.asfortranarray(np.array([[0.0, -1.0, -3.0, -2.0, 1.0], [0.0, 0.5, -2.0, -4.0, 1.0]]).T)
    sm = H.StateMatrix.create(2, 5, np.log(pp), True)
    st = np.asarray(sm.states)
    # two independent trains, free to overlap; seed 3 puts both troughs on one sample three times
    y = H.create_signal(T, sigma, pp[:1], mu[:, :1], seed=3) + H.create_signal(T, 0.0, pp[1:], mu[:, 1:], seed=1003)
    xo, _ = O.viterbi(y, to_oracle_sm(O, sm), mu, sigma)
    xo = np.asarray(xo).astype(np.int64)
    shared = int(np.sum((st[0, xo - 1] == 3) & (st[1, xo - 1] == 4)))
    assert shared >= 1, "the CPU decode has no sample with both troughs"
    opts = dict(bin=1, half_bins=8, refractory=6, coincidence=0)
    H.set_option("engine", H.ENGINE_BLOCKED)
    try:
        plan = H.Plan(T, sm, mu, sigma)
        assert plan.info()["engine"] == H.ENGINE_BLOCKED
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(torch.from_numpy(y).cuda(), dx, dll)
        cg = plan.correlograms(dx, **opts)
        lists = plan.extract_spiketimes(dx)
        plan.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    assert np.array_equal(dx.cpu().numpy(), xo)
    same(parts(cg), CM.brute(lists, 1, 8, 6, 0), "overlap model")
    assert cg.counts[0, 1, 8] == cg.counts[1, 0, 8] == cg.coincidence[0, 1] == cg.coincidence[1, 0] == shared


# ---- 11: the Python layers --------------------------------------------------------------------------------------
def test_models_and_sort_data(H):
    y, onsets, temps = FA.drifting(H, 2, 0.4)
    T = 15_000
    raw_y = np.round(y[:T] * 1000).astype(np.int16)
    spike_forms = np.zeros((FA.K_D, 1, 2))
    spike_forms[:, 0, :] = temps * 1000
    args = (spike_forms, [1.0 / 300.0 ** 2], list(FA.PP_D), raw_y)
    plain = H.sort_data(*args, dosave=False, chunksize=5000)
    out = H.sort_data(*args, dosave=False, chunksize=5000, correlograms=True)
    assert set(out) - set(plain) == {"ccg", "ccg_lags", "isi_violations"}
    assert set(plain) == {"mlseq", "ll", "waveforms", "lp", "sigma"}
    assert all(np.array_equal(out[k], plain[k]) for k in plain)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), True)
    tm = H.HMMSpikeTemplateModel(sm, np.asfortranarray(spike_forms[:, 0, :]), 300.0)
    m0 = H.fit(tm, raw_y, 5000)
    lists = H.extract_spiketimes(m0)
    assert all(len(t) > 20 for t in lists)
    want = CM.fast(lists, 30, 50, 30, 2)
    assert np.array_equal(out["ccg"], want[0]) and np.array_equal(out["isi_violations"], want[1])
    assert np.array_equal(out["ccg_lags"], (np.arange(100) - 50) * 30)
    opt = H.sort_data(*args, dosave=False, chunksize=5000, correlograms=dict(bin=7, half_bins=9, refractory=100))
    assert np.array_equal(opt["ccg"], CM.fast(lists, 7, 9, 100, 2)[0]) and opt["ccg"].shape == (2, 2, 18)
    assert np.array_equal(opt["isi_violations"], CM.fast(lists, 7, 9, 100, 2)[1])
    # a list of models contributes its extract_spiketimes lists in order
    m1 = H.HMMSpikingModel(tm, np.roll(m0.ml_seq, 3), 0.0, raw_y)
    l1 = H.extract_spiketimes(m1)
    cg = H.correlograms([m0, m1], bin=3, half_bins=6, refractory=20, coincidence=3)
    same(parts(cg), parts(H.correlograms(lists + l1, bin=3, half_bins=6, refractory=20, coincidence=3)), "models")
    same(parts(cg), CM.fast(lists + l1, 3, 6, 20, 3), "models vs model")
    mixed = H.correlograms([m0, l1[0], l1[1]], bin=3, half_bins=6, refractory=20, coincidence=3)
    same(parts(mixed), parts(cg), "models and lists mixed")
    dup = H.duplicate_units(cg)
    assert [p[:2] for p in dup] == [(0, 2), (1, 3), (2, 0), (3, 1)]          # the path moved by three samples
    H.shutdown()
