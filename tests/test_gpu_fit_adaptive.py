"""hmmsort_fit_adaptive, the drift-tracking chunked decode, with hmmsort_stats_blend and
hmmsort_reconstruct_tracked.  The decode of every chunk is checked against the oracle's viterbi under the model the
track says that chunk was decoded with (path and ll with ==), the model sequence against the device's own
path_stats / path_finish with the blend redone in numpy (==), and the point of it all on the drifting recording
D(seed, 0.4) of tests/fit_adaptive_model.py: the fixed-model loop loses the units, the adaptive loop keeps them."""
import ctypes as C

import numpy as np
import pytest

import fit_adaptive_model as FA
import path_stats_model as PS
from conftest import to_oracle_sm

pytestmark = pytest.mark.gpu

INF = float("inf")


# ---- helpers -------------------------------------------------------------------------------------
def adaptive(H, y, sm, mu, sigma, cs, halflife, warmup=0, us=True, ul=False, cap=None, want_final=True):
    """hmmsort_fit_adaptive without raising: (rc, ml_seq, ll, ModelTrack)"""
    from hmmsort_amd.api import _fit_adaptive_call
    return _fit_adaptive_call(H.HMMSpikeTemplateModel(sm, mu, sigma), y, cs, halflife, warmup, us, ul, cap, want_final)[:4]


def chunked(H, y, sm, mu, sigma, cs):
    """hmmsort_fit_chunked without raising: (rc, ml_seq, ll)"""
    from hmmsort_amd.api import _model_args
    from hmmsort_amd._lib import lib, ptr
    keep, margs = _model_args(sm, mu, sigma)
    ml = np.full(len(y), -9, dtype=np.int16)
    ll = C.c_double(np.nan)
    rc = lib().hmmsort_fit_chunked(ptr(y), len(y), int(cs), *margs, ptr(ml), C.cast(C.byref(ll), C.c_void_p))
    return rc, ml, ll.value


@pytest.fixture(scope="module")
def cases(H):
    """name -> (y, onsets, StateMatrix, templates, chunksize): D(1, 0.4) with the 2 x 16 ring model in chunks of 4 000,
    and the same drift on 24 000 samples of a 2 x 12 model with overlaps (144 states) in chunks of 3 000"""
    y, onsets, temps = FA.drifting(H, 1, 0.4)
    ring = (y, onsets, H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False), temps, 4000)
    y2, onsets2, temps2 = FA.drifting(H, 1, 0.4, T=24_000, K=12)
    return {"ring": ring, "overlap": (y2, onsets2, H.StateMatrix.create(2, 12, np.log(FA.PP_D), True), temps2, 3000)}


@pytest.fixture(scope="module")
def tracked(H, cases):
    """(name, update_lp) -> (rc, ml, ll, track) with half-life 8 000, warmup 0, update_sigma 1, computed once"""
    out = {}
    for name, (y, onsets, sm, temps, cs) in cases.items():
        for ul in (False, True):
            out[name, ul] = adaptive(H, y, sm, temps, FA.SIGMA_D, cs, 8000.0, 0, True, ul)
    H.shutdown()
    return out


def replay_model(H, y, sm, ml, tk, cs, halflife, us, ul):
    """the model sequence redone from the final path: per chunk the device's path_stats over own_c, the blend in numpy
    with the reported w_c, the device's path_finish under model c -> mu, sigma (and the list) of chunk c + 1, which
    must be the track's bit for bit.  Returns the lists the chunks were decoded with."""
    import torch
    from hmmsort_amd.device import Plan
    T, K, N, S = len(y), sm.K, sm.N, sm.nstates
    dy, dx = torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(np.ascontiguousarray(ml)).cuda()
    lA, lists, acc = sm, [], None
    for c in range(tk.n):
        lists.append(lA)
        mu_c, sig_c = np.asfortranarray(tk.mu[c]), float(tk.sigma[c])
        plan = Plan(cs, lA, mu_c, sig_c)
        try:
            dnew = torch.zeros(plan.path_stats_len(), dtype=torch.float64, device="cuda")
            lo, hi = (int(v) for v in tk.own[c])
            plan.path_stats(dy, dx, T, lo, hi, tk.first[c] == 1, dnew)
            want_w = 2.0 ** (-(hi - lo) / halflife)
            assert abs(tk.w[c] - want_w) <= 4 * np.spacing(want_w), (c, tk.w[c], want_w)
            new = dnew.cpu().numpy()
            acc = FA.blend(np.zeros_like(new) if acc is None else acc, tk.w[c], new)
            if c + 1 == tk.n:
                break
            out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
            plan.path_finish(torch.from_numpy(acc).cuda(), out)
            o = out.cpu().numpy()
        finally:
            plan.close()
        nlp = len(o) - K * N - 1 - S
        mu_n, sig_n, lp = o[:K * N].reshape((K, N), order="F"), float(o[K * N]), o[K * N + 1:K * N + 1 + nlp].copy()
        assert np.array_equal(mu_n, tk.mu[c + 1]), (c, np.abs(mu_n - tk.mu[c + 1]).max())
        assert tk.sigma[c + 1] == (sig_n if us and np.isfinite(sig_n) and sig_n > 0 else sig_c), (c, tk.sigma[c + 1], sig_n)
        if ul:
            lA = H.StateMatrix.from_states(lA.states, lA.pi, K, lp, lA.resolve_overlaps)
    return lists


def check_decode(O, y, lists, ml, ll, tk, cs):
    """every chunk of the track decoded by the oracle under (list, mu_c, sigma_c) and stitched by fit.jl's rule"""
    T = len(y)
    want, total, own, n = np.ones(T, dtype=np.int16), 0.0, [], 0

    def decode(i, j, c):
        assert c < tk.n and i == tk.first[c], (c, i)
        return O.viterbi(y[i - 1:j], to_oracle_sm(O, lists[c]), np.asfortranarray(tk.mu[c]), float(tk.sigma[c]))

    for c, i, j, x, llc, l, kk, last in FA.walk(decode, T, cs):
        if l <= kk:
            want[i + l - 2:i + kk - 1] = x[l - 1:kk]
        total += llc
        own.append(FA.owned(i, l, kk, last, T))
        n += 1
    assert n == tk.n and last
    assert np.array_equal(ml, want), np.flatnonzero(ml != want)[:8]
    print("ll %.17g, oracle chunks %.17g" % (ll, total))
    assert ll == total
    assert tk.own.tolist() == [list(o) for o in own]


# ---- 1. decode consistency ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring", "overlap"])
def test_every_chunk_is_the_oracle_decode_under_its_model(O, H, cases, tracked, name):
    y, onsets, sm, temps, cs = cases[name]
    rc, ml, ll, tk = tracked[name, False]
    assert rc == 0 and tk.n >= 8
    assert np.array_equal(tk.mu[0], temps) and tk.sigma[0] == FA.SIGMA_D
    assert np.abs(tk.mu[-1] - temps).max() > 0.1          # the model did move
    check_decode(O, y, [sm] * tk.n, ml, ll, tk, cs)


# ---- 2. model consistency ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring", "overlap"])
def test_model_sequence_is_stats_blend_finish(H, cases, tracked, name):
    y, onsets, sm, temps, cs = cases[name]
    rc, ml, ll, tk = tracked[name, False]
    assert rc == 0
    replay_model(H, y, sm, ml, tk, cs, 8000.0, True, False)
    assert tk.final is not None and tk.final[3][:2] == [0, 0]


@pytest.mark.parametrize("name", ["ring", "overlap"])
def test_update_lp_rebuilds_the_list_like_a_hard_step(O, H, cases, tracked, name):
    y, onsets, sm, temps, cs = cases[name]
    rc, ml, ll, tk = tracked[name, True]
    assert rc == 0, H._lib.last_error()
    lists = replay_model(H, y, sm, ml, tk, cs, 8000.0, True, True)
    assert any(not np.array_equal(a.transitions["lp"], sm.transitions["lp"]) for a in lists[1:])
    check_decode(O, y, lists, ml, ll, tk, cs)


def test_update_sigma_off_keeps_the_callers(H, cases):
    y, onsets, sm, temps, cs = cases["ring"]
    rc, ml, ll, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, cs, 8000.0, 0, False, False)
    assert rc == 0 and np.all(tk.sigma == FA.SIGMA_D)
    replay_model(H, y, sm, ml, tk, cs, 8000.0, False, False)


# ---- 3. it tracks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_adaptive_loop_keeps_the_units_the_fixed_loop_loses(H, seed):
    y, onsets, temps = FA.drifting(H, seed, 0.4)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False)
    T = len(y)
    rc0, ml0, ll0 = chunked(H, y, sm, temps, FA.SIGMA_D, 4000)
    rc1, ml1, ll1, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, 4000, 8000.0)
    assert rc0 == 0 and rc1 == 0
    f, n, fx = FA.recall(ml0, onsets, sm, 32_000, T - 16)
    a, n1, ax = FA.recall(ml1, onsets, sm, 32_000, T - 16)
    print("seed %d: hmmsort_fit_chunked %d/%d (+%d), hmmsort_fit_adaptive %d/%d (+%d)" % (seed, f, n, fx, a, n1, ax))
    assert f <= 0.55 * n
    assert a >= 0.95 * n and ax <= 3


def test_stationary_recording_decodes_like_the_fixed_loop(H):
    y, onsets, temps = FA.drifting(H, 1, 1.0)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False)
    rc0, ml0, ll0 = chunked(H, y, sm, temps, FA.SIGMA_D, 4000)
    rc1, ml1, ll1, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, 4000, 8000.0)
    differ = int(np.sum(ml0 != ml1))
    print("no drift: %d of %d samples differ" % (differ, len(y)))
    assert rc0 == 0 and rc1 == 0 and differ <= len(y) // 1000


# ---- 4. degenerate settings ------------------------------------------------------------------------------
def test_never_forget_never_replace_is_fit_chunked(H, cases):
    for name in ("ring", "overlap"):
        y, onsets, sm, temps, cs = cases[name]
        rc0, ml0, ll0 = chunked(H, y, sm, temps, FA.SIGMA_D, cs)
        rc1, ml1, ll1, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, cs, INF, len(y))
        assert rc0 == 0 and rc1 == 0
        assert np.array_equal(ml0, ml1) and ll0 == ll1
        assert np.all(tk.w == 1.0) and all(np.array_equal(m, temps) for m in tk.mu) and np.all(tk.sigma == FA.SIGMA_D)
    H.shutdown()


def test_final_model_is_the_hard_step_of_the_whole_path(H):
    """D(2, 1.0) cut to 12 000 samples in chunks of 4 400: the owned ranges tile [0, T) (asserted; pinned on the CPU in
    test_fit_adaptive_cpu.py), so with w = 1 the accumulator holds the statistics of the whole path added chunk by
    chunk: integer slots exact, sums reordered."""
    y, onsets, temps = FA.drifting(H, 2, 1.0, T=12_000)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False)
    T = len(y)
    rc, ml, ll, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, 4400, INF, T)
    assert rc == 0 and tk.n == 3
    assert tk.own[0, 0] == 0 and tk.own[-1, 1] == T and np.array_equal(tk.own[1:, 0], tk.own[:-1, 1])
    models, steps = H.fit_step_channels(H.HMMSpikeTemplateModel(sm, temps, FA.SIGMA_D), [y], 4400)
    lA_s, mu_s, sig_s, counts_s = steps[0]
    lA_f, mu_f, sig_f, counts_f = tk.final
    assert np.array_equal(models[0].ml_seq, ml) and models[0].ll == ll
    assert counts_f == counts_s
    assert np.array_equal(lA_f.transitions, lA_s.transitions) and np.array_equal(lA_f.pi, lA_s.pi)
    st = PS.path_stats(y, ml, sm.states, sm.transitions, sm.K, by_template=True)
    L = sm.K - 1
    for l in range(sm.N):
        for k in range(1, sm.K):
            e = l * L + k - 1
            if st["c"][e] > 0:
                bound = T * 2.0 ** -52 * st["abs"][e] / st["c"][e]
                assert abs(mu_f[k, l] - mu_s[k, l]) <= bound, (k, l, mu_f[k, l], mu_s[k, l], bound)
            else:
                assert mu_f[k, l] == mu_s[k, l] == temps[k, l]
    m = PS.finish(st, sm.states, temps)
    print("sigma' %.17g (chunks) %.17g (whole path)" % (sig_f, sig_s))
    assert abs(sig_f - sig_s) <= 2 * PS.sigma_bound(m, T) * sig_s
    H.shutdown()


@pytest.mark.parametrize("cs", [0, 6000, 9000])
def test_one_chunk_that_holds_the_recording(H, cs):
    y, onsets, temps = FA.drifting(H, 3, 0.4, T=6000)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False)
    rc0, ml0, ll0 = chunked(H, y, sm, temps, FA.SIGMA_D, cs)
    rc1, ml1, ll1, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, cs, 8000.0, cap=4)
    assert rc0 == 0 and rc1 == 0 and np.array_equal(ml0, ml1) and ll0 == ll1
    assert tk.n == 1 and tk.first.tolist() == [1] and tk.own.tolist() == [[0, 6000]]
    assert np.array_equal(tk.mu[0], temps) and tk.sigma[0] == FA.SIGMA_D
    assert abs(tk.w[0] - 2.0 ** -0.75) <= 4 * np.spacing(2.0 ** -0.75)
    models, steps = H.fit_step_channels(H.HMMSpikeTemplateModel(sm, temps, FA.SIGMA_D), [y], cs or None)
    assert np.array_equal(tk.final[1], steps[0][1]) and tk.final[2] == steps[0][2] and tk.final[3] == steps[0][3]
    H.shutdown()


def test_one_sample(H):
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False)
    temps = FA.templates_d(H)
    rc, ml, ll, tk = adaptive(H, np.array([0.25]), sm, temps, FA.SIGMA_D, 100, 8000.0, cap=4)
    assert rc == 0 and ml.tolist() == [1] and ll == 0.0 and tk.n == 0
    assert np.array_equal(tk.final[1], temps)              # no row was visited: every mean is kept
    H.shutdown()


def test_refusals_before_any_gpu_work(H, cases):
    y, onsets, sm, temps, cs = cases["ring"]
    E = H._lib.EINVAL
    for halflife, warmup in ((0.0, 0), (-1.0, 0), (float("nan"), 0), (8000.0, -1)):
        rc, ml, ll, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, cs, halflife, warmup)
        assert rc == E and tk.n == 0 and not ml.any(), (halflife, warmup, rc)
    from hmmsort_amd import _lib
    from hmmsort_amd.api import _model_args
    keep, margs = _model_args(sm, temps, FA.SIGMA_D)
    model = _lib.Model(*margs)
    ml, ll = np.zeros(len(y), dtype=np.int16), np.zeros(1)
    rc = _lib.lib().hmmsort_fit_adaptive(_lib.ptr(y), _lib.SAMPLES_F64, len(y), cs, C.byref(model), None, _lib.ptr(ml),
                                         _lib.ptr(ll), None, None)
    assert rc == E and "null" in _lib.last_error()


def test_track_smaller_than_the_number_of_chunks(H, cases, tracked):
    y, onsets, sm, temps, cs = cases["ring"]
    rc, ml, ll, full = tracked["ring", False]
    rc2, ml2, ll2, tk = adaptive(H, y, sm, temps, FA.SIGMA_D, cs, 8000.0, cap=5)
    assert rc2 == 0 and np.array_equal(ml, ml2) and ll == ll2
    assert tk.n == full.n > 5 and len(tk.first) == 5
    assert np.array_equal(tk.first, full.first[:5]) and np.array_equal(tk.own, full.own[:5])
    assert np.array_equal(tk.w, full.w[:5]) and np.array_equal(tk.mu, full.mu[:5]) and np.array_equal(tk.sigma, full.sigma[:5])
    rc3, ml3, ll3, none = adaptive(H, y, sm, temps, FA.SIGMA_D, cs, 8000.0, cap=0, want_final=False)
    assert rc3 == 0 and none.n == full.n and np.array_equal(ml, ml3) and ll == ll3
    H.shutdown()


def test_enosilent_leaves_the_partial_track(H):
    """the -3 fixture of tests/test_gpu_fit_native.py: chunks of 40 samples of a busy recording; the leading trim of
    some chunk runs off it.  With the model never replaced the loop is hmmsort_fit_chunked's up to there."""
    temps = np.asfortranarray(np.stack([H.create_spike_template(30, 3.0, 0.8, 0.2),
                                        H.create_spike_template(30, 4.0, 0.3, 0.2)], axis=1))
    pp = [0.03, 0.03]
    sm = H.StateMatrix.create(2, 30, np.log(pp), False)
    y = H.create_signal(6000, 0.3, pp, temps, seed=33)
    rc0, ml0, ll0 = chunked(H, y, sm, temps, 0.3, 40)
    rc1, ml1, ll1, tk = adaptive(H, y, sm, temps, 0.3, 40, INF, len(y), cap=400)
    assert rc0 == rc1 == H._lib.ENOSILENT and "fit.jl:26" in H._lib.last_error()
    assert np.array_equal(ml0, ml1) and ll0 == ll1
    assert 1 <= tk.n < 400 and tk.first[0] == 1 and tk.own[0, 0] == 0 and tk.final is None
    assert np.all(np.diff(tk.first) > 0) and np.all(tk.own[1:, 0] >= tk.own[:-1, 1]) and np.all(tk.own[:, 1] >= tk.own[:, 0])
    assert ml1[tk.own[-1, 1]:].max() == 1                  # nothing was written past the last finished chunk
    H.shutdown()


def test_python_entries(H, cases, tracked):
    """api.fit_adaptive is the raw call; sort_data(adapt_halflife=...) adds the track to the reference's output"""
    y, onsets, sm, temps, cs = cases["ring"]
    rc, ml, ll, tk = tracked["ring", False]
    model, track = H.fit_adaptive(H.HMMSpikeTemplateModel(sm, temps, FA.SIGMA_D), y, cs, 8000.0)
    assert np.array_equal(model.ml_seq, ml) and model.ll == ll and track.n == tk.n and np.array_equal(track.mu, tk.mu)
    with pytest.raises(H.HmmsortError):
        H.fit_adaptive(H.HMMSpikeTemplateModel(sm, temps, FA.SIGMA_D), y, cs, 0.0)
    # the CLI flow decodes with the overlap model of the same templates, from int16 samples
    T = 15_000
    raw = np.round(y[:T] * 1000).astype(np.int16)
    spike_forms = np.zeros((FA.K_D, 1, 2))
    spike_forms[:, 0, :] = temps * 1000
    args = (spike_forms, [1.0 / 300.0 ** 2], list(FA.PP_D), raw)
    plain = H.sort_data(*args, dosave=False, chunksize=5000)
    out = H.sort_data(*args, dosave=False, chunksize=5000, adapt_halflife=8000)
    assert set(out) - set(plain) == {"waveforms_track", "sigma_track", "chunk_first"}
    n = len(out["chunk_first"])
    assert n >= 3 and out["chunk_first"][0] == 1 and out["waveforms_track"].shape == (n, FA.K_D, 2)
    assert np.array_equal(out["waveforms_track"][0], spike_forms[:, 0, :]) and out["sigma_track"][0] == plain["sigma"]
    assert out["mlseq"].shape == plain["mlseq"].shape and np.array_equal(out["waveforms"], plain["waveforms"])
    H.shutdown()


# ---- 5. the two device entries alone ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100_003])
def test_stats_blend_against_numpy(H, n):
    import torch
    rng = np.random.default_rng(n)
    acc0 = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, size=n)
    new = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, size=n)
    dnew = torch.from_numpy(new).cuda()
    for w in (0.0, 1.0, 0.3):
        for tail in sorted({0, min(3, n), n}):
            dacc = torch.from_numpy(acc0).cuda()
            H.stats_blend(dacc, w, dnew, n, tail)
            got = dacc.cpu().numpy()
            want = FA.blend(acc0, w, new, tail)
            assert np.array_equal(got.view(np.int64), want.view(np.int64)), (n, w, tail, np.flatnonzero(got != want)[:4])
    assert np.array_equal(dnew.cpu().numpy(), new)


def test_stats_blend_refusals(H):
    import torch
    d = torch.zeros(8, dtype=torch.float64, device="cuda")
    for w, n, tail in ((-0.1, 8, 3), (1.5, 8, 3), (float("nan"), 8, 3), (0.5, 2, 3), (0.5, 8, -1)):
        with pytest.raises(H.HmmsortError) as e:
            H.stats_blend(d, w, d, n, tail)
        assert e.value.code == H._lib.EINVAL
    assert not d.cpu().numpy().any()


def test_reconstruct_tracked_against_numpy(H):
    K, N, T = 7, 2, 1000                                   # not a multiple of the workgroup size
    sm = H.StateMatrix.create(N, K, np.log([0.01, 0.006]), True)
    S = sm.nstates
    rng = np.random.default_rng(9)
    x = rng.integers(1, S + 1, size=T).astype(np.int16)
    x[[0, 300, 301, 999]] = [S + 1, 0, -4, S + 7]           # ids out of range
    first = np.array([1, 301, 640], dtype=np.int64)
    mu = rng.standard_normal((3, K, N))
    tk = H.ModelTrack(3, first, None, None, mu, None)
    got = H.reconstruct_tracked(x, sm, tk)
    want = np.full(T, np.nan)
    for t in range(T):
        c = int(np.searchsorted(first, t + 1, side="right")) - 1
        if 1 <= x[t] <= S:
            a = 0.0
            for l in range(N):
                a += mu[c, sm.states[l, x[t] - 1] - 1, l]
            want[t] = a
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 4
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok])
    # one chunk is reconstruct_signal
    one = H.ModelTrack(1, first[:1], None, None, mu[:1], None)
    xv = np.clip(x, 1, S).astype(np.int16)
    assert np.array_equal(H.reconstruct_tracked(xv, sm, one), H.reconstruct_signal(xv, sm, np.asfortranarray(mu[0])))
    # samples before the first chunk have no model; the starts must ascend
    late = H.ModelTrack(1, np.array([11], dtype=np.int64), None, None, mu[:1], None)
    out = H.reconstruct_tracked(xv, sm, late)
    assert np.isnan(out[:10]).all() and not np.isnan(out[10:]).any()
    with pytest.raises(H.HmmsortError):
        H.reconstruct_tracked(xv, sm, H.ModelTrack(2, np.array([5, 5], dtype=np.int64), None, None, mu[:2], None))


def test_reconstruct_tracked_at_the_largest_table(H):
    """8 192 chunk starts fill the LDS table; one more is refused"""
    K, N, n = 3, 1, 8192
    sm = H.StateMatrix.create(N, K, np.log([0.01]), False)
    T = n + 37
    x = (np.arange(T) % sm.nstates + 1).astype(np.int16)
    first = np.arange(1, n + 1, dtype=np.int64)
    mu = np.arange(n * K * N, dtype=np.float64).reshape(n, K, N)
    got = H.reconstruct_tracked(x, sm, H.ModelTrack(n, first, None, None, mu, None))
    c = np.minimum(np.arange(T), n - 1)
    assert np.array_equal(got, mu[c, sm.states[0, x - 1] - 1, 0])
    more = np.arange(1, n + 2, dtype=np.int64)
    with pytest.raises(H.HmmsortError) as e:
        H.reconstruct_tracked(x, sm, H.ModelTrack(n + 1, more, None, None, np.zeros((n + 1, K, N)), None))
    assert e.value.code == H._lib.EUNSUP


def test_reconstruction_follows_the_track(H, cases, tracked):
    """the residual of the tracked reconstruction on the drifted tail is smaller than that of the caller's templates"""
    y, onsets, sm, temps, cs = cases["ring"]
    rc, ml, ll, tk = tracked["ring", False]
    tail = slice(32_000, len(y))
    r_track = y - H.reconstruct_tracked(ml, sm, tk)
    r_fixed = y - H.reconstruct_signal(ml, sm, temps)
    assert np.sum(r_track[tail] ** 2) < 0.8 * np.sum(r_fixed[tail] ** 2)
