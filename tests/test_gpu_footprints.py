"""hmmsort_footprints / _device / hmmsort_plan_footprints against the numpy model
tests/footprint_model.py: sum, sumsq, nused and n must come out equal to the bit from the host form (fp64 and int16),
the device form on torch tensors, the plan form (single, batched, an overlap model on the blocked engine) and
sort_data; every refusal returns its code, names its argument and writes nothing; and on a synthetic four-channel
block the footprints and the coincidence counts together find and resolve the neuron that two channels see."""
import ctypes as C

import numpy as np
import pytest

import footprint_model as FM

pytestmark = pytest.mark.gpu

NAMES = ("sum", "sumsq", "nused", "n")


@pytest.fixture(scope="module")
def cases():
    return FM.cases()


@pytest.fixture(scope="module")
def wanted(cases):
    """the model's result of every shared case, computed once"""
    return {k: FM.model(*v) for k, v in cases.items()}


def parts(fp):
    return fp.sum, fp.sumsq, fp.n_used, fp.n


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
        assert len(bad) == 0, (what, name, len(bad), bad[:4].tolist(), g[tuple(bad[:4].T)], w[tuple(bad[:4].T)])


def run(H, case):
    y, lists, pre, W, chan = case
    fp = H.footprints(y, lists, pre=pre, W=W, channels=chan)
    assert fp.pre == pre and np.array_equal(fp.channels, FM.table_of(len(lists), y.shape[0], chan))
    return fp


# ---- 1: degenerate lists ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w1", "edges", "w51"])
def test_degenerate_lists(H, cases, wanted, name):
    key = "degenerate_" + name
    fp = run(H, cases[key])
    same(parts(fp), wanted[key], key)
    y = cases[key][0]
    if name == "w1":
        assert fp.n_used.tolist() == [0, 1] and np.array_equal(fp.sum[1, :, 0], y[:, 16]) and not fp.sum[0].any()
    elif name == "edges":
        assert fp.n_used.tolist() == [0, 1, 2] and fp.n.tolist() == [0, 1, 5]
        assert np.array_equal(fp.sum[2], y[:, 0:10] + y[:, 40:50])
    else:
        assert not fp.n_used.any() and not fp.sum.any() and not fp.sumsq.any() and fp.n.tolist() == [0, 1, 5]
        assert fp.peak_channel.tolist() == [-1, -1, -1]


# ---- 2: seams -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", FM.SEAM_W)
def test_seams(H, cases, wanted, W):
    key = "seam_W%d" % W
    fp = run(H, cases[key])
    same(parts(fp), wanted[key], key)
    assert fp.n.tolist() == list(FM.SEAM_N) and fp.n_used.tolist() == [n - 2 for n in FM.SEAM_N]
    again = run(H, cases[key])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts(fp), parts(again)))


def test_seams_slot_boundary_inside_a_window(H, cases, wanted):
    fp = run(H, cases["seam_M5_W60"])             # M W = 300: just above 256
    same(parts(fp), wanted["seam_M5_W60"], "M = 5, W = 60")
    assert fp.sum.shape == (4, 5, 60) and np.array_equal(fp.sum[:, 2], fp.sum[:, 3])      # channel 1 twice


# ---- 3: channel tables --------------------------------------------------------------------------------------------
def test_channel_tables(H, cases, wanted):
    y, lists, pre, W, chan = cases["channel_table"]
    fp = run(H, cases["channel_table"])
    same(parts(fp), wanted["channel_table"], "table")
    full = H.footprints(y, lists, pre=pre, W=W)
    assert full.sum.shape == (4, 3, W) and fp.sum.shape == (4, 4, W)                      # M != C
    for u in range(4):
        for m in range(4):
            c = chan[u, m]
            if c < 0:
                assert not fp.sum[u, m].any() and not fp.sumsq[u, m].any()
            else:
                assert fp.sum[u, m].tobytes() == full.sum[u, c].tobytes()
                assert fp.sumsq[u, m].tobytes() == full.sumsq[u, c].tobytes()
    assert np.array_equal(fp.n_used, full.n_used) and fp.peak_channel[2] == -1     # unit 2 lists no channel
    one = H.footprints(y, lists, pre=pre, W=W, channels=[2, 0])                           # one list for every unit
    assert one.sum.tobytes() == full.sum[:, [2, 0]].tobytes()


# ---- 4: int16 -----------------------------------------------------------------------------------------------------
def test_int16_block(H, cases):
    _, lists, pre, W, _ = cases["seam_W60"]
    rng = np.random.default_rng(44)
    raw = rng.integers(-32768, 32768, (3, 40_000)).astype(np.int16)
    a = H.footprints(raw, lists, pre=pre, W=W)
    b = H.footprints(raw.astype(np.float64), lists, pre=pre, W=W)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(parts(a), parts(b)))
    same(parts(a), FM.model(raw.astype(np.float64), lists, pre, W), "int16")
    assert np.abs(a.sum).max() > 32768


# ---- 5: the device form -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["seam_W65", "channel_table", "degenerate_edges"])
def test_device_form(H, cases, wanted, key):
    import torch
    device = H.device
    y, lists, pre, W, chan = cases[key]
    offs = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    d_y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    d_t = torch.from_numpy(np.concatenate(lists).astype(np.int64)).cuda()
    fp = device.footprints(d_y, d_t, offs, pre=pre, W=W, channels=chan)
    same(parts(fp), wanted[key], key)
    host = run(H, cases[key])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts(fp), parts(host)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    fp2 = device.footprints(d_y, d_t, offs, pre=pre, W=W, channels=chan, stream=side.cuda_stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts(fp), parts(fp2)))


# ---- 6: the plan form ---------------------------------------------------------------------------------------------
def ring_setup(H, nC, T=4000, K=12, seed=60):
    pp, sg = (0.01, 0.008), 0.3
    base = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                       H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    mus = [np.asfortranarray(base * (1.0 + 0.1 * c)) for c in range(nC)]
    ys = [H.create_signal(T, sg, pp, mus[c], seed=seed + c) for c in range(nC)]
    sm = H.StateMatrix.create(2, K, np.log(pp), False)
    return sm, mus, ys, sg


@pytest.mark.parametrize("nC", [1, 2])
def test_plan_form(H, nC):
    import torch
    T = 4000
    sm, mus, ys, sg = ring_setup(H, nC, T)
    rng = np.random.default_rng(61)
    block = FM.wide_block(rng, 3, T)
    block[0] = ys[0]                                  # the channel the plan was sorted on, and two others
    d_block = torch.from_numpy(block).cuda()
    dx = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
    dll = torch.zeros(nC, dtype=torch.float64, device="cuda")
    chan = np.tile(np.array([2, -1, 0, 0], dtype=np.int32), (2 * nC, 1))
    H.set_option("engine", H.ENGINE_AUTO if nC == 1 else H.ENGINE_WAVE)
    try:
        if nC == 1:
            plan = H.Plan(T, sm, mus[0], sg)
            plan.viterbi(torch.from_numpy(ys[0]).cuda(), dx, dll)
        else:
            plan = H.Plan.batched(T, [sm] * nC, mus, [sg] * nC)
            plan.viterbi(torch.from_numpy(np.stack(ys)).cuda(), dx, dll)
        fp = plan.footprints(dx, d_block, pre=5, W=14)
        fpc = plan.footprints(dx, d_block, pre=5, W=14, channels=chan, stream=torch.cuda.current_stream().cuda_stream)
        plan.close()
        lists = []
        for c in range(nC):
            one = H.Plan(T, sm, mus[c], sg)
            lists += one.extract_spiketimes(dx[c])
            one.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    assert len(lists) == 2 * nC and all(len(t) > 10 for t in lists)
    host = H.footprints(block, lists, pre=5, W=14)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts(fp), parts(host)))
    same(parts(fp), FM.model(block, lists, 5, 14), "plan form, %d channel(s)" % nC)
    same(parts(fpc), FM.model(block, lists, 5, 14, chan), "plan form with a table")
    assert fp.sum.shape == (2 * nC, 3, 14) and fpc.sum.shape == (2 * nC, 4, 14)


def test_plan_form_overlap_model_on_the_blocked_engine(H):
    import torch
    pp, sg, T, K = (0.02, 0.015), 0.4, 4100, 12
    mu = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                     H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    sm = H.StateMatrix.create(2, K, np.log(pp), True)
    y = H.create_signal(T, sg, pp[:1], mu[:, :1], seed=3) + H.create_signal(T, 0.0, pp[1:], mu[:, 1:], seed=1003)
    block = np.stack([y, y[::-1].copy(), 0.5 * y])
    H.set_option("engine", H.ENGINE_BLOCKED)
    try:
        plan = H.Plan(T, sm, mu, sg)
        assert plan.info()["engine"] == H.ENGINE_BLOCKED
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(torch.from_numpy(y).cuda(), dx, dll)
        fp = plan.footprints(dx, torch.from_numpy(block).cuda(), pre=4, W=16)
        lists = plan.extract_spiketimes(dx)
        plan.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    assert all(len(t) > 10 for t in lists)
    same(parts(fp), FM.model(block, lists, 4, 16), "overlap model")
    assert fp.peak_channel.tolist() == [0, 0]


# ---- 7: refusals --------------------------------------------------------------------------------------------------
SENT_F, SENT_I = -7.25, -77


def raw_call(H, y=None, lists=None, C_=2, T=50, U=None, pre=3, W=10, M=2, chan=None, stype=None, n=True, opt=True,
             counts=None, null_y=False, null_times=False):
    """hmmsort_footprints on sentinel-filled outputs -> rc; whatever the call returns, a refusal must not have written"""
    L = H._lib
    y = np.zeros((2, 50)) if y is None else y
    lists = [np.array([5, 9]), np.array([7])] if lists is None else lists
    lists = [np.ascontiguousarray(t, dtype=np.int64) for t in lists]
    U = len(lists) if U is None else U
    ptrs = (C.c_void_p * max(len(lists), 1))(*[t.ctypes.data if len(t) else None for t in lists])
    cnt = np.array([len(t) for t in lists] + [0], dtype=np.int64) if counts is None else np.asarray(counts, np.int64)
    size = 4096
    s, q = np.full(size, SENT_F), np.full(size, SENT_F)
    nu, nn = np.full(size, SENT_I, dtype=np.int64), np.full(size, SENT_I, dtype=np.int64)
    ch = None if chan is None else np.ascontiguousarray(chan, dtype=np.int32)
    o = L.FpOpt(pre, W, M, None if ch is None else ch.ctypes.data)
    out = L.FpOut(s.ctypes.data, q.ctypes.data, nu.ctypes.data, nn.ctypes.data if n else None)
    rc = L.lib().hmmsort_footprints(None if null_y else L.ptr(y), L.SAMPLES_F64 if stype is None else stype, C_, T, U,
                                    None if null_times else ptrs, L.ptr(cnt), C.byref(o) if opt else None,
                                    C.byref(out))
    if rc != 0:
        assert np.all(s == SENT_F) and np.all(q == SENT_F) and np.all(nu == SENT_I) and np.all(nn == SENT_I)
    return rc


def test_refusals(H):
    L = H._lib
    one = np.array([7])

    def refused(code, *words, **kw):
        rc = raw_call(H, **kw)
        assert rc == code and all(w in L.last_error() for w in words), (rc, L.last_error(), words)

    refused(L.EINVAL, "null", null_y=True)                      # a null required argument, one by one
    refused(L.EINVAL, "null", null_times=True)
    refused(L.EINVAL, "null", n=False)
    refused(L.EINVAL, "null", opt=False)
    refused(L.EINVAL, "C = 0", C_=0)
    refused(L.EINVAL, "C = 1025", C_=1025)
    refused(L.EINVAL, "T = 0", T=0)
    refused(L.EINVAL, "T = %d" % ((1 << 36) + 1), T=(1 << 36) + 1)
    refused(L.EINVAL, "U = 0", U=0)
    refused(L.EINVAL, "U = 4097", lists=[one] * 4097)
    refused(L.EINVAL, "W = 0", W=0)
    refused(L.EINVAL, "W = 1025", W=1025)
    refused(L.EINVAL, "pre = -1", pre=-1)
    refused(L.EINVAL, "pre = %d" % ((1 << 20) + 1), pre=(1 << 20) + 1)
    refused(L.EINVAL, "M = 0", M=0, chan=[[0], [0]])
    refused(L.EINVAL, "M = 1025", M=1025, chan=np.zeros((2, 1025)))
    refused(L.EINVAL, "chan", "unit 1", "slot 0", "channel 2", M=2, chan=[[0, 1], [2, 0]])
    refused(L.EINVAL, "chan", "unit 0", "slot 1", "channel -2", M=2, chan=[[0, -2], [1, 0]])
    refused(L.EINVAL, "counts", "unit 1", "-3", counts=[2, -3, 0])
    refused(L.EINVAL, "unit 1", "position 0", "time 0", lists=[np.array([5, 9]), np.array([0, 7])])
    refused(L.EINVAL, "unit 0", "position 2", "2^40", lists=[np.array([1, 2, (1 << 40) + 1]), one])
    refused(L.EINVAL, "unit 1", "position 2", "ascending", lists=[np.array([5, 9]), np.array([4, 7, 7])])
    refused(L.EINVAL, "unit 0", "position 1", "ascending", lists=[np.array([4, 3]), one])
    refused(L.EINVAL, "sample_type", stype=L.SAMPLES_F32)
    refused(L.EINVAL, "sample_type", stype=L.SAMPLES_I32)
    refused(L.EUNSUP, str(4096 * 1024 * 1024), "entries", lists=[one] * 4096, M=1024, W=1024,
            chan=np.zeros((4096, 1024)))
    refused(L.EUNSUP, str(4096 * 1024 * 65), "entries", lists=[one] * 4096, C_=1024, W=65)      # M = C without a table
    with pytest.raises(H.HmmsortError) as e:
        H.footprints(np.zeros((2, 50)), [[5, 9], [7, 7]])
    assert e.value.code == L.EINVAL and "unit 1" in str(e.value)
    assert raw_call(H) == 0                                      # and the input the refusals varied is taken
    assert raw_call(H, W=51) == 0                                # W > T is legal


def test_refusals_of_the_device_and_plan_forms(H):
    import torch
    device = H.device
    L = H._lib
    d_y = torch.zeros((2, 50), dtype=torch.float64, device="cuda")
    d_t = torch.tensor([5, 9, 7], dtype=torch.int64, device="cuda")
    for offs, words in (([0, 2, 1], ("unit 1", "-1")), ([-1, 2, 3], ("offs[0]",))):
        with pytest.raises(H.HmmsortError) as e:
            device.footprints(d_y, d_t, offs, pre=3, W=10)
        assert e.value.code == L.EINVAL and all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(H.HmmsortError) as e:
        device.footprints(d_y, d_t, [0, 2, 3], pre=3, W=10, channels=[0, 2])
    assert e.value.code == L.EINVAL and "channel 2" in str(e.value)
    # times the device form cannot check are harmless: a window that leaves the block is not used, whatever the time
    wild = torch.tensor([-5, 0, 7, 1 << 62, -(1 << 62)], dtype=torch.int64, device="cuda")
    fp = device.footprints(d_y + 1.0, wild, [0, 5], pre=3, W=10)
    assert fp.n.tolist() == [5] and fp.n_used.tolist() == [1] and np.all(fp.sum == 1.0)
    sm, mus, _, sg = ring_setup(H, 1)
    plan = H.Plan(4000, sm, mus[0], sg)
    d_b = torch.zeros((2, 4000), dtype=torch.float64, device="cuda")
    dx = torch.ones(4000, dtype=torch.int16, device="cuda")
    with pytest.raises(H.HmmsortError) as e:
        plan.footprints(dx, d_b, pre=3, W=2000)
    assert e.value.code == L.EINVAL and "W = 2000" in str(e.value)
    with pytest.raises(ValueError):
        plan.footprints(dx, d_y)                                 # 50 samples per channel, the plan has 4000
    fp = plan.footprints(dx, d_b, pre=3, W=10)                   # a silent path: no events, zeros
    assert fp.n.tolist() == [0, 0] and not fp.sum.any() and fp.sum.shape == (2, 2, 10)
    plan.close()


# ---- 8: end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(H):
    """four channels: neuron A on channel 0 (amplitude 1.0) and, two samples later, on channel 1 (0.6); neuron B on
    channel 2; channel 3 noise.  Channels 0-2 sorted by a batched plan of one template each, under the true templates."""
    import torch
    T, K, sg = 20_000, 30, 0.3
    tA, tB = H.create_spike_template(K, 3.0, 0.8, 0.2), H.create_spike_template(K, 4.0, 0.3, 0.2)
    trainA = H.create_signal(T, 0.0, [0.008], tA[:, None], seed=80)
    trainB = H.create_signal(T, 0.0, [0.006], tB[:, None], seed=81)
    noise = sg * np.random.default_rng(82).standard_normal((4, T))
    lateA = np.concatenate([np.zeros(2), trainA[:-2]])
    block = noise + np.stack([trainA, 0.6 * lateA, trainB, np.zeros(T)])
    mus = [np.asfortranarray(m[:, None]) for m in (tA, 0.6 * tA, tB)]
    sms = [H.StateMatrix.create(1, K, np.log([p]), False) for p in (0.008, 0.008, 0.006)]
    d_block = torch.from_numpy(block).cuda()
    dx = torch.zeros((3, T), dtype=torch.int16, device="cuda")
    dll = torch.zeros(3, dtype=torch.float64, device="cuda")
    H.set_option("engine", H.ENGINE_WAVE)
    try:
        plan = H.Plan.batched(T, sms, mus, [sg] * 3)
        plan.viterbi(d_block[:3].contiguous(), dx, dll)
        cg = plan.correlograms(dx, coincidence=3)
        fp = plan.footprints(dx, d_block, pre=20, W=60)
        plan.close()
        lists = []
        for c in range(3):
            one = H.Plan(T, sms[c], mus[c], sg)
            lists += one.extract_spiketimes(dx[c])
            one.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    return block, lists, cg, fp


def test_end_to_end_duplicate_across_channels(H, probe):
    block, lists, cg, fp = probe
    assert all(len(t) > 60 for t in lists)
    same(parts(fp), FM.model(block, lists, 20, 60), "probe")
    dup = [p[:2] for p in H.duplicate_units(cg)]
    assert (0, 1) in dup and (1, 0) in dup and all(2 not in p for p in dup)
    assert fp.peak_channel.tolist() == [0, 0, 2]
    sim, lag = H.footprint_similarity(fp)
    assert sim[0, 1] > 0.9 and abs(int(lag[0, 1])) == 2 and lag[1, 0] == -lag[0, 1]
    assert lag[0, 1] == -2                      # unit 1's spikes are 2 samples late, so its mean sits 2 samples early
    keep, pairs = H.resolve_duplicates(cg, fp)
    assert keep.tolist() == [True, False, True] and [p[:2] for p in pairs] == [(0, 1)]
    x = H.unit_locations(fp, [0.0, 10.0, 20.0, 30.0])
    assert 0.0 < x[0] < 5.0 and 0.0 < x[1] < 5.0 and 15.0 < x[2] < 25.0


def test_sort_data_returns_the_footprints(H):
    T, K = 12_000, 16
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                        H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    pp = (0.01, 0.006)
    y = H.create_signal(T, 0.3, pp, temps, seed=85)
    rng = np.random.default_rng(86)
    cols = np.stack([y, 0.5 * y + 0.3 * rng.standard_normal(T), 0.3 * rng.standard_normal(T)], axis=1)
    raw = np.round(cols * 1000).astype(np.int16)                   # (T, C), as acquisition writes it
    spike_forms = np.zeros((K, 1, 2))
    spike_forms[:, 0, :] = temps * 1000
    args = (spike_forms, [1.0 / 300.0 ** 2], list(pp), raw)
    plain = H.sort_data(*args, dosave=False, chunksize=4000, preprocess={}, channel=0)
    out = H.sort_data(*args, dosave=False, chunksize=4000, preprocess={}, channel=0, footprints=True)
    assert set(plain) == {"mlseq", "ll", "waveforms", "lp", "sigma"}
    assert set(out) - set(plain) == {"footprint", "footprint_n", "peak_channel"}
    assert all(np.array_equal(out[k], plain[k]) for k in plain)
    sm = H.StateMatrix.create(2, K, np.log(pp), True)
    tm = H.HMMSpikeTemplateModel(sm, np.asfortranarray(spike_forms[:, 0, :]), 300.0)
    lists = H.extract_spiketimes(H.fit(tm, raw[:, 0].astype(np.float64), 4000))
    assert all(len(t) > 20 for t in lists)
    block = np.ascontiguousarray(raw.T.astype(np.float64))
    s, q, nused, n = FM.model(block, lists, 20, 60)
    want = H.Footprints(s, q, nused, n, FM.table_of(2, 3, None), 20)
    assert out["footprint"].shape == (2, 3, 60) and out["footprint"].tobytes() == want.mean.tobytes()
    assert np.array_equal(out["footprint_n"], nused) and out["peak_channel"].tolist() == [0, 0]
    opt = H.sort_data(*args, dosave=False, chunksize=4000, preprocess={}, channel=0, footprints=dict(pre=4, W=9))
    s2, q2, nused2, _ = FM.model(block, lists, 4, 9)
    assert opt["footprint"].tobytes() == H.Footprints(s2, q2, nused2, n, want.channels, 4).mean.tobytes()
    with pytest.raises(ValueError) as e:
        H.sort_data(*args, dosave=False, footprints=True)
    assert "preprocess" in str(e.value)
    H.shutdown()
