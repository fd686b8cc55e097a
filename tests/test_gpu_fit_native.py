"""The chunked decode fit(HMMSpikingModel, templates, X, chunksize) (fit.jl:11-42) as native C-ABI calls:
hmmsort_chunk_stitch (the stitch rule as kernels), hmmsort_fit_chunked / _i16 (one channel) and
hmmsort_fit_channels (many channels, each with its own model, in step on streams of their own).  Everything is
compared with the oracle's restatement hmm_oracle_fit_chunked: path with array_equal, ll with ==.  Every test
first asserts the oracle's own return code, so a changed random stream shows as a failed precondition."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm, two_templates

pytestmark = pytest.mark.gpu


# ---- helpers -------------------------------------------------------------------------------------
def templates(H, N, K):
    return two_templates(H, K) if N == 2 else np.asfortranarray(four_templates(H, K)[:, :N])


def make(H, N, K, pp, T, seed, overlaps, temps=None, cut=None):
    """(signal, StateMatrix, templates): create_signal(T, 0.3, pp, temps, seed), optionally cut short"""
    temps = templates(H, N, K) if temps is None else temps
    sm = H.StateMatrix.create(N, K, np.log(pp), overlaps)
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    return (y if cut is None else y[:cut].copy()), sm, temps


def native(H, y, sm, mu, sigma, chunksize):
    """hmmsort_fit_chunked / _i16 without raising: (rc, ml_seq, ll, message)"""
    from hmmsort_amd.api import _model_args
    from hmmsort_amd._lib import last_error, lib, ptr
    y = np.ascontiguousarray(y)
    keep, margs = _model_args(sm, mu, sigma)
    ml = np.full(len(y), -9, dtype=np.int16)
    ll = C.c_double(np.nan)
    entry = lib().hmmsort_fit_chunked_i16 if y.dtype == np.int16 else lib().hmmsort_fit_chunked
    rc = entry(ptr(y), len(y), int(chunksize), *margs, ptr(ml), C.cast(C.byref(ll), C.c_void_p))
    return rc, ml, ll.value, (last_error() if rc else "")


def channels(H, ys, models, chunksize, devices=None):
    """hmmsort_fit_channels without raising: (rc, [ml_seq], ll array, status list, message)"""
    from hmmsort_amd import _lib
    from hmmsort_amd.api import _model_args
    n, T = len(ys), len(ys[0])
    ys = [np.ascontiguousarray(y) for y in ys]
    keep, recs = [], (_lib.Model * n)()
    for c, (sm, mu, sigma) in enumerate(models):
        k, m = _model_args(sm, mu, sigma)
        keep.append(k)
        recs[c] = _lib.Model(*m)
    ml = [np.full(T, -9, dtype=np.int16) for _ in range(n)]
    ll = np.full(n, np.nan)
    status = (C.c_int * n)(*([99] * n))
    yp = (C.c_void_p * n)(*[y.ctypes.data for y in ys])
    op = (C.c_void_p * n)(*[m.ctypes.data for m in ml])
    dev = (C.c_int * len(devices))(*devices) if devices else None
    stype = _lib.SAMPLES_I16 if ys[0].dtype == np.int16 else _lib.SAMPLES_F64
    rc = _lib.lib().hmmsort_fit_channels(n, yp, stype, T, int(chunksize), recs, dev, len(devices) if devices else 0,
                                         op, _lib.ptr(ll), status)
    return rc, ml, ll, list(status), (_lib.last_error() if rc else "")


def agree(H, O, y, sm, mu, sigma, chunksize, expect_rc=0, exact_ll=True):
    """the native call against the oracle: its return code first, then the path bit for bit and ll with ==.
    exact_ll=False is for a chunk that is the whole recording: that result is hmmsort_viterbi's, ll included, and
    hmmsort_viterbi keeps the 1e-9 relative of the time-parallel engines (tests/test_gpu_wave_viterbi.py)."""
    orc, oml, oll = O.fit_chunked(np.asarray(y, dtype=np.float64), to_oracle_sm(O, sm), mu, sigma, chunksize)
    assert orc == expect_rc, ("oracle precondition", orc)
    rc, ml, ll, msg = native(H, y, sm, mu, sigma, chunksize)
    assert rc == (0 if expect_rc == 0 else H._lib.ENOSILENT), (rc, msg)
    assert np.array_equal(ml, oml), np.flatnonzero(ml != oml)[:8]
    print("chunksize %d: ll %.17g, oracle %.17g, difference %.3g" % (chunksize, ll, oll, ll - oll))
    assert abs(ll - oll) <= 1e-9 * abs(oll), (ll, oll)
    if exact_ll:
        assert ll == oll, (ll, oll)
    return rc, ml, ll, msg


# ---- 1. the stitch kernels alone ---------------------------------------------------------------
GUARD = 8
PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def stitch_rule(x, silent, lead, trail):
    """fit.jl:24-36 on one decoded chunk whose silent samples are at the 0-based positions `silent`:
    (l, kk, the guarded destination as it must read afterwards)"""
    k = len(x)
    l, kk = 1, k
    if lead:
        l = int(silent[0]) + 1 if len(silent) else k + 1
    if trail:
        kk = int(silent[-1]) + 1 if len(silent) else 0
    dst = np.full(k + 2 * GUARD, -7, dtype=np.int16)
    if l <= kk:
        dst[GUARD + l - 1:GUARD + kk] = x[l - 1:kk]
    return l, kk, dst


class Stitcher:
    def __init__(self, H, k):
        import torch
        self.torch, self.k = torch, k
        self.fn = H._lib.lib().hmmsort_chunk_stitch
        self.dx = torch.empty(k, dtype=torch.int16, device="cuda")
        self.dst = torch.empty((4, k + 2 * GUARD), dtype=torch.int16, device="cuda")
        self.lk = torch.empty((4, 2), dtype=torch.int64, device="cuda")

    def check(self, x):
        torch, k = self.torch, self.k
        self.dx.copy_(torch.from_numpy(x))
        self.dst.fill_(-7)
        self.lk.fill_(-99)
        st = torch.cuda.current_stream().cuda_stream
        for n, (lead, trail) in enumerate(PAIRS):
            rc = self.fn(self.dx.data_ptr(), k, lead, trail, self.dst[n].data_ptr() + 2 * GUARD,
                         self.lk[n].data_ptr(), st)
            assert rc == 0
        dst, lk = self.dst.cpu().numpy(), self.lk.cpu().numpy()
        silent = np.flatnonzero(~(x > 1))
        for n, (lead, trail) in enumerate(PAIRS):
            l, kk, want = stitch_rule(x, silent, lead, trail)
            assert (lk[n, 0], lk[n, 1]) == (l, kk), (k, lead, trail, lk[n], l, kk)
            assert np.array_equal(dst[n], want), (k, lead, trail, l, kk, np.flatnonzero(dst[n] != want)[:8])


@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 100_000])
def test_stitch_kernel_on_crafted_chunks(H, k):
    s = Stitcher(H, k)
    rng = np.random.default_rng(k)
    busy = rng.integers(2, 900, size=k).astype(np.int16)          # no silent sample
    s.check(np.ones(k, dtype=np.int16))                           # all silent
    s.check(busy)
    for p in (0, k - 1):                                          # silent at the first / last sample only
        x = busy.copy()
        x[p] = 1
        s.check(x)
    # silent at one position p, for every p within +-1 of a multiple of 64 (which covers 256 and 1024)
    ps = sorted({m + d for m in range(0, k + 1, 64) for d in (-1, 0, 1) if 0 <= m + d < k})
    for p in ps:
        x = busy.copy()
        x[p] = 1
        s.check(x)
    for _ in range(20):
        x = busy.copy()
        x[rng.random(k) >= 0.9] = 1
        s.check(x)


def test_stitch_kernel_refuses_bad_arguments(H):
    import torch
    fn = H._lib.lib().hmmsort_chunk_stitch
    d = torch.zeros(16, dtype=torch.int16, device="cuda")
    lk = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert fn(d.data_ptr(), 0, 1, 1, d.data_ptr(), lk.data_ptr(), None) == H._lib.EINVAL
    assert fn(d.data_ptr(), 1 << 31, 1, 1, d.data_ptr(), lk.data_ptr(), None) == H._lib.EINVAL
    assert fn(None, 4, 1, 1, d.data_ptr(), lk.data_ptr(), None) == H._lib.EINVAL


# ---- 2. ring model, wave and strict chunk plans ------------------------------------------------
@pytest.mark.parametrize("pp,seed,chunks", [([0.03, 0.03], 7, (1500, 300)), ([0.004, 0.003], 33, (700, 2500))])
def test_ring_model_chunks(O, H, pp, seed, chunks):
    y, sm, temps = make(H, 2, 30, pp, 6000, seed, False)
    raw = np.round(100.0 * y).astype(np.int16)
    temps100 = np.asfortranarray(temps * 100.0)
    from hmmsort_amd.device import Plan
    engines = {1500: H.ENGINE_WAVE, 300: H.ENGINE_STRICT}        # the two plans this case is about
    for cs in chunks:
        if cs in engines:
            with_plan = Plan(cs, sm, temps, 0.3)
            try:
                assert with_plan.info()["engine"] == engines[cs], cs
            finally:
                with_plan.close()
        _, ml, _, _ = agree(H, O, y, sm, temps, 0.3, cs)
        assert ml.max() > 1
        agree(H, O, raw, sm, temps100, 30.0, cs)                  # int16 samples, widened on the device
    H.shutdown()


# ---- 3. whole recording and boundary sizes -----------------------------------------------------
def test_whole_recording_and_boundary_sizes(O, H):
    y, sm, temps = make(H, 2, 30, [0.004, 0.003], 6000, 33, False)
    x, llv = H.viterbi(y, sm, temps, 0.3)
    for cs in (0, 6000, 7000):
        rc, ml, ll, msg = native(H, y, sm, temps, 0.3, cs)
        assert rc == 0, msg
        assert np.array_equal(ml, x) and ll == llv, cs
    for cs in (6000, 7000):
        agree(H, O, y, sm, temps, 0.3, cs, exact_ll=False)        # hmmsort_viterbi's value, asserted above
    _, _, ll, _ = agree(H, O, y, sm, temps, 0.3, 3001)
    assert ll != llv
    agree(H, O, y, sm, temps, 0.3, 5999, expect_rc=-3)           # a two-sample last chunk without a silent sample
    agree(H, O, y, sm, temps, 0.3, 2, expect_rc=-2)
    rc, ml, ll, msg = native(H, y[:1].copy(), sm, temps, 0.3, 100)
    assert rc == 0 and ml.tolist() == [1] and ll == 0.0
    H.shutdown()


# ---- 4. both fatal edges with their partial results --------------------------------------------
def test_leading_trim_off_the_chunk_is_enosilent(O, H):
    y, sm, temps = make(H, 2, 30, [0.03, 0.03], 6000, 33, False)
    rc, ml, ll, msg = agree(H, O, y, sm, temps, 0.3, 40, expect_rc=-3)
    assert rc == H._lib.ENOSILENT and "fit.jl:26" in msg and "chunk at sample" in msg
    assert ml.max() > 1                                           # chunks before the fatal one were written
    H.shutdown()


@pytest.mark.parametrize("seed,cs", [(13, 35), (22, 40)])
def test_chunk_that_does_not_advance_is_enosilent(O, H, seed, cs):
    y, sm, temps = make(H, 2, 30, [0.03, 0.03], 3000, seed, False)
    rc, ml, ll, msg = agree(H, O, y, sm, temps, 0.3, cs, expect_rc=-2)
    assert rc == H._lib.ENOSILENT and "fit.jl:41" in msg and "would not advance" in msg
    assert ll != 0.0                                              # the fatal chunk's ll was added (oracle: after)
    H.shutdown()


# ---- 5. overlap models on the blocked engine ---------------------------------------------------
def overlap_case(O, H, N, K, pp, T, seed, chunks):
    y, sm, temps = make(H, N, K, pp, T, seed, True)
    tm = H.HMMSpikeTemplateModel(sm, temps, 0.3)
    from hmmsort_amd.device import Plan
    for cs in chunks:
        with_plan = Plan(cs, sm, temps, 0.3)
        try:
            assert with_plan.info()["engine"] == H.ENGINE_BLOCKED
        finally:
            with_plan.close()
        _, ml, ll, _ = agree(H, O, y, sm, temps, 0.3, cs)
        f = H.fit(tm, y, cs)                                      # the host loop and the native loop agree:
        assert np.array_equal(f.ml_seq, ml)                       # the same arrays; api.fit adds the blocked plans'
        assert abs(f.ll - ll) <= 1e-9 * abs(ll), (f.ll, ll)       # own ll, which is summed in parts (1e-9 relative)
    H.shutdown()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_overlap_two_templates_blocked_chunks(O, H, seed):
    overlap_case(O, H, 2, 12, [0.02, 0.015], 24_000, seed, (4096, 6000))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_overlap_three_templates_blocked_chunks(O, H, seed):
    overlap_case(O, H, 3, 8, [0.02, 0.015, 0.01], 24_000, seed, (4096, 6000))


def test_overlap_900_states_blocked_chunks(O, H):
    overlap_case(O, H, 2, 30, [0.01, 0.008], 30_000, 1, (5000,))


# ---- 6. the ladder inside the loop -------------------------------------------------------------
@pytest.mark.parametrize("overlaps", [False, True])
@pytest.mark.parametrize("seed", [1, 2])
def test_duplicate_templates_go_through_the_ladder(O, H, seed, overlaps):
    t1 = two_templates(H, 12)[:, 0]
    twins = np.asfortranarray(np.stack([t1, t1], 1))
    y, sm, temps = make(H, 2, 12, [0.02, 0.015], 24_000, seed, overlaps, temps=twins)
    try:
        for cs in (4096, 6000):
            H.shutdown()
            H.viterbi(y[:cs].copy(), sm, temps, 0.3)              # what the existing entry leaves for the first chunk
            first = H.get_option("last_escalations")
            agree(H, O, y, sm, temps, 0.3, cs)
            assert H.get_option("last_escalations") >= first >= 0
        H.set_option("escalate", 0)
        rc, ml, ll, msg = native(H, y, sm, temps, 0.3, 4096)
        assert rc in (0, H._lib.ENOSILENT), msg                   # it returns; the path is the time-parallel one
        assert H.get_option("last_escalations") == 0
    finally:
        H.set_option("escalate", 1)
        H.shutdown()


# ---- 7. channels --------------------------------------------------------------------------------
T_CH, CS_CH = 6000, 1500


@pytest.fixture(scope="module")
def five(O, H):
    """five different models (N, K, overlaps mixed) of cases 2 and 5, cut to 6 000 samples, with the oracle's answer
    and the single-channel native answer of each"""
    cases = [make(H, 2, 30, [0.03, 0.03], 6000, 7, False),
             make(H, 2, 30, [0.004, 0.003], 6000, 33, False),
             make(H, 2, 12, [0.02, 0.015], 24_000, 2, True, cut=T_CH),
             make(H, 3, 8, [0.02, 0.015, 0.01], 24_000, 1, True, cut=T_CH),
             make(H, 2, 30, [0.01, 0.008], 30_000, 2, True, cut=T_CH)]
    ys = [c[0] for c in cases]
    models = [(c[1], c[2], 0.3) for c in cases]
    single = []
    for y, (sm, mu, sg) in zip(ys, models):
        rc, ml, ll, _ = agree(H, O, y, sm, mu, sg, CS_CH)         # asserts the oracle returns 0
        single.append((ml, ll))
    return ys, models, single


def same_as_single(out, single):
    rc, ml, ll, status, msg = out
    assert rc == 0 and status == [0] * len(single), (rc, status, msg)
    for c, (ml1, ll1) in enumerate(single):
        assert np.array_equal(ml[c], ml1) and ll[c] == ll1, c


@pytest.mark.parametrize("streams", [1, 4])
@pytest.mark.parametrize("devices", [None, [0], [0, 0]])
def test_channels_equal_their_single_channel_decodes(H, five, devices, streams):
    ys, models, single = five
    H.set_option("fit_streams", streams)
    try:
        import torch
        before = torch.cuda.current_device()
        same_as_single(channels(H, ys, models, CS_CH, devices), single)
        assert torch.cuda.current_device() == before
    finally:
        H.set_option("fit_streams", 4)
        H.shutdown()


def test_python_fit_channels(H, five):
    ys, models, single = five
    tms = [H.HMMSpikeTemplateModel(sm, mu, sg) for sm, mu, sg in models]
    out = H.fit_channels(tms, ys, CS_CH, devices=[0, 0])
    for m, (ml1, ll1) in zip(out, single):
        assert np.array_equal(m.ml_seq, ml1) and m.ll == ll1
    same = H.fit_channels(tms[0], np.stack([ys[0], ys[0]]), CS_CH)  # one model for every row of a C x T array
    assert all(np.array_equal(m.ml_seq, single[0][0]) and m.ll == single[0][1] for m in same)
    H.shutdown()


def test_a_channel_without_silent_sample_does_not_stop_the_others(O, H, five):
    """Channel 2 becomes the -3 fixture of case 4, which needs chunksize 40 for the whole call.  At that chunk size
    the oracle also ends the 900-state model of channel 4 at fit.jl:26, so for this run channel 4 takes the
    two-template overlap model channel 2 gave up (the oracle returns 0 on it, asserted below): only channel 2 fails,
    the other four complete, and every channel holds what its own single-channel call and the oracle hold."""
    ys, models, _ = five
    ys, models = list(ys), list(models)
    ys[4], models[4] = ys[2], models[2]
    ys[2], sm, temps = make(H, 2, 30, [0.03, 0.03], 6000, 33, False)
    models[2] = (sm, temps, 0.3)
    want = [0, 0, -3, 0, 0]
    single = []
    for c, (y, (sm, mu, sg)) in enumerate(zip(ys, models)):
        single.append(agree(H, O, y, sm, mu, sg, 40, expect_rc=want[c]))
    rc, ml, ll, status, msg = channels(H, ys, models, 40, [0, 0])
    E = H._lib.ENOSILENT
    assert status == [0, 0, E, 0, 0] and rc == E
    assert msg.startswith("channel 2:") and "fit.jl:26" in msg
    for c, (_, ml1, ll1, _) in enumerate(single):
        assert np.array_equal(ml[c], ml1) and ll[c] == ll1, c
    with pytest.raises(H.HmmsortError, match="channel 2"):
        H.fit_channels([H.HMMSpikeTemplateModel(*m) for m in models], ys, 40)
    H.shutdown()


def test_fit_streams_range(H):
    from hmmsort_amd._lib import lib
    assert H.get_option("fit_streams") == 4
    for bad in (0, 17, -1):
        assert lib().hmmsort_set_option(b"fit_streams", bad) == H._lib.EINVAL
    assert H.get_option("fit_streams") == 4
    for ok in (1, 16, 4):
        H.set_option("fit_streams", ok)
        assert H.get_option("fit_streams") == ok


def test_shutdown_returns_the_memory_and_the_cache_stays_bounded(H, five):
    import torch
    ys, models, single = five
    H.shutdown()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    same_as_single(channels(H, ys, models, CS_CH, [0, 0]), single)
    same_as_single(channels(H, ys, models, CS_CH, None), single)   # now on plans the first call left
    H.shutdown()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= free0 - (8 << 20)       # the margin of test_gpu_host_cache.py


def test_four_host_threads_fit_channels_at_once(H, five):
    ys, models, single = five
    order = [[0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 0, 4, 1, 3], [1, 1, 3, 3, 0]]
    out, errs = [None] * 4, []

    def work(n):
        try:
            for _ in range(2):
                out[n] = channels(H, [ys[c] for c in order[n]], [models[c] for c in order[n]], CS_CH,
                                  [0, 0] if n % 2 else None)
        except Exception as e:                                    # noqa: BLE001 - reported below
            errs.append(e)

    th = [threading.Thread(target=work, args=(n,)) for n in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    H.shutdown()
    assert not errs, errs
    for n in range(4):
        same_as_single(out[n], [single[c] for c in order[n]])
