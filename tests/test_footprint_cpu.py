"""The numpy model of the footprints (tests/footprint_model.py) against the definition, the proof that the order it
states can be told from other orders, the host functions that turn footprints into decisions on hand-built arrays, and
the library's exports.  No GPU."""
import ctypes

import numpy as np
import pytest

import footprint_model as FM

CASES = FM.cases()


def hand(H, mean, n_used=None, channels=None, pre=0):
    """a Footprints whose mean is `mean` ([U][M][W]): sum = mean * n_used"""
    mean = np.asarray(mean, dtype=np.float64)
    U, M, _ = mean.shape
    nu = np.full(U, 4, dtype=np.int64) if n_used is None else np.asarray(n_used, dtype=np.int64)
    ch = np.tile(np.arange(M, dtype=np.int32), (U, 1)) if channels is None else np.asarray(channels, dtype=np.int32)
    s = mean * nu[:, None, None]
    return H.Footprints(s, s * mean, nu, nu.copy(), ch, pre)


# ---- the model against the definition ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_model_against_brute(name):
    """n and nused exactly; sum and sumsq to 1e-12 relative.  The scale of `relative` is the sum of the addends'
    magnitudes: a serial fold of n terms is off by at most (n - 1) 2^-53 of that sum (5.7e-14 for 513 spikes), while
    no order of adding bounds the error against the magnitude of a sum that cancels.  For sumsq, whose addends are all
    positive, the two scales are one."""
    y, lists, pre, W, chan = CASES[name]
    s, q, nused, n = FM.model(y, lists, pre, W, chan)
    bs, bq, bnused, bn, sa = FM.brute(y, lists, pre, W, chan)
    assert np.array_equal(n, bn) and np.array_equal(nused, bnused)
    assert n.tolist() == [len(t) for t in lists]
    assert np.all(np.abs(s - bs) <= 1e-12 * sa), np.max(np.abs(s - bs) / np.maximum(sa, 1e-300))
    assert np.all(np.abs(q - bq) <= 1e-12 * bq), np.max(np.abs(q - bq) / np.maximum(bq, 1e-300))
    table = FM.table_of(len(lists), y.shape[0], chan)
    assert not s[table < 0].any() and not q[table < 0].any() and not s[nused == 0].any()


def test_model_edges_written_out():
    y, lists, pre, W, _ = CASES["degenerate_edges"]
    s, q, nused, n = FM.model(y, lists, pre, W)
    assert nused.tolist() == [0, 1, 2] and n.tolist() == [0, 1, 5]
    assert np.array_equal(s[1], y[:, 13:23]) and np.array_equal(q[1], y[:, 13:23] * y[:, 13:23])
    assert np.array_equal(s[2], y[:, 0:10] + y[:, 40:50])
    s, q, nused, n = FM.model(*CASES["degenerate_w51"][:4])
    assert not nused.any() and not s.any() and not q.any() and n.tolist() == [0, 1, 5]


# ---- the order test has teeth -------------------------------------------------------------------------------------
def test_the_order_can_be_told_from_other_orders():
    """One unit of 513 spikes on the wide-range block; the first entry (first tile) and the last entry (last tile) are
    unused.  Both a pairwise sum of the snippets and the fold that cuts its tiles by used index differ from the model in
    at least one entry of sum: an == against the model on the GPU tells a wrong order from the right one."""
    y, lists, pre, W, _ = FM.seam_case(60)
    t = lists[3]
    assert len(t) == 513 and not FM.used(t[0], pre, W, y.shape[1]) and not FM.used(t[-1], pre, W, y.shape[1])
    s, q, nused, _ = FM.model(y, [t], pre, W)
    assert nused[0] == 511
    starts = np.array([int(v) - 1 - pre for v in t[1:-1]])
    snips = np.stack([y[:, a:a + W] for a in starts])              # [511][C][W]
    assert np.any(np.sum(snips, axis=0) != s[0]), "np.sum gives the model's bits: the data cannot tell orders apart"
    s2, q2, nused2, _ = FM.model(y, [t], pre, W, cut_by_used=True)
    assert nused2[0] == 511
    assert np.any(s2 != s), "cutting tiles by used index gives the model's bits"
    assert np.any(q2 != q)
    assert np.allclose(s2, s, rtol=0, atol=1e-9 * np.abs(snips).sum(axis=0).max())   # the same sums all the same


# ---- derived quantities on hand-built footprints ------------------------------------------------------------------
def test_mean_std_ptp_and_peak_channel(H):
    mean = np.zeros((4, 3, 5))
    mean[0, 1] = [0, -2, 1, 0, 0]            # ptp 3 on slot 1
    mean[0, 2] = [0, -1, 0.5, 0, 0]
    mean[1, 0] = [0, -1, 1, 0, 0]            # a tie between slots 0 and 2: the lower slot
    mean[1, 2] = [1, 0, 0, 0, -1]
    mean[3, 2] = [0, 5, 0, 0, 0]             # unit 3 lists channels (7, -1, 4): slot 2 is channel 4
    mean[3, 1] = [0, 9, 0, 0, 0]             # an empty slot is never the peak, whatever it holds
    ch = [[0, 1, 2], [0, 1, 2], [0, 1, 2], [7, -1, 4]]
    fp = hand(H, mean, n_used=[4, 2, 0, 3], channels=ch)
    assert np.array_equal(fp.mean[[0, 1, 3]], mean[[0, 1, 3]]) and not fp.mean[2].any()
    assert fp.ptp[0].tolist() == [0, 3, 1.5] and fp.ptp[1].tolist() == [2, 0, 2]
    assert fp.peak_channel.tolist() == [1, 0, -1, 4]
    # spread: two spikes 1 and 3 on one entry -> sum 4, sumsq 10, mean 2, sample variance 2
    one = H.Footprints(np.full((1, 1, 1), 4.0), np.full((1, 1, 1), 10.0), np.array([2]), np.array([2]),
                       np.zeros((1, 1), dtype=np.int32), 0)
    assert one.mean[0, 0, 0] == 2.0 and abs(one.std[0, 0, 0] - np.sqrt(2.0)) < 1e-15
    single = H.Footprints(np.full((1, 1, 1), 4.0), np.full((1, 1, 1), 16.0), np.array([1]), np.array([1]),
                          np.zeros((1, 1), dtype=np.int32), 0)
    assert single.std[0, 0, 0] == 0.0


def test_unit_locations(H):
    mean = np.zeros((3, 3, 4))
    mean[0, 0, 1], mean[0, 1, 1], mean[0, 2, 1] = 2.0, 1.0, 0.0       # ptp^2 = 4, 1, 0 at x = 0, 10, 20
    mean[1, 1, 2], mean[1, 2, 2] = 3.0, 3.0                           # equal weights at 10 and 20
    fp = hand(H, mean, n_used=[5, 5, 0])
    x = H.unit_locations(fp, [0.0, 10.0, 20.0])
    assert x.shape == (3,) and x[0] == (4 * 0 + 1 * 10) / 5 == 2.0 and x[1] == 15.0 and np.isnan(x[2])
    xy = H.unit_locations(fp, [[0.0, 1.0], [10.0, 1.0], [20.0, 4.0]])
    assert xy.shape == (3, 2) and xy[0].tolist() == [2.0, 1.0] and xy[1].tolist() == [15.0, 2.5]
    # a table: unit 0 lists channels 2 and 0 only
    sub = H.Footprints(fp.sum[:1, :2], fp.sumsq[:1, :2], fp.n_used[:1], fp.n[:1], np.array([[2, 0]], dtype=np.int32), 0)
    assert H.unit_locations(sub, [0.0, 10.0, 20.0])[0] == (4 * 20 + 1 * 0) / 5


def test_footprint_similarity(H):
    W = 48
    k = np.arange(W, dtype=np.float64)
    wave = np.exp(-0.5 * ((k - 20.0) / 2.0) ** 2) - 0.5 * np.exp(-0.5 * ((k - 26.0) / 3.0) ** 2)
    wave[np.abs(wave) < 1e-6] = 0.0           # zero well inside the window's ends, so a shift loses nothing
    assert not wave[:4].any() and not wave[-4:].any()
    mean = np.zeros((3, 2, W))
    mean[0, 0], mean[0, 1] = wave, 0.4 * wave
    mean[1, 0], mean[1, 1] = 0.7 * np.roll(wave, 3), 0.28 * np.roll(wave, 3)   # unit 0, 3 samples later and smaller
    mean[2, 0], mean[2, 1] = 0.4 * wave, -wave                                 # another shape across the channels
    fp = hand(H, mean)
    sim, lag = H.footprint_similarity(fp, max_lag=10)
    assert sim.shape == (3, 3) and np.array_equal(np.diag(sim), np.ones(3))
    assert lag[0, 1] == 3 and lag[1, 0] == -3 and abs(sim[0, 1] - 1.0) < 1e-12 and sim[1, 0] == sim[0, 1]
    assert sim[0, 2] < 0.5 and np.array_equal(sim, sim.T) and np.array_equal(lag, -lag.T)
    sim2, lag2 = H.footprint_similarity(fp, max_lag=2)           # the shift is out of reach: the nearest lag, below 1
    assert lag2[0, 1] == 2 and sim2[0, 1] < 1.0 - 1e-3
    # disjoint channel sets: 0; a shared channel in different slots is found
    apart = hand(H, mean[:2], channels=[[0, 1], [2, 3]])
    s3, l3 = H.footprint_similarity(apart)
    assert s3[0, 1] == 0.0 and s3[1, 0] == 0.0 and l3[0, 1] == 0
    cross = hand(H, np.stack([mean[0], mean[0][::-1]]), channels=[[0, 1], [1, 0]])
    s4, l4 = H.footprint_similarity(cross)
    assert abs(s4[0, 1] - 1.0) < 1e-12 and l4[0, 1] == 0
    flat = hand(H, np.stack([mean[0], np.zeros((2, W))]))        # a zero norm
    assert H.footprint_similarity(flat)[0][0, 1] == 0.0


def test_resolve_duplicates(H):
    W = 30
    k = np.arange(W, dtype=np.float64)
    wave = np.exp(-0.5 * ((k - 12.0) / 2.0) ** 2)
    other = np.sin(k)                                            # nothing like `wave`
    z = np.zeros((4, 4, 2), dtype=np.int64)

    def cg_of(coinc, n):
        return H.Correlograms(z[:len(n), :len(n)], np.array([-1, 0]), np.zeros(len(n), dtype=np.int64),
                              np.asarray(coinc, dtype=np.int64), np.asarray(n, dtype=np.int64))

    # a chain a-b, b-c: b is the smallest and goes first, so the pair b-c is skipped and c stays
    mean = np.zeros((3, 1, W))
    mean[0, 0], mean[1, 0], mean[2, 0] = 3.0 * wave, 1.0 * wave, 2.0 * wave
    fp = hand(H, mean)
    cg = cg_of([[0, 9, 0], [9, 0, 9], [0, 9, 0]], [10, 10, 10])
    keep, pairs = H.resolve_duplicates(cg, fp)
    assert keep.tolist() == [True, False, True] and len(pairs) == 1
    assert pairs[0][:3] == (0, 1, 0.9) and abs(pairs[0][3] - 1.0) < 1e-12 and pairs[0][4] == 0
    # listed in one direction only is enough; the fraction reported is the larger one
    cg1 = cg_of([[0, 2, 0], [9, 0, 0], [0, 0, 0]], [10, 10, 10])
    keep, pairs = H.resolve_duplicates(cg1, fp)
    assert keep.tolist() == [True, False, True] and pairs[0][:3] == (0, 1, 0.9)
    # the tie rule: equal largest ptp, the higher index goes
    mean_t = np.zeros((3, 1, W))
    mean_t[0, 0], mean_t[1, 0], mean_t[2, 0] = wave, wave, other
    keep, pairs = H.resolve_duplicates(cg_of([[0, 8, 0], [8, 0, 0], [0, 0, 0]], [10, 10, 10]), hand(H, mean_t))
    assert keep.tolist() == [True, False, True] and pairs[0][:2] == (0, 1)
    # two neurons that fire together: coincident, but another shape -- both stay
    keep, pairs = H.resolve_duplicates(cg_of([[0, 0, 9], [0, 0, 0], [9, 0, 0]], [10, 10, 10]), hand(H, mean_t))
    assert keep.all() and pairs == []
    # ... until the similarity asked for is low enough (|cos| of unrelated shapes is small, not negative enough)
    sim = H.footprint_similarity(hand(H, mean_t))[0][0, 2]
    assert 0.0 <= sim < 0.8


# ---- exports --------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_footprint_calls(H):
    L = ctypes.CDLL(H._lib.LIB_PATH)
    for name in ("hmmsort_footprints", "hmmsort_footprints_device", "hmmsort_plan_footprints"):
        assert hasattr(L, name), "missing export: " + name
        assert name in H._lib.SIGNATURES
    assert ctypes.sizeof(H._lib.FpOpt) == 32 and ctypes.sizeof(H._lib.FpOut) == 32
