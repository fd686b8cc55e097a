"""The rules of hmmsort_unit_stability as tests/stability_model.py states them, on the CPU: each rule is
shown to differ from its plausible neighbour, so a model (or a device) that followed the neighbour would be found out;
and the host-side finishers on cases whose answer is known."""
from fractions import Fraction
from statistics import NormalDist

import numpy as np
import pytest

import stability_model as SM


@pytest.fixture(scope="module")
def heavy():
    """one unit, 8 time bins: heavy-tailed values with ties, signed zeros, infinities and NaNs"""
    rng = np.random.default_rng(5)
    n, T = 4000, 80_000
    t = np.sort(rng.choice(T, n, replace=False)).astype(np.int64) + 1
    v = np.round(rng.standard_t(2, n), 1)
    v[rng.random(n) < 0.1] = np.nan
    v[rng.random(n) < 0.03] = 0.0
    v[rng.random(n) < 0.03] = -0.0
    v[rng.random(n) < 0.005] = np.inf
    v[17], v[3000] = -np.inf, -np.inf
    return t, v, T, 10_000


def segments(t, v, bin):
    b = SM.bin_of(t, bin)
    return [v[(b == k) & ~np.isnan(v)] for k in range(int(b.max()) + 1)]


def test_keys_order_and_round_trip():
    v = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, np.inf])
    k = SM.keys(v)
    assert (np.diff(k.astype(object)) > 0).all()
    assert SM.unkeys(k).tobytes() == v.tobytes()


def test_quantile_is_an_input_not_an_interpolation(heavy):
    t, v, T, bin = heavy
    r = SM.unit_stability([t], [v], T, bin, (1, 2, 3), 4)
    for b, seg in enumerate(segments(t, v, bin)):
        assert r.valid[0, b] == len(seg) and len(seg) > 300
        for k in range(3):
            assert np.any(seg.view(np.uint64) == r.quant[0, b, k:k + 1].view(np.uint64))   # bit for bit an input
    six = np.array([32.0, 1.0, 16.0, 2.0, 8.0, 4.0])     # (m - 1) / 4 = 1.25: np.quantile interpolates to 2.5
    assert SM.order_stats(six, (1,), 4)[0] == 2.0 and np.quantile(six, 0.25) == 2.5
    # floor((m - 1) q), not ceil: four values, the median is the second, and the upper order statistic the third
    assert SM.order_stats(np.array([4.0, 1.0, 3.0, 2.0]), (1,), 2)[0] == 2.0
    assert SM.order_stats(np.array([4.0, 1.0, 3.0, 2.0]), (0, 1, 2, 3), 3).tolist() == [1.0, 2.0, 3.0, 4.0]
    assert SM.rank(1, 2, 4) == 1 and SM.rank(1, 3, 3) == 0 and SM.rank(2, 3, 3) == 1 and SM.rank(1 << 20, 1 << 20, 7) == 6


def test_signed_zeros_are_told_apart_unlike_np_sort():
    seg = np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0])
    q = SM.order_stats(seg, (0, 2, 3, 5), 5)
    assert np.signbit(q).tolist() == [True, True, False, False]
    assert not np.signbit(np.sort(seg)[0])                # np.sort leaves +0.0 in front: the zeros compare equal
    assert np.isnan(SM.order_stats(np.zeros(0), (1,), 2)).all()
    both = SM.order_stats(np.array([np.inf, -np.inf, 1.0]), (0, 1, 2), 2)
    assert both.tolist() == [-np.inf, 1.0, np.inf]


def test_sums_are_tiled_and_the_square_is_not_fused(heavy):
    seg = np.array([1e16] + [1.0] * 511)
    s, q = SM.tiled_sums(seg)
    assert s == 1e16 + 256.0 and SM.fold(seg) == 1e16     # the second tile's ones survive only in the tiled order
    assert q == 1e32 + 256.0
    rng = np.random.default_rng(9)
    tile = rng.standard_normal(256)
    fused = 0.0
    for x in tile:                                        # fma(x, x, acc): one rounding of the exact value
        fused = float(Fraction(fused) + Fraction(float(x)) ** 2)
    assert SM.tiled_sums(tile)[1] != fused
    t, v, T, bin = heavy
    r = SM.unit_stability([t], [v], T, bin, (), 1)
    for b, seg in enumerate(segments(t, v, bin)):
        assert (r.sum[0, b], r.sumsq[0, b]) == SM.tiled_sums(seg) or np.isnan(r.sum[0, b])
    assert np.isnan(r.usum[0]) and r.usumsq[0] == np.inf  # +Inf and -Inf meet in the unit sum
    assert r.usumsq[0] == SM.fold(r.sumsq[0])
    assert SM.tiled_sums(np.zeros(0)) == (0.0, 0.0) and not np.signbit(SM.tiled_sums(np.array([-0.0]))[0])


def test_bins_are_cut_at_t_minus_one():
    t = np.array([1, 10, 11, 20, 21, 25], dtype=np.int64)
    r = SM.unit_stability([t], None, 25, 10)
    assert r.count.tolist() == [[2, 2, 2]] and r.valid is None
    assert np.bincount(t // 10, minlength=3).tolist() == [1, 2, 3]     # what t / bin would count
    assert SM.time_bins(25, 10) == 3 and SM.time_bins(30, 10) == 3 and SM.time_bins(1, 7) == 1
    assert SM.bin_samples(r).tolist() == [10, 10, 5]
    assert SM.firing_rate(r, 10.0).tolist() == [[2.0, 2.0, 4.0]]


def test_histogram_edges():
    v = np.array([-1.0, -0.0, 0.0, 0.25, 0.5, 0.999, 1.0, 2.0, np.inf, -np.inf])
    h, under, over = SM.histogram(v, 4, 0.0, 4.0)
    assert h.tolist() == [2, 1, 1, 1] and under == 2 and over == 3   # -0.0 lands in bin 0, 1.0 is at HB


@pytest.mark.parametrize("B", [1, 2, 7, 10])
def test_presence_ratio_of_a_unit_silent_in_the_second_half(B):
    bin = 50
    first = -(-B // 2)                                    # ceil(B / 2) bins with spikes
    t = np.concatenate([b * bin + np.array([1, 7, 50]) for b in range(first)]).astype(np.int64)
    r = SM.unit_stability([t, t[:0]], None, B * bin, bin)
    assert SM.presence_ratio(r).tolist() == [first / B, 0.0]
    assert SM.presence_ratio(r, min_count=4).tolist() == [0.0, 0.0]
    short = SM.unit_stability([t], None, B * bin + 3, bin)         # one more, short bin: left out
    assert short.count.shape == (1, B + 1) and SM.presence_ratio(short).tolist() == [first / B]
    only = SM.unit_stability([np.array([2], dtype=np.int64)], None, 3, bin)
    assert SM.presence_ratio(only).tolist() == [1.0]               # the short bin is the only one


def gaussian(seed, truncated):
    rng = np.random.default_rng(seed)
    v = 1.0 + 0.15 * rng.standard_normal(20_000)
    t = np.arange(1, len(v) + 1, dtype=np.int64)
    if truncated:
        keep = v >= 1.0 + 0.15 * NormalDist().inv_cdf(0.2)
        t, v = t[keep], v[keep]
    return SM.unit_stability([t], [v], 20_000, 1000, (1,), 2, (512, 0.0, 128.0))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_amplitude_cutoff_of_a_truncated_gaussian(seed):
    """20 000 amplitudes N(1, 0.15^2), histogram of 512 bins over 0..4, whole and with the lowest 20 % removed.  A
    symmetric density that lost its lowest fifth has 0.2 / 0.8 = 0.25 of what is left above the mirror point.
    Measured with this model: seed 1: 0.00015 whole, 0.26640 truncated; seed 2: 0.00005, 0.23513; seed 3: 0.00015,
    0.27418.  The truncated figure moves by +-0.02 over the seeds, because the peak of a sampled histogram sits a few
    bins off the mode; the margin is three times that spread about the expected value, 0.25 +- 0.06.  The whole
    sample's figure is the two-sided tail beyond its own smallest value, a few spikes in 20 000: below 0.002."""
    whole, cut = SM.amplitude_cutoff(gaussian(seed, False))[0], SM.amplitude_cutoff(gaussian(seed, True))[0]
    print("amplitude cutoff: whole %.5f, truncated %.5f" % (whole, cut))
    assert whole < 0.002 and abs(cut - 0.25) < 0.06 and cut > 50 * whole


def test_amplitude_drift_and_empty_units():
    t = np.arange(1, 301, dtype=np.int64)
    v = np.concatenate([np.full(100, 2.0), np.full(100, 1.5), np.full(100, 1.0)])
    r = SM.unit_stability([t, t[:0], t[:5]], [v, v[:0], v[:5]], 300, 100, (1, 2, 3), 4, (8, 0.0, 2.0))
    d = SM.amplitude_drift(r)
    assert d[0] == (2.0 - 1.0) / 1.5 and np.isnan(d[1]) and np.isnan(d[2])    # five values are below min_valid
    assert SM.amplitude_drift(r, min_valid=5)[2] == 0.0
    assert np.isnan(SM.amplitude_cutoff(r)[1]) and r.uvalid.tolist() == [300, 0, 5]
    with pytest.raises(ValueError):
        SM.amplitude_drift(SM.unit_stability([t], [v], 300, 100, (1,), 4))


def test_api_finishers_state_the_same(H):
    r = gaussian(2, True)
    us = H.UnitStability(*[getattr(r, k) for k in ("n", "count", "valid", "quant", "sum", "sumsq", "uvalid", "uquant",
                                                   "umin", "umax", "usum", "usumsq", "hist", "under", "over")],
                         r.T, r.bin, r.q_num, r.q_den, r.hist_lo, r.hist_scale)
    assert np.array_equal(us.amplitude_cutoff(), SM.amplitude_cutoff(r))
    assert np.array_equal(us.amplitude_drift(), SM.amplitude_drift(r), equal_nan=True)
    assert np.array_equal(us.presence_ratio(3), SM.presence_ratio(r, 3))
    assert np.array_equal(us.firing_rate(30_000.0), SM.firing_rate(r, 30_000.0))
    assert H.quantile_fractions((0.25, 0.5, 0.75)) == ((1, 2, 3), 4)
    assert H.quantile_fractions((1 / 3, 0.9)) == ((10, 27), 30) and H.quantile_fractions(()) == ((), 1)
    num, den = H.quantile_fractions((1 / 4093, 1 / 4091, 1 / 4089))      # the common denominator passes 2^20
    assert den == 1 << 20 and num == (256, 256, 256)
