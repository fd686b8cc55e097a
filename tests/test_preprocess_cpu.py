"""The numpy model of the front end (preprocess_model.py) checked on its own, and api.design_fir against scipy.  The
device result is compared with this model bit for bit in test_gpu_preprocess.py; here the model itself is shown to
compute the filter and the references it claims to."""
import numpy as np
import pytest

import preprocess_model as PM

GROUP_SIZES = (1, 2, 3, 4, 5, 8, 33, 64)


def test_filter_against_an_extended_precision_sum(H):
    """the folded filter in float64 against np.convolve in longdouble over the mirrored signal: within the textbook
    bound (P + 2) 2^-53 sum|h| max|x| of a recursive sum of P + 1 rounded products of rounded pair sums"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("longdouble is no wider than float64 here")
    rng = np.random.default_rng(7)
    for P, T in ((1, 2), (7, 100), (256, 5000)):
        h = H.design_fir(30000.0, low=300.0, ntaps=2 * P + 1) if P > 1 else np.array([-0.25, 0.5, -0.25])
        x = rng.standard_normal((2, T)) * 3.0
        f = PM.fir(x, h[P:])
        full = np.concatenate([h[P:][::-1], h[P + 1:]]).astype(np.longdouble)   # the filter the half stands for
        idx = PM.mirror_index(T, P)
        worst = 0.0
        for c in range(2):
            ref = np.convolve(x[c, idx].astype(np.longdouble), full, mode="valid")
            assert ref.shape == (T,)
            worst = max(worst, float(np.abs(f[c].astype(np.longdouble) - ref).max()))
        bound = (P + 2) * 2.0 ** -53 * float(np.abs(full).sum()) * float(np.abs(x).max())
        print("P = %d: max error %.3g, bound %.3g" % (P, worst, bound))
        assert worst <= bound


def test_design_against_scipy(H):
    signal = pytest.importorskip("scipy.signal")
    fs = 30000.0
    for ntaps in (129, 257, 513):
        for low, high in ((300.0, None), (None, 6000.0), (300.0, 6000.0)):
            h = H.design_fir(fs, low, high, ntaps)
            cut = [f for f in (low, high) if f is not None]
            ref = signal.firwin(ntaps, cut, window="hamming", pass_zero=(low is None), fs=fs)
            assert h.shape == (ntaps,)
            assert np.abs(h - ref).max() <= 1e-15, (ntaps, low, high)
            assert np.abs(h - h[::-1]).max() <= 1e-16


def test_design_refuses_what_it_cannot_build(H):
    for bad in (dict(), dict(low=0.0), dict(high=15000.0), dict(low=500.0, high=300.0), dict(low=300.0, ntaps=256)):
        with pytest.raises(ValueError):
            H.design_fir(30000.0, **bad)


@pytest.mark.parametrize("mode", ("median", "mean"))
def test_references(mode):
    """median: x - np.median(x, axis=0) exactly, on small integers (many ties) and on normal input; mean: the
    sequential sum in channel order divided by G"""
    rng = np.random.default_rng(11)
    T = 257
    for C in GROUP_SIZES:
        for x in (rng.integers(-3, 4, size=(C, T)).astype(np.float64), rng.standard_normal((C, T))):
            out = PM.reference(x, mode)
            if mode == "median":
                assert np.array_equal(out, x - np.median(x, axis=0)), C
            else:
                s = np.zeros(T)
                for c in range(C):
                    s = s + x[c]
                assert np.array_equal(out, x - s / C), C
                assert np.abs(out - (x - x.mean(axis=0))).max() <= 64 * C * np.finfo(float).eps * np.abs(x).max()
            if C == 1:
                assert np.all(out == 0)


def test_groups_and_excluded_channels():
    rng = np.random.default_rng(12)
    x = rng.standard_normal((7, 50))
    group = [0, 1, 0, -1, 1, 0, 5]
    out = PM.reference(x, "median", group)
    assert np.array_equal(out[[0, 2, 5]], x[[0, 2, 5]] - np.median(x[[0, 2, 5]], axis=0))
    assert np.array_equal(out[[1, 4]], x[[1, 4]] - np.median(x[[1, 4]], axis=0))
    assert np.array_equal(out[3], x[3]) and np.all(out[6] == 0)


def test_integer_common_term_leaves_the_median_reference_unchanged():
    rng = np.random.default_rng(13)
    for C in GROUP_SIZES:
        x = rng.integers(-500, 500, size=(C, 300))
        s = rng.integers(-20000, 20000, size=300)
        assert np.array_equal(PM.preprocess(x + s, mode="median"), PM.preprocess(x, mode="median"))


def test_dyadic_taps_on_a_constant_signal_give_zero():
    half = np.array([0.5, -0.125, -0.125])           # the full filter sums to 0
    for T in (3, 4, 50):
        x = np.full((2, T), 7, dtype=np.int16)
        assert np.all(PM.preprocess(x, half) == 0.0)


def test_mirror_and_identity():
    assert PM.mirror_index(5, 3).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    x = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert np.array_equal(PM.preprocess(x), x.astype(np.float64))
    assert np.array_equal(PM.preprocess(x, keep=[2, 0]), x[[2, 0]].astype(np.float64))
