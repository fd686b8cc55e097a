"""The numpy model of the whitening stages (whiten_model.py) and the host finish (api.noise_covariance,
api.whitening_matrix, api.Whitening).  No GPU.

The device is compared with the model by ==, so the model's rules have to be distinguishable: on heavy-tailed data
every other plausible way of forming the sums (numpy's pairwise sum, a matrix product, tiles cut by quiet index, no
tiles, a fused multiply-add) and the mix (a matrix product, the slots in another order) gives other bits, shown here."""
import math
from fractions import Fraction

import numpy as np
import pytest

import whiten_model as WM


def _case(seed, C=5, T=1300):
    rng = np.random.default_rng(seed)
    Y = WM.heavy_tailed(rng, C, T)
    quiet = WM.quiet_mask(Y, np.full(C, 300.0), 1)
    return Y, quiet


@pytest.fixture(scope="module", params=(5, 6, 7))
def case(request):
    Y, quiet = _case(request.param)
    return Y, quiet, WM.sums(Y, quiet)


def test_about_four_in_ten_samples_are_quiet(case):
    Y, quiet, _ = case
    assert 0.25 < quiet.mean() < 0.55


def test_sums_differ_from_numpy_reductions(case):
    Y, quiet, (s1, s2) = case
    Yq = Y[:, quiet]
    assert np.any(s1 != Yq.sum(1))
    assert np.any(s2 != Yq @ Yq.T)


def test_sums_differ_from_other_tilings(case):
    Y, quiet, (s1, s2) = case
    b1, b2 = WM.sums(Y, quiet, by_quiet_index=True)
    assert np.any(s1 != b1) and np.any(s2 != b2)
    u1, u2 = WM.sums(Y, quiet, tile=Y.shape[1])
    assert np.any(s1 != u1) and np.any(s2 != u2)


def test_sums_differ_from_a_fused_fold(case):
    """the same fold with p + y_i y_j rounded once (what a fused multiply-add computes), in exact rationals.  About
    half the entries differ; all of j >= i are formed (a second of work), since any one 2 x 2 corner agrees by chance
    for about one seed in sixteen (the first corner does for seed 6)"""
    Y, quiet, (_, s2) = case
    nC = Y.shape[0]
    fused = np.array(s2)
    for i in range(nC):
        for j in range(i, nC):
            s = 0.0
            for t0 in range(0, Y.shape[1], WM.TILE):
                p = 0.0
                for t in np.nonzero(quiet[t0:t0 + WM.TILE])[0] + t0:
                    p = float(Fraction(p) + Fraction(float(Y[i, t])) * Fraction(float(Y[j, t])))
                s = s + p
            fused[i, j] = s
    assert np.any(fused != s2)


def test_s2_is_exactly_symmetric(case):
    _, _, (_, s2) = case
    assert np.array_equal(s2, s2.T)


def test_sums_are_within_the_bound_of_a_serial_sum(case):
    """a sum of n addends in any order errs by at most (n - 1) u sum|a| to first order, each product by u |a|"""
    Y, quiet, (s1, s2) = case
    Yq = Y[:, quiet]
    n = Yq.shape[1]
    u = 2.0 ** -53
    for i in range(Y.shape[0]):
        assert abs(s1[i] - math.fsum(Yq[i])) <= (n + 2) * u * math.fsum(np.abs(Yq[i]))
        for j in range(Y.shape[0]):
            prod = [Fraction(float(a)) * Fraction(float(b)) for a, b in zip(Yq[i], Yq[j])]
            exact, mass = sum(prod), sum(abs(p) for p in prod)
            assert abs(Fraction(float(s2[i, j])) - exact) <= Fraction((n + 2) * u) * mass


def test_mix_differs_from_a_matrix_product_and_from_reversed_slots():
    rng = np.random.default_rng(5)
    Y = WM.heavy_tailed(rng, 5, 1300)
    W = rng.standard_normal((5, 5))
    nbr = np.tile(np.arange(5), (5, 1))
    out = WM.mix(Y, nbr, W)
    assert np.any(out != W @ Y)
    assert np.any(out != WM.mix(Y, nbr[:, ::-1], W[:, ::-1]))
    assert np.allclose(out, W @ Y, rtol=1e-9, atol=1e-9 * np.abs(Y).max())


def test_mix_skips_empty_slots_and_adds_repeats():
    Y = np.arange(12.0).reshape(3, 4)
    nbr = np.array([[2, -1, 2], [-1, -1, -1], [0, 1, -1]])
    w = np.array([[1.0, 7.0, 0.5], [3.0, 3.0, 3.0], [2.0, -1.0, 9.0]])
    out = WM.mix(Y, nbr, w)
    assert np.array_equal(out, np.stack([1.5 * Y[2], np.zeros(4), 2.0 * Y[0] - Y[1]]))


def test_quiet_mask_against_the_definition():
    rng = np.random.default_rng(8)
    Y = rng.standard_normal((3, 700))
    Y[1, 350], Y[2, 699], Y[0, 0] = np.nan, np.inf, -9.0
    thr = np.array([2.5, 2.0, 3.0])
    loud = np.array([any(not abs(Y[c, t]) <= thr[c] for c in range(3)) for t in range(700)])
    assert loud[350] and loud[699] and loud[0]
    for guard in (0, 1, 3, 300, 65536):
        want = np.array([not loud[max(0, t - guard):t + guard + 1].any() for t in range(700)])
        assert np.array_equal(WM.quiet_mask(Y, thr, guard), want), guard


def test_noise_scale_is_the_median_rule():
    rng = np.random.default_rng(9)
    for T in (1, 3, 255, 1001):
        Y = rng.standard_normal((4, T))
        assert np.array_equal(WM.noise_scale(Y), np.median(np.abs(Y), axis=1) / WM.MAD_TO_SIGMA)
    Y = np.array([[3.0, -1.0, 2.0, -4.0]])                 # even T: the lower of the two middle values
    assert WM.noise_scale(Y)[0] == 2.0 / WM.MAD_TO_SIGMA


# ---- host finish -------------------------------------------------------------------------------------------------
def _cov(rng, n):
    A = rng.standard_normal((n, n))
    return A @ A.T + n * np.eye(n)


def test_noise_covariance_order_and_refusal(H):
    rng = np.random.default_rng(10)
    Y = rng.standard_normal((4, 500))
    s1, s2 = Y.sum(1), Y @ Y.T
    m = s1 / 500.0
    assert np.array_equal(H.noise_covariance(500, s1, s2), s2 / 500.0 - np.outer(m, m))
    assert np.allclose(H.noise_covariance(500, s1, s2), np.cov(Y, bias=True))
    for n in (0, 1):
        with pytest.raises(ValueError):
            H.noise_covariance(n, s1, s2)


def test_whitening_matrix_whitens(H):
    rng = np.random.default_rng(11)
    cov = _cov(rng, 8)
    nbr, W = H.whitening_matrix(cov, eps_rel=0)
    assert nbr.dtype == np.int32 and np.array_equal(nbr, np.tile(np.arange(8), (8, 1)))
    assert np.abs(W @ cov @ W.T - np.eye(8)).max() < 1e-9
    assert np.abs(W - W.T).max() < 1e-12


def test_whitening_matrix_is_finite_for_a_singular_covariance(H):
    rng = np.random.default_rng(12)
    Y = rng.standard_normal((6, 4000))
    Y = Y - Y.mean(0)                                      # mean-referenced: the channels sum to zero
    cov = np.cov(Y, bias=True)
    assert np.linalg.eigvalsh(cov)[0] < 1e-12
    _, W = H.whitening_matrix(cov)
    assert np.all(np.isfinite(W)) and np.abs(W).max() < 2e3


def test_local_whitening(H):
    rng = np.random.default_rng(13)
    cov = _cov(rng, 8)
    _, W = H.whitening_matrix(cov, eps_rel=0)
    nbr, w = H.whitening_matrix(cov, neighbors=np.tile(np.arange(8), (8, 1)), eps_rel=0)
    assert np.abs(w - W).max() < 1e-12
    perm = np.array([np.roll(np.arange(8), c) for c in range(8)])           # any order of the neighbours
    nbr, w = H.whitening_matrix(cov, neighbors=perm, eps_rel=0)
    wh = H.Whitening(None, None, 30, 0, None, None, cov, nbr, w)
    assert np.abs(wh.matrix - W).max() < 1e-12
    nbr, w = H.whitening_matrix(cov, neighbors=np.arange(8)[:, None], eps_rel=0)
    assert np.allclose(w[:, 0], 1.0 / np.sqrt(np.diag(cov)), rtol=1e-15)
    # three nearest by position, then index; -1 padding
    nbr, w = H.whitening_matrix(cov, neighbors=(np.arange(8.0)[:, None], 3), eps_rel=0)
    assert nbr[0].tolist() == [0, 1, 2] and nbr[4].tolist() == [4, 3, 5] and nbr[7].tolist() == [7, 6, 5]
    pad = np.concatenate([nbr, np.full((8, 2), -1, dtype=np.int32)], axis=1)
    nbr2, w2 = H.whitening_matrix(cov, neighbors=pad, eps_rel=0)
    assert np.array_equal(w2[:, :3], w) and np.all(w2[:, 3:] == 0)
    for c in range(8):
        ids = nbr[c]
        sub = cov[np.ix_(ids, ids)]
        lam, V = np.linalg.eigh(sub)
        assert np.allclose(w[c], ((V / np.sqrt(lam)) @ V.T)[0], rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        H.whitening_matrix(cov, neighbors=np.ones((8, 2), dtype=int))       # own channel missing


def test_whitening_scale_templates_and_matrix(H):
    nbr = np.array([[0, 1, -1], [1, 0, 2], [2, 2, -1]], dtype=np.int32)
    w = np.array([[2.0, 0.5, 9.0], [3.0, -1.0, 0.25], [1.0, 0.5, 9.0]])
    wh = H.Whitening(None, None, 30, 0, None, None, None, nbr, w)
    assert np.array_equal(wh.matrix, np.array([[2.0, 0.5, 0.0], [-1.0, 3.0, 0.25], [0.0, 0.0, 1.5]]))
    mu = np.arange(6.0).reshape(3, 2)
    assert np.array_equal(wh.scale_templates(mu, 1), 3.0 * mu)
    assert np.array_equal(wh.scale_templates(mu, 2), 1.5 * mu)


def test_driver_option_parsing(H):
    sd = H.sortdata
    opts, _ = sd._front_end_taps(dict(reference="median"))
    assert opts["whiten"] is None
    assert sd._front_end_taps(dict(whiten=True))[0]["whiten"] == {}
    assert sd._front_end_taps(dict(whiten=dict(guard=5)))[0]["whiten"] == {"guard": 5}
    with pytest.raises(TypeError):
        sd._front_end_taps(dict(whiten=dict(gard=5)))
