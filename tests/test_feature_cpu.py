"""The numpy model of the features and the isolation (tests/feature_model.py): the proof that the orders it states
can be told from other orders, its survival function against scipy, the science case in the model alone, the host
functions of the api on hand-built arrays, and every refusal of the library that comes before it needs a device.
No GPU."""
import ctypes as C

import numpy as np
import pytest
from scipy.stats import chi2

import feature_model as M
import footprint_model as FM


# ---- the order tests have teeth -------------------------------------------------------------------------------------
def test_the_projection_order_can_be_told_from_a_matrix_product():
    y, lists, pre, W = M.seam_case(60)
    rng = np.random.default_rng(1)
    basis, centre = M.random_basis(rng, 3, 3, W)
    f, use, n, nused = M.features(y, lists[:1], pre, W, None, basis, centre)
    snip, _, _, _ = M.features(y, lists[:1], pre, W, None, None, centre)
    blas = np.concatenate([snip[:, m * W:(m + 1) * W] @ basis[m].T for m in range(3)], axis=1)
    blas[use == 0] = 0.0
    assert f.shape == blas.shape == (255, 9)
    assert np.count_nonzero(f != blas) > 0, "a matrix product gives the model's bits: the data cannot tell orders apart"
    scale = np.concatenate([np.abs(snip[:, m * W:(m + 1) * W]) @ np.abs(basis[m]).T for m in range(3)], axis=1)
    assert np.all(np.abs(f - blas) <= 1e-13 * scale)                   # the same numbers all the same


def test_the_distance_order_can_be_told_from_einsum():
    feat, offs, used, mu, vinv = M.iso_case(24)
    rng = np.random.default_rng(2)
    feat = feat * 10.0 ** rng.uniform(-3.0, 3.0, feat.shape)
    d2 = M.d2_rows(feat, mu[0], vinv[0])
    d = feat - mu[0]
    ein = np.einsum("ra,ab,rb->r", d, vinv[0], d)
    ein = np.where(ein > 0, ein, 0.0)
    assert np.count_nonzero(d2 != ein) > 0, "einsum gives the model's bits"
    scale = np.einsum("ra,ab,rb->r", np.abs(d), np.abs(vinv[0]), np.abs(d))
    assert np.all(np.abs(d2 - ein) <= 1e-12 * scale)


def test_the_moment_tiles_are_cut_by_list_entry():
    y, lists, pre, W = M.seam_case(7)
    t = lists[3]
    f, use, n, nused = M.features(y, [t], pre, W, [0, 2])
    assert len(t) == 513 and use[0] == 0 and use[-1] == 0 and nused[0] == 511
    a1, a2 = M.moments(f, use, n, 1)
    c1, c2 = M.moments(f, use, n, 1, cut_by_used=True)
    assert np.any(a1 != c1) and np.any(a2 != c2), "cutting tiles by used index gives the model's bits"
    assert np.allclose(a2, c2, rtol=1e-9, atol=0) and np.array_equal(a2[0, 0], a2[0, 0].T)
    b1, b2 = M.moments(f, use, n, 2)                                   # mode 1: the diagonal blocks of mode 2
    assert b2.shape == (1, 2, 7, 7) and np.array_equal(b2[0, 1], a2[0, 0, 7:, 7:]) and np.array_equal(
        b1.reshape(-1), a1.reshape(-1))


def test_export_rows_are_the_blocks_samples():
    y, lists, pre, W = M.seam_case(7)
    f, use, n, nused = M.features(y, lists, pre, W, [2, 0, 2])
    r = 300                                                            # unit 1, entry 45
    a = int(lists[1][45]) - 1 - pre
    assert use[r] and np.array_equal(f[r], np.concatenate([y[2, a:a + W], y[0, a:a + W], y[2, a:a + W]]))
    assert not f[0].any() and not use[0] and n.tolist() == list(FM.SEAM_N)


# ---- the survival function ----------------------------------------------------------------------------------------
def test_survival_function_against_scipy():
    """within 1e-12 relative on the issue's grid; 2.4e-14 is what the form itself measures there"""
    x = np.array([0.0, 0.3, 5.0, 40.0, 300.0])
    worst = 0.0
    for F in (1, 2, 3, 4, 6, 9, 24, 64):
        got, want = M.chi2_sf(x, F), chi2.sf(x, F)
        rel = np.abs(got - want) / want
        worst = max(worst, rel.max())
        assert np.all(rel <= 1e-12), (F, rel)
    print("largest relative difference: %.3g" % worst)
    assert M.chi2_sf(np.array([1e6, np.inf]), 24).tolist() == [0.0, 0.0]


# ---- the science case, in the model alone ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def science():
    out = {}
    for Mch in (1, 2):
        y, lists, pre, W, chan, events = M.science_case(Mch)
        out[Mch] = M.pipeline(y, lists, pre, W, chan, 3)
        noise = _unassigned(events, lists, 3)
        out[Mch, "noise"] = M.pipeline(y, lists + [noise], pre, W, chan, 3)
        out[Mch, "same space"] = M.pipeline(y, lists, pre, W, chan, 3, space=out[Mch, "noise"][5])
        out["n_noise"] = len(noise)
    return out


def _unassigned(events, lists, tol):
    import hmmsort_amd as H
    return H.unassigned_events(events, lists, tol)


def test_science_second_channel_separates_the_similar_pair(science):
    iso1, lr1, closer1, _, nused1, _ = science[1]
    iso2, lr2, closer2, _, nused2, _ = science[2]
    assert nused1.tolist() == nused2.tolist() == [150, 150, 150]
    for u in (0, 1):
        assert iso2[u] > iso1[u] and lr2[u] < lr1[u], (u, iso1, iso2, lr1, lr2)
    assert np.argmax(iso1) == 2 and np.argmax(iso2) == 2               # the separated unit
    for cl in (closer1, closer2):
        assert cl[0, 1] + cl[1, 0] >= cl[0, 2] + cl[2, 0] and cl[0, 1] + cl[1, 0] >= cl[1, 2] + cl[2, 1]
    assert closer1[0, 1] + closer1[1, 0] > closer1[0, 2] + closer1[2, 0] + closer1[1, 2] + closer1[2, 1]
    assert closer1[0, 1] + closer1[1, 0] > closer2[0, 1] + closer2[1, 0]


def test_science_a_noise_cluster_never_raises_the_distance(science):
    """In one feature space (the basis pooled over all four lists) a unit's mean and covariance do not depend on the
    other lists, so more non-member rows can only lower the order statistic; the space itself moves a little when the
    fourth list joins the pool, which is why the comparison fixes it."""
    assert science["n_noise"] == 70
    for Mch in (1, 2):
        iso, isn = science[Mch, "same space"][0], science[Mch, "noise"][0]
        assert len(isn) == 4 and np.all(isn[:3] <= iso), (Mch, iso, isn)
    assert science[1, "noise"][0][0] < science[1, "same space"][0][0]  # and lowers it where the noise looks like A


# ---- host functions -----------------------------------------------------------------------------------------------
def test_pca_basis(H):
    rng = np.random.default_rng(5)
    W, n = 6, 400
    axes = np.linalg.qr(rng.standard_normal((W, W)))[0]
    x = (rng.standard_normal((n, W)) * np.array([9.0, 4.0, 2.0, 0.5, 0.2, 0.1])) @ axes.T + 3.0
    b1 = np.stack([x[:150].sum(0), x[150:].sum(0)])[:, None, :]
    b2 = np.stack([x[:150].T @ x[:150], x[150:].T @ x[150:]])[:, None, :, :]
    basis, centre = H.pca_basis(b1, b2, [150, 250], P=3)
    assert basis.shape == (1, 3, W) and centre.shape == (1, W) and np.allclose(centre[0], x.mean(0))
    assert np.allclose(basis[0] @ basis[0].T, np.eye(3), atol=1e-12)
    for p in range(3):
        assert abs(abs(basis[0, p] @ axes[:, p]) - 1.0) < 0.05
        assert basis[0, p][np.argmax(np.abs(basis[0, p]))] > 0
    mb, mc = M.pca(b1, b2, [150, 250], 3)
    assert np.array_equal(mb, basis) and np.array_equal(mc, centre)
    with pytest.raises(ValueError):
        H.pca_basis(b1, b2, [150, 250], P=7)


def test_unit_gaussians_marks_what_cannot_be_scored(H):
    rng = np.random.default_rng(6)
    F = 3
    x = rng.standard_normal((50, F)) + 2.0
    g1 = np.stack([x.sum(0), x[:3].sum(0), np.stack([x[:, 0], x[:, 0], x[:, 2]], 1).sum(0), np.zeros(F)])
    flat = np.stack([x[:, 0], x[:, 0], x[:, 2]], 1)
    g2 = np.stack([x.T @ x, x[:3].T @ x[:3], flat.T @ flat, np.zeros((F, F))])
    mu, vinv = H.unit_gaussians(g1, g2, [50, 3, 50, 0])
    assert np.allclose(mu[0], x.mean(0)) and np.allclose(vinv[0], np.linalg.inv(np.cov(x.T)), rtol=1e-9)
    for u in (1, 2, 3):                                                # n <= F; singular; empty
        assert np.isnan(vinv[u, 0, 0]) and not mu[u].any() and not vinv[u].ravel()[1:].any()


def test_unassigned_events(H):
    ev = H.unassigned_events([5, 50, 100, 103, 103], [[48, 49], [110]], tol=5)
    assert ev.tolist() == [5, 100, 103] and ev.dtype == np.int64
    assert H.unassigned_events([5, 50], [[], []], 3).tolist() == [5, 50]
    assert H.unassigned_events([], [[4]], 3).tolist() == []
    assert H.unassigned_events([10, 13, 14], [[10]], 3).tolist() == [14]


def test_isolation_result_l_ratio(H):
    lpair = np.array([[0.0, 2.0, 4.0], [1.0, 0.0, 1.0], [np.nan, 0.0, np.nan]])
    iso = H.api._isolation_result(np.zeros(3), np.zeros((3, 3), dtype=np.int64), lpair, np.array([3, 0, 5]), None,
                                  None, None)
    assert iso.l_ratio[0] == 2.0 and np.isnan(iso.l_ratio[1]) and np.isnan(iso.l_ratio[2])


# ---- exports and refusals -----------------------------------------------------------------------------------------
def test_the_library_exports_the_feature_calls(H):
    L = C.CDLL(H._lib.LIB_PATH)
    for name in ("hmmsort_snippet_features", "hmmsort_snippet_features_device", "hmmsort_plan_snippet_features",
                 "hmmsort_cluster_isolation", "hmmsort_cluster_isolation_device"):
        assert hasattr(L, name), "missing export: " + name
        assert name in H._lib.SIGNATURES
    assert C.sizeof(H._lib.FeatOpt) == 64 and C.sizeof(H._lib.FeatOut) == 72 and C.sizeof(H._lib.IsoOut) == 24


SENT_F, SENT_I = -7.25, -77


def feat_call(H, lists=None, C_=2, T=50, U=None, pre=3, W=10, M_=2, chan=None, P=1, basis=None, centre=None,
              moments=0, stype=None, n=True, opt=True, null_y=False, moment_arrays=True, counts=None):
    """hmmsort_snippet_features on sentinel-filled outputs -> rc; a refusal must not have written"""
    L = H._lib
    y = np.zeros((2, 50))
    lists = [np.array([5, 9]), np.array([7])] if lists is None else lists
    lists = [np.ascontiguousarray(t, dtype=np.int64) for t in lists]
    U = len(lists) if U is None else U
    ptrs = (C.c_void_p * max(len(lists), 1))(*[t.ctypes.data if len(t) else None for t in lists])
    cnt = np.array([len(t) for t in lists] + [0], dtype=np.int64) if counts is None else np.asarray(counts, np.int64)
    fl = [np.full(4096, SENT_F) for _ in range(5)]
    used = np.full(4096, 0x55, dtype=np.uint8)
    nu, nn = np.full(4096, SENT_I, dtype=np.int64), np.full(4096, SENT_I, dtype=np.int64)
    ch = None if chan is None else np.ascontiguousarray(chan, dtype=np.int32)
    bs = None if basis is None else np.ascontiguousarray(basis, dtype=np.float64)
    ce = None if centre is None else np.ascontiguousarray(centre, dtype=np.float64)
    o = L.FeatOpt(pre, W, M_, L.ptr(ch), P, L.ptr(bs), L.ptr(ce), moments)
    mp = [L.ptr(a) if moment_arrays else None for a in fl[1:]]
    out = L.FeatOut(L.ptr(fl[0]), L.ptr(used), 0, L.ptr(nn) if n else None, L.ptr(nu), *mp)
    rc = L.lib().hmmsort_snippet_features(None if null_y else L.ptr(y), L.SAMPLES_F64 if stype is None else stype, C_,
                                          T, U, ptrs, L.ptr(cnt), C.byref(o) if opt else None, C.byref(out))
    assert rc != 0                                                     # no device here, or a refusal
    assert all(np.all(a == SENT_F) for a in fl) and np.all(used == 0x55)
    assert np.all(nu == SENT_I) and np.all(nn == SENT_I)
    return rc


def test_feature_refusals(H):
    L = H._lib
    one = np.array([7])

    def refused(code, *words, **kw):
        rc = feat_call(H, **kw)
        assert rc == code and all(w in L.last_error() for w in words), (rc, L.last_error(), words)

    refused(L.EINVAL, "null", null_y=True)
    refused(L.EINVAL, "null", n=False)
    refused(L.EINVAL, "null", opt=False)
    refused(L.EINVAL, "C = 0", C_=0)
    refused(L.EINVAL, "T = 0", T=0)
    refused(L.EINVAL, "U = 0", U=0)
    refused(L.EINVAL, "U = 4097", lists=[one] * 4097)
    refused(L.EINVAL, "W = 0", W=0)
    refused(L.EINVAL, "W = 1025", W=1025)
    refused(L.EINVAL, "pre = -1", pre=-1)
    refused(L.EINVAL, "M = 0", M_=0, chan=[0])
    refused(L.EINVAL, "M = 1025", M_=1025, chan=np.zeros(1025))
    refused(L.EINVAL, "chan", "slot 1", "channel 2", chan=[0, 2])
    refused(L.EINVAL, "chan", "slot 0", "channel -1", chan=[-1, 0])      # no empty slots in the common row
    refused(L.EINVAL, "counts", "unit 1", "-3", counts=[2, -3, 0])
    refused(L.EINVAL, "unit 1", "position 0", "time 0", lists=[np.array([5, 9]), np.array([0, 7])])
    refused(L.EINVAL, "unit 1", "position 2", "ascending", lists=[np.array([5, 9]), np.array([4, 7, 7])])
    refused(L.EINVAL, "sample_type", stype=L.SAMPLES_F32)
    refused(L.EINVAL, "moments = 3", moments=3)
    refused(L.EINVAL, "moments = 1", "b1", moments=1, moment_arrays=False)
    refused(L.EINVAL, "moments = 2", "g1", moments=2, moment_arrays=False)
    refused(L.EINVAL, "P = 0", P=0)
    refused(L.EINVAL, "P = 0", P=0, basis=np.ones((2, 1, 10)))
    refused(L.EINVAL, "P = 11", "W = 10", P=11, basis=np.ones((2, 11, 10)))
    bad = np.ones((2, 3, 10))
    bad[1, 2, 4] = np.inf
    refused(L.EINVAL, "basis", "slot 1", "component 2", "sample 4", P=3, basis=bad)
    bad = np.zeros((2, 10))
    bad[0, 9] = np.nan
    refused(L.EINVAL, "centre", "slot 0", "sample 9", centre=bad)
    refused(L.EUNSUP, "moments = 1", "P = 129", W=129, T=200, moments=1)               # no basis: P := W
    refused(L.EUNSUP, "moments = 2", "F = 65", "13", "5", M_=13, chan=[0] * 13, P=5, W=5, basis=np.ones((13, 5, 5)),
            moments=2)
    refused(L.EUNSUP, str(4096 * 2 * 128 * 128), "4096 * 2 * 128 * 128", lists=[one] * 4096, W=128, T=200, moments=1)
    # (U * F * F cannot pass 2^26 while U <= 4096 and F <= 64 hold: 2^24 at the most)
    big = np.arange(1, 1 << 21 | 1, dtype=np.int64)                                         # 2^21 entries x F = 2048
    refused(L.EUNSUP, "n_total * F", str((1 << 21) + 1), "2048", lists=[big, np.array([1 << 30])], W=1024, T=2000)


def iso_call(H, n=3, F=2, U=2, offs=(0, 2, 3), mu=None, vinv=None, null=None, out=True):
    L = H._lib
    feat = np.zeros((max(n, 1), max(F, 1)))
    offs = np.asarray(offs, dtype=np.int64)
    mu = np.zeros((U, F)) if mu is None else np.asarray(mu, dtype=np.float64)
    vinv = np.tile(np.eye(max(F, 1)), (max(U, 1), 1, 1)) if vinv is None else np.asarray(vinv, dtype=np.float64)
    d2, cl, lp = np.full(4096, SENT_F), np.full(4096, SENT_I, dtype=np.int64), np.full(4096, SENT_F)
    o = L.IsoOut(L.ptr(d2), L.ptr(cl), L.ptr(lp))
    args = {"feat": L.ptr(feat), "offs": L.ptr(offs), "mu": L.ptr(mu), "vinv": L.ptr(vinv)}
    if null:
        args[null] = None
    rc = L.lib().hmmsort_cluster_isolation(args["feat"], n, F, U, args["offs"], None, args["mu"], args["vinv"],
                                           C.byref(o) if out else None)
    assert rc != 0
    assert np.all(d2 == SENT_F) and np.all(cl == SENT_I) and np.all(lp == SENT_F)
    return rc


def test_isolation_refusals(H):
    L = H._lib

    def refused(code, *words, **kw):
        rc = iso_call(H, **kw)
        assert rc == code and all(w in L.last_error() for w in words), (rc, L.last_error(), words)

    for name in ("offs", "mu", "vinv", "feat"):
        refused(L.EINVAL, "null", null=name)
    refused(L.EINVAL, "null", out=False)
    refused(L.EINVAL, "F = 0", F=0)
    refused(L.EINVAL, "F = 65", F=65)
    refused(L.EINVAL, "U = 0", U=0)
    refused(L.EINVAL, "U = 4097", U=4097, offs=np.zeros(4098))
    refused(L.EINVAL, "offs[0] = -1", offs=(-1, 1, 2))
    refused(L.EINVAL, "unit 1", "-1", offs=(0, 2, 1))
    refused(L.EINVAL, "n = 4", "spans 3", n=4)
    refused(L.EINVAL, "mu", "unit 1", "feature 0", mu=[[0, 0], [np.inf, 0]])
    v = np.tile(np.eye(2), (2, 1, 1))
    v[0, 1, 0] = np.nan
    refused(L.EINVAL, "Vinv", "unit 0", "(1, 0)", vinv=v)
    v = np.tile(np.eye(2), (2, 1, 1))
    v[1, 0, 0] = np.inf                                                # only a NaN there means "not scored"
    refused(L.EINVAL, "Vinv", "unit 1", "(0, 0)", vinv=v)
    nbig = (1 << 30) // 4096 + 1
    refused(L.EUNSUP, "U * n", "4096", str(nbig), U=4096, F=1, n=nbig,
            offs=np.concatenate([np.zeros(4096), [nbig]]))
