"""hmmsort_snippet_features / hmmsort_cluster_isolation and their device and plan forms against the
numpy model tests/feature_model.py: rows, used bytes, counts, moments, the isolation distance and the confusion counts
must come out equal to the bit; lpair, which goes through the device's exp / erfc / sqrt, within four times the
rounding bound of its chain.  Shapes are small: the seam lists of the footprints (255, 256, 257 and 513 entries)."""
import ctypes as C

import numpy as np
import pytest

import feature_model as M
import footprint_model as FM

pytestmark = pytest.mark.gpu


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(~((got == want) | ((got != got) & (want != want))))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[:4].T)], want[tuple(bad[:4].T)])


def check_features(sf, y, lists, pre, W, chan, basis, centre, mode, what):
    """a SnippetFeatures with host rows against the model, bit for bit; returns the model's rows"""
    f, use, n, nused = M.features(y, lists, pre, W, chan, basis, centre)
    same(sf.features, f, what + ": rows")
    same(sf.used, use, what + ": used")
    same(sf.n, n, what + ": n")
    same(sf.n_used, nused, what + ": nused")
    Mch = y.shape[0] if chan is None else len(chan)
    if mode == 1:
        m1, m2 = M.moments(f, use, n, Mch)
        same(sf.b1, m1, what + ": b1")
        same(sf.b2, m2, what + ": b2")
    if mode == 2:
        m1, m2 = M.moments(f, use, n, 1)
        same(sf.g1, m1[:, 0], what + ": g1")
        same(sf.g2, m2[:, 0], what + ": g2")
    return f, use, n, nused


# ---- 1: features and moments at the seams -------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 7, 60, 64, 65])
def test_seams(H, W):
    y, lists, pre, W = M.seam_case(W)
    rng = np.random.default_rng(100 + W)
    for chan in ([1], None):                                           # M = 1 and M = 3
        Mch = 1 if chan else 3
        for P in (1, 3, 5):
            if P > W:
                continue
            basis, centre = M.random_basis(rng, Mch, P, W)
            for mode in (1, 2):
                sf = H.snippet_features(y, lists, pre=pre, W=W, channels=chan, basis=basis, centre=centre, moments=mode)
                check_features(sf, y, lists, pre, W, chan, basis, centre, mode, "W %d M %d P %d mode %d" % (W, Mch, P,
                                                                                                          mode))
    assert sf.n.tolist() == list(FM.SEAM_N) and sf.n_used.tolist() == [n - 2 for n in FM.SEAM_N]
    assert not sf.used[0] and not sf.used[254] and not sf.features[0].any() and not sf.features[254].any()
    again = H.snippet_features(y, lists, pre=pre, W=W, channels=chan, basis=basis, centre=centre, moments=2)
    assert again.features.tobytes() == sf.features.tobytes() and again.g2.tobytes() == sf.g2.tobytes()
    nb = H.snippet_features(y, lists, pre=pre, W=W, basis=basis, moments=0)              # a basis without a centre
    check_features(nb, y, lists, pre, W, None, basis, None, 0, "no centre")


def test_export_is_the_block_itself(H):
    y, lists, pre, W = M.seam_case(60)
    sf = H.snippet_features(y, lists, pre=pre, W=W)
    f, use, n, nused = check_features(sf, y, lists, pre, W, None, None, None, 0, "export")
    assert sf.features.shape == (sum(FM.SEAM_N), 3 * W) and sf.b1 is None and sf.g1 is None
    for r in (1, 300, 1280 - 1):
        u = int(np.searchsorted(sf.offs, r, side="right")) - 1
        a = int(lists[u][r - sf.offs[u]]) - 1 - pre
        assert sf.features[r].tobytes() == y[:, a:a + W].tobytes()
    only = H.snippet_features(y, lists, pre=pre, W=W, moments=0, features=False)
    assert only.features is None and only.used is None and np.array_equal(only.n_used, nused)


def test_no_basis_with_a_centre_and_mode_1_at_P_60(H):
    y, lists, pre, W = M.seam_case(60)
    _, centre = M.random_basis(np.random.default_rng(7), 3, 1, W)
    sf = H.snippet_features(y, lists, pre=pre, W=W, centre=centre, moments=1)
    check_features(sf, y, lists, pre, W, None, None, centre, 1, "centre, mode 1, P = W = 60")
    assert sf.b2.shape == (4, 3, 60, 60) and np.array_equal(sf.b2, sf.b2.transpose(0, 1, 3, 2))


def test_mode_1_at_P_128(H):
    y, lists, pre, W = M.seam_case(128)
    sf = H.snippet_features(y, lists, pre=pre, W=W, channels=[2], moments=1, features=False)
    f, use, n, nused = M.features(y, lists, pre, W, [2])
    m1, m2 = M.moments(f, use, n, 1)
    same(sf.b1, m1, "b1")
    same(sf.b2, m2, "b2")
    assert sf.b2.shape == (4, 1, 128, 128)


@pytest.mark.parametrize("Mch,P", [(1, 1), (3, 8), (2, 32)])
def test_mode_2_at_F_1_24_64(H, Mch, P):
    y, lists, pre, W = M.seam_case(60)
    chan = {1: [0], 3: None, 2: [0, 2]}[Mch]
    basis, centre = M.random_basis(np.random.default_rng(8 + P), Mch, P, W)
    sf = H.snippet_features(y, lists, pre=pre, W=W, channels=chan, basis=basis, centre=centre, moments=2)
    check_features(sf, y, lists, pre, W, chan, basis, centre, 2, "F = %d" % (Mch * P))
    assert sf.g2.shape == (4, Mch * P, Mch * P)
    none = H.snippet_features(y, lists, pre=pre, W=W, channels=chan, basis=basis, centre=centre, moments=2,
                              features=False)                          # the rows live in a workspace
    assert none.features is None and none.g2.tobytes() == sf.g2.tobytes() and none.g1.tobytes() == sf.g1.tobytes()


def test_channel_row_with_a_repeat_and_reversed(H):
    y, lists, pre, W = M.seam_case(7)
    chan = [2, 1, 1, 0]
    basis, centre = M.random_basis(np.random.default_rng(9), 4, 3, W)
    sf = H.snippet_features(y, lists, pre=pre, W=W, channels=chan, basis=basis, centre=centre, moments=1)
    check_features(sf, y, lists, pre, W, chan, basis, centre, 1, "chan")
    raw = H.snippet_features(y, lists, pre=pre, W=W, channels=chan, moments=2)          # F = 28 without a basis
    check_features(raw, y, lists, pre, W, chan, None, None, 2, "chan, no basis")
    assert raw.features[:, 7:14].tobytes() == raw.features[:, 14:21].tobytes()


def test_an_empty_unit_and_a_window_longer_than_the_block(H):
    rng = np.random.default_rng(10)
    y = FM.wide_block(rng, 2, 50)
    lists = [np.zeros(0, dtype=np.int64), np.array([17]), np.array([3, 4, 44, 45, 1 << 40]), np.zeros(0, dtype=np.int64)]
    basis, centre = M.random_basis(rng, 2, 2, 10)
    for mode in (1, 2):
        sf = H.snippet_features(y, lists, pre=3, W=10, basis=basis, centre=centre, moments=mode)
        check_features(sf, y, lists, 3, 10, None, basis, centre, mode, "empty unit")
    assert sf.n.tolist() == [0, 1, 5, 0] and sf.n_used.tolist() == [0, 1, 2, 0] and not sf.g2[0].any()
    basis, centre = M.random_basis(rng, 2, 2, 51)
    for mode in (1, 2):
        sf = H.snippet_features(y, lists, pre=3, W=51, basis=basis, centre=centre, moments=mode)
        check_features(sf, y, lists, 3, 51, None, basis, centre, mode, "W > T")
    assert not sf.n_used.any() and not sf.used.any() and not sf.features.any() and not sf.g2.any()
    none = H.snippet_features(y, [lists[0]], pre=3, W=10, moments=1)                     # no entry at all
    assert none.features.shape == (0, 20) and none.n.tolist() == [0] and not none.b2.any()


def test_int16_block(H):
    _, lists, pre, W = M.seam_case(60)
    rng = np.random.default_rng(44)
    raw = rng.integers(-32768, 32768, (3, 40_000)).astype(np.int16)
    basis, centre = M.random_basis(rng, 3, 3, W)
    a = H.snippet_features(raw, lists, pre=pre, W=W, basis=basis, centre=centre, moments=2)
    b = H.snippet_features(raw.astype(np.float64), lists, pre=pre, W=W, basis=basis, centre=centre, moments=2)
    assert a.features.tobytes() == b.features.tobytes() and a.g2.tobytes() == b.g2.tobytes()
    check_features(a, raw.astype(np.float64), lists, pre, W, None, basis, centre, 2, "int16")
    e = H.snippet_features(raw, lists, pre=pre, W=W, channels=[1])
    assert np.array_equal(e.features[5], raw[1, lists[0][5] - 1 - pre:lists[0][5] - 1 - pre + W].astype(np.float64))


# ---- 2: the device and plan forms ---------------------------------------------------------------------------------
def test_device_form_on_a_second_stream(H):
    import torch
    y, lists, pre, W = M.seam_case(65)
    basis, centre = M.random_basis(np.random.default_rng(11), 3, 5, W)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    d_y = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    d_t = torch.from_numpy(np.concatenate(lists).astype(np.int64)).cuda()
    host = H.snippet_features(y, lists, pre=pre, W=W, basis=basis, centre=centre, moments=2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for stream in (None, side.cuda_stream):
        dev = H.device.snippet_features(d_y, d_t, offs, pre=pre, W=W, basis=basis, centre=centre, moments=2,
                                        stream=stream)
        assert dev.features.cpu().numpy().tobytes() == host.features.tobytes()
        assert dev.used.cpu().numpy().tobytes() == host.used.tobytes()
        assert dev.g1.tobytes() == host.g1.tobytes() and dev.g2.tobytes() == host.g2.tobytes()
        assert np.array_equal(dev.n, host.n) and np.array_equal(dev.n_used, host.n_used)
    # a sub-range of the lists: offs[0] > 0 moves row 0
    sub = H.device.snippet_features(d_y, d_t, offs[1:], pre=pre, W=W, moments=1, centre=centre)
    want = H.snippet_features(y, lists[1:], pre=pre, W=W, moments=1, centre=centre)
    assert sub.features.cpu().numpy().tobytes() == want.features.tobytes() and sub.b2.tobytes() == want.b2.tobytes()
    with pytest.raises(H.HmmsortError) as e:
        H.device.snippet_features(d_y, d_t, [0, 2, 1], pre=pre, W=W)
    assert e.value.code == H._lib.EINVAL and "unit 1" in str(e.value)
    wild = torch.tensor([-5, 0, 70, 1 << 62, -(1 << 62)], dtype=torch.int64, device="cuda")
    sf = H.device.snippet_features(d_y, wild, [0, 5], pre=3, W=10, moments=2, channels=[0])
    assert sf.n_used.tolist() == [1] and sf.used.cpu().numpy().tolist() == [0, 0, 1, 0, 0]


def ring_setup(H, nC, T=4000, K=12, seed=60):
    pp, sg = (0.01, 0.008), 0.3
    base = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                       H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    mus = [np.asfortranarray(base * (1.0 + 0.1 * c)) for c in range(nC)]
    ys = [H.create_signal(T, sg, pp, mus[c], seed=seed + c) for c in range(nC)]
    sm = H.StateMatrix.create(2, K, np.log(pp), False)
    return sm, mus, ys, sg


def plan_rows_equal_the_host_form(H, plan, dx, block, lists, pre, W):
    import torch
    rng = np.random.default_rng(12)
    d_block = torch.from_numpy(block).cuda()
    basis, centre = M.random_basis(rng, block.shape[0], 3, W, wide=False)
    for kw in (dict(moments=1), dict(basis=basis, centre=centre, moments=2)):
        got = plan.snippet_features(dx, d_block, pre=pre, W=W, **kw)
        want = H.snippet_features(block, lists, pre=pre, W=W, **kw)
        assert got.features.cpu().numpy().tobytes() == want.features.tobytes() and len(want.features) > 40
        assert got.used.cpu().numpy().tobytes() == want.used.tobytes()
        assert np.array_equal(got.n, want.n) and np.array_equal(got.n_used, want.n_used)
        for name in ("b1", "b2", "g1", "g2"):
            a, b = getattr(got, name), getattr(want, name)
            assert (a is None and b is None) or a.tobytes() == b.tobytes(), name
    check_features(want, block, lists, pre, W, None, basis, centre, 2, "plan form")
    # cap_rows one short: no row, no byte, no error; the counts and the moments all the same
    L = H._lib
    n_total, F = int(want.n.sum()), want.features.shape[1]
    d_f = torch.full((n_total, F), -7.25, dtype=torch.float64, device="cuda")
    d_u = torch.full((n_total,), 0x55, dtype=torch.uint8, device="cuda")
    U = len(lists)
    n, g1, g2 = np.zeros(U, dtype=np.int64), np.zeros((U, F)), np.zeros((U, F, F))
    bs, ce = np.ascontiguousarray(basis), np.ascontiguousarray(centre)
    opt = L.FeatOpt(pre, W, 0, None, 3, L.ptr(bs), L.ptr(ce), 2)
    out = L.FeatOut(d_f.data_ptr(), d_u.data_ptr(), n_total - 1, L.ptr(n), None, None, None, L.ptr(g1), L.ptr(g2))
    L.check(L.lib().hmmsort_plan_snippet_features(plan._h, C.c_void_p(dx.data_ptr()), C.c_void_p(d_block.data_ptr()),
                                                  block.shape[0], C.byref(opt), C.byref(out), None))
    assert bool((d_f == -7.25).all()) and bool((d_u == 0x55).all())
    assert np.array_equal(n, want.n) and g2.tobytes() == want.g2.tobytes() and g1.tobytes() == want.g1.tobytes()
    out.cap_rows = n_total
    L.check(L.lib().hmmsort_plan_snippet_features(plan._h, C.c_void_p(dx.data_ptr()), C.c_void_p(d_block.data_ptr()),
                                                  block.shape[0], C.byref(opt), C.byref(out), None))
    assert d_f.cpu().numpy().tobytes() == want.features.tobytes()


@pytest.mark.parametrize("nC", [1, 2])
def test_plan_form(H, nC):
    import torch
    T = 4000
    sm, mus, ys, sg = ring_setup(H, nC, T)
    block = FM.wide_block(np.random.default_rng(61), 3, T)
    block[0] = ys[0]
    dx = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
    dll = torch.zeros(nC, dtype=torch.float64, device="cuda")
    H.set_option("engine", H.ENGINE_AUTO if nC == 1 else H.ENGINE_WAVE)
    try:
        if nC == 1:
            plan = H.Plan(T, sm, mus[0], sg)
            plan.viterbi(torch.from_numpy(ys[0]).cuda(), dx, dll)
        else:
            plan = H.Plan.batched(T, [sm] * nC, mus, [sg] * nC)
            plan.viterbi(torch.from_numpy(np.stack(ys)).cuda(), dx, dll)
        lists = []
        for c in range(nC):
            one = H.Plan(T, sm, mus[c], sg)
            lists += one.extract_spiketimes(dx[c])
            one.close()
        assert len(lists) == 2 * nC and all(len(t) > 10 for t in lists)
        plan_rows_equal_the_host_form(H, plan, dx, block, lists, 5, 14)
        plan.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)


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
        lists = plan.extract_spiketimes(dx)
        assert all(len(t) > 10 for t in lists)
        plan_rows_equal_the_host_form(H, plan, dx, block, lists, 4, 16)
        iso = plan.cluster_isolation(dx, torch.from_numpy(block).cuda(), pre=4, W=16, P=2, channels=[0, 1])
        want = H.cluster_isolation(block, lists, pre=4, W=16, P=2, channels=[0, 1])
        assert not np.isnan(want.distance).all() and not np.isnan(want.l_ratio).any()
        assert iso.distance.tobytes() == want.distance.tobytes() and iso.closer.tobytes() == want.closer.tobytes()
        plan.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)


# ---- 3: isolation ---------------------------------------------------------------------------------------------------
def lpair_bound(F, tiles=3):
    """the roundings of one entry's chain -- the fold across tiles, within a tile, the series, and eight for h, the
    exponential's argument and the products around the series -- times 2^-53; all terms are positive"""
    return (tiles + 256 + F / 2 + 8) * 2.0 ** -53


def check_isolation(got, feat, offs, used, mu, vinv, what):
    d2, closer, lpair = got
    F = np.asarray(feat).shape[1]
    iso, cl, lp, _ = M.isolation(feat, offs, used, mu, vinv)
    same(d2, iso, what + ": iso_d2")
    same(closer, cl, what + ": closer")
    assert lpair.shape == lp.shape and np.array_equal(np.isnan(lpair), np.isnan(lp)), what
    ok = ~np.isnan(lp)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(lp[ok] > 1e-290, np.abs(lpair[ok] - lp[ok]) / lp[ok], 0.0)
    worst = float(rel.max()) if rel.size else 0.0
    print("lpair %s: largest relative difference %.3g (rounding bound %.3g) over %d entries in [%.3g, %.3g]"
          % (what, worst, lpair_bound(F), int(np.count_nonzero(lp[ok] > 1e-290)), lp[ok].min(initial=0.0),
             lp[ok].max(initial=0.0)))
    assert np.allclose(lpair[ok], lp[ok], rtol=4 * lpair_bound(F), atol=1e-300), (what, worst)
    return iso, cl, lp


@pytest.mark.parametrize("F", [1, 2, 3, 24, 64])
def test_isolation_against_the_model(H, F):
    feat, offs, used, mu, vinv = M.iso_case(F)
    assert not np.array_equal(vinv[0], vinv[0].T) or F == 1            # Vinv is not symmetric
    got = H.isolation_scores(feat, offs, mu, vinv, used)
    iso, cl, lp = check_isolation(got, feat, offs, used, mu, vinv, "F = %d" % F)
    assert not np.isnan(iso).any() and (cl >= 0).all()
    assert np.count_nonzero(lp > 1e-290) >= 6                          # the comparison of lpair is not empty
    allused = H.isolation_scores(feat, offs, mu, vinv)
    check_isolation(allused, feat, offs, None, mu, vinv, "F = %d, all used" % F)
    again = H.isolation_scores(feat, offs, mu, vinv, used)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_isolation_device_form(H):
    import torch
    feat, offs, used, mu, vinv = M.iso_case(24, seed=1)
    host = H.isolation_scores(feat, offs, mu, vinv, used)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    d_f, d_u = torch.from_numpy(feat).cuda(), torch.from_numpy(used).cuda()
    for stream in (None, side.cuda_stream):
        dev = H.device.isolation_scores(d_f, offs, mu, vinv, d_used=d_u, stream=stream)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(host, dev))
    dev = H.device.isolation_scores(d_f, offs, mu, vinv)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(H.isolation_scores(feat, offs, mu, vinv), dev))


def test_isolation_rank_edges(H):
    feat, offs, _, mu, vinv = M.iso_case(3, counts=(40, 39, 1), seed=2, unused=False)
    # one unit: no non-member
    d2, closer, lpair = H.isolation_scores(feat[:40], offs[:2], mu[:1], vinv[:1])
    assert np.isnan(d2[0]) and closer.tolist() == [[0]] and lpair.tolist() == [[0.0]]
    # units of 40 and 39: unit 0 has n_o = n_u - 1 (NaN), unit 1 has non-members to spare
    got = H.isolation_scores(feat[:79], offs[:3], mu[:2], vinv[:2])
    iso, _, _ = check_isolation(got, feat[:79], offs[:3], None, mu[:2], vinv[:2], "n_o = n_u - 1")
    assert np.isnan(iso[0]) and not np.isnan(iso[1])
    # 40 against 39 + 1: n_o = n_u, the largest non-member distance
    got = H.isolation_scores(feat, offs, mu, vinv)
    iso, _, _ = check_isolation(got, feat, offs, None, mu, vinv, "n_o = n_u")
    assert iso[0] == M.d2_rows(feat[40:], mu[0], vinv[0]).max()
    # the same through unused rows: 41 members of which one is not used
    feat2, offs2, _, mu2, vinv2 = M.iso_case(3, counts=(41, 39, 1), seed=2, unused=False)
    used = np.ones(81, dtype=np.uint8)
    used[7] = 0
    got = H.isolation_scores(feat2, offs2, mu2, vinv2, used)
    iso, _, _ = check_isolation(got, feat2, offs2, used, mu2, vinv2, "n_o = n_u by an unused row")
    assert iso[0] == M.d2_rows(feat2[41:], mu2[0], vinv2[0]).max()


def test_isolation_ties_are_exact_and_closer_is_strict(H):
    feat, offs, used, mu, vinv = M.iso_case(3, seed=3, dup=True)
    assert np.array_equal(feat[0], feat[1]) and np.array_equal(feat[600], feat[601])
    got = H.isolation_scores(feat, offs, mu, vinv, used)
    check_isolation(got, feat, offs, used, mu, vinv, "ties")
    # two units with one Gaussian: every distance ties with the row's own, so nothing is strictly closer
    mu[1], vinv[1] = mu[0], vinv[0]
    d2, closer, _ = H.isolation_scores(feat, offs, mu, vinv, used)
    assert closer[0, 1] == 0 and closer[1, 0] == 0
    check_isolation((d2, closer, _), feat, offs, used, mu, vinv, "equal Gaussians")


def test_isolation_not_scored_unit_and_indefinite_vinv(H):
    feat, offs, used, mu, vinv = M.iso_case(2, seed=4)
    vinv[1] = np.inf                                                   # not read: only [0][0] decides
    vinv[1, 0, 0] = np.nan
    mu[1] = np.nan
    got = H.isolation_scores(feat, offs, mu, vinv, used)
    iso, cl, lp = check_isolation(got, feat, offs, used, mu, vinv, "not scored")
    assert np.isnan(iso[1]) and not np.isnan(iso[[0, 2, 3]]).any()
    assert (cl[1, [0, 2, 3]] == -1).all() and (cl[[0, 2, 3], 1] == -1).all() and cl[1, 1] == 0 and cl[0, 2] >= 0
    assert np.isnan(lp[1, [0, 2, 3]]).all() and lp[0, 1] > 0          # its spikes still count against the others
    # an indefinite Vinv: q < 0 is clamped to +0.0
    feat, offs, used, mu, vinv = M.iso_case(2, seed=5)
    vinv[0] = np.array([[1.0, 0.0], [0.3, -2.0]])
    got = H.isolation_scores(feat, offs, mu, vinv, used)
    check_isolation(got, feat, offs, used, mu, vinv, "indefinite")
    d = M.d2_rows(feat, mu[0], vinv[0])
    assert np.count_nonzero(d == 0.0) > 100 and got[2][0, 1] > 50.0   # Q_F(0) = 1 per clamped row


# ---- 4: refusals that need the device forms -------------------------------------------------------------------------
def test_refusals_of_the_plan_form(H):
    import torch
    L = H._lib
    sm, mus, _, sg = ring_setup(H, 1)
    plan = H.Plan(4000, sm, mus[0], sg)
    d_b = torch.zeros((2, 4000), dtype=torch.float64, device="cuda")
    dx = torch.ones(4000, dtype=torch.int16, device="cuda")
    with pytest.raises(H.HmmsortError) as e:
        plan.snippet_features(dx, d_b, pre=3, W=2000)
    assert e.value.code == L.EINVAL and "W = 2000" in str(e.value)
    with pytest.raises(H.HmmsortError) as e:
        plan.snippet_features(dx, d_b, pre=3, W=10, channels=[0, 2])
    assert e.value.code == L.EINVAL and "channel 2" in str(e.value)
    with pytest.raises(ValueError):
        plan.snippet_features(dx, torch.zeros((2, 50), dtype=torch.float64, device="cuda"))
    sf = plan.snippet_features(dx, d_b, pre=3, W=10, moments=2)        # a silent path: no events, zeros
    assert sf.n.tolist() == [0, 0] and sf.features.shape == (0, 20) and not sf.g2.any()
    plan.close()


# ---- 5: end to end --------------------------------------------------------------------------------------------------
def test_cluster_isolation_end_to_end(H):
    """api.cluster_isolation on the science case equals the model's pipeline on everything that is exact, given the
    model's basis equals the api's (both take numpy's eigh of the same bytes)"""
    import torch
    y, lists, pre, W, chan, events = M.science_case(2)
    noise = H.unassigned_events(events, lists, 3)
    iso = H.cluster_isolation(y, lists + [noise], pre=pre, W=W, channels=chan, P=3, keep_features=True)
    d2, lr, closer, lpair, nused, (basis, centre) = M.pipeline(y, lists + [noise], pre, W, chan, 3)
    same(iso.basis, basis, "basis")
    same(iso.centre, centre, "centre")
    same(iso.distance, d2, "distance")
    same(iso.closer, closer, "closer")
    same(iso.n_used, nused, "n_used")
    assert np.allclose(iso.lpair, lpair, rtol=4 * lpair_bound(6, tiles=1), atol=1e-300)
    assert np.allclose(iso.l_ratio, lr, rtol=4 * lpair_bound(6, tiles=1) + 2.0 ** -50, atol=1e-300)
    assert iso.features.shape == (520, 6) and np.argmax(iso.distance[:3]) == 2
    offs = np.concatenate([[0], np.cumsum([len(t) for t in lists + [noise]])]).astype(np.int64)
    dev = H.device.cluster_isolation(torch.from_numpy(y).cuda(), torch.from_numpy(np.concatenate(lists + [noise])).cuda(),
                                     offs, pre=pre, W=W, channels=chan, P=3)
    assert dev.distance.tobytes() == iso.distance.tobytes() and dev.lpair.tobytes() == iso.lpair.tobytes()
    assert dev.closer.tobytes() == iso.closer.tobytes() and dev.features is None


def test_sort_data_returns_the_isolation(H):
    T, K = 12_000, 16
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                        H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    pp = (0.01, 0.006)
    y = H.create_signal(T, 0.3, pp, temps, seed=85)
    rng = np.random.default_rng(86)
    cols = np.stack([y, 0.5 * y + 0.3 * rng.standard_normal(T), 0.3 * rng.standard_normal(T)], axis=1)
    raw = np.round(cols * 1000).astype(np.int16)
    spike_forms = np.zeros((K, 1, 2))
    spike_forms[:, 0, :] = temps * 1000
    args = (spike_forms, [1.0 / 300.0 ** 2], list(pp), raw)
    plain = H.sort_data(*args, dosave=False, chunksize=4000)
    none = H.sort_data(*args, dosave=False, chunksize=4000, isolation=None)
    assert set(plain) == set(none) == {"mlseq", "ll", "waveforms", "lp", "sigma"}
    assert all(np.array_equal(none[k], plain[k]) for k in plain)
    sm = H.StateMatrix.create(2, K, np.log(pp), True)
    tm = H.HMMSpikeTemplateModel(sm, np.asfortranarray(spike_forms[:, 0, :]), 300.0)
    lists = H.extract_spiketimes(H.fit(tm, raw[:, 0].astype(np.float64), 4000))
    assert all(len(t) > 20 for t in lists)

    def equal(out, want):
        ui = out["unit_isolation"]
        assert set(ui) == {"distance", "l_ratio", "lpair", "closer", "n_used"}
        for k in ui:
            assert np.asarray(ui[k]).tobytes() == np.asarray(getattr(want, k)).tobytes(), k

    one = H.sort_data(*args, dosave=False, chunksize=4000, isolation=True)                 # the channel alone
    assert set(one) - set(plain) == {"unit_isolation"} and all(np.array_equal(one[k], plain[k]) for k in plain)
    equal(one, H.cluster_isolation(raw[:, 0].astype(np.float64), lists))
    assert not np.isnan(one["unit_isolation"]["distance"]).all()             # the larger unit lacks non-members
    blk = H.sort_data(*args, dosave=False, chunksize=4000, preprocess={}, channel=0,
                      isolation=dict(pre=4, W=12, P=2, channels=[0, 1]))                   # the preprocessed block
    equal(blk, H.cluster_isolation(np.ascontiguousarray(raw.T.astype(np.float64)), lists, pre=4, W=12, P=2,
                                   channels=[0, 1]))
    H.shutdown()
