"""Spatial whitening on the device (csrc/whiten.hip: noise scale, quiet mask, sums, channel mix) against the numpy
model of whiten_model.py.  Every comparison is np.array_equal or bytes: the contract fixes the order and the rounding
of every operation (test_whiten_cpu.py shows that other orders give other bits).

Shapes: the sums are cut into tiles of 256 samples and the mask is made in tiles of 1024, so T = 255 / 256 / 257, 513,
1300 and 10 007 are a tile, its neighbours and several ragged ones; the sums kernel takes blocks of 16, 32 or 64
channels (C <= 16, <= 32, beyond), hence C = 16 / 17 / 33 beside the small ones, and C = 1024 has 136 block pairs.
guard = 300 reaches over tiles of the sums, guard = 3000 (in its own test) over tiles of the mask.  The mix stages
256 samples per workgroup up to C = 16, 128 up to 32, 64 up to 128, then fewer than a wave (32 at 130, 16 at 1024),
where a wave no longer works on one row: T = 63 / 64 / 65 are a wave and its neighbours."""
import ctypes as C

import numpy as np
import pytest

import whiten_model as WM

pytestmark = pytest.mark.gpu

T_LIST = (1, 255, 256, 257, 513, 1300, 10007)
C_LIST = (1, 2, 5, 16, 17, 33)
GUARDS = (0, 1, 3, 300)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def cov_dev(H, Y, threshold=4.0, guard=30, thr=None, stream=None):
    """(sigma, thr, n_quiet, s1, s2, mask) of the device form"""
    import torch
    d_q = torch.full((Y.shape[1],), 7, dtype=torch.uint8, device="cuda")
    r = H.device.noise_covariance(dev(Y), threshold, guard, thr, d_quiet=d_q, stream=stream)
    return r + (d_q.cpu().numpy(),)


def assert_cov(got, want, what):
    """got: cov_dev's tuple; want: WM.noise_cov's"""
    sigma, thr, n, s1, s2, mask = got
    wsigma, wthr, wquiet, wn, ws1, ws2 = want
    if wsigma is None:
        assert sigma is None, what
    else:
        assert np.array_equal(sigma, wsigma), what
    assert np.array_equal(thr, wthr), what
    assert mask.tobytes() == wquiet.astype(np.uint8).tobytes(), what
    assert n == wn, what
    assert np.array_equal(s1, ws1), what
    assert np.array_equal(s2, ws2), what
    assert np.array_equal(s2, s2.T), what


def heavy_block(C_, T, seed):
    """heavy-tailed data (about 0.4 of the samples quiet at thr = 300 for five channels, fewer for more); the last
    sample of the first tile and the first of the second are loud"""
    Y = WM.heavy_tailed(np.random.default_rng(seed), C_, T)
    for t in (255, 256, 1023, 1024):
        if t < T:
            Y[t % C_, t] = 1e6
    return Y


# ---- noise scale ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", (1, 3, 8))
def test_noise_scale(H, C_):
    rng = np.random.default_rng(50 + C_)
    for T in (1, 2, 255, 1024, 10007):
        ties = rng.integers(-3, 4, size=(C_, T)).astype(np.float64)
        normal = rng.standard_normal((C_, T)) * 10.0 ** rng.integers(-3, 4, size=(C_, 1))
        for Y in (ties, normal):
            got = H.device.noise_scale(dev(Y))
            assert np.array_equal(got, WM.noise_scale(Y)), (C_, T)
    assert np.array_equal(H.device.noise_scale(dev(normal[0])), WM.noise_scale(normal[:1]))   # 1-D: one channel


# ---- mask and sums -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_", C_LIST)
@pytest.mark.parametrize("T", T_LIST)
def test_mask_and_sums_every_shape(H, T, C_):
    heavy = heavy_block(C_, T, 1000 * C_ + T)
    normal = np.random.default_rng(7 + 1000 * C_ + T).standard_normal((C_, T)) * np.linspace(0.5, 20.0, C_)[:, None]
    for guard in GUARDS:
        thr = np.full(C_, 300.0 if C_ <= 5 else 3000.0)      # some samples stay quiet with many channels too
        assert_cov(cov_dev(H, heavy, guard=guard, thr=thr), WM.noise_cov(heavy, guard=guard, thr=thr),
                   ("heavy", T, C_, guard))
        assert_cov(cov_dev(H, normal, 3.0, guard), WM.noise_cov(normal, 3.0, guard), ("normal", T, C_, guard))


def test_all_loud_and_none_loud(H):
    rng = np.random.default_rng(60)
    Y = rng.standard_normal((5, 1300))
    sigma, thr, n, s1, s2, mask = cov_dev(H, Y, guard=2, thr=np.full(5, 1e-300))
    assert n == 0 and not mask.any()
    assert np.array_equal(s1, np.zeros(5)) and np.array_equal(s2, np.zeros((5, 5)))
    assert not np.signbit(s1).any() and not np.signbit(s2).any()
    got = cov_dev(H, Y, guard=2, thr=np.full(5, 100.0))
    assert got[2] == 1300 and got[5].all()
    assert_cov(got, WM.noise_cov(Y, guard=2, thr=np.full(5, 100.0)), "none loud")
    with pytest.raises(ValueError):
        H.noise_covariance(n, s1, s2)


def test_non_finite_samples_are_loud_and_stay_out(H):
    rng = np.random.default_rng(61)
    Y = rng.standard_normal((3, 2000))
    Y[1, 700], Y[2, 1500], Y[0, 1999] = np.nan, np.inf, -np.inf
    thr = np.full(3, 50.0)
    got = cov_dev(H, Y, guard=4, thr=thr)
    mask = got[5]
    loud = np.zeros(2000, dtype=bool)
    for t in (700, 1500, 1999):
        loud[max(0, t - 4):t + 5] = True
    assert np.array_equal(mask.astype(bool), ~loud)
    assert np.all(np.isfinite(got[3])) and np.all(np.isfinite(got[4]))
    assert_cov(got, WM.noise_cov(Y, guard=4, thr=thr), "non-finite")


def test_guard_beyond_the_mask_tile(H):
    rng = np.random.default_rng(62)
    Y = rng.standard_normal((2, 20000))
    Y[0, 5000], Y[1, 5001], Y[1, 17000] = 99.0, 99.0, -99.0
    thr = np.full(2, 50.0)
    for guard in (1023, 1024, 3000, 65536):
        assert_cov(cov_dev(H, Y, guard=guard, thr=thr), WM.noise_cov(Y, guard=guard, thr=thr), guard)
    assert cov_dev(H, Y, guard=3000, thr=thr)[2] == 20000 - 6002 - 6000
    assert cov_dev(H, Y, guard=-1, thr=thr)[5].tobytes() == WM.quiet_mask(Y, thr, 30).astype(np.uint8).tobytes()


def test_explicit_thresholds_equal_threshold_times_sigma(H):
    rng = np.random.default_rng(63)
    Y = rng.standard_normal((5, 4000)) * np.array([1.0, 3.0, 0.1, 10.0, 2.0])[:, None]
    a = cov_dev(H, Y, 3.5, 3)
    b = cov_dev(H, Y, None, 3, thr=3.5 * WM.noise_scale(Y))
    assert np.array_equal(a[0], WM.noise_scale(Y)) and b[0] is None
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)
    default = cov_dev(H, Y, None, None)                   # NaN threshold, negative guard: 4.0 and 30
    assert_cov(default, WM.noise_cov(Y, 4.0, 30), "defaults")
    L = H._lib
    s, n, s1, s2 = np.zeros(5), np.zeros(1, dtype=np.int64), np.zeros(5), np.zeros((5, 5))
    out = L.NoiseOut(s.ctypes.data, n.ctypes.data, s1.ctypes.data, s2.ctypes.data, None)
    L.check(L.lib().hmmsort_noise_cov_device(C.c_void_p(dev(Y).data_ptr()), 5, 4000, None, C.byref(out), None))
    assert n[0] == default[2] and np.array_equal(s2, default[4]) and np.array_equal(s, default[0])


def test_same_bytes_twice(H):
    Y = heavy_block(17, 10007, 64)
    a = cov_dev(H, Y, 4.0, 3)
    b = cov_dev(H, Y, 4.0, 3)
    for x, y in zip(a, b):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes()


def test_1024_channels(H):
    rng = np.random.default_rng(65)
    Y = rng.standard_normal((1024, 300))
    thr = np.full(1024, 3.9)
    want = WM.noise_cov(Y, guard=1, thr=thr)
    assert 20 < want[3] < 280
    assert_cov(cov_dev(H, Y, guard=1, thr=thr), want, "C = 1024")


def test_1024_channels_in_rounds(H):
    """a tile's partials are 8 MB at C = 1024 and 32 MB of them are in flight: four tiles take two rounds of the fold,
    the second continuing the first"""
    rng = np.random.default_rng(66)
    Y = rng.standard_normal((1024, 900))
    thr = np.full(1024, 3.6)
    want = WM.noise_cov(Y, guard=1, thr=thr)
    assert 150 < want[3] < 600 and want[2][768:].any()
    assert_cov(cov_dev(H, Y, guard=1, thr=thr), want, "C = 1024, two rounds")


# ---- mix -----------------------------------------------------------------------------------------------------------
def mix_dev(H, Y, nbr, w, inplace=False):
    d = dev(Y)
    out = H.device.channel_mix(d, nbr, w, d if inplace else None)
    assert (out.data_ptr() == d.data_ptr()) == inplace
    if not inplace:
        assert d.cpu().numpy().tobytes() == np.ascontiguousarray(Y).tobytes()     # the input is left alone
    return out.cpu().numpy()


@pytest.mark.parametrize("T", (1, 63, 64, 65, 1023, 4097, 10007))
def test_mix_identity_permutation_and_dense(H, T):
    rng = np.random.default_rng(70 + T)
    for C_ in (1, 5, 20, 33, 64):
        Y = WM.heavy_tailed(rng, C_, T)
        eye_n, eye_w = np.arange(C_)[:, None], np.ones((C_, 1))
        assert mix_dev(H, Y, eye_n, eye_w).tobytes() == Y.tobytes()
        perm = rng.permutation(C_)
        assert mix_dev(H, Y, perm[:, None], eye_w).tobytes() == Y[perm].tobytes()
        nbr, W = np.tile(np.arange(C_), (C_, 1)), rng.standard_normal((C_, C_))
        want = WM.mix(Y, nbr, W)
        assert np.array_equal(mix_dev(H, Y, nbr, W), want), (C_, "dense")
        assert mix_dev(H, Y, nbr, W, inplace=True).tobytes() == want.tobytes(), (C_, "dense in place")
        assert np.array_equal(mix_dev(H, Y, nbr[:, ::-1], W[:, ::-1]), WM.mix(Y, nbr[:, ::-1], W[:, ::-1]))


@pytest.mark.parametrize("M", (1, 2, 5, 16, 33, 64))
def test_mix_slots_holes_repeats_and_empty_rows(H, M):
    rng = np.random.default_rng(80 + M)
    for C_, R, T in ((7, 7, 1300), (7, 3, 257), (5, 12, 1300), (40, 40, 513), (130, 9, 300)):
        Y = WM.heavy_tailed(rng, C_, T)
        nbr = rng.integers(-1, C_, size=(R, M)).astype(np.int32)      # repeats, any order, holes
        nbr[R // 2] = -1                                              # an all-empty row
        w = rng.standard_normal((R, M))
        want = WM.mix(Y, nbr, w)
        assert np.all(want[R // 2] == 0)
        got = mix_dev(H, Y, nbr, w)
        assert got.shape == (R, T) and np.array_equal(got, want), (C_, R, T)
        if R == C_:
            assert mix_dev(H, Y, nbr, w, inplace=True).tobytes() == got.tobytes()


def test_mix_1024_channels(H):
    rng = np.random.default_rng(90)
    Y = rng.standard_normal((1024, 70))
    nbr, W = np.tile(np.arange(1024), (1024, 1)), rng.standard_normal((1024, 1024))
    want = WM.mix(Y, nbr, W)
    assert np.array_equal(mix_dev(H, Y, nbr, W), want)
    assert mix_dev(H, Y, nbr, W, inplace=True).tobytes() == want.tobytes()
    nbr2 = nbr.copy()
    nbr2[3, 1000] = -1                                                # no longer the dense pattern
    assert np.array_equal(mix_dev(H, Y, nbr2, W), WM.mix(Y, nbr2, W))


# ---- interface -----------------------------------------------------------------------------------------------------
def test_host_form_equals_device_form_and_a_second_stream(H):
    import torch
    Y = heavy_block(5, 4097, 91)
    want = WM.noise_cov(Y, 4.0, 3)
    host = H.noise_sums(Y, 4.0, 3)
    got = cov_dev(H, Y, 4.0, 3)
    for x, y in zip(host, got[:5]):
        assert np.array_equal(x, y)
    assert_cov(got, want, "device")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        assert_cov(cov_dev(H, Y, 4.0, 3, stream=side.cuda_stream), want, "second stream")
        assert_cov(cov_dev(H, Y, 4.0, 3), want, "current stream")
    rng = np.random.default_rng(92)
    nbr, w = rng.integers(-1, 5, size=(3, 4)), rng.standard_normal((3, 4))
    assert H.channel_mix(Y, nbr, w).tobytes() == WM.mix(Y, nbr, w).tobytes()
    d_out = H.device.channel_mix(dev(Y), nbr, w, stream=side.cuda_stream)
    assert d_out.cpu().numpy().tobytes() == WM.mix(Y, nbr, w).tobytes()
    nbr, w = np.tile(np.arange(5), (5, 1)), rng.standard_normal((5, 5))
    assert H.channel_mix(Y, nbr, w).tobytes() == WM.mix(Y, nbr, w).tobytes()      # the host form mixes in place


def test_whiten_equals_the_model_composed_with_the_host_finish(H):
    Y = np.random.default_rng(93).standard_normal((6, 5000)) * np.array([1, 2, 3, 1, 2, 3.0])[:, None]
    Y[1:4] += 2.0 * np.random.default_rng(94).standard_normal(5000)
    for kw in (dict(), dict(neighbors=(np.arange(6.0)[:, None], 3)), dict(threshold=3.0, guard=5, eps_rel=0.0),
               dict(thr=np.full(6, 30.0))):
        out, wh = H.whiten(Y, **kw)
        sigma, thr, quiet, n, s1, s2 = WM.noise_cov(Y, kw.get("threshold", 4.0), kw.get("guard", 30), kw.get("thr"))
        nbr, w = H.whitening_matrix(H.noise_covariance(n, s1, s2), kw.get("neighbors"), kw.get("eps_rel", 1e-6))
        assert wh.n_quiet == n and np.array_equal(wh.s1, s1) and np.array_equal(wh.s2, s2)
        assert np.array_equal(wh.thr, thr) and wh.guard == kw.get("guard", 30)
        assert (wh.sigma is None) if sigma is None else np.array_equal(wh.sigma, sigma)
        assert np.array_equal(wh.nbr, nbr) and np.array_equal(wh.w, w)
        assert out.tobytes() == WM.mix(Y, nbr, w).tobytes()
        again, same = H.whiten(Y, whitening=wh)
        assert same is wh and again.tobytes() == out.tobytes()
        assert wh.apply(Y).tobytes() == out.tobytes()
    out, wh = H.whiten(Y, eps_rel=0.0)
    q = WM.quiet_mask(Y, wh.thr, 30)
    assert np.abs(np.cov(out[:, q], bias=True) - np.eye(6)).max() < 1e-9
    import torch
    d = dev(Y)
    d_out, _ = H.device.whiten(d, eps_rel=0.0)
    assert d_out.data_ptr() != d.data_ptr() and d_out.cpu().numpy().tobytes() == out.tobytes()
    d_in, _ = H.device.whiten(d, eps_rel=0.0, inplace=True)
    assert d_in.data_ptr() == d.data_ptr() and torch.equal(d_in, d_out)


def _noise_call(L, form, y, C_, T, opt, outs, null=None):
    """hmmsort_noise_cov[_device] with an out record over `outs` (sigma, n, s1, s2), the member `null` left NULL"""
    p = {k: (None if k == null else v.ctypes.data) for k, v in zip(("sigma", "n", "s1", "s2"), outs)}
    out = L.NoiseOut(p["sigma"], p["n"], p["s1"], p["s2"], None)
    o = None if opt is None else C.byref(opt)
    if form == "device":
        return L.lib().hmmsort_noise_cov_device(y, C_, T, o, C.byref(out), None)
    return L.lib().hmmsort_noise_cov(y, C_, T, o, C.byref(out))


def test_noise_refusals_leave_the_outputs_alone(H):
    import torch
    L = H._lib
    nan = float("nan")
    Y = np.random.default_rng(95).standard_normal((4, 50))
    d = dev(Y)
    good, zero, neg, bad = np.full(4, 3.0), np.array([3, 0, 3, 3.0]), np.array([3, 3, -1, 3.0]), np.array([nan, 3, 3, 3])
    cases = [
        (dict(C_=0), "C = 0"), (dict(C_=1025), "C = 1025"), (dict(T=0), "T = 0"), (dict(T=2 ** 36 + 1), "T = "),
        (dict(opt=L.NoiseOpt(4.0, None, 65537)), "guard = 65537"), (dict(opt=L.NoiseOpt(-1.0, None, 30)), "threshold"),
        (dict(opt=L.NoiseOpt(nan, zero.ctypes.data, 30)), "thr[1]"),
        (dict(opt=L.NoiseOpt(nan, neg.ctypes.data, 30)), "thr[2]"),
        (dict(opt=L.NoiseOpt(nan, bad.ctypes.data, 30)), "thr[0]"),
        (dict(null="n"), "n_quiet"), (dict(null="s1"), "s1"), (dict(null="s2"), "s2"), (dict(y=None), "y"),
    ]
    for form, y in (("device", C.c_void_p(d.data_ptr())), ("host", C.c_void_p(Y.ctypes.data))):
        for kw, word in cases:
            outs = (np.full(4, 7.0), np.full(1, 7, dtype=np.int64), np.full(4, 7.0), np.full((4, 4), 7.0))
            a = dict(y=y, C_=4, T=50, opt=L.NoiseOpt(4.0, good.ctypes.data, 30), null=None)
            a.update(kw)
            rc = _noise_call(L, form, a["y"], a["C_"], a["T"], a["opt"], outs, a["null"])
            assert rc == L.EINVAL, (form, kw, rc)
            assert word in L.last_error() and "noise_cov" in L.last_error(), (form, kw, L.last_error())
            assert all(np.all(o == 7) for o in outs), (form, kw)
    # a null record; a device mask in the host form
    assert L.lib().hmmsort_noise_cov_device(C.c_void_p(d.data_ptr()), 4, 50, None, None, None) == L.EINVAL
    assert "out" in L.last_error()
    outs = (np.full(4, 7.0), np.full(1, 7, dtype=np.int64), np.full(4, 7.0), np.full((4, 4), 7.0))
    d_q = torch.full((50,), 7, dtype=torch.uint8, device="cuda")
    rec = L.NoiseOut(outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, outs[3].ctypes.data, d_q.data_ptr())
    assert L.lib().hmmsort_noise_cov(C.c_void_p(Y.ctypes.data), 4, 50, None, C.byref(rec)) == L.EINVAL
    assert "d_quiet" in L.last_error() and all(np.all(o == 7) for o in outs) and bool((d_q == 7).all())
    # noise scale
    s = np.full(4, 7.0)
    f = L.lib().hmmsort_noise_scale_device
    assert f(C.c_void_p(d.data_ptr()), 0, 50, L.ptr(s), None) == L.EINVAL and "C = 0" in L.last_error()
    assert f(C.c_void_p(d.data_ptr()), 4, 50, None, None) == L.EINVAL and "sigma" in L.last_error()
    assert f(None, 4, 50, L.ptr(s), None) == L.EINVAL and np.all(s == 7)
    # sigma NULL is allowed
    outs = (np.full(4, 7.0), np.zeros(1, dtype=np.int64), np.zeros(4), np.zeros((4, 4)))
    assert _noise_call(L, "device", C.c_void_p(d.data_ptr()), 4, 50, None, outs, "sigma") == 0
    assert np.all(outs[0] == 7) and np.array_equal(outs[3], WM.noise_cov(Y)[5])


def test_mix_refusals_leave_the_output_alone(H):
    import torch
    L = H._lib
    Y = np.random.default_rng(96).standard_normal((4, 50))
    nbr, w = np.tile(np.arange(4, dtype=np.int32), (4, 1)), np.ones((4, 4))
    hi, lo = nbr.copy(), nbr.copy()
    hi[2, 1], lo[3, 0] = 4, -2
    d_in = dev(Y)
    d_out = torch.full((6, 50), 7.0, dtype=torch.float64, device="cuda")
    h_out = np.full((6, 50), 7.0)
    cases = [
        (dict(C_=0), "C = 0"), (dict(C_=1025), "C = 1025"), (dict(R=0), "R = 0"), (dict(R=1025), "R = 1025"),
        (dict(M=0), "M = 0"), (dict(M=1025), "M = 1025"), (dict(T=0), "T = 0"), (dict(T=2 ** 36 + 1), "T = "),
        (dict(nbr=hi), "nbr[2][1] = 4"), (dict(nbr=lo), "nbr[3][0] = -2"),
        (dict(nbr=None), "nbr"), (dict(w=None), "w"), (dict(src=None), "in"), (dict(dst=None), "out"),
    ]
    for form, src, dst in (("device", d_in.data_ptr(), d_out.data_ptr()), ("host", Y.ctypes.data, h_out.ctypes.data)):
        f = L.lib().hmmsort_channel_mix_device if form == "device" else L.lib().hmmsort_channel_mix
        tail = (None,) if form == "device" else ()
        for kw, word in cases:
            a = dict(src=src, dst=dst, C_=4, T=50, R=4, M=4, nbr=nbr, w=w)
            a.update(kw)
            rc = f(a["src"], a["C_"], a["T"], a["R"], a["M"], L.ptr(a["nbr"]), L.ptr(a["w"]), a["dst"], *tail)
            assert rc == L.EINVAL, (form, kw, rc)
            assert word in L.last_error() and "channel_mix" in L.last_error(), (form, kw, L.last_error())
        # in place with R != C; ranges that overlap in part, either way round
        assert f(src, 4, 50, 3, 4, L.ptr(nbr), L.ptr(w), src, *tail) == L.EINVAL and "R == C" in L.last_error()
        two = np.ascontiguousarray(nbr[:2] % 2)
        for a, b in ((src, src + 8 * 60), (src + 8 * 60, src)):
            assert f(a, 2, 50, 2, 4, L.ptr(two), L.ptr(w), b, *tail) == L.EINVAL
            assert "overlap" in L.last_error()
    torch.cuda.synchronize()
    assert bool((d_out == 7).all()) and np.all(h_out == 7)
    assert d_in.cpu().numpy().tobytes() == Y.tobytes()


# ---- end to end ----------------------------------------------------------------------------------------------------
def _shared_noise_recording(H, seed, K=60, T=40_000):
    """the two templates on channel 0 of four; independent noise 0.3 and two noise sources shared by all channels
    with gains of different size and sign, which no common reference removes"""
    from conftest import two_templates
    temps = two_templates(H, K)
    pp = [0.003, 0.002]
    y0, onsets = H.create_signal(T, 0.3, pp, temps, seed=seed, return_states=True)
    rng = np.random.default_rng(100 + seed)
    z = rng.standard_normal((2, T))
    Y = 0.3 * rng.standard_normal((4, T))
    Y[0] = y0
    g1, g2 = np.array([3.0, 3.6, 2.7, 3.3]), np.array([2.4, -2.1, 2.7, -1.8])
    Y += g1[:, None] * z[0] + g2[:, None] * z[1]
    troughs = [(o + int(np.argmin(temps[:, j])) + 1, j) for o, j in onsets if o + K <= T]   # 1-based
    return temps, pp, Y, troughs


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_end_to_end_shared_noise(H, seed):
    """decoded whole with the two true templates as a ring model.  Whitened (templates scaled by w[0][0], sigma 1):
    every true spike and nothing else.  Raw channel 0 with its own noise scale as sigma: fewer than half; behind a
    median reference: fewer than 3/4.  The CPU model of the same rules with the CPU checker's decode gives, for seeds
    1 / 2 / 3: 156 / 139 / 163 true spikes, all found with as many events when whitened; 44 / 40 / 43 raw; 89 / 75 /
    82 median-referenced."""
    from test_gpu_preprocess import _found
    temps, pp, Y, troughs = _shared_noise_recording(H, seed)
    sm = H.StateMatrix.create(2, temps.shape[0], np.log(pp), False)
    out, wh = H.whiten(Y, 4.0, 30, eps_rel=0)
    tm = H.HMMSpikeTemplateModel(sm, wh.scale_templates(temps, 0), 1.0)
    assert np.array_equal(tm.mu, temps * wh.w[0, 0])
    hit, n = _found(H, tm, out[0], troughs)
    raw = H.HMMSpikeTemplateModel(sm, temps, float(wh.sigma[0]))
    hit0, n0 = _found(H, raw, Y[0], troughs)
    med = H.preprocess(np.ascontiguousarray(Y.T), None, "median")
    ref = H.HMMSpikeTemplateModel(sm, temps, float(WM.noise_scale(med)[0]))
    hit1, n1 = _found(H, ref, med[0], troughs)
    print("seed %d: %d true spikes; whitened %d found, %d events; raw %d found, %d events; median reference %d found, "
          "%d events" % (seed, len(troughs), hit, n, hit0, n0, hit1, n1))
    assert hit == len(troughs) and n == len(troughs)
    assert hit0 < 0.5 * len(troughs)
    assert hit1 < 0.75 * len(troughs)


# ---- driver --------------------------------------------------------------------------------------------------------
def test_sort_data_with_whiten_equals_sort_data_on_the_whitened_row(H):
    from conftest import two_templates
    K, T, c = 20, 6000, 3
    temps = two_templates(H, K) * 100.0
    pp = [0.004, 0.003]
    rng = np.random.default_rng(9)
    chans = [H.create_signal(T, 30.0, pp, temps, seed=10 + i) for i in range(5)]
    common = 200.0 * np.sin(2 * np.pi * 50.0 * np.arange(T) / 30000.0) + 40.0 * rng.standard_normal(T)
    raw = np.ascontiguousarray(np.round(np.stack(chans, axis=1) + common[:, None]).astype(np.int16))   # (T, 5)
    pre = dict(fs=30000, low=300, ntaps=129, reference="median")
    clean = H.preprocess(raw, H.design_fir(30000, low=300, ntaps=129), "median")
    white, wh = H.whiten(clean)
    # the templates as they appear on the whitened channel, in units of its noise
    args = (wh.scale_templates(temps, c)[:, None, :], [1.0], pp)
    b = H.sort_data(*args, white[c], dosave=False)
    for whiten in (True, wh, dict(threshold=4.0, guard=30)):
        a = H.sort_data(*args, raw, dosave=False, preprocess=dict(pre, whiten=whiten), channel=c)
        assert sorted(a) == sorted(list(b) + ["whitening"])
        for key in b:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
        assert sorted(a["whitening"]) == ["n_quiet", "nbr", "sigma", "w"]
        assert np.array_equal(a["whitening"]["w"], wh.w) and np.array_equal(a["whitening"]["nbr"], wh.nbr)
        assert a["whitening"]["n_quiet"] == wh.n_quiet and np.array_equal(a["whitening"]["sigma"], wh.sigma)
    assert (b["mlseq"] > 1).any()
    # footprints are measured on the whitened block
    f = H.sort_data(*args, raw, dosave=False, preprocess=dict(pre, whiten=True), channel=c, footprints=dict(pre=5, W=K))
    assert np.array_equal(f["mlseq"], b["mlseq"]) and "whitening" in f
    tm = H.HMMSpikeTemplateModel(H.StateMatrix.create(2, K, np.log(pp), True), np.asfortranarray(args[0][:, 0, :]), 1.0)
    lists = H.extract_spiketimes(H.fit(tm, white[c], 100_000))
    assert np.array_equal(f["footprint"], H.footprints(white, lists, pre=5, W=K).mean)
    # without whiten: the keys of before
    plain = H.sort_data(temps[:, None, :], [1 / 900.0], pp, raw, dosave=False, preprocess=pre, channel=c)
    assert sorted(plain) == ["ll", "lp", "mlseq", "sigma", "waveforms"]
    # local whitening through the driver: neighbours by channel index
    loc = H.sort_data(*args, raw, dosave=False, preprocess=dict(pre, whiten=dict(neighbors=3)), channel=c)
    assert loc["whitening"]["nbr"].shape == (5, 3) and loc["whitening"]["nbr"][c].tolist() == [3, 2, 4]
    # learn_templates
    learned = H.learn_templates(raw, 2, K, nsteps=1, preprocess=dict(pre, whiten=True), channel=c)
    again = H.learn_templates(white[c], 2, K, nsteps=1)
    assert sorted(learned) == sorted(list(again) + ["whitening"])
    assert all(np.array_equal(learned[k], again[k]) for k in again)
    assert np.array_equal(learned["whitening"]["w"], wh.w)
    assert sorted(H.learn_templates(raw, 2, K, nsteps=1, preprocess=pre, channel=c)) == ["cinv", "p", "spikeForms"]
