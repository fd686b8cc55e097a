"""The front end on the device (csrc/preprocess.hip: zero-phase FIR filter, common reference) against the numpy model
of preprocess_model.py.  Every comparison is np.array_equal: the contract fixes the order and the rounding of every
operation, so the device result is the model's bit for bit (the sign of a zero aside, which == ignores).

Shapes: the filter's tile is 1024 samples, so T = 1023 / 1024 / 1025 are a tile and its neighbours, T = P + 1 a
recording barely longer than the halo, T = 4096 + P and 10 007 several tiles with a ragged last one; P = 4096 is a
halo four times the tile.  A sample-major slab holds 16 channels at most and fewer as P grows (3 at P = 256, 1 from
P = 1000 on), so C = 5, 8, 33 give slabs that do not divide C.  The reference kernels change at group sizes 4, 8 and
16 (registers) and above (LDS for the median, a two-pass loop for the mean), hence the sizes below."""
import ctypes as C

import numpy as np
import pytest

import preprocess_model as PM

pytestmark = pytest.mark.gpu

TYPES = (np.int16, np.int32, np.float32, np.float64)
P_LIST = (0, 1, 7, 64, 256, 1000, 4096)
C_LIST = (1, 2, 3, 5, 8, 33)
CHANNEL_MAJOR, SAMPLE_MAJOR = 0, 1


def t_list(P):
    return sorted(T for T in {P + 1, 1023, 1024, 1025, 4096 + P, 10007} if T >= P + 1)


PT_CASES = [(P, T) for P in P_LIST for T in t_list(P)]


def dyadic_half(P):
    """taps that are small multiples of 1/8: with integer samples every product and sum is exact in any order"""
    half = ((3 * np.arange(P + 1)) % 7 - 3) / 8.0
    half[0] = 0.5
    return half


def design_half(H, P):
    if P == 0:
        return np.array([0.75])
    if P < 4:
        return np.array([0.6, -0.3])[:P + 1] if P == 1 else np.array([0.6, -0.3, 0.1, 0.05])[:P + 1]
    return H.design_fir(30000.0, low=300.0, ntaps=2 * P + 1)[P:].copy()


def samples(rng, C_, T, dtype, integer):
    """(C, T) in the sample type: integers of three digits, or normal values (scaled and rounded for integer types)"""
    if integer:
        return rng.integers(-999, 1000, size=(C_, T)).astype(dtype)
    x = rng.standard_normal((C_, T)) * 3.0
    return np.round(x * 500.0).astype(dtype) if np.issubdtype(dtype, np.integer) else x.astype(dtype)


def block(x, layout):
    """the raw block of (C, T) samples as the C ABI takes it"""
    return np.ascontiguousarray(x.T) if layout == SAMPLE_MAJOR else np.ascontiguousarray(x)


def call(H, buf, layout, C_, T, half=None, ref=0, group=None, keep=None, out=None, stype=None, P=None):
    """hmmsort_preprocess as it is; returns (code, out)"""
    L = H._lib
    half = None if half is None else np.ascontiguousarray(half, dtype=np.float64)
    grp = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    kp = None if keep is None else np.ascontiguousarray(keep, dtype=np.int32)
    if P is None:                                        # P given: a `half` field that disagrees with the array
        P = 0 if half is None else len(half) - 1
    opt = L.PreOpt(None if half is None else half.ctypes.data, P, ref, None if grp is None else grp.ctypes.data,
                   None if kp is None else kp.ctypes.data, 0 if kp is None else len(kp))
    if out is None:
        out = np.full((C_ if kp is None else len(kp), T), np.nan)
    if stype is None:
        stype = [np.dtype(t) for t in TYPES].index(buf.dtype)      # HMMSORT_SAMPLES_I16 .. F64 are 0 .. 3
    rc = L.lib().hmmsort_preprocess(L.ptr(buf), stype, layout, C_, T, C.byref(opt), L.ptr(out))
    return rc, out


def run(H, x, layout, half=None, ref=0, group=None, keep=None):
    rc, out = call(H, block(x, layout), layout, x.shape[0], x.shape[1], half, ref, group, keep)
    assert rc == 0, H._lib.last_error()
    return out


REFS = {None: 0, "median": 1, "mean": 2}


# ---- filter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,T", PT_CASES)
def test_filter_every_halo_and_length(H, P, T):
    """every (P, T); layout, sample type and C rotate so that each value occurs with small and large halos"""
    k = PT_CASES.index((P, T))
    layout, dtype = k % 2, TYPES[(k // 2) % 4]
    C_ = (1, 2, 3)[k % 3] if P >= 1000 else C_LIST[k % 6]
    rng = np.random.default_rng(100 + k)
    xi = samples(rng, C_, T, dtype, True)
    assert np.array_equal(run(H, xi, layout, dyadic_half(P)), PM.preprocess(xi, dyadic_half(P))), "indexing"
    xn = samples(rng, C_, T, dtype, False)
    assert np.array_equal(run(H, xn, layout, design_half(H, P)), PM.preprocess(xn, design_half(H, P))), "rounding"


@pytest.mark.parametrize("layout", (CHANNEL_MAJOR, SAMPLE_MAJOR))
@pytest.mark.parametrize("dtype", TYPES)
def test_filter_every_layout_type_and_channel_count(H, layout, dtype):
    rng = np.random.default_rng(7)
    for C_ in C_LIST:
        for P, T in ((7, 1025), (256, 2500)):
            xi = samples(rng, C_, T, dtype, True)
            assert np.array_equal(run(H, xi, layout, dyadic_half(P)), PM.preprocess(xi, dyadic_half(P))), (C_, P)
            xn = samples(rng, C_, T, dtype, False)
            assert np.array_equal(run(H, xn, layout, design_half(H, P)), PM.preprocess(xn, design_half(H, P))), (C_, P)


def test_no_fused_multiply_add(H):
    """the data on which a fused acc + h * s differs from the two-step one in most samples: were the device to fuse,
    the equality above would be luck; here the difference is shown to exist"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, 4096))
    half = design_half(H, 64)
    got = run(H, x, CHANNEL_MAJOR, half)
    assert np.array_equal(got, PM.fir(x, half))
    xe = x[0, PM.mirror_index(4096, 64)].astype(np.longdouble)
    acc = np.float64(half[0]) * x[0]
    for j in range(1, 65):   # every step with the product kept exact until the addition (what an FMA computes)
        s = (xe[64 - j:64 - j + 4096].astype(np.float64) + xe[64 + j:64 + j + 4096].astype(np.float64))
        acc = (acc.astype(np.longdouble) + np.longdouble(half[j]) * s.astype(np.longdouble)).astype(np.float64)
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert np.count_nonzero(acc != got[0]) > 1000


def test_non_finite_samples_stay_inside_the_window(H):
    x = np.zeros((2, 3000))
    x[0, 1500], x[1, 10] = np.inf, np.nan
    half = design_half(H, 7)          # P = 7 is no multiple of the lag block: the taps beyond it must not be used
    got = run(H, x, SAMPLE_MAJOR, half)
    bad = ~np.isfinite(got)
    assert np.array_equal(np.nonzero(bad[0])[0], np.arange(1493, 1508))
    assert np.array_equal(np.nonzero(bad[1])[0], np.arange(3, 18))
    assert np.all(got[~bad] == 0)


# ---- identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TYPES)
def test_identity_is_the_widening_and_a_transposition(H, dtype):
    import torch
    rng = np.random.default_rng(5)
    L = H._lib
    for C_, T in ((1, 1), (3, 1025), (5, 4097)):
        x = samples(rng, C_, T, dtype, np.issubdtype(dtype, np.integer))
        for layout in (CHANNEL_MAJOR, SAMPLE_MAJOR):
            out = run(H, x, layout)
            assert np.array_equal(out, x.astype(np.float64))
            d_raw = torch.from_numpy(block(x, layout)).cuda()
            d_out = H.device.preprocess(d_raw, layout)
            assert d_out.shape == (C_, T) and np.array_equal(d_out.cpu().numpy(), out)
            # hmmsort_samples_to_f64 of every channel
            d_w = torch.empty(T, dtype=torch.float64, device="cuda")
            for c in range(C_):
                first, stride = (c, C_) if layout == SAMPLE_MAJOR else (c * T, 1)
                L.check(L.lib().hmmsort_samples_to_f64(C.c_void_p(d_raw.data_ptr() + first * x.itemsize),
                                                       int(TYPES.index(dtype)), T, stride,
                                                       C.c_void_p(d_w.data_ptr()), None))
                torch.cuda.synchronize()
                assert np.array_equal(d_w.cpu().numpy(), out[c])


# ---- reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("median", "mean"))
@pytest.mark.parametrize("G", (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64))
def test_reference_group_sizes(H, mode, G):
    rng = np.random.default_rng(20 + G)
    T = 1000                                            # no multiple of a workgroup
    for x in (rng.integers(-3, 4, size=(G, T)).astype(np.int16), rng.standard_normal((G, T))):
        got = run(H, x, SAMPLE_MAJOR, None, REFS[mode])
        assert np.array_equal(got, PM.preprocess(x, None, mode)), G
        again = run(H, x, SAMPLE_MAJOR, None, REFS[mode])
        assert got.tobytes() == again.tobytes()
    if G == 1:
        assert np.all(got == 0)


@pytest.mark.parametrize("mode", ("median", "mean"))
def test_reference_groups_exclusions_and_ties(H, mode):
    rng = np.random.default_rng(31)
    T = 777
    x = rng.standard_normal((12, T))
    x[:, 100:200] = 2.5                                 # all-equal columns
    x[:, 300:400] = rng.integers(0, 2, size=(12, 100))  # two values only
    half = design_half(H, 64)
    for group in ([0, 1] * 6, [0, 1, 2] * 4, [3, -1, 3, 7, -5, 7, 3, 3, -1, 7, 9, 3], None):
        got = run(H, x, SAMPLE_MAJOR, half, REFS[mode], group)
        assert np.array_equal(got, PM.preprocess(x, half, mode, group)), group
    flat = run(H, x, CHANNEL_MAJOR, None, REFS[mode])
    assert np.all(flat[:, 100:200] == 0)


def test_mean_takes_a_group_the_median_refuses(H):
    rng = np.random.default_rng(32)
    x = rng.integers(-100, 100, size=(100, 300)).astype(np.int32)
    assert np.array_equal(run(H, x, SAMPLE_MAJOR, None, 2), PM.preprocess(x, None, "mean"))
    group = [0] * 64 + [1] * 36
    assert np.array_equal(run(H, x, SAMPLE_MAJOR, None, 1, group), PM.preprocess(x, None, "median", group))


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals(H):
    L = H._lib
    x = np.arange(40, dtype=np.float64).reshape(4, 10)
    buf = block(x, SAMPLE_MAJOR)
    half8, long_half = np.ones(9), np.ones(4098)
    big = np.zeros(5000)
    cases = [
        (dict(C_=0), L.EINVAL, "C = 0"), (dict(C_=1025), L.EINVAL, "C = 1025"),
        (dict(T=0), L.EINVAL, "T = 0"), (dict(T=8, half=half8), L.EINVAL, "half"),
        (dict(buf=big, C_=1, T=5000, half=long_half), L.EINVAL, "half = 4097"),
        (dict(half=half8, P=-1), L.EINVAL, "half = -1"),
        (dict(stype=4), L.EINVAL, "sample_type"), (dict(stype=-1), L.EINVAL, "sample_type"),
        (dict(layout=2), L.EINVAL, "layout"), (dict(ref=3), L.EINVAL, "reference"),
        (dict(keep=[0, 4]), L.EINVAL, "keep[1] = 4"), (dict(keep=[-1]), L.EINVAL, "keep[0] = -1"),
        (dict(buf=np.zeros((3, 65)), C_=65, T=3, ref=1), L.EUNSUP, "group 0"),
        (dict(buf=np.zeros((3, 70)), C_=70, T=3, ref=1, group=[5] * 65 + [-1] * 5), L.EUNSUP, "group 5"),
    ]
    for kw, code, word in cases:
        a = dict(buf=buf, layout=SAMPLE_MAJOR, C_=4, T=10)
        a.update(kw)
        out = np.full((max(a["C_"], 1), max(a["T"], 1)), np.nan)
        rc, out = call(H, a.pop("buf"), a.pop("layout"), a.pop("C_"), a.pop("T"), out=out, **a)
        assert rc == code, (kw, rc, L.last_error())
        assert word in L.last_error() and "preprocess" in L.last_error(), (kw, L.last_error())
        assert np.all(np.isnan(out)), kw
    # null arguments
    opt = L.PreOpt(None, 0, 0, None, None, 0)
    out = np.full((4, 10), np.nan)
    assert L.lib().hmmsort_preprocess(None, 3, 1, 4, 10, C.byref(opt), L.ptr(out)) == L.EINVAL
    assert "in" in L.last_error() and np.all(np.isnan(out))
    assert L.lib().hmmsort_preprocess(L.ptr(buf), 3, 1, 4, 10, C.byref(opt), None) == L.EINVAL
    assert "out" in L.last_error()
    # overlapping ranges: the output starts inside the input
    both = np.full(200, np.nan)
    assert L.lib().hmmsort_preprocess(C.c_void_p(both.ctypes.data), 3, 1, 4, 10, C.byref(opt),
                                      C.c_void_p(both.ctypes.data + 8 * 39)) == L.EINVAL
    assert "overlap" in L.last_error() and np.all(np.isnan(both))
    assert L.lib().hmmsort_preprocess(C.c_void_p(both.ctypes.data + 8 * 39), 3, 1, 4, 10, C.byref(opt),
                                      C.c_void_p(both.ctypes.data)) == L.EINVAL
    # no options at all: the widening
    assert L.lib().hmmsort_preprocess(L.ptr(buf), 3, 1, 4, 10, None, L.ptr(out)) == 0
    assert np.array_equal(out, x)


def test_device_form_refusals(H):
    import torch
    L = H._lib
    d = torch.full((4, 10), float("nan"), dtype=torch.float64, device="cuda")
    opt = L.PreOpt(None, 0, 0, None, None, 0)
    f = L.lib().hmmsort_preprocess_device
    p = C.c_void_p(d.data_ptr())
    assert f(p, 3, 0, 4, 10, C.byref(opt), p, None) == L.EINVAL and "overlap" in L.last_error()
    assert f(None, 3, 0, 4, 10, C.byref(opt), p, None) == L.EINVAL and "in" in L.last_error()
    d_in = torch.zeros((3, 65), dtype=torch.float64, device="cuda")
    d_out = torch.full((65, 3), float("nan"), dtype=torch.float64, device="cuda")
    opt = L.PreOpt(None, 0, 1, None, None, 0)
    assert f(C.c_void_p(d_in.data_ptr()), 3, 1, 65, 3, C.byref(opt), C.c_void_p(d_out.data_ptr()), None) == L.EUNSUP
    assert "group 0" in L.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(d).all()) and bool(torch.isnan(d_out).all())


# ---- host and device form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", (CHANNEL_MAJOR, SAMPLE_MAJOR))
def test_host_and_device_form_agree_and_keep_selects_rows(H, layout):
    import torch
    rng = np.random.default_rng(41)
    x = samples(rng, 5, 4097, np.int16, False)
    full = H.design_fir(30000.0, low=300.0, high=6000.0, ntaps=129)
    group = [0, 0, -1, 0, 0]
    raw = np.ascontiguousarray(x.T) if layout == SAMPLE_MAJOR else np.asfortranarray(x.T)    # (T, C) either way
    for ref in (None, "median", "mean"):
        host = H.preprocess(raw, full, ref, group)
        assert np.array_equal(host, PM.preprocess(x, full[64:], ref, group))
        d_raw = torch.from_numpy(block(x, layout)).cuda()
        dev = H.device.preprocess(d_raw, layout, full, ref, group)
        assert dev.cpu().numpy().tobytes() == host.tobytes()
        for keep in ([3], [4, 0, 0], [2]):
            part = H.preprocess(raw, full, ref, group, keep=keep)
            assert part.shape == (len(keep), 4097) and part.tobytes() == host[keep].tobytes(), (ref, keep)
    one = H.preprocess(x[1], full)                       # 1-D: one channel
    assert one.shape == (1, 4097) and np.array_equal(one[0], H.preprocess(raw, full)[1])


# ---- end to end ----------------------------------------------------------------------------------------------------
def _recording(H, seed, K=60, T=40_000):
    from conftest import two_templates
    temps = two_templates(H, K)
    pp = [0.003, 0.002]
    y, onsets = H.create_signal(T, 0.3, pp, temps, seed=seed, return_states=True)
    t = np.arange(T)
    y = y + (3.0 * np.sin(2 * np.pi * 50.0 * t / 30000.0) + 2.0 * t / T)
    troughs = [(o + int(np.argmin(temps[:, j])) + 1, j) for o, j in onsets if o + K <= T]   # 1-based
    return temps, pp, y, troughs


def _found(H, tm, signal, troughs):
    """true spikes with an extracted time of their own template within +-2 samples of their trough, and the number of
    extracted events of all templates"""
    times = H.extract_spiketimes(H.fit(tm, signal, None))
    hit = sum(1 for q, j in troughs if len(times[j]) and np.abs(times[j] - q).min() <= 2)
    return hit, sum(len(t) for t in times)


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_end_to_end_drift_and_hum(H, seed):
    """a clean channel plus 50 Hz hum and a ramp, as a (T, 1) block, decoded whole with the two true templates as a
    ring model: behind sort_data's front end with a 300 Hz high-pass every true spike is found and nothing else;
    without it fewer than 3/4 are.  (sort_data itself decodes with the overlap model, whose unconstrained first
    state may add an event at sample 1; that it sorts the front end's output is the next test.)"""
    temps, pp, y, troughs = _recording(H, seed)
    tm = H.HMMSpikeTemplateModel(H.StateMatrix.create(2, temps.shape[0], np.log(pp), False), temps, 0.3)
    clean = H.sortdata.front_end(y[:, None], dict(fs=30000, low=300, ntaps=257), 0)
    assert clean.shape == y.shape
    hit, n = _found(H, tm, clean, troughs)
    hit0, n0 = _found(H, tm, y, troughs)
    print("seed %d: %d true spikes; with the front end %d found, %d events; without %d found, %d events"
          % (seed, len(troughs), hit, n, hit0, n0))
    assert hit == len(troughs) and n == len(troughs)
    assert hit0 < 0.75 * len(troughs)


def test_sort_data_on_a_raw_block_equals_sort_data_on_the_front_end_output(H):
    from conftest import two_templates
    K, T, c = 20, 6000, 3
    temps = two_templates(H, K) * 100.0
    pp = [0.004, 0.003]
    rng = np.random.default_rng(9)
    chans = [H.create_signal(T, 30.0, pp, temps, seed=10 + i) for i in range(5)]
    common = 200.0 * np.sin(2 * np.pi * 50.0 * np.arange(T) / 30000.0) + 40.0 * rng.standard_normal(T)
    raw = np.ascontiguousarray(np.round(np.stack(chans, axis=1) + common[:, None]).astype(np.int16))   # (T, 5)
    pre = dict(fs=30000, low=300, ntaps=129, reference="median")
    args = (temps[:, None, :], [1 / 900.0], pp)
    a = H.sort_data(*args, raw, dosave=False, preprocess=pre, channel=c)
    clean = H.preprocess(raw, H.design_fir(30000, low=300, ntaps=129), "median")[c]
    b = H.sort_data(*args, clean, dosave=False)
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert (a["mlseq"] > 1).any()
    with pytest.raises(ValueError):
        H.sort_data(*args, raw, dosave=False, channel=2)
    learned = H.learn_templates(raw, 2, K, nsteps=1, preprocess=pre, channel=c)
    again = H.learn_templates(clean, 2, K, nsteps=1)
    assert all(np.array_equal(learned[k], again[k]) for k in learned)
