"""hmmsort_unit_stability and its device and plan forms against the numpy model tests/stability_model.py:
every table must come out equal byte for byte (NaN in the same places), from the host form, the device form, the plan
form on every engine, api.unit_stability and sort_data.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import fit_adaptive_model as FA
import stability_model as SM
from conftest import to_oracle_sm

pytestmark = pytest.mark.gpu

TABLES = ("n", "count", "valid", "quant", "sum", "sumsq", "uvalid", "uquant", "umin", "umax", "usum", "usumsq", "hist",
          "under", "over")
# the wave, tile, LDS-capacity and multi-pass edges: one wave serves 64 keys, a sum tile holds 256, a workgroup sweeps
# 2 048 keys in LDS and re-reads a longer range from memory in every pass
EDGES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049)
LONG = 70_003


def same(got, want, what=""):
    for k in TABLES:
        g, w = getattr(got, k), getattr(want, k)
        if w is None:
            assert g is None, (what, k)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        if g.dtype == np.int64:
            bad = np.argwhere(g != w)
        else:
            gn, wn = np.isnan(g), np.isnan(w)
            bad = np.argwhere((gn != wn) | (~gn & ~wn & (g.view(np.uint64) != w.view(np.uint64))))
        assert len(bad) == 0, (what, k, bad[:4].tolist(), g[tuple(bad[:4].T)], w[tuple(bad[:4].T)])


def unit_of(rng, lengths, bin, kind):
    """one unit with lengths[b] spikes in time bin b, and its values"""
    t, v = [], []
    for b, n in enumerate(lengths):
        t.append(b * bin + 1 + np.sort(rng.choice(bin, n, replace=False)))
        v.append(values_of(rng, n, kind))
    return np.concatenate(t).astype(np.int64), np.concatenate(v)


def values_of(rng, n, kind):
    if kind == "equal":                       # the ranks fall among equal keys
        return np.full(n, rng.standard_normal())
    if kind == "nan":
        return np.full(n, np.nan)
    if kind == "special":                     # mixed signs, subnormals, signed zeros, infinities
        pool = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2e-308, -1e-310, np.inf, -np.inf, 1.0, -1.0, 1e300, -1e300, 3.5])
        return pool[rng.integers(0, len(pool), n)]
    v = np.round(rng.standard_t(2, n), 1)     # heavy tail with ties
    v[rng.random(n) < 0.1] = np.nan
    v[rng.random(n) < 0.05] = 0.0
    v[rng.random(n) < 0.05] = -0.0
    return v


def model_and_host(H, times, values, T, bin, quantiles, hist):
    q_num, q_den = H.quantile_fractions(quantiles)
    mh = None if hist is None else (hist[0], hist[1], float(np.float64(hist[0]) / (np.float64(hist[2]) - hist[1])))
    want = SM.unit_stability(times, values, T, bin, q_num, q_den, mh)
    got = H.unit_stability(times, values, T=T, bin=bin, quantiles=quantiles, hist=hist)
    return got, want


def device_form(H, times, values, T, bin, quantiles, hist, lead=3):
    """the same lists resident, behind offsets that do not start at 0"""
    import torch
    offs = lead + np.concatenate([[0], np.cumsum([len(t) for t in times])]).astype(np.int64)
    dt = torch.from_numpy(np.concatenate([np.full(lead, -7, dtype=np.int64)] + list(times))).cuda()
    dv = None
    if values is not None:
        dv = torch.from_numpy(np.concatenate([np.full(lead, 1e9)] + list(values))).cuda()
    return H.device.unit_stability(dt, offs, dv, T=T, bin=bin, quantiles=quantiles, hist=hist)


@pytest.fixture(scope="module")
def long_unit():
    """every edge length and one segment of about 70 000 values in one unit, heavy-tailed values"""
    rng = np.random.default_rng(18)
    lengths = EDGES + (LONG, 300)
    bin = 70_010
    t, v = unit_of(rng, lengths, bin, "heavy")
    t[0] = bin + 1                                     # the first spike of bin 1 sits on the bin's first sample
    T = len(lengths) * bin - 1000                      # not a multiple of bin
    t = t[t <= T]
    return [t], [v[:len(t)]], T, bin


def test_edge_lengths_one_unit(H, long_unit):
    times, values, T, bin = long_unit
    got, want = model_and_host(H, times, values, T, bin, (0.25, 0.5, 0.75), (64, -8.0, 8.0))
    same(got, want, "host form")
    assert want.count[0, :12].tolist() == list(EDGES) and want.count[0, 12] == LONG
    assert want.valid[0, 12] < LONG and np.isnan(want.quant[0, 0]).all() and want.uvalid[0] > 60_000
    same(device_form(H, times, values, T, bin, (0.25, 0.5, 0.75), (64, -8.0, 8.0)), want, "device form")
    again = H.unit_stability(times, values, T=T, bin=bin, hist=(64, -8.0, 8.0))
    assert all(getattr(got, k).tobytes() == getattr(again, k).tobytes() for k in TABLES)


def test_eight_quantiles_of_a_denominator_that_is_no_power_of_two(H, long_unit):
    times, values, T, bin = long_unit
    qs = tuple(k / 7 for k in range(8))
    assert H.quantile_fractions(qs) == (tuple(range(8)), 7)
    got, want = model_and_host(H, times, values, T, bin, qs, None)
    same(got, want, "nq = 8")
    ok = want.uvalid > 0
    assert np.array_equal(want.uquant[ok, 0], want.umin[ok]) and np.array_equal(want.uquant[ok, 7], want.umax[ok])
    assert got.hist.shape == (1, 0)                    # HB = 0
    got0, want0 = model_and_host(H, times, values, T, bin, (), None)
    same(got0, want0, "nq = 0")
    assert got0.quant.shape == want0.count.shape + (0,)


def test_two_units_equal_values_and_all_nan(H):
    rng = np.random.default_rng(19)
    lengths, bin = (1, 2, 64, 65, 257, 2049, 300), 2100
    T = len(lengths) * bin
    t0, v0 = unit_of(rng, lengths, bin, "equal")
    t1, v1 = unit_of(rng, lengths[::-1], bin, "nan")
    t1[-1] = T                                          # a spike on the last sample
    for form in (model_and_host, None):
        if form:
            got, want = form(H, [t0, t1], [v0, v1], T, bin, (0.1, 0.5, 1.0), (16, -3.0, 3.0))
        else:
            got = device_form(H, [t0, t1], [v0, v1], T, bin, (0.1, 0.5, 1.0), (16, -3.0, 3.0))
        same(got, want, "equal / nan")
    assert not want.valid[1].any() and np.isnan(want.quant[1]).all() and np.isnan(want.umin[1])
    assert not want.usum[1] and not want.hist[1].any() and want.uvalid[1] == 0
    assert (want.quant[0, :, 0] == want.quant[0, :, 2]).all()


def test_five_units_empty_ones_and_special_values(H):
    rng = np.random.default_rng(20)
    lengths, bin = (257, 0, 65, 2, 1, 700), 1000
    T = len(lengths) * bin - 300                        # the last bin is short
    t1, v1 = unit_of(rng, lengths[:5] + (400,), bin, "special")
    t3, v3 = unit_of(rng, (0, 3, 0, 0, 64, 0), bin, "heavy")
    t1, v1 = t1[t1 < T], v1[t1 < T]
    t1[0], t1[-1] = 1, T                               # spikes on the first and the last sample
    e = np.zeros(0, dtype=np.int64)
    times, values = [e, t1, e, t3, e], [np.zeros(0), v1, np.zeros(0), v3, np.zeros(0)]
    got, want = model_and_host(H, times, values, T, bin, (0.0, 1 / 3, 0.5, 0.9), (8, -1.0, 1.0))
    same(got, want, "five units")
    assert want.n.tolist() == [0, len(t1), 0, len(t3), 0] and np.isnan(want.usum[1])   # +Inf and -Inf meet
    same(device_form(H, times, values, T, bin, (0.0, 1 / 3, 0.5, 0.9), (8, -1.0, 1.0)), want, "five units, device")
    # counts alone
    got, want = model_and_host(H, times, None, T, bin, (0.5,), None)
    same(got, want, "values = NULL")
    assert got.valid is None and got.count.sum() == len(t1) + len(t3)
    same(device_form(H, times, None, T, bin, (0.5,), None), want, "values = NULL, device")


def test_bin_of_one_sample_and_one_bin(H):
    rng = np.random.default_rng(21)
    T = 97
    times = [np.array([1, 2, 50, 96, 97], dtype=np.int64), np.sort(rng.choice(T, 40, replace=False)).astype(np.int64) + 1]
    values = [values_of(rng, 5, "special"), values_of(rng, 40, "heavy")]
    got, want = model_and_host(H, times, values, T, 1, (0.5,), (4, -2.0, 2.0))
    same(got, want, "bin = 1")
    assert want.count.shape == (2, T) and want.count[0, 0] == want.count[0, 96] == 1 and want.count.max() == 1
    for bin in (T, T + 5, 1 << 40):
        got, want = model_and_host(H, times, values, T, bin, (0.5,), (4, -2.0, 2.0))
        same(got, want, "B = 1")
        assert want.count.shape == (2, 1)
    # the bins are cut at (t - 1) / bin: sample `bin` is the last of bin 0
    got, want = model_and_host(H, [np.array([10, 11, 20, 21], dtype=np.int64)], None, 30, 10, (), None)
    same(got, want, "cut")
    assert got.count.tolist() == [[1, 2, 1]]


def test_histogram_edges_under_and_over(H):
    HB, lo, hi = 4096, -2.0, 2.0
    edges = lo + np.arange(HB) / 1024.0                 # every left edge, exactly
    extra = np.array([-3.0, -np.inf, np.nextafter(lo, -9.0), hi, np.nextafter(hi, 0.0), 5.0, np.inf, np.nan, -0.0])
    v = np.concatenate([edges, extra, edges[::7]])
    t = np.arange(1, len(v) + 1, dtype=np.int64) * 3
    got, want = model_and_host(H, [t], [v], 3 * len(v), 5000, (0.5,), (HB, lo, hi))
    same(got, want, "histogram")
    # the value just below hi is over as well: (v - lo) rounds up to 4.0, and the contract rounds the difference first
    assert want.under[0] == 3 and want.over[0] == 4 and want.hist[0].sum() == len(v) - 8
    assert want.hist[0, 0] == 2 and want.hist[0, 4095] == 2 and want.hist[0, 2048] == 2 and want.hist[0].min() == 1


# ---- refusals -----------------------------------------------------------------------------------------------------
FILL_I, FILL_F = -77, 123.25


def raw(H, times, values=None, T=100, bin=10, q_num=(1, 2, 3), q_den=4, nq=None, HB=4, lo=0.0, scale=1.0, U=None,
        n=True, opt=True, counts=None):
    """hmmsort_unit_stability with every output filled beforehand -> rc; a call that refuses must not have written"""
    L = H._lib
    times = [np.ascontiguousarray(t, dtype=np.int64) for t in times]
    U = len(times) if U is None else U
    ptrs = (C.c_void_p * max(len(times), 1))(*[t.ctypes.data if len(t) else None for t in times])
    vptrs = None
    if values is not None:
        values = [np.ascontiguousarray(v, dtype=np.float64) for v in values]
        vptrs = (C.c_void_p * max(len(values), 1))(*[v.ctypes.data if len(v) else None for v in values])
    cnt = np.array([len(t) for t in times] + [0], dtype=np.int64) if counts is None else np.array(counts, dtype=np.int64)
    bufs = {k: (np.full(4096, FILL_I, dtype=np.int64) if k in ("n", "count", "valid", "uvalid", "hist", "under", "over")
                else np.full(4096, FILL_F)) for k, _ in L.StabOut._fields_}
    o = L.StabOpt(T, bin, len(q_num) if nq is None else nq, (C.c_int64 * 8)(*q_num[:8]), q_den, HB, lo, scale)
    out = L.StabOut(*[bufs[k].ctypes.data if (n or k != "n") else None for k, _ in L.StabOut._fields_])
    rc = L.lib().hmmsort_unit_stability(U, ptrs, vptrs, L.ptr(cnt), C.byref(o) if opt else None, C.byref(out))
    untouched = all((b == (FILL_I if b.dtype == np.int64 else FILL_F)).all() for b in bufs.values())
    assert rc == 0 or untouched
    return rc


def test_refusals(H):
    L = H._lib
    ok = [np.array([3, 9, 10]), np.array([4])]
    okv = [np.array([1.0, np.nan, 2.0]), np.array([0.5])]

    def refused(code, *words, **kw):
        rc = raw(H, kw.pop("times", ok), kw.pop("values", okv), **kw)
        assert rc == code and all(w in L.last_error() for w in words), (rc, L.last_error())

    refused(L.EINVAL, "null", n=False)
    refused(L.EINVAL, "null", opt=False)
    rc = L.lib().hmmsort_unit_stability(2, None, None, None, None, None)
    assert rc == L.EINVAL and "null" in L.last_error()
    refused(L.EINVAL, "U = 0", U=0)
    refused(L.EINVAL, "U = 4097", times=[ok[1]] * 4097, values=None)
    refused(L.EINVAL, "T = 0", T=0)
    refused(L.EINVAL, "T = %d" % ((1 << 40) + 1), T=(1 << 40) + 1)
    refused(L.EINVAL, "bin = 0", bin=0)
    refused(L.EUNSUP, "B = %d" % ((1 << 24) + 1), T=(1 << 24) + 1, bin=1)
    refused(L.EUNSUP, "%d segments" % (2 * (1 << 23) + 2), T=(1 << 23) + 1, bin=1)
    refused(L.EINVAL, "nq = 9", nq=9)
    refused(L.EINVAL, "nq = -1", nq=-1)
    refused(L.EINVAL, "q_den = 0", q_den=0)
    refused(L.EINVAL, "q_den = %d" % ((1 << 20) + 1), q_den=(1 << 20) + 1)
    refused(L.EINVAL, "q_num[1] = 5", q_num=(1, 5, 3))
    refused(L.EINVAL, "q_num[0] = -1", q_num=(-1, 2, 3))
    refused(L.EINVAL, "counts", "unit 1", counts=[3, -1, 0])
    refused(L.EINVAL, "times", "unit 0", "time 0", times=[np.array([0, 7]), ok[1]], values=[okv[0][:2], okv[1]])
    refused(L.EINVAL, "times", "unit 0", "time 101", "T = 100", times=[np.array([3, 9, 101]), ok[1]])
    refused(L.EINVAL, "times", "unit 1", "ascending", times=[ok[0], np.array([4, 4])], values=[okv[0], okv[0][:2]])
    refused(L.EINVAL, "HB = 4097", HB=4097)
    refused(L.EINVAL, "HB = -1", HB=-1)
    for bad in (0.0, -1.0, np.inf, np.nan):
        refused(L.EINVAL, "hist_scale", scale=bad)
    refused(L.EINVAL, "hist_lo", lo=np.inf)
    assert raw(H, ok, okv, scale=np.nan, HB=0) == 0           # without a histogram its numbers are not looked at
    with pytest.raises(H.HmmsortError) as e:
        H.unit_stability([ok[0], [5, 5]], T=100, bin=10)
    assert e.value.code == L.EINVAL and "unit 1" in str(e.value)
    with pytest.raises(H.HmmsortError) as e:
        H.unit_stability(ok, okv, T=100, bin=10, quantiles=tuple(k / 9 for k in range(9)))
    assert e.value.code == L.EINVAL and "nq = 9" in str(e.value)
    assert raw(H, ok, okv) == 0 and raw(H, ok, None) == 0    # and the lists the refusals varied are taken


# ---- the plan form ------------------------------------------------------------------------------------------------
N_P, K_P, T_P, PP_P, SG_P = 2, 20, 6000, (0.012, 0.009), 0.3
OPTS_P = dict(bin=700, quantiles=(0.25, 0.5, 0.75), hist=(32, 0.0, 2.0))


def templates_p(H, scale=1.0):
    return np.asfortranarray(np.stack([H.create_spike_template(K_P, 3.0, 0.8, 0.2),
                                       H.create_spike_template(K_P, 4.0, 0.3, 0.2)], axis=1) * scale)


def plan_reference(H, plan, dy, dx, nC):
    """the model fed with extract_spiketimes and spike_fit's amp of the same plan"""
    fits = plan.spike_fit(dy, dx)
    fits = fits if nC > 1 else [fits]
    times = [f.times for ch in fits for f in ch]
    amps = [f.amp for ch in fits for f in ch]
    if nC == 1:
        ex = plan.extract_spiketimes(dx)
        assert all(np.array_equal(a, b) for a, b in zip(ex, times))
    q_num, q_den = H.quantile_fractions(OPTS_P["quantiles"])
    return SM.unit_stability(times, amps, T_P, OPTS_P["bin"], q_num, q_den, (32, 0.0, 16.0)), times


@pytest.mark.parametrize("engine", ["WAVE", "RING", "BLOCKED", "STRICT"])
def test_plan_form_on_every_engine(H, engine):
    import torch
    sm = H.StateMatrix.create(N_P, K_P, np.log(PP_P), False)
    mu = templates_p(H)
    y = H.create_signal(T_P, SG_P, PP_P, mu, seed=180)
    H.set_option("engine", getattr(H, "ENGINE_" + engine))
    try:
        plan = H.Plan(T_P, sm, mu, SG_P)
        assert plan.info()["engine"] == getattr(H, "ENGINE_" + engine)
        dy = torch.from_numpy(y).cuda()
        dx = torch.zeros(T_P, dtype=torch.int16, device="cuda")
        plan.viterbi(dy, dx, torch.zeros(1, dtype=torch.float64, device="cuda"))
        got = plan.unit_stability(dy, dx, **OPTS_P)
        got2 = plan.unit_stability(dy, dx, stream=torch.cuda.current_stream().cuda_stream, **OPTS_P)
        want, times = plan_reference(H, plan, dy, dx, 1)
        plan.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    same(got, want, engine)
    same(got2, want, engine + ", stream")
    assert all(len(t) > 15 for t in times) and (want.valid > 0).sum() > 12


def test_plan_form_batched_and_int16(H):
    import torch
    nC = 3
    sm = H.StateMatrix.create(N_P, K_P, np.log(PP_P), False)
    mus = [templates_p(H, 100.0), templates_p(H, 130.0)[:, ::-1].copy(order="F"), templates_p(H, 90.0)]
    raw_y = np.stack([np.round(H.create_signal(T_P, 100 * SG_P, PP_P, mus[c], seed=190 + c)) for c in range(nC)])
    raw_y = raw_y.astype(np.int16)
    L = H._lib
    H.set_option("engine", H.ENGINE_WAVE)
    try:
        plan = H.Plan.batched(T_P, [sm] * nC, mus, [100 * SG_P] * nC)
        d_raw = torch.from_numpy(raw_y).cuda()
        dy = torch.empty((nC, T_P), dtype=torch.float64, device="cuda")
        L.check(L.lib().hmmsort_samples_to_f64(d_raw.data_ptr(), L.SAMPLES_I16, nC * T_P, 1, dy.data_ptr(), None))
        assert np.array_equal(dy.cpu().numpy(), raw_y.astype(np.float64))
        dx = torch.zeros((nC, T_P), dtype=torch.int16, device="cuda")
        plan.viterbi(dy, dx, torch.zeros(nC, dtype=torch.float64, device="cuda"))
        got = plan.unit_stability(dy, dx, **OPTS_P)
        want, times = plan_reference(H, plan, dy, dx, nC)
        with pytest.raises(H.HmmsortError) as e:
            L.check(L.lib().hmmsort_plan_unit_stability(plan._h, None, dx.data_ptr(), None, None, None))
        assert e.value.code == L.EINVAL and "null" in str(e.value)
        plan.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    same(got, want, "batched")
    assert got.count.shape == (nC * N_P, 9) and all(len(t) > 20 for t in times)


# ---- end to end: the drifting recording ---------------------------------------------------------------------------
# Fixed on the CPU first (the oracle's decode of D(2, g) with the fixed model, model spike fit, this file's model), then
# asserted exactly: the chain is bit-exact.  See test_drift_end_to_end's docstring for the figures.
def drift_case(H, g):
    import torch
    y, _onsets, temps = FA.drifting(H, 2, g)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False)
    plan = H.Plan(len(y), sm, temps, FA.SIGMA_D)
    try:
        dy = torch.from_numpy(y).cuda()
        dx = torch.zeros(len(y), dtype=torch.int16, device="cuda")
        plan.viterbi(dy, dx, torch.zeros(1, dtype=torch.float64, device="cuda"))
        st = plan.unit_stability(dy, dx, bin=len(y) // 3, quantiles=(0.5,), hist=(64, 0.0, 2.0))
        fits = plan.spike_fit(dy, dx)
    finally:
        plan.close()
    want = SM.unit_stability([f.times for f in fits], [f.amp for f in fits], len(y), len(y) // 3, (1,), 2,
                             (64, 0.0, 32.0))
    same(st, want, "drift %g" % g)
    return st, dx.cpu().numpy(), y, sm, temps


def test_drift_end_to_end(H, O):
    """The drifting recording of the fit_adaptive tests, amplitudes falling to 0.4 of their start, decoded with the
    fixed model: the per-bin median amplitude of each unit falls across the thirds of the recording, and
    amplitude_drift exceeds that of the same recording without drift.  The figures were fixed on the CPU first -- the
    oracle's decode, tests/spike_fit_model.py for the amplitudes, then tests/stability_model.py -- and are asserted
    exactly, since the chain is bit-exact:
      medians per third, with drift   [0.9089051623515765, 0.7111292490056746, 0.5809142046720049] (unit 0),
                                      [0.8889641508195584, 0.6828223664226923, 0.5585771218849775] (unit 1);
      amplitude_drift                 0.42805675735096005, 0.4488639641137055 with drift,
                                      0.012879935128319359, 0.008716755187322022 without."""
    st, x, y, sm, temps = drift_case(H, 0.4)
    flat, x1, y1, _, _ = drift_case(H, 1.0)
    for xx, yy in ((x, y), (x1, y1)):
        xo, _ = O.viterbi(yy, to_oracle_sm(O, sm), temps, FA.SIGMA_D)
        assert np.array_equal(xx, np.asarray(xo))
    med = st.quant[:, :, 0]
    d, d1 = st.amplitude_drift(), flat.amplitude_drift()
    print("medians per third", med.tolist(), "drift", d.tolist(), "without drift", d1.tolist())
    assert (st.valid >= 20).all() and (flat.valid >= 20).all()
    assert (med[:, 0] > med[:, 1]).all() and (med[:, 1] > med[:, 2]).all()
    assert (d > d1).all()
    assert med.tolist() == [[0.9089051623515765, 0.7111292490056746, 0.5809142046720049],
                            [0.8889641508195584, 0.6828223664226923, 0.5585771218849775]]
    assert d.tolist() == [0.42805675735096005, 0.4488639641137055]
    assert d1.tolist() == [0.012879935128319359, 0.008716755187322022]
    assert np.array_equal(d, SM.amplitude_drift(st)) and np.array_equal(d1, SM.amplitude_drift(flat))
    assert np.array_equal(st.presence_ratio(), [1.0, 1.0])
    assert np.array_equal(st.amplitude_cutoff(), SM.amplitude_cutoff(st))
    assert np.array_equal(st.firing_rate(30_000.0), SM.firing_rate(st, 30_000.0))


# ---- sort_data ----------------------------------------------------------------------------------------------------
def test_sort_data_switch(H):
    y, _onsets, temps = FA.drifting(H, 2, 0.4)
    T = 15_000
    raw_y = np.round(y[:T] * 1000).astype(np.int16)
    spike_forms = np.zeros((FA.K_D, 1, 2))
    spike_forms[:, 0, :] = temps * 1000
    args = (spike_forms, [1.0 / 300.0 ** 2], list(FA.PP_D), raw_y)
    plain = H.sort_data(*args, dosave=False, chunksize=5000)
    out = H.sort_data(*args, dosave=False, chunksize=5000, stability=True)
    assert set(out) - set(plain) == {"unit_stability"}
    assert set(plain) == {"mlseq", "ll", "waveforms", "lp", "sigma"}
    assert all(np.array_equal(out[k], plain[k]) for k in plain)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), True)
    tm = H.HMMSpikeTemplateModel(sm, np.asfortranarray(spike_forms[:, 0, :]), 300.0)
    m0 = H.fit(tm, raw_y, 5000)
    fits = H.spike_fit(m0)
    assert all(len(f.times) > 20 for f in fits)
    us = out["unit_stability"]
    want = H.unit_stability([f.times for f in fits], [f.amp for f in fits], T=T, bin=us["bin"],
                            quantiles=(0.25, 0.5, 0.75), hist=(512, 0.0, 4.0))
    for k in ("count", "valid", "quant", "sum", "sumsq", "uquant", "hist"):
        assert us[k].tobytes() == getattr(want, k).tobytes(), k
    assert np.array_equal(us["presence_ratio"], want.presence_ratio())
    assert np.array_equal(us["amplitude_cutoff"], want.amplitude_cutoff(), equal_nan=True)
    opt = H.sort_data(*args, dosave=False, chunksize=5000, stability=dict(bin=2500, quantiles=(0.5,), hist=None))
    w2 = H.unit_stability([f.times for f in fits], [f.amp for f in fits], T=T, bin=2500, quantiles=(0.5,))
    assert opt["unit_stability"]["count"].shape == (2, 6)
    assert opt["unit_stability"]["quant"].tobytes() == w2.quant.tobytes() and "amplitude_cutoff" not in opt["unit_stability"]
    H.shutdown()
