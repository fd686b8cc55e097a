"""hmmsort_spike_fit / hmmsort_plan_spike_fit against the numpy model tests/spike_fit_model.py: times,
amp, rss, energy, nused, counts and summary must come out bit for bit (NaNs by position), from the host form and the
plan form, for fp64 and int16 samples, under a model track, through Plan.batched, api.spike_fit and sort_data."""
import ctypes as C

import numpy as np
import pytest

import fit_adaptive_model as FA
import spike_fit_model as SF

pytestmark = pytest.mark.gpu

FIELDS = ("times", "amp", "rss", "energy", "nused", "summary")


def same(got, want, what=""):
    """library SpikeFit list == model dict list, bit for bit"""
    assert len(got) == len(want)
    for a, (g, w) in enumerate(zip(got, want)):
        for k in FIELDS:
            gv, wv = getattr(g, k), w[k]
            assert gv.shape == wv.shape, (what, a, k, gv.shape, wv.shape)
            bad = np.flatnonzero(~((gv == wv) | (np.isnan(gv) & np.isnan(wv)))) if gv.dtype.kind == "f" else \
                np.flatnonzero(gv != wv)
            assert len(bad) == 0, (what, a, k, bad[:4], gv[bad[:4]], wv[bad[:4]])


def model_of(H, sm, mu, sigma, y, x):
    return H.HMMSpikingModel(H.HMMSpikeTemplateModel(sm, mu, sigma), x, 0.0, y)


def templates(H, N, K, rng):
    base = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    return np.asfortranarray(np.stack([H.create_spike_template(K, base[i % 4][0] * rng.uniform(0.8, 1.2), *base[i % 4][1:])
                                       for i in range(N)], 1))


def ring_path(st, counts, T, rng, gap=6):
    """a path of a no-overlap table: template a fires counts[a] times, in random order, 0..gap silent samples
    between spikes (back to back included), silence up to T"""
    N, K = st.shape[0], int(st.max())
    sid = {}
    for j in range(1, st.shape[1]):
        a = int(np.flatnonzero(st[:, j] > 1)[0])
        sid[(a, int(st[a, j]))] = j + 1
    x = [1] * int(rng.integers(0, gap + 1))
    for a in rng.permutation(np.repeat(np.arange(N), counts)):
        x += [sid[(int(a), k)] for k in range(2, K + 1)] + [1] * int(rng.integers(0, gap + 1))
    assert len(x) <= T, (len(x), T)
    return np.array(x + [1] * (T - len(x)), dtype=np.int16)


def signal_of(x, st, mu, sigma, rng, gain=(0.6, 1.2)):
    """the path's reconstruction with a slowly varying gain, plus noise"""
    rec = mu[st[:, x.astype(np.int64) - 1].astype(np.int64) - 1, np.arange(st.shape[0])[:, None]].sum(0)
    return rec * np.linspace(gain[0], gain[1], len(x)) + sigma * rng.standard_normal(len(x))


def check_case(H, sm, mu, sigma, y, x, what):
    want = SF.spike_fit(y, x, np.asarray(sm.states), mu)
    got = H.spike_fit(model_of(H, sm, mu, sigma, y, x))
    same(got, want, what)
    same(H.spike_fit(model_of(H, sm, mu, sigma, y, x)), want, what + " again")       # the same bits twice
    return got, want


# ---- shapes ---------------------------------------------------------------------------------------------------
def test_a_overlap_model_across_the_compaction_block(H):
    rng = np.random.default_rng(11)
    pp, sigma, T = (0.03, 0.02), 0.5, 4100
    mu = np.asfortranarray(np.array([[0.0, -1.0, -3.0, -2.0, 1.0], [0.0, 0.5, -2.0, -4.0, 1.0]]).T)
    sm = H.StateMatrix.create(2, 5, np.log(pp), True)
    y = H.create_signal(T, sigma, pp, mu, seed=4)
    x, _ll = H.viterbi(y, sm, mu, sigma)
    got, want = check_case(H, sm, mu, sigma, y, x, "decode")
    assert all(len(g.times) > 20 for g in got)
    # a random Int16 array over -2..S+2: partial events everywhere, windows across sample 4096 and both ends
    xr = rng.integers(-2, sm.nstates + 3, T).astype(np.int16)
    st = np.asarray(sm.states)
    col = lambda a, b: int(np.flatnonzero((st[0] == a) & (st[1] == b))[0]) + 1  # noqa: E731
    xr[0], xr[T - 1] = col(3, 1), col(1, 4)                       # troughs on the first and the last sample
    xr[4094:4098] = [col(2, 1), col(3, 1), col(4, 1), col(5, 1)]  # a whole spike of template 0 across sample 4096
    got, want = check_case(H, sm, mu, sigma, y, xr, "random ids")
    t0, t1 = got[0].times.tolist(), got[1].times.tolist()
    assert t0[0] == 1 and t1[-1] == T and got[0].nused[t0.index(4096)] == 4
    assert min(int(g.nused.min()) for g in got) == 1 and all(len(g.times) > 256 for g in got)


@pytest.mark.parametrize("N,K,T,counts", [(2, 130, 20_000, (70, 50)),          # (b) more phases than lanes
                                          (16, 8, 30_000, (120,) * 16),        # (d)
                                          (2, 5, 9_000, (700, 300)),           # (f) 3 and 2 blocks, ragged
                                          (1, 2100, 12_000, (4,))])            # more phases than one LDS tile holds
def test_ring_shapes(H, N, K, T, counts):
    rng = np.random.default_rng(N * 1000 + K)
    mu = templates(H, N, K, rng)
    sm = H.StateMatrix.create(N, K, np.log(np.full(N, 0.01 / N)), False)
    st = np.asarray(sm.states)
    x = ring_path(st, counts, T, rng)
    y = signal_of(x, st, mu, 0.3, rng)
    got, want = check_case(H, sm, mu, 0.3, y, x, "ring %dx%d" % (N, K))
    assert [len(g.times) for g in got] == list(counts)
    for g in got:      # the spikes were written at a gain in 0.6..1.2 and every window is whole
        assert np.all(g.nused == K - 1) and g.summary[1] == len(g.times) and 0.5 < np.median(g.amp) < 1.3


def test_c_one_phase_and_e_recording_shorter_than_a_template(H):
    rng = np.random.default_rng(5)
    mu1 = np.asfortranarray(np.array([[0.0], [-2.0]]))
    sm1 = H.StateMatrix.create(1, 2, np.log([0.05]), False)
    x = rng.integers(0, 4, 300).astype(np.int16)
    got, _ = check_case(H, sm1, mu1, 0.4, rng.standard_normal(300), x, "K = 2")
    assert len(got[0].times) > 30 and np.all(got[0].nused == 1) and len(got[0].summary) == 11
    mu = np.asfortranarray(np.array([[0.0, -1.0, -3.0, -2.0, 1.0], [0.0, 0.5, -2.0, -4.0, 1.0]]).T)
    sm = H.StateMatrix.create(2, 5, np.log([0.01, 0.01]), True)
    st = np.asarray(sm.states)
    col = lambda a, b: int(np.flatnonzero((st[0] == a) & (st[1] == b))[0]) + 1  # noqa: E731
    x3 = np.array([col(2, 3), col(3, 4), col(4, 5)], dtype=np.int16)
    got, _ = check_case(H, sm, mu, 0.4, np.array([0.5, -2.0, 1.5]), x3, "T = 3")
    assert [g.times.tolist() for g in got] == [[2], [2]] and [g.nused.tolist() for g in got] == [[3], [3]]
    # T == 0: zero counts, zero summary but the template's own smm
    got = H.spike_fit(model_of(H, sm, mu, 0.4, np.zeros(0), np.zeros(0, dtype=np.int16)))
    for a, g in enumerate(got):
        assert len(g.times) == 0 and g.summary[7] == SF.fit_template(np.zeros(0), np.zeros(0), st, mu, a)["summary"][7] > 0
        assert not np.delete(g.summary, 7).any()


# ---- the raw call: cap protocol, refusals -----------------------------------------------------------------------
def raw_fit(H, y, x, st, mu, cap, nch=0, first=None, mut=None, stype=None, counts=True, N=None, K=None, fill=-7):
    """hmmsort_spike_fit on sentinel-filled arrays -> (rc, dict of arrays)"""
    L = H._lib
    st = np.asfortranarray(st, dtype=np.int16)
    mu = np.asfortranarray(mu, dtype=np.float64)
    N = st.shape[0] if N is None else N
    K = mu.shape[0] if K is None else K
    b = dict(times=np.full((N, cap), fill, dtype=np.int64), amp=np.full((N, cap), float(fill)),
             rss=np.full((N, cap), float(fill)), energy=np.full((N, cap), float(fill)),
             nused=np.full((N, cap), fill, dtype=np.int32), counts=np.full(N, fill, dtype=np.int64),
             summary=np.full((N, 8 + 3 * (max(K, 1) - 1)), float(fill)))
    out = L.SpikeFitOut(*[b[k].ctypes.data for k in ("times", "amp", "rss", "energy", "nused")], cap,
                        b["counts"].ctypes.data if counts else None, b["summary"].ctypes.data)
    stype = (L.SAMPLES_I16 if y.dtype == np.int16 else L.SAMPLES_F64) if stype is None else stype
    rc = L.lib().hmmsort_spike_fit(L.ptr(y), stype, len(y), L.ptr(x), L.ptr(st), N, st.shape[1], L.ptr(mu), K, nch,
                                   L.ptr(first), L.ptr(mut), C.byref(out))
    return rc, b


@pytest.fixture(scope="module")
def small(H):
    """a 2 x 5 ring case with 40 and 25 events, its model result, and an int16 signal"""
    rng = np.random.default_rng(21)
    mu = np.asfortranarray(np.array([[0.0, -100.0, -300.0, -200.0, 100.0], [0.0, 50.0, -200.0, -400.0, 100.0]]).T)
    sm = H.StateMatrix.create(2, 5, np.log([0.01, 0.01]), False)
    st = np.asarray(sm.states)
    x = ring_path(st, (40, 25), 700, rng)
    y = np.round(signal_of(x, st, mu, 30.0, rng)).astype(np.int16)
    return sm, st, mu, x, y, SF.spike_fit(y.astype(np.float64), x, st, mu)


def test_cap_protocol(H, small):
    sm, st, mu, x, y, want = small
    yf = y.astype(np.float64)
    sums = []
    for cap in (0, 10, 40, 64):
        rc, b = raw_fit(H, yf, x, st, mu, cap)
        assert rc == 0 and b["counts"].tolist() == [40, 25]
        sums.append(b["summary"].copy())
        for a in range(2):
            n = min(cap, int(b["counts"][a]))
            for k in FIELDS[:5]:
                assert np.array_equal(b[k][a, :n], want[a][k][:n]), (cap, a, k)
                assert np.all(b[k][a, n:] == -7), (cap, a, k)               # beyond min(count, cap): untouched
    assert all(np.array_equal(s, np.stack([w["summary"] for w in want])) for s in sums)


def test_int16_samples_equal_their_fp64_values(H, small):
    sm, st, mu, x, y, want = small
    assert y.dtype == np.int16
    same(H.spike_fit(model_of(H, sm, mu, 30.0, y, x)), want, "int16")
    same(H.spike_fit(model_of(H, sm, mu, 30.0, y.astype(np.float64), x)), want, "fp64")


def test_plan_form_equals_host_form(H, small):
    import torch
    sm, st, mu, x, y, want = small
    plan = H.Plan(len(x), sm, mu, 30.0)
    try:
        dy, dx = torch.from_numpy(y.astype(np.float64)).cuda(), torch.from_numpy(x).cuda()
        same(plan.spike_fit(dy, dx, stream=torch.cuda.current_stream().cuda_stream), want, "plan")
        same(plan.spike_fit(dy, dx), want, "plan, null stream")
    finally:
        plan.close()


def test_batched_wave_plan_equals_single_calls(H):
    import torch
    rng = np.random.default_rng(33)
    nC, N, K, T = 3, 2, 20, 37_001
    sm = H.StateMatrix.create(N, K, np.log([0.003, 0.002]), False)
    st = np.asarray(sm.states)
    mus = [templates(H, N, K, rng) for _ in range(nC)]
    xs = np.stack([ring_path(st, (150 + 60 * c, 280 - 30 * c), T, rng, gap=40) for c in range(nC)])
    ys = np.stack([signal_of(xs[c], st, mus[c], 0.3, rng) for c in range(nC)])
    H.set_option("engine", H.ENGINE_WAVE)
    try:
        plan = H.Plan.batched(T, [sm] * nC, mus, [0.3] * nC)
        got = plan.spike_fit(torch.from_numpy(ys).cuda(), torch.from_numpy(xs).cuda())
        # a batched plan takes no track
        tk = H.ModelTrack(1, np.array([1], dtype=np.int64), None, None, mus[0][None], None)
        with pytest.raises(H.HmmsortError) as e:
            plan.spike_fit(torch.from_numpy(ys).cuda(), torch.from_numpy(xs).cuda(), track=tk)
        assert e.value.code == H._lib.EINVAL and "batched" in str(e.value)
        plan.close()
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    assert len(got) == nC
    for c in range(nC):
        one = H.spike_fit(model_of(H, sm, mus[c], 0.3, ys[c], xs[c]))
        assert [len(f.times) for f in one] == [150 + 60 * c, 280 - 30 * c]
        for g, o in zip(got[c], one):
            for k in FIELDS:
                assert np.array_equal(getattr(g, k), getattr(o, k)), (c, k)
    same(got[1], SF.spike_fit(ys[1], xs[1], st, mus[1]), "channel 1")


def test_refusals(H, small):
    sm, st, mu, x, y, want = small
    L = H._lib
    yf = y.astype(np.float64)

    def refused(code, word, **kw):
        args = dict(y=yf, x=x, st=st, mu=mu, cap=4)
        args.update(kw)
        rc, _ = raw_fit(H, **args)
        assert rc == code and word in L.last_error(), (rc, L.last_error())

    refused(L.EINVAL, "null", counts=False)
    rc = L.lib().hmmsort_spike_fit(L.ptr(yf), L.SAMPLES_F64, len(yf), L.ptr(x), None, 2, st.shape[1], L.ptr(mu), 5, 0,
                                   None, None, None)
    assert rc == L.EINVAL and "null" in L.last_error()
    refused(L.EINVAL, "33", st=np.ones((33, st.shape[1]), dtype=np.int16), mu=np.zeros((5, 33)))
    refused(L.EINVAL, "K = 1", K=1)
    refused(L.EINVAL, "HMMSORT_SAMPLES", stype=L.SAMPLES_F32)
    two = np.stack([mu.T.ravel(), mu.T.ravel()])
    refused(L.EINVAL, "ascend", nch=2, first=np.array([5, 5], dtype=np.int64), mut=two)
    refused(L.EINVAL, "first[0]", nch=2, first=np.array([0, 5], dtype=np.int64), mut=two)
    refused(L.EUNSUP, "8193", nch=8193, first=np.arange(1, 8194, dtype=np.int64), mut=np.zeros((8193, 10)))
    flat = mu.copy()
    flat[:, 1] = np.abs(flat[:, 1])                       # template 1: minimum in the silent row
    refused(L.EINVAL, "template 1", mu=flat)
    with pytest.raises(ValueError):
        SF.fit_template(yf, x, st, flat, 1)
    # the plan form refuses the same model
    plan = H.Plan(len(x), sm, flat, 30.0)
    try:
        import torch
        with pytest.raises(H.HmmsortError) as e:
            plan.spike_fit(torch.from_numpy(yf).cuda(), torch.from_numpy(x).cuda())
        assert e.value.code == L.EINVAL and "template 1" in str(e.value)
    finally:
        plan.close()


# ---- the model track ------------------------------------------------------------------------------------------
def test_track_of_the_drift_tracking_decode(H):
    y, onsets, temps = FA.drifting(H, 1, 0.4)
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), False)
    st = np.asarray(sm.states)
    model, tk = H.fit_adaptive(H.HMMSpikeTemplateModel(sm, temps, FA.SIGMA_D), y, 4000, 8000.0)
    x = model.ml_seq
    tracked = H.spike_fit(model, tk)
    same(tracked, SF.spike_fit(y, x, st, temps, (tk.first, tk.mu)), "track")
    fixed = H.spike_fit(model)
    same(fixed, SF.spike_fit(y, x, st, temps), "fixed model, same path")
    for a in range(2):
        late = tracked[a].times - 1 >= 32_000
        mt, mf = np.median(tracked[a].amp[late]), np.median(fixed[a].amp[late])
        print("template %d: late median amp %.3f under the track, %.3f under the fixed model (%d events)"
              % (a, mt, mf, late.sum()))
        assert late.sum() > 30 and abs(mt - 1.0) < abs(mf - 1.0)
    # the plan form takes the track too
    import torch
    plan = H.Plan(len(y), sm, temps, FA.SIGMA_D)
    try:
        got = plan.spike_fit(torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda(), track=tk)
    finally:
        plan.close()
    for g, o in zip(got, tracked):
        assert all(np.array_equal(getattr(g, k), getattr(o, k), equal_nan=(k != "times" and k != "nused")) for k in FIELDS)
    # a track that starts late: the events before first[0] are NaN and counted
    late_tk = H.ModelTrack(tk.n - 2, tk.first[2:], None, None, tk.mu[2:], None)
    got = H.spike_fit(model, late_tk)
    same(got, SF.spike_fit(y, x, st, temps, (late_tk.first, late_tk.mu)), "late track")
    for a in range(2):
        early = got[a].times < late_tk.first[0]
        assert early.sum() > 5 and np.all(np.isnan(got[a].amp[early])) and np.all(got[a].nused[early] == 0)
        assert not np.any(np.isnan(got[a].amp[~early])) and got[a].summary[0] == len(got[a].times)
        assert got[a].summary[1] == np.sum(got[a].nused == FA.K_D - 1)
    H.shutdown()


# ---- Python layers above ----------------------------------------------------------------------------------------
def test_unit_quality_and_sort_data(H):
    y, onsets, temps = FA.drifting(H, 2, 0.4)
    T = 15_000
    raw = np.round(y[:T] * 1000).astype(np.int16)
    spike_forms = np.zeros((FA.K_D, 1, 2))
    spike_forms[:, 0, :] = temps * 1000
    args = (spike_forms, [1.0 / 300.0 ** 2], list(FA.PP_D), raw)
    parent = H.sort_data(*args, dosave=False, chunksize=5000)
    plain = H.sort_data(*args, dosave=False, chunksize=5000, quality=False)
    assert set(plain) == set(parent) == {"mlseq", "ll", "waveforms", "lp", "sigma"}
    assert all(np.array_equal(plain[k], parent[k]) for k in parent)
    out = H.sort_data(*args, dosave=False, chunksize=5000, quality=True)
    assert set(out) - set(plain) == {"spiketimes", "amplitude", "residual", "unit_quality"}
    assert all(np.array_equal(out[k], plain[k]) for k in plain)
    # the same through api.spike_fit / api.unit_quality on the stitched path of the overlap model
    sm = H.StateMatrix.create(2, FA.K_D, np.log(FA.PP_D), True)
    tm = H.HMMSpikeTemplateModel(sm, np.asfortranarray(spike_forms[:, 0, :]), 300.0)
    modelf = H.fit(tm, raw, 5000)
    assert np.array_equal(H.unroll_mlseq(modelf.ml_seq, sm), out["mlseq"])
    fits = H.spike_fit(modelf)
    same(fits, SF.spike_fit(raw.astype(np.float64), modelf.ml_seq, np.asarray(sm.states), tm.mu), "overlap decode")
    uq = H.unit_quality(modelf)
    for a in range(2):
        assert np.array_equal(out["spiketimes"][a], fits[a].times) and np.array_equal(out["amplitude"][a], fits[a].amp)
        assert np.array_equal(out["residual"][a], fits[a].rss) and len(fits[a].times) > 20
        q = uq[a]
        assert out["unit_quality"]["n"][a] == q.n == len(fits[a].times) and out["unit_quality"]["chi2"][a] == q.chi2
        assert np.array_equal(out["unit_quality"]["waveform"][:, a], q.waveform)
        s = fits[a].summary
        assert q.n_full == s[1] and q.mean_amp == s[2] / s[1] and q.sd_expected == 300.0 / np.sqrt(s[7])
        # D(2, 0.4) has lost a fifth of its amplitude by sample 15 000: the summary shows it
        assert 0.8 < q.mean_amp < 1.0 and 0.5 < q.sd_amp / q.sd_expected < 2.5 and 0.8 < q.chi2 < 2.0
    # with the drift-tracking decode the run's own track is passed on
    ad = H.sort_data(*args, dosave=False, chunksize=5000, adapt_halflife=8000, quality=True)
    assert {"waveforms_track", "amplitude", "unit_quality"} <= set(ad)
    H.shutdown()
