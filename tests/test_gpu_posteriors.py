"""Smoothed state posteriors on the device (hmmsort_plan_posteriors and friends, INTEGRATION.md "Posteriors")
against the numpy restatement of their definitions from the CPU oracle's forward/backward
(tests/posterior_model.py), for every state and sample.

Tolerance (absolute, on probabilities): tol = max(1e-8, 10 * max_t |sum_s gamma_t(s) - 1|) from the ORACLE's
gamma alone on each input -- 1e-8 is the project's E-step bar, the factor 10 headroom over the oracle's own
rounding -- with 1e-6 as a ceiling that fails whatever the oracle's defect.  logz: 1e-10 relative.  Every test
prints the largest error it saw before asserting."""
import ctypes as C

import numpy as np
import pytest

import posterior_model as PM
from conftest import four_templates, to_oracle_sm

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_options(H):
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)
    yield
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)


def make_templates(H, N, K):
    base = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    amps = [(base[i % 4][0] * (1 + 0.13 * (i // 4)), base[i % 4][1] + 0.03 * (i // 4), base[i % 4][2])
            for i in range(N)]
    return np.asfortranarray(np.stack([H.create_spike_template(K, *a) for a in amps], 1))


def make_case(H, N, K, T, sigma, seed, inside_spike=False, overlaps=False):
    temps = make_templates(H, N, K)
    pp = np.full(N, 0.003) * min(1.0, 60.0 / K) * min(1.0, 4.0 / N)
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    if inside_spike:   # the recording starts at phase 11 of template 0
        y[:K - 10] += temps[10:, 0]
    sm = H.StateMatrix.create(N, K, np.log(pp), overlaps)
    mu = np.asfortranarray(temps.copy())
    mu[0, :] = 0
    return y, sm, mu


class Dev:
    """outputs of one plan.posteriors (+ decode) call, copied to the host"""

    def __init__(self, H, y, sm, mu, sigma, decode=True, plan=None):
        import torch
        T, N = len(y), sm.N
        self.plan = plan if plan is not None else H.Plan(T, sm, mu, sigma)
        self.dy = torch.from_numpy(np.ascontiguousarray(y)).cuda()
        on = torch.full((N, T), np.nan, dtype=torch.float64, device="cuda")
        oc, si = torch.full_like(on, np.nan), torch.full((T,), np.nan, dtype=torch.float64, device="cuda")
        lz = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
        self.plan.posteriors(self.dy, on, oc, si, lz)
        xm = torch.zeros(T, dtype=torch.int16, device="cuda")
        if decode:
            self.plan.posterior_decode(xm)
        torch.cuda.synchronize()
        d = self.plan.diagnostics()
        assert d[3] == 0 and d[5] == 0, d
        self.onset, self.occ, self.silent = on.cpu().numpy(), oc.cpu().numpy(), si.cpu().numpy()
        self.logz, self.xm = float(lz.cpu()[0]), xm.cpu().numpy()


def check_against_oracle(name, dev, g, z, states, tol):
    onset, occ, silent = PM.marginals(g, states)
    errs = dict(onset=np.abs(dev.onset - onset).max(), occ=np.abs(dev.occ - occ).max(),
                silent=np.abs(dev.silent - silent).max(), logz=abs(dev.logz - z) / abs(z))
    print("%s: tol %.3g  max|d onset| %.3g  max|d occ| %.3g  max|d silent| %.3g  rel d logz %.3g"
          % (name, tol, errs["onset"], errs["occ"], errs["silent"], errs["logz"]))
    assert errs["onset"] <= tol and errs["occ"] <= tol and errs["silent"] <= tol, errs
    assert errs["logz"] <= 1e-10, errs


def check_decode(name, xm, g, tol):
    T = g.shape[1]
    top = np.sort(np.partition(g, -2, axis=0)[-2:], axis=0)
    gap = top[1] - top[0]
    chosen = g[xm.astype(np.int64) - 1, np.arange(T)]
    short = float((top[1] - chosen).max())
    close = gap <= 1e-6
    print("%s: decode  worst shortfall %.3g  share of samples with top-two gap <= 1e-6: %.3g"
          % (name, short, close.mean()))
    assert xm.min() >= 1 and xm.max() <= g.shape[0]
    assert short <= 2 * tol                                   # every sample
    assert close.mean() <= 1e-3
    assert np.array_equal(xm[~close], PM.decode(g)[~close])


CASES = [
    # N, K, T, sigma, seed, inside_spike, block, halo
    (1, 20, 300, 0.3, 1, False, 0, 0),            # below the wave engine's 512 samples: the strict path serves it
    (1, 20, 600, 0.3, 12, True, 0, 0),            # one chain, head-dominated
    (2, 60, 520, 1.0, 13, False, 0, 0),
    (1, 20, 9_000, 1.0, 2, False, 0, 0),
    (2, 60, 300, 1.0, 3, False, 0, 0),
    (2, 60, 6_000, 0.3, 4, True, 0, 0),           # starts inside a spike
    (4, 60, 20_000, 1.0, 5, False, 0, 0),
    (4, 60, 40_001, 0.3, 6, False, 512, 256),     # many short chains, ragged end
    (4, 60, 40_001, 1.0, 7, True, 0, 0),
    (8, 128, 3_000, 0.3, 8, False, 0, 0),
    (8, 128, 3_000, 1.0, 9, False, 0, 0),
    (16, 64, 3_000, 0.3, 10, False, 0, 0),
    (16, 64, 3_000, 1.0, 11, True, 0, 0),
]


@pytest.mark.parametrize("N,K,T,sigma,seed,inside,block,halo", CASES)
def test_posteriors_match_oracle(O, H, N, K, T, sigma, seed, inside, block, halo):
    """Largest errors seen on the MI355X are listed per shape in DESIGN.md section 3.5."""
    H.set_option("block", block)
    H.set_option("halo", halo)
    y, sm, mu = make_case(H, N, K, T, sigma, seed, inside)
    g, z = PM.gamma(O, y, to_oracle_sm(O, sm), mu, sigma)
    tol = PM.tolerance(g)
    dev = Dev(H, y, sm, mu, sigma)
    wave_takes = T >= max(512, 4 * (K - 1))
    assert dev.plan.info()["engine"] == (H.ENGINE_WAVE if wave_takes else H.ENGINE_STRICT)
    name = "N=%d K=%d T=%d sigma=%g" % (N, K, T, sigma)
    check_against_oracle(name, dev, g, z, sm.states, tol)
    check_decode(name, dev.xm, g, tol)
    if inside:
        # rings already running at t = 0 hold the mass, not rings that start there (which of several similar
        # templates is running may stay ambiguous at sigma = 1)
        assert dev.occ[:, 0].sum() > 0.99 and dev.onset[:, 0].sum() < 1e-3
    # expected spike counts = sum_t onset
    cnt = dev.plan.expected_counts()
    assert np.allclose(cnt, PM.marginals(g, sm.states)[0].sum(1), rtol=0, atol=tol * T)
    assert np.allclose(cnt, dev.onset.sum(1), rtol=1e-12, atol=1e-12)


def consistency(H, dev, y, sm, mu, sigma, tol):
    """size-independent properties (also run at 10 M samples in test_gpu_posteriors_fullsize.py)"""
    import torch
    N, L = sm.N, sm.K - 1
    tot = dev.occ.sum(0) + dev.silent
    print("max |sum_a occ + silent - 1| = %.3g" % np.abs(tot - 1).max())
    assert np.abs(tot - 1).max() <= tol
    for arr in (dev.onset, dev.occ, dev.silent):
        assert arr.min() >= -tol and arr.max() <= 1 + tol
    assert np.isfinite(dev.logz)
    stats = torch.zeros(dev.plan.stats_len(), dtype=torch.float64, device="cuda")
    dev.plan.estep(dev.dy, stats)
    torch.cuda.synchronize()
    G0 = stats.cpu().numpy()[:N * L].reshape(N, L).sum(1)
    rel = np.abs(dev.occ.sum(1) - G0) / G0
    print("sum_t occ against sum_k G0 of the E-step: rel %.3g" % rel.max())
    assert rel.max() <= 1e-9


@pytest.mark.parametrize("sigma", [0.3, 1.0])
def test_internal_consistency(H, sigma):
    y, sm, mu = make_case(H, 4, 60, 300_000, sigma, 21)
    consistency(H, Dev(H, y, sm, mu, sigma), y, sm, mu, sigma, 1e-8)


def test_wave_path_equals_strict_path_at_200k(H):
    """Largest difference measured on the MI355X: DESIGN.md section 3.5."""
    y, sm, mu = make_case(H, 4, 60, 200_000, 1.0, 22)
    wave = Dev(H, y, sm, mu, 1.0)
    assert wave.plan.info()["engine"] == H.ENGINE_WAVE
    H.set_option("engine", H.ENGINE_STRICT)
    strict = Dev(H, y, sm, mu, 1.0)
    assert strict.plan.info()["engine"] == H.ENGINE_STRICT
    d = dict(onset=np.abs(wave.onset - strict.onset).max(), occ=np.abs(wave.occ - strict.occ).max(),
             silent=np.abs(wave.silent - strict.silent).max(), logz=abs(wave.logz - strict.logz) / abs(strict.logz))
    differ = wave.xm != strict.xm
    print("wave against strict at T = 200 000:", d, "decodes differ at %d samples" % differ.sum())
    assert d["onset"] <= 1e-6 and d["occ"] <= 1e-6 and d["silent"] <= 1e-6 and d["logz"] <= 1e-10
    # the decodes may differ only where the top two candidates are within the bar of each other
    if differ.any():
        L = sm.K - 1

        def value(dev, x):   # gamma of state x[t] at t from a path's own outputs
            a, k = (x - 2) // L, (x - 2) % L
            t = np.arange(len(x))
            v = np.where(x == 1, dev.silent, 0.0)
            ok = (x > 1) & (t - k >= 0)
            v[ok] = dev.onset[a[ok], (t - k)[ok]]
            return v, (x == 1) | ok
        xs, xw = strict.xm.astype(np.int64), wave.xm.astype(np.int64)
        v1, ok1 = value(strict, xs)
        v2, ok2 = value(strict, xw)
        both = differ & ok1 & ok2
        assert np.abs(v1[both] - v2[both]).max(initial=0.0) <= 2e-6
        assert (differ & ~both).sum() == 0
    assert np.allclose(wave.plan.expected_counts(), strict.plan.expected_counts(), rtol=0, atol=1e-6 * 200_000)


@pytest.mark.parametrize("sigma", [0.3, 1.0])
def test_spike_confidence_matches_definition(O, H, sigma):
    import torch
    N, K, T = 4, 60, 20_000
    y, sm, mu = make_case(H, N, K, T, sigma, 31)
    osm = to_oracle_sm(O, sm)
    g, _ = PM.gamma(O, y, osm, mu, sigma)
    tol = PM.tolerance(g)
    x, _ = O.viterbi(y, osm, mu, sigma)
    x = np.asarray(x, dtype=np.int16)
    # an event in the first and one in the last J samples (any int16 path over the model's states is allowed)
    q0 = PM.trough_values(mu)[0]
    x[1] = 2 + (q0 - 2)
    x[T - 2] = 2 + (q0 - 2)
    dev = Dev(H, y, sm, mu, sigma, decode=False)
    dx = torch.from_numpy(x).cuda()
    ref_times = dev.plan.extract_spiketimes(dx)
    lo_all = []
    for J in (0, 2, 5):
        got = dev.plan.spike_confidence(dx, J)
        want = PM.confidence(g, sm.states, mu, x, J)
        for a in range(N):
            assert np.array_equal(got[a][0], want[a][0]) and np.array_equal(got[a][0], ref_times[a])
            err = np.abs(got[a][1] - want[a][1]).max(initial=0.0)
            assert err <= (2 * J + 1) * tol, (J, a, err)
            assert np.all(got[a][1] <= 1.0)
        allc = np.concatenate([c for _, c in got])
        print("sigma %g J %d: %d events, confidence %.3f .. %.3f" % (sigma, J, len(allc), allc.min(), allc.max()))
        lo_all.append(allc.min())
        assert 2 in got[0][0] and T - 1 in got[0][0]
    if sigma == 1.0:
        assert lo_all[0] < 0.9          # not 1 everywhere
    # default jitter is 2
    assert np.array_equal(dev.plan.spike_confidence(dx)[0][1], dev.plan.spike_confidence(dx, 2)[0][1])


def test_posterior_call_does_not_disturb_the_plan(H):
    import torch
    N, K, T = 4, 60, 1_000_000
    temps = four_templates(H, K)
    pp = [0.003, 0.001, 0.002, 0.0015]
    y = H.create_signal(T, 0.3, pp, temps, seed=41)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    plan = H.Plan(T, sm, temps, 0.3)
    dy = torch.from_numpy(y).cuda()

    def estep_and_decode():
        stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.profile(True)
        plan.estep(dy, stats)
        names = set(plan.profile_read())
        plan.profile(False)
        plan.viterbi(dy, dx, dll)
        torch.cuda.synchronize()
        return stats.cpu().numpy(), dx.cpu().numpy(), names
    s0, x0, n0 = estep_and_decode()
    on = torch.zeros((N, T), dtype=torch.float64, device="cuda")
    plan.profile(True)
    plan.posteriors(dy, on, None, None, None)
    npost = set(plan.profile_read())
    plan.profile(False)
    s1, x1, n1 = estep_and_decode()
    assert s0.tobytes() == s1.tobytes() and x0.tobytes() == x1.tobytes()
    # the E-step runs the fused backward sweep before and after: no stand-alone statistics kernel, no posterior sweep
    assert "kw_bwd" in n0 and "kw_gsum" not in n0 and n0 == n1
    assert "kw_bwd_post" in npost and "kw_fb_check" in npost and "kw_gsum" not in npost and "kw_stats_final" not in npost
    # ... and a decode needs a posterior call after the last E-step
    with pytest.raises(H.HmmsortError):
        plan.posterior_decode(torch.zeros(T, dtype=torch.int16, device="cuda"))


def test_batched_plan_equals_single_plans(H):
    import torch
    N, K, T, nC = 4, 60, 50_000, 3
    cases = [make_case(H, N, K, T, s, 50 + i) for i, s in enumerate((0.3, 0.6, 1.0))]
    sigmas = [0.3, 0.6, 1.0]
    mus = [np.asfortranarray(c[2] * f) for c, f in zip(cases, (1.0, 0.9, 1.1))]
    singles = [Dev(H, c[0], c[1], m, s) for c, m, s in zip(cases, mus, sigmas)]
    plan = H.Plan.batched(T, [c[1] for c in cases], mus, sigmas)
    dy = torch.from_numpy(np.stack([c[0] for c in cases])).cuda()
    on = torch.zeros((nC, N, T), dtype=torch.float64, device="cuda")
    oc, si = torch.zeros_like(on), torch.zeros((nC, T), dtype=torch.float64, device="cuda")
    lz = torch.zeros(nC, dtype=torch.float64, device="cuda")
    xm = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
    plan.posteriors(dy, on, oc, si, lz)
    plan.posterior_decode(xm)
    torch.cuda.synchronize()
    cnt = plan.expected_counts()
    for c, s in enumerate(singles):
        assert np.array_equal(on[c].cpu().numpy(), s.onset) and np.array_equal(oc[c].cpu().numpy(), s.occ)
        assert np.array_equal(si[c].cpu().numpy(), s.silent) and np.array_equal(xm[c].cpu().numpy(), s.xm)
        assert float(lz[c]) == s.logz
        assert np.array_equal(cnt[c], s.plan.expected_counts())
    conf = plan.spike_confidence(xm, 2)
    for c, s in enumerate(singles):
        import torch as _t
        one = s.plan.spike_confidence(_t.from_numpy(s.xm).cuda(), 2)
        for a in range(N):
            assert np.array_equal(conf[c][a][0], one[a][0]) and np.array_equal(conf[c][a][1], one[a][1])
    # one signal and one model in every channel: the same logz
    plan2 = H.Plan.batched(T, [cases[0][1]] * nC, [mus[0]] * nC, [0.3] * nC)
    dy2 = torch.from_numpy(np.stack([cases[0][0]] * nC)).cuda()
    plan2.posteriors(dy2, None, None, None, lz)
    torch.cuda.synchronize()
    l = lz.cpu().numpy()
    assert np.isfinite(l).all() and l[0] == l[1] == l[2]


def test_sharded_plan_is_refused(H):
    import torch
    y, sm, mu = make_case(H, 4, 60, 100_000, 0.3, 61)
    H.set_option("block", 4096)
    plan = H.Plan(len(y), sm, mu, 0.3)
    plan.set_shard(0, 50_000, True, False)
    with pytest.raises(H.HmmsortError) as e:
        plan.posteriors(torch.from_numpy(y).cuda(), torch.zeros((4, len(y)), dtype=torch.float64, device="cuda"))
    assert e.value.code == H._lib.EINVAL and "shard" in str(e.value)


@pytest.mark.parametrize("N,K,overlaps,engine", [(2, 20, True, "auto"), (4, 60, False, "strict")])
def test_strict_path_matches_oracle(O, H, N, K, overlaps, engine):
    T, sigma = 4_000, 1.0
    y, sm, mu = make_case(H, N, K, T, sigma, 71, overlaps=overlaps)
    g, z = PM.gamma(O, y, to_oracle_sm(O, sm), mu, sigma)
    tol = PM.tolerance(g)
    if engine == "strict":
        H.set_option("engine", H.ENGINE_STRICT)
    p = H.posteriors(y, sm, mu, sigma)             # host entry: the overlap model goes to the strict path by itself
    xm = H.posterior_decode(y, sm, mu, sigma)

    class R:
        onset, occ, silent, logz = p.onset, p.occ, p.silent, p.logz
    name = "strict N=%d K=%d overlaps=%s" % (N, K, overlaps)
    check_against_oracle(name, R, g, z, sm.states, tol)
    check_decode(name, xm, g, tol)
    # confidence through api.spike_confidence, aligned with api.extract_spiketimes
    x, ll = H.viterbi(y, sm, mu, sigma)
    model = H.HMMSpikingModel(H.HMMSpikeTemplateModel(sm, mu, sigma), x, ll, y)
    got = H.spike_confidence(model)
    want = PM.confidence(g, sm.states, mu, x, 2)
    times = H.extract_spiketimes(model)
    for a in range(N):
        assert np.array_equal(got[a][0], times[a]) and np.array_equal(got[a][0], want[a][0])
        assert np.abs(got[a][1] - want[a][1]).max(initial=0.0) <= 5 * tol


def test_strict_limit_is_named(H):
    y, sm, mu = make_case(H, 2, 20, 50_000, 0.3, 81, overlaps=True)
    H.set_option("strict_limit_mb", 1)
    try:
        with pytest.raises(H.HmmsortError) as e:
            H.posteriors(y, sm, mu, 0.3)
        assert e.value.code == H._lib.ENOMEM and "strict_limit_mb" in str(e.value)
    finally:
        H.set_option("strict_limit_mb", 0)


def test_host_entry_equals_plan_path_and_skips_null_outputs(H):
    y, sm, mu = make_case(H, 4, 60, 30_000, 1.0, 91)
    dev = Dev(H, y, sm, mu, 1.0)
    p = H.posteriors(y, sm, mu, 1.0)
    assert np.array_equal(p.onset, dev.onset) and np.array_equal(p.occ, dev.occ)
    assert np.array_equal(p.silent, dev.silent) and p.logz == dev.logz
    assert np.array_equal(H.posterior_decode(y, sm, mu, 1.0), dev.xm)
    # raw C ABI with NULL outputs: only logz, then only silent
    from hmmsort_amd._lib import TRANS_DTYPE, check, lib, ptr
    st = np.asfortranarray(sm.states, dtype=np.int16)
    tr = np.ascontiguousarray(sm.transitions, dtype=TRANS_DTYPE)
    muf = np.asfortranarray(mu, dtype=np.float64)
    margs = (ptr(st), sm.N, sm.K, sm.nstates, ptr(tr), len(tr), ptr(muf), 1.0)
    lz = np.zeros(1)
    check(lib().hmmsort_posteriors(ptr(y), len(y), *margs, None, None, None, None, ptr(lz)))
    assert lz[0] == dev.logz
    si = np.zeros(len(y))
    check(lib().hmmsort_posteriors(ptr(y), len(y), *margs, None, None, ptr(si), None, None))
    assert np.array_equal(si, dev.silent)
    L = C.CDLL(H._lib.LIB_PATH)
    for n in ("hmmsort_plan_posteriors", "hmmsort_plan_posterior_decode", "hmmsort_plan_spike_confidence",
              "hmmsort_plan_expected_counts", "hmmsort_posteriors"):
        assert hasattr(L, n)


def test_sort_data_confidence(H):
    K, N, T = 20, 2, 6_000
    temps = make_templates(H, N, K)
    pp = [0.004, 0.003]
    y = H.create_signal(T, 0.5, pp, temps, seed=95)
    forms = temps[:, None, :]
    base = H.sort_data(forms, [1 / 0.25], pp, y, dosave=False, chunksize=2_000)
    out = H.sort_data(forms, [1 / 0.25], pp, y, dosave=False, chunksize=2_000, confidence=True)
    assert sorted(base) == ["ll", "lp", "mlseq", "sigma", "waveforms"]
    assert sorted(out) == sorted(list(base) + ["spiketimes", "confidence"])
    assert np.array_equal(out["mlseq"], base["mlseq"])
    for a in range(N):
        t, c = out["spiketimes"][a], out["confidence"][a]
        assert len(t) == len(c) and len(t) > 0 and np.all((c >= 0) & (c <= 1)) and np.all(np.diff(t) > 0)
