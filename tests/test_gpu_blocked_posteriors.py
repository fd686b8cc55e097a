"""Posteriors of overlap models on the blocked engine (generic_estep.hip, bes_block_post; DESIGN.md section 3.5
"Blocked path"): hmmsort_plan_posteriors on a blocked plan keeps the gamma the time-parallel E-step forms and
forgets, reduced per sample into onset / occ / trough / silent / arg max, without S x T arrays.

Yardsticks and tolerances are those of test_gpu_posteriors.py: the CPU oracle's gamma (posterior_model.gamma),
tol = posterior_model.tolerance(g) = max(1e-8, 10 x the oracle's own column-sum defect), logz 1e-10 relative,
the decode by check_decode's rule.  Against the strict path and the plan's own E-step the bars are the project's
1e-8 absolute on probabilities and 1e-9 relative on sums.  Every test prints the largest error it saw before
asserting; the figures measured on the MI355X are in DESIGN.md section 3.5."""
import numpy as np
import pytest

import posterior_model as PM
from test_gpu_posteriors import Dev, check_against_oracle, check_decode, make_case, to_oracle_sm

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_options(H):
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)
    yield
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)
    H.shutdown()


def blocked_dev(H, y, sm, mu, sigma, block=0, halo=0, decode=True):
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option("block", block)
    H.set_option("halo", halo)
    dev = Dev(H, y, sm, mu, sigma, decode=decode)
    assert dev.plan.info()["engine"] == H.ENGINE_BLOCKED
    return dev


CASES = [
    # N, K, T, sigma, seed, inside_spike, block
    (2, 20, 4_000, 0.3, 101, False, 448),       # 9 blocks
    (2, 20, 4_000, 1.0, 102, True, 128),        # starts inside a spike; blocks shorter than the warm-up of 256
    (2, 20, 9_000, 0.3, 103, False, 1024),      # 9 blocks, ragged end
    (2, 20, 9_000, 1.0, 104, False, 512),       # 18 blocks
    (3, 12, 4_000, 1.0, 105, False, 448),       # three templates, 1 728 states
]


@pytest.mark.parametrize("N,K,T,sigma,seed,inside,block", CASES)
def test_blocked_posteriors_match_oracle(O, H, N, K, T, sigma, seed, inside, block):
    import torch
    y, sm, mu = make_case(H, N, K, T, sigma, seed, inside, overlaps=True)
    osm = to_oracle_sm(O, sm)
    g, z = PM.gamma(O, y, osm, mu, sigma)
    tol = PM.tolerance(g)
    dev = blocked_dev(H, y, sm, mu, sigma, block=block)
    info = dev.plan.info()
    assert info["nchains"] >= 8, info
    if block == 128:
        assert info["block"] < info["halo"], info
    name = "blocked N=%d K=%d T=%d sigma=%g block=%d" % (N, K, T, sigma, info["block"])
    check_against_oracle(name, dev, g, z, sm.states, tol)
    check_decode(name, dev.xm, g, tol)
    if inside:
        # the recording starts in phase 11 of template 0: the mass at t = 0 sits on running spikes, not on onsets
        print("%s: occ[:, 0] = %s, sum_a onset[:, 0] = %.3g (oracle: %s)" % (
            name, dev.occ[:, 0], dev.onset[:, 0].sum(), PM.marginals(g[:, :1], sm.states)[1][:, 0]))
        assert dev.occ[0, 0] > 0.5 > dev.onset[:, 0].sum()
    # expected spike counts = sum_t onset
    cnt = dev.plan.expected_counts()
    rel = np.abs(cnt - dev.onset.sum(1)) / dev.onset.sum(1)
    print("%s: expected_counts against sum_t onset: rel %.3g" % (name, rel.max()))
    assert rel.max() <= 1e-12
    # per-spike confidence on the oracle's Viterbi path, at jitter 0 and 2
    x, _ = O.viterbi(y, osm, mu, sigma)
    x = np.asarray(x, dtype=np.int16)
    dx = torch.from_numpy(x).cuda()
    times = dev.plan.extract_spiketimes(dx)
    for J in (0, 2):
        got = dev.plan.spike_confidence(dx, J)
        want = PM.confidence(g, sm.states, mu, x, J)
        worst = 0.0
        for a in range(N):
            assert np.array_equal(got[a][0], want[a][0]) and np.array_equal(got[a][0], times[a])
            worst = max(worst, float(np.abs(got[a][1] - want[a][1]).max(initial=0.0)))
        print("%s: spike_confidence jitter %d: %d spikes, max |d| %.3g" % (name, J, sum(len(t) for t in times), worst))
        assert worst <= 5 * tol


def test_blocked_against_strict_and_own_estep(H):
    """blocked against strict plan on one input; sum_t of the marginals against G0 of the plan's own E-step; the
    E-step statistics and the Viterbi path of the plan are bitwise what they were before the posterior call"""
    import torch
    N, K, T, sigma = 2, 20, 20_000, 1.0
    y, sm, mu = make_case(H, N, K, T, sigma, 111, overlaps=True)
    H.set_option("engine", H.ENGINE_BLOCKED)
    plan = H.Plan(T, sm, mu, sigma)
    assert plan.info()["engine"] == H.ENGINE_BLOCKED       # EUNSUP from plan.posteriors before the blocked path
    dy = torch.from_numpy(y).cuda()

    def estep_and_decode():
        stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.estep(dy, stats)
        plan.viterbi(dy, dx, dll)
        torch.cuda.synchronize()
        return stats.cpu().numpy(), dx.cpu().numpy()
    s0, x0 = estep_and_decode()
    # the E-step has invalidated nothing yet, and no posterior call has been made: a decode is refused
    with pytest.raises(H.HmmsortError):
        plan.posterior_decode(torch.zeros(T, dtype=torch.int16, device="cuda"))
    blocked = Dev(H, y, sm, mu, sigma, plan=plan)
    cb = plan.expected_counts()
    s1, x1 = estep_and_decode()
    assert s0.tobytes() == s1.tobytes() and x0.tobytes() == x1.tobytes()
    # ... and the plan's next E-step invalidates the posteriors
    with pytest.raises(H.HmmsortError):
        plan.posterior_decode(torch.zeros(T, dtype=torch.int16, device="cuda"))
    S = sm.nstates
    G0 = s1[:S]
    sil = abs(blocked.silent.sum() - G0[0]) / G0[0]
    occ = max(abs(blocked.occ[a].sum() - G0[sm.states[a] > 1].sum()) / G0[sm.states[a] > 1].sum() for a in range(N))
    print("sum_t silent / occ against G0 of the plan's E-step: rel %.3g / %.3g" % (sil, occ))
    assert sil <= 1e-9 and occ <= 1e-9
    tot = blocked.occ.sum(0) + blocked.silent           # >= 1: a sample inside two spikes counts for both templates
    assert blocked.onset.min() >= 0 and blocked.occ.max() <= 1 + 1e-8 and tot.min() >= 1 - 1e-8
    H.set_option("engine", H.ENGINE_STRICT)
    strict = Dev(H, y, sm, mu, sigma)
    assert strict.plan.info()["engine"] == H.ENGINE_STRICT
    d = dict(onset=np.abs(blocked.onset - strict.onset).max(), occ=np.abs(blocked.occ - strict.occ).max(),
             silent=np.abs(blocked.silent - strict.silent).max(),
             logz=abs(blocked.logz - strict.logz) / abs(strict.logz))
    differ = blocked.xm != strict.xm
    print("blocked against strict at T = 20 000:", d, "decodes differ at %d samples" % differ.sum())
    assert d["onset"] <= 1e-8 and d["occ"] <= 1e-8 and d["silent"] <= 1e-8 and d["logz"] <= 1e-10
    assert differ.mean() <= 1e-3
    assert np.allclose(cb, strict.plan.expected_counts(), rtol=1e-9, atol=0)


def test_short_warmup_is_flagged_and_the_host_entry_escalates(O, H):
    """a warm-up of 64 samples (option halo = 8 rounds up to the smallest the geometry allows) is one ring length at
    K = 60: the plan's certificates say so, and the host entry under engine = BLOCKED widens it"""
    import torch
    N, K, T, sigma = 2, 60, 6_000, 1.0
    y, sm, mu = make_case(H, N, K, T, sigma, 121, overlaps=True)
    g, z = PM.gamma(O, y, to_oracle_sm(O, sm), mu, sigma)
    tol = PM.tolerance(g)
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option("halo", 8)
    plan = H.Plan(T, sm, mu, sigma)
    assert plan.info()["engine"] == H.ENGINE_BLOCKED
    plan.posteriors(torch.from_numpy(y).cuda(), None, None, None, None)      # every output NULL: certificates only
    torch.cuda.synchronize()
    d = plan.diagnostics()
    print("halo %d: certificates %s" % (plan.info()["halo"], d[3:7]))
    assert d[3] + d[5] > 0, d
    plan.close()
    p = H.posteriors(y, sm, mu, sigma)
    esc = H.get_option("last_escalations")
    xm = H.posterior_decode(y, sm, mu, sigma)
    assert esc >= 1 and H.get_option("last_escalations") >= 1

    class R:
        onset, occ, silent, logz = p.onset, p.occ, p.silent, p.logz
    check_against_oracle("escalated host entry (%d escalations)" % esc, R, g, z, sm.states, tol)
    check_decode("escalated host entry", xm, g, tol)


def test_refusals_and_null_outputs(H):
    import torch
    y, sm, mu = make_case(H, 2, 20, 8_000, 0.3, 131, overlaps=True)
    H.set_option("engine", H.ENGINE_BLOCKED)
    plan = H.Plan(len(y), sm, mu, 0.3)
    dy = torch.from_numpy(y).cuda()
    # a blocked plan takes no time shard at all (set_shard is the wave and ring engines'): nothing sharded can
    # reach the posterior call
    with pytest.raises(H.HmmsortError) as e:
        plan.set_shard(0, 4_000, True, False)
    assert e.value.code == H._lib.EUNSUP
    # NULL outputs: only logz, then only silent, then only occ
    full = Dev(H, y, sm, mu, 0.3, plan=plan)
    lz = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
    plan.posteriors(dy, None, None, None, lz)
    torch.cuda.synchronize()
    assert float(lz.cpu()[0]) == full.logz
    si = torch.full((len(y),), np.nan, dtype=torch.float64, device="cuda")
    plan.posteriors(dy, None, None, si, None)
    oc = torch.full((2, len(y)), np.nan, dtype=torch.float64, device="cuda")
    plan.posteriors(dy, None, oc, None, None)
    xm = torch.zeros(len(y), dtype=torch.int16, device="cuda")
    plan.posterior_decode(xm)
    torch.cuda.synchronize()
    assert np.array_equal(si.cpu().numpy(), full.silent) and np.array_equal(oc.cpu().numpy(), full.occ)
    assert np.array_equal(xm.cpu().numpy(), full.xm)
    assert np.array_equal(plan.expected_counts(), full.plan.expected_counts())
    # set_model invalidates the posteriors
    plan.set_model(sm, mu, 0.35)
    with pytest.raises(H.HmmsortError):
        plan.expected_counts()
    plan.close()
    # a model whose two state columns do not fit the LDS: refused, with the limit and the way out named
    yb, smb, mub = make_case(H, 2, 100, 4_000, 0.3, 132, overlaps=True)
    assert smb.nstates == 10_000
    big = H.Plan(len(yb), smb, mub, 0.3)
    assert big.info()["engine"] == H.ENGINE_BLOCKED and big.stats_len() == 0
    with pytest.raises(H.HmmsortError) as e:
        big.posteriors(torch.from_numpy(yb).cuda(), None, None, None, lz)
    assert e.value.code == H._lib.EUNSUP and "156 KB" in str(e.value) and "strict" in str(e.value), str(e.value)
    big.close()


def test_host_entries_follow_the_engine_option(H):
    y, sm, mu = make_case(H, 2, 20, 12_000, 1.0, 141, overlaps=True)
    dev = blocked_dev(H, y, sm, mu, 1.0)
    p = H.posteriors(y, sm, mu, 1.0)                       # option "engine" is still ENGINE_BLOCKED
    assert H.get_option("last_escalations") == 0
    assert np.array_equal(p.onset, dev.onset) and np.array_equal(p.occ, dev.occ)
    assert np.array_equal(p.silent, dev.silent) and p.logz == dev.logz
    assert np.array_equal(H.posterior_decode(y, sm, mu, 1.0), dev.xm)
    # AUTO: the overlap model goes to the strict path, as before
    H.set_option("engine", H.ENGINE_AUTO)
    pa, xa = H.posteriors(y, sm, mu, 1.0), H.posterior_decode(y, sm, mu, 1.0)
    H.set_option("engine", H.ENGINE_STRICT)
    ps, xs = H.posteriors(y, sm, mu, 1.0), H.posterior_decode(y, sm, mu, 1.0)
    assert np.array_equal(pa.onset, ps.onset) and np.array_equal(pa.occ, ps.occ)
    assert np.array_equal(pa.silent, ps.silent) and pa.logz == ps.logz and np.array_equal(xa, xs)
    d = max(np.abs(p.onset - ps.onset).max(), np.abs(p.occ - ps.occ).max(), np.abs(p.silent - ps.silent).max())
    print("host entry, blocked against strict: max |d| %.3g" % d)
    assert d <= 1e-8
    # api.spike_confidence follows the option too
    x, ll = H.viterbi(y, sm, mu, 1.0)
    model = H.HMMSpikingModel(H.HMMSpikeTemplateModel(sm, mu, 1.0), x, ll, y)
    cs = H.spike_confidence(model)
    H.set_option("engine", H.ENGINE_BLOCKED)
    cb = H.spike_confidence(model)
    for a in range(2):
        assert np.array_equal(cb[a][0], cs[a][0]) and np.abs(cb[a][1] - cs[a][1]).max(initial=0.0) <= 5e-8


def test_sort_data_confidence_on_the_blocked_path(H):
    from test_gpu_posteriors import make_templates
    K, N, T = 20, 2, 6_000
    temps = make_templates(H, N, K)
    pp = [0.004, 0.003]
    y = H.create_signal(T, 0.5, pp, temps, seed=95)
    forms = temps[:, None, :]
    base = H.sort_data(forms, [1 / 0.25], pp, y, dosave=False, chunksize=2_000, confidence=True)
    H.set_option("engine", H.ENGINE_BLOCKED)
    out = H.sort_data(forms, [1 / 0.25], pp, y, dosave=False, chunksize=2_000, confidence=True)
    assert np.array_equal(out["mlseq"], base["mlseq"])
    worst = 0.0
    for a in range(N):
        assert np.array_equal(out["spiketimes"][a], base["spiketimes"][a]) and len(out["spiketimes"][a]) > 0
        worst = max(worst, float(np.abs(out["confidence"][a] - base["confidence"][a]).max()))
    print("sort_data confidences, blocked against the default path: max |d| %.3g" % worst)
    assert worst <= 1e-8
    # 2 x 60 = 3 600 states at chunksize 100 000 on 300 000 samples: the strict path would need 5.8 GB per chunk
    K, T = 60, 300_000
    temps = make_templates(H, N, K)
    pp = [0.002, 0.0015]
    y = H.create_signal(T, 0.5, pp, temps, seed=96)
    out = H.sort_data(temps[:, None, :], [1 / 0.25], pp, y, dosave=False, chunksize=100_000, confidence=True)
    for a in range(N):
        t, c = out["spiketimes"][a], out["confidence"][a]
        assert len(t) == len(c) and len(t) > 100 and np.all((c >= 0) & (c <= 1)) and np.all(np.diff(t) > 0)
        print("template %d: %d spikes, confidence %.3f .. %.3f, median %.3f" % (a, len(t), c.min(), c.max(), np.median(c)))
