"""The escalation ladder of the host-buffer entry points (hmmsort_viterbi, hmmsort_em_step, hmmsort_posteriors;
csrc/host_calls.cpp): the rows that differ between the three entries and that no other test holds.  escalate = 0
returns the first attempt as it is, a named engine that runs out of retries answers HMMSORT_ENOCONV (and one whose
second sweep certifies itself does not), a named engine that cannot serve the call is replaced by the strict one,
and a plan rebuilt on the way is not cached.

Every expected value is what the library did before the three entries shared one driver; inputs are those of
test_gpu_blocked.py, test_gpu_blocked_estep.py, test_gpu_blocked_posteriors.py and test_gpu_host_cache.py."""
import numpy as np
import pytest

from test_gpu_blocked_estep import overlap_case
from test_gpu_posteriors import make_case

pytestmark = pytest.mark.gpu

OPTIONS = dict(engine=0, block=0, halo=0, escalate=1, plan_cache=4, strict_limit_mb=0, blocked_hbm_columns=0,
               tie_debug=0)


@pytest.fixture(autouse=True)
def default_options(H):
    H.shutdown()
    for k, v in OPTIONS.items():
        H.set_option(k, v)
    try:
        yield
    finally:
        for k, v in OPTIONS.items():
            H.set_option(k, v)
        H.shutdown()


def _templates(H, K, n):
    par = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)][:n]
    return np.asfortranarray(np.stack([H.create_spike_template(K, a, b, c) for a, b, c in par], 1))


def short_warmup_decode_case(H):
    """test_gpu_blocked.py::test_warmup_too_short_is_flagged_and_escalated"""
    temps = _templates(H, 60, 2)
    pp = [0.02, 0.02]
    sm = H.StateMatrix.create(2, 60, np.log(pp), True)
    y = H.create_signal(20000, 0.3, pp, temps, seed=13)
    return y, sm, temps


def plan_decode(H, y, sm, mu, sigma):
    import torch
    p = H.Plan(len(y), sm, mu, sigma)
    dy = torch.from_numpy(y).cuda()
    dx = torch.zeros(len(y), dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    p.viterbi(dy, dx, dll)
    torch.cuda.synchronize()
    d = p.diagnostics()
    info = p.info()
    p.close()
    return dx.cpu().numpy(), float(dll.cpu()[0]), d, info


def test_escalate_off_decode_returns_the_first_attempt(H):
    y, sm, temps = short_warmup_decode_case(H)
    H.set_option("block", 256)
    H.set_option("halo", 64)          # shorter than one spike: boundaries fail the certificate
    H.set_option("escalate", 0)
    x, ll = H.viterbi(y, sm, temps, 0.3)
    assert H.get_option("last_escalations") == 0
    xp, llp, d, info = plan_decode(H, y, sm, temps, 0.3)
    assert info["engine"] == H.ENGINE_BLOCKED
    assert d[0] > 0, d
    assert np.array_equal(x, xp) and ll == llp


def test_escalate_off_em_step_returns_the_first_attempt(H):
    import torch
    y, sm, mu0 = overlap_case(H, 2, 60, 20_000, seed=11)
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option("halo", 8)           # rounds up to 64 samples, one ring length at K = 60
    H.set_option("escalate", 0)
    sm_n, mu_n, sig_n = H.train_step(y, sm, mu0.copy(order="F"), 0.4)
    assert H.get_option("last_escalations") == 0
    plan = H.Plan(len(y), sm, mu0, 0.4)
    assert plan.info()["engine"] == H.ENGINE_BLOCKED
    dy = torch.from_numpy(y).cuda()
    stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
    out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
    plan.estep(dy, stats)
    plan.mstep(stats, out)
    torch.cuda.synchronize()
    d = plan.diagnostics()
    assert d[3] + d[5] > 0, d
    o = out.cpu().numpy()
    KN, S = sm.K * sm.N, sm.nstates
    nlp = plan.mstep_len() - KN - 1 - S
    plan.close()
    assert np.array_equal(mu_n, o[:KN].reshape(sm.N, sm.K).T) and sig_n == o[KN]
    want = H.StateMatrix.from_states(sm.states, o[KN + 1 + nlp:], sm.K, o[KN + 1:KN + 1 + nlp].copy(),
                                     sm.resolve_overlaps)
    assert np.array_equal(sm_n.transitions["lp"], want.transitions["lp"])


def test_escalate_off_posteriors_return_the_first_attempt(H):
    import torch
    N, K, T, sigma = 2, 60, 6_000, 1.0
    y, sm, mu = make_case(H, N, K, T, sigma, 121, overlaps=True)
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option("halo", 8)
    H.set_option("escalate", 0)
    p = H.posteriors(y, sm, mu, sigma)
    assert H.get_option("last_escalations") == 0
    plan = H.Plan(T, sm, mu, sigma)
    assert plan.info()["engine"] == H.ENGINE_BLOCKED
    on = torch.full((N, T), np.nan, dtype=torch.float64, device="cuda")
    oc, si = torch.full_like(on, np.nan), torch.full((T,), np.nan, dtype=torch.float64, device="cuda")
    lz = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
    plan.posteriors(torch.from_numpy(y).cuda(), on, oc, si, lz)
    torch.cuda.synchronize()
    d = plan.diagnostics()
    plan.close()
    assert d[3] + d[5] > 0, d
    assert np.array_equal(p.onset, on.cpu().numpy()) and np.array_equal(p.occ, oc.cpu().numpy())
    assert np.array_equal(p.silent, si.cpu().numpy()) and p.logz == float(lz.cpu()[0])


def test_named_wave_engine_with_open_ties_is_enoconv(H):
    # test_gpu_host_cache.py::test_strict_fallback_that_does_not_fit_returns_the_time_parallel_path: twins on a ring
    # model, resolver off.  Under AUTO the strict engine decides; a named engine has nowhere to go.
    K, N, T = 40, 2, 200_000
    t1 = H.create_spike_template(K, 3.0, 0.8, 0.2)
    temps = np.asfortranarray(np.stack([t1, t1], 1))
    pp = [0.004, 0.004]
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    y = H.create_signal(T, 0.3, pp, temps, seed=3)
    H.set_option("tie_debug", 2)
    H.set_option("engine", H.ENGINE_WAVE)
    with pytest.raises(H.HmmsortError) as e:
        H.viterbi(y, sm, temps, 0.3)
    assert e.value.code == H._lib.ENOCONV and "near-ties" in str(e.value), str(e.value)
    assert H.get_option("last_escalations") == 1


def test_named_blocked_engine_drops_the_pair_sweep_and_returns_the_generic_sweeps_path(H):
    # test_gpu_blocked.py::test_pair_sweep_duplicate_templates_fall_back under a named engine.  The pair sweep flags
    # near-ties on the path and is dropped once; the generic blocked sweep (the reference's operation order per
    # block) then certifies every boundary and flags nothing, so the call never comes to the rung where a named
    # engine would answer ENOCONV: it returns that sweep's path, which is the strict engine's.
    K, T = 30, 30_000
    t1 = H.create_spike_template(K, 3.0, 0.8, 0.2)
    temps = np.asfortranarray(np.stack([t1, t1], 1))
    pp = [0.004, 0.004]
    sm = H.StateMatrix.create(2, K, np.log(pp), True)
    y = H.create_signal(T, 0.3, pp, temps, seed=9)
    H.set_option("engine", H.ENGINE_STRICT)
    xs, lls = H.viterbi(y, sm, temps, 0.3)
    H.shutdown()
    H.set_option("engine", H.ENGINE_BLOCKED)
    x, ll = H.viterbi(y, sm, temps, 0.3)
    assert H.get_option("last_escalations") >= 1           # the pair sweep was dropped
    assert np.array_equal(x, xs) and abs(ll - lls) <= 1e-9 * abs(lls)
    p = H.Plan(T, sm, temps, 0.3)                           # the plan a first attempt builds: pair sweep, open ties
    sweep = p.overlap_sweep()
    p.close()
    _, _, d, info = plan_decode(H, y, sm, temps, 0.3)
    assert info["engine"] == H.ENGINE_BLOCKED and sweep == 2 and d[0] + d[7] > 0, (sweep, d)


def test_named_blocked_engine_that_cannot_serve_em_step_ends_on_strict(H):
    import time
    y, sm, mu0 = overlap_case(H, 3, 60, 4_096, seed=17)
    assert sm.nstates == 10_621
    res = {}
    for engine in (H.ENGINE_BLOCKED, H.ENGINE_STRICT):
        H.set_option("engine", engine)
        t0 = time.perf_counter()
        res[engine] = H.train_step(y, sm, mu0.copy(order="F"), 0.4)
        print("em_step, 10 621 states x 4 096 samples, engine %d: %.2f s" % (engine, time.perf_counter() - t0))
        assert H.get_option("last_escalations") == 0
        H.shutdown()
    plan = H.Plan(len(y), sm, mu0, 0.4)                  # option "engine" is ENGINE_STRICT: the strict plan
    assert plan.info()["engine"] == H.ENGINE_STRICT
    plan.close()
    H.set_option("engine", H.ENGINE_BLOCKED)
    plan = H.Plan(len(y), sm, mu0, 0.4)                  # the blocked plan exists but has no E-step for this model
    assert plan.info()["engine"] == H.ENGINE_BLOCKED and plan.stats_len() == 0
    plan.close()
    (sm_b, mu_b, sig_b), (sm_s, mu_s, sig_s) = res[H.ENGINE_BLOCKED], res[H.ENGINE_STRICT]
    assert np.isfinite(mu_s).all() and np.array_equal(mu_b, mu_s) and sig_b == sig_s
    assert np.array_equal(sm_b.transitions["lp"], sm_s.transitions["lp"])


def test_rebuilt_plan_is_not_cached_and_a_first_attempt_plan_is(H):
    y, sm, temps = short_warmup_decode_case(H)
    H.set_option("block", 256)
    H.set_option("halo", 64)
    x1, ll1 = H.viterbi(y, sm, temps, 0.3)
    e1 = H.get_option("last_escalations")
    x2, ll2 = H.viterbi(y, sm, temps, 0.3)
    e2 = H.get_option("last_escalations")
    assert e1 >= 1 and e2 == e1                            # the second call starts from the options again
    assert np.array_equal(x1, x2) and ll1 == ll2
    H.shutdown()
    H.set_option("block", 0)
    H.set_option("halo", 0)
    x3, ll3 = H.viterbi(y, sm, temps, 0.3)
    assert H.get_option("last_escalations") == 0
    x4, ll4 = H.viterbi(y, sm, temps, 0.3)                 # on the plan the first call left
    assert H.get_option("last_escalations") == 0
    assert np.array_equal(x3, x1) and np.array_equal(x3, x4) and ll3 == ll4
