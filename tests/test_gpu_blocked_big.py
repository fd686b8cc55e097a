"""Blocked E-step and posteriors with the state columns in device memory (csrc/generic_estep_big.hip, option
"blocked_hbm_columns"; DESIGN.md section 3.1c "Columns in device memory"): overlap models past the ~9 900 states
the LDS columns hold -- 2 x 100 (10 000 states), 3 x 60 (10 621) and 4 x 60 (21 123), the last two being what the
reference's command line builds for three and four templates.

Yardsticks and bars, none taken from what the device produced:
  1  E-step + M-step against the CPU oracle's update from its own alpha / beta: mu, sigma, lp, pp at 1e-8
     (test_gpu_blocked_estep.py's comparison)
  2  the same kernels forced (option 2) onto models the LDS kernels take, at 10^6 samples: 2 x 20 against
     tests/golden/estep_at_size/H.npz with test_gpu_estep_at_size's own checks, 2 x 60 against
     tests/golden/blocked_post_at_size/P60.npz (1e-8 on the window marginals and on the state sums, 1e-10 on logz)
     and against the LDS kernels on the same input at 1e-8 (the estep_at_size fixtures hold no 2 x 60 case)
  3  posteriors against the oracle's gamma: tol = posterior_model.tolerance(g), logz 1e-10, the decode equal to the
     oracle's arg max wherever its top-two gap exceeds 1e-6 (at most 1e-3 of the samples may be closer, asserted
     on the oracle alone); spike_confidence and expected_counts against posterior_model
  4  200 000 samples against the extended-precision reference (tests/golden/big_overlap_at_size): sum_t gamma per
     state, sigma, lp 1e-8 relative, mu 1e-8 absolute, logz 1e-10, window marginals 1e-8, decode as in 3
  5  the host entries and sort_data(confidence=True) follow the option; off, they return what they returned
  6  off by default: the refusal of tests/test_gpu_blocked_posteriors.py stands
A plan-API caller reads the boundary certificates and widens the warm-up when one fails (as the tests of P60 do);
plan_with_certificates() does that and the tests print the warm-up they ended at.  Every test prints the largest
error it saw before asserting; the figures measured on the MI355X are in DESIGN.md section 3.1c."""
import functools
import os
import sys

import numpy as np
import pytest

import posterior_model as PM
from conftest import to_oracle_sm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu
KEY = "blocked_hbm_columns"
RTOL = 1e-8


@pytest.fixture(autouse=True)
def default_options(H):
    for k in ("engine", "block", "halo", KEY):
        H.set_option(k, 0)
    try:
        yield
    finally:
        for k in ("engine", "block", "halo", KEY):
            H.set_option(k, 0)
        H.shutdown()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(np.abs(b), 1e-300)).max())


def plan_with_certificates(H, T, sm, mu, sigma, run, halos=(0, 512, 1024)):
    """a blocked plan on which run(plan) left every boundary certified: the default warm-up first, then wider ones.
    Returns (plan, what run returned, diagnostics)"""
    import torch
    first = None
    for halo in halos:
        H.set_option("halo", halo)
        plan = H.Plan(T, sm, mu, sigma)
        assert plan.info()["engine"] == H.ENGINE_BLOCKED
        res = run(plan)
        torch.cuda.synchronize()
        diag = plan.diagnostics()
        first = first or diag
        if diag[3] == 0 and diag[5] == 0:
            if halo:
                print("certified at a warm-up of %d samples (default: %s)" % (plan.info()["halo"], first[3:7]), flush=True)
            return plan, res, diag
        print("warm-up %d: certificates %s, widening" % (plan.info()["halo"], diag[3:7]), flush=True)
        plan.close()
    raise AssertionError(("certificates still fail at a warm-up of %d samples" % halos[-1], first, diag))


def estep_mstep(dy):
    import torch

    def run(plan):
        assert plan.stats_len() > 0
        stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
        out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
        plan.estep(dy, stats)
        plan.mstep(stats, out)
        return stats, out
    return run


class Post:
    """outputs of plan.posteriors + posterior_decode on the host"""

    def __init__(self, plan, dy, N, T):
        import torch
        on = torch.full((N, T), np.nan, dtype=torch.float64, device="cuda")
        oc, si = torch.full_like(on, np.nan), torch.full((T,), np.nan, dtype=torch.float64, device="cuda")
        lz = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
        xm = torch.zeros(T, dtype=torch.int16, device="cuda")
        plan.posteriors(dy, on, oc, si, lz)
        plan.posterior_decode(xm)
        torch.cuda.synchronize()
        self.onset, self.occ, self.silent = on.cpu().numpy(), oc.cpu().numpy(), si.cpu().numpy()
        self.logz, self.xm = float(lz.cpu()[0]), xm.cpu().numpy()


# ---------------------------------------------------------------------------------------------- small cases, oracle

SMALL = {(2, 100): 10_000, (3, 60): 10_621, (4, 60): 21_123}
T_SMALL = 4_096


@functools.lru_cache(maxsize=None)
def small_case(N, K):
    """inputs of a T = 4 096 case and the oracle's alpha / beta (0.7 GB each at 21 123 states)"""
    import hmmsort_amd as H
    from oracle import oracle as O
    import make_big_overlap_at_size as G
    temps, pp = G.overlap_model(N, K)
    y = H.create_signal(T_SMALL, 1.0, pp, temps, seed=400 + 10 * N + K)
    sm = H.StateMatrix.create(N, K, np.log(pp), True)
    assert sm.nstates == SMALL[(N, K)]
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    sigma = 1.15
    osm = to_oracle_sm(O, sm)
    al, be = O.forward(y, osm, mu, sigma), O.backward(y, osm, mu, sigma)
    return dict(y=y, sm=sm, osm=osm, mu=mu, sigma=sigma, al=al, be=be, N=N, K=K)


@pytest.mark.parametrize("N,K", list(SMALL))
def test_estep_matches_oracle(O, H, N, K):
    import torch
    c = small_case(N, K)
    sm, T = c["sm"], T_SMALL
    osm_n, omu, osig, olp, opp = O.update(c["al"], c["be"], c["osm"], c["mu"], c["sigma"], c["y"])
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option(KEY, 1)
    dy = torch.from_numpy(c["y"]).cuda()
    plan, (stats, out), diag = plan_with_certificates(H, T, sm, c["mu"], c["sigma"], estep_mstep(dy))
    try:
        info = plan.info()
        o, s = out.cpu().numpy(), stats.cpu().numpy()
    finally:
        plan.close()
    if H.get_option("halo") == 0:
        # default geometry: warm-up max(256, 4 (K - 1)) rounded up to 64 samples, blocks of twice that -- 8 blocks
        # and 7 certified boundaries at K = 60, 5 blocks of 896 at K = 100
        want = (512, 256, 8) if K == 60 else (896, 448, 5)
        assert (info["block"], info["halo"], info["nchains"]) == want, info
    S, KN = sm.nstates, K * N
    nsrc1 = int((sm.transitions["src"] == 1).sum())
    assert len(s) == 2 * S + nsrc1 + 2 and len(o) == KN + 1 + (nsrc1 - 1) + S
    mu = o[:KN].reshape((K, N), order="F")
    sig, lp, pp = o[KN], o[KN + 1:KN + nsrc1], o[KN + nsrc1:]
    assert len(lp) == len(olp) == nsrc1 - 1                  # xb[2:end]
    errs = dict(mu_abs=float(np.abs(mu - omu).max()), sigma=abs(sig - osig) / osig, lp=rel(lp, olp),
                pp_abs=float(np.abs(pp - opp).max()), mass=abs(s[:S].sum() - T) / T)
    print("%d x %d (%d states, block %d, halo %d, %d blocks, workspace %.2f GB): " % (
        N, K, S, info["block"], info["halo"], info["nchains"], info["workspace_bytes"] / 1e9)
        + "  ".join("%s %.3g" % kv for kv in errs.items()) + "  certificates %s" % (diag[3:7],), flush=True)
    assert np.allclose(mu, omu, rtol=RTOL, atol=1e-11), errs
    assert errs["sigma"] <= 1e-9 and errs["mass"] <= 1e-9, errs
    assert np.allclose(lp, olp, rtol=RTOL, atol=1e-11), errs
    assert np.allclose(pp, opp, rtol=RTOL, atol=1e-8), errs
    assert diag[3] == 0 and diag[5] == 0, diag


@pytest.mark.parametrize("N,K", [(3, 60), (4, 60)])
def test_posteriors_match_oracle(O, H, N, K):
    import torch
    c = small_case(N, K)
    sm, T, mu = c["sm"], T_SMALL, c["mu"]
    m = c["al"][:, -1].max()
    z = float(m + np.log(np.exp(c["al"][:, -1] - m).sum()))
    g = np.exp(c["al"] + c["be"] - z)                        # posterior_model.gamma from the cached sweeps
    tol = PM.tolerance(g)
    # the decode rule's cap, on the oracle alone
    top = np.sort(np.partition(g, -2, axis=0)[-2:], axis=0)
    close = (top[1] - top[0]) <= 1e-6
    assert close.mean() <= 1e-3, close.mean()
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option(KEY, 1)
    dy = torch.from_numpy(c["y"]).cuda()
    plan, dev, diag = plan_with_certificates(H, T, sm, mu, c["sigma"], lambda p: Post(p, dy, N, T))
    try:
        name = "%d x %d (%d states, halo %d)" % (N, K, sm.nstates, plan.info()["halo"])
        onset, occ, silent = PM.marginals(g, sm.states)
        errs = dict(onset=np.abs(dev.onset - onset).max(), occ=np.abs(dev.occ - occ).max(),
                    silent=np.abs(dev.silent - silent).max(), logz=abs(dev.logz - z) / abs(z))
        differ = int((dev.xm[~close] != PM.decode(g)[~close]).sum())
        print("%s: tol %.3g  " % (name, tol) + "  ".join("%s %.3g" % kv for kv in errs.items())
              + "  decode differs at %d of %d clear samples (%d within 1e-6)" % (differ, (~close).sum(), close.sum()),
              flush=True)
        assert errs["onset"] <= tol and errs["occ"] <= tol and errs["silent"] <= tol, errs
        assert errs["logz"] <= 1e-10, errs
        assert dev.xm.min() >= 1 and dev.xm.max() <= sm.nstates and differ == 0
        cnt = plan.expected_counts()
        erc = rel(cnt, onset.sum(1))
        print("%s: expected_counts rel %.3g" % (name, erc), flush=True)
        assert erc <= RTOL
        # per-spike confidence (and through it the trough mass) on the oracle's Viterbi path
        x, _ = O.viterbi(c["y"], c["osm"], mu, c["sigma"])
        x = np.asarray(x, dtype=np.int16)
        dx = torch.from_numpy(x).cuda()
        for J in (0, 2):
            got = plan.spike_confidence(dx, J)
            want = PM.confidence(g, sm.states, mu, x, J)
            worst = 0.0
            for a in range(N):
                assert np.array_equal(got[a][0], want[a][0])
                worst = max(worst, float(np.abs(got[a][1] - want[a][1]).max(initial=0.0)))
            print("%s: spike_confidence jitter %d: %d spikes, max |d| %.3g" % (
                name, J, sum(len(w[0]) for w in want), worst), flush=True)
            assert sum(len(w[0]) for w in want) > 0 and worst <= 5 * tol
    finally:
        plan.close()


# ------------------------------------------------------------------------------- the same kernels on known ground

def test_forced_on_2x20_meets_the_estep_fixture(H):
    import test_gpu_estep_at_size as E
    c = E.case("H")
    sm = E.product_sm(H, c)
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option(KEY, 2)
    s, o, diag, info, z = E.run_plan(H, c, sm, logz=True)
    assert info["engine"] == H.ENGINE_BLOCKED
    S, r = sm.nstates, c["ref"]
    first = np.nonzero(c["osm"].src == 1)[0]
    G0, G1, X = s[:S], s[S:2 * S], s[2 * S:2 * S + len(first)]
    assert len(s) == 2 * S + len(first) + 2
    errs = dict(G0=rel(G0, r["sg"]), G1=rel(G1, r["sgy"]), X=rel(X, r["sxi"][first]),
                Gamma0=rel(s[2 * S + len(first)], r["sg"][0] - r["gl"][0]), sum_y2=rel(s[-1], r["sum_y2"]),
                logz=abs(z - r["loglik"]) / abs(r["loglik"]))
    print("H (2 x 20, 10^6 samples) forced onto the device-memory columns: "
          + "  ".join("%s %.3g" % kv for kv in errs.items()), flush=True)
    assert errs["G0"] <= RTOL and errs["X"] <= RTOL and errs["Gamma0"] <= RTOL and errs["sum_y2"] <= RTOL, errs
    assert np.all(np.abs(G1 - r["sgy"]) <= RTOL * np.abs(r["sgy"]) + 1e-11 * r["sg"]), errs
    assert errs["logz"] <= 1e-10
    E.check_mstep("H forced", o, c, len(first) - 1)
    assert diag[3] == 0 and diag[5] == 0, diag


def test_forced_on_2x60_meets_the_fixture_and_the_lds_kernels(H):
    import torch
    import test_gpu_blocked_posteriors_at_size as B
    c = B.case("P60")
    r, N, T = c["ref"], c["N"], len(c["y"])
    sm = H.StateMatrix.create(N, c["K"], np.log(c["pp"]), True)
    assert sm.nstates == 3600
    H.set_option("engine", H.ENGINE_BLOCKED)
    dy = torch.from_numpy(c["y"]).cuda()
    res = {}
    for mode in (2, 0):
        H.set_option(KEY, mode)
        es = estep_mstep(dy)

        def run(plan):
            stats, out = es(plan)
            return stats.cpu().numpy(), out.cpu().numpy(), Post(plan, dy, N, T)
        # P60 needs 512 samples of warm-up (tests/test_gpu_blocked_posteriors_at_size.py); both kernels get the same
        plan, res[mode], diag = plan_with_certificates(H, T, sm, c["mu"], c["sigma"], run, halos=(512, 1024))
        info = plan.info()
        plan.close()
        print("P60 option %d: block %d, halo %d, workspace %.2f GB, certificates %s" % (
            mode, info["block"], info["halo"], info["workspace_bytes"] / 1e9, diag[3:7]), flush=True)
    (s2, o2, p2), (s0, o0, p0) = res[2], res[0]
    S = sm.nstates
    # against the extended-precision reference: state sums, logz, window marginals, decode
    worst = dict(onset=0.0, occ=0.0, silent=0.0)
    differ = 0
    for i, (lo, hi) in enumerate(c["win"]):
        worst["onset"] = max(worst["onset"], float(np.abs(p2.onset[:, lo:hi] - r["w%d_onset" % i]).max()))
        worst["occ"] = max(worst["occ"], float(np.abs(p2.occ[:, lo:hi] - r["w%d_occ" % i]).max()))
        worst["silent"] = max(worst["silent"], float(np.abs(p2.silent[lo:hi] - r["w%d_silent" % i]).max()))
        clear = r["w%d_gap" % i] > 1e-6
        differ += int((p2.xm[lo:hi][clear] != r["w%d_xm" % i][clear]).sum())
    eg, ez = rel(s2[:S], r["sg"]), abs(p2.logz - r["loglik"]) / abs(r["loglik"])
    print("P60 forced against the reference: " + "  ".join("%s %.3g" % kv for kv in worst.items())
          + "  G0 rel %.3g  logz rel %.3g  decode differs at %d clear window samples" % (eg, ez, differ), flush=True)
    assert max(worst.values()) <= 1e-8 and eg <= RTOL and ez <= 1e-10 and differ == 0
    assert float(r["close_share"]) <= 1e-3
    # against the LDS kernels: same recursion, same order of operations per state.  The whole statistics vector
    # [G0 | G1 | X | Gamma0 | sum y^2] and the whole M-step vector [mu | sigma | lp | pp (log, absolute)]
    KN = N * c["K"]
    assert len(o2) == len(o0) and len(s2) == len(s0)
    pp2, pp0 = o2[len(o2) - S:], o0[len(o0) - S:]
    fin = np.isfinite(pp0)                                   # log of a posterior that underflowed is -inf in both
    assert np.array_equal(fin, np.isfinite(pp2)) and np.array_equal(pp2[~fin], pp0[~fin])
    d = dict(stats=rel(s2[:S], s0[:S]), G1_abs=float(np.abs(s2[S:2 * S] - s0[S:2 * S]).max()),
             X_Gamma0_sumy2=rel(s2[2 * S:], s0[2 * S:]), mstep_mu=float(np.abs(o2[:KN] - o0[:KN]).max()),
             mstep_sigma_lp=rel(o2[KN:len(o2) - S], o0[KN:len(o0) - S]),
             mstep_pp=float(np.abs(pp2[fin] - pp0[fin]).max(initial=0.0)),
             onset=float(np.abs(p2.onset - p0.onset).max()), occ=float(np.abs(p2.occ - p0.occ).max()),
             silent=float(np.abs(p2.silent - p0.silent).max()), logz=abs(p2.logz - p0.logz) / abs(p0.logz),
             decode=float((p2.xm != p0.xm).mean()))
    print("P60 device-memory columns against LDS columns: " + "  ".join("%s %.3g" % kv for kv in d.items()), flush=True)
    assert max(v for k, v in d.items() if k != "decode") <= 1e-8, d
    assert d["decode"] <= 1e-3, d


# --------------------------------------------------------------------- at size, extended-precision reference

@functools.lru_cache(maxsize=None)
def big_case(name):
    import make_big_overlap_at_size as G
    import make_estep_at_size as G0
    y, osm, mu, sigma, pp, win = G.inputs(name)
    h = G0.hashes(y, osm, mu, sigma)
    path = os.path.join(G.OUT, name + ".npz")
    assert os.path.exists(path), "fixture %s is missing" % path
    ref = G.load(name)
    if str(ref["sha_y"]) != h["sha_y"] or str(ref["sha_model"]) != h["sha_model"] or \
            not np.array_equal(ref["windows"], win):
        print("case %s: the regenerated inputs do not hash to the fixture's (another random stream?): "
              "recomputing the reference live" % name)
        ref = G.reference(y, osm, mu, sigma, win, threads=16)
    N, K = G.CASES[name][:2]
    return dict(name=name, y=y, osm=osm, mu=mu, sigma=sigma, pp=pp, win=win, ref=ref, N=N, K=K)


@pytest.mark.parametrize("name", ["M3", "M4"])
def test_at_200k_against_reference(H, name):
    import torch
    c = big_case(name)
    r, N, K, T = c["ref"], c["N"], c["K"], len(c["y"])
    sm = H.StateMatrix.create(N, K, np.log(c["pp"]), True)
    tr = sm.transitions
    assert np.array_equal(tr["src"], c["osm"].src) and np.array_equal(tr["dst"], c["osm"].dst)
    assert np.array_equal(tr["lp"], c["osm"].val) and np.array_equal(sm.states, c["osm"].states)
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option(KEY, 1)
    dy = torch.from_numpy(c["y"]).cuda()
    es = estep_mstep(dy)
    q = PM.trough_values(c["mu"])
    st = c["osm"].states

    def run(plan):
        stats, out = es(plan)
        return stats.cpu().numpy(), out.cpu().numpy(), Post(plan, dy, N, T)
    plan, (s, o, p), diag = plan_with_certificates(H, T, sm, c["mu"], c["sigma"], run)
    try:
        info = plan.info()
        # trough mass through spike_confidence at jitter 0 on a path that sits in template a's trough state
        wtr = []
        for lo, hi in c["win"]:
            rows = []
            for a in range(N):
                others = np.ones(st.shape[1], bool)
                for b in range(N):
                    if b != a:
                        others &= st[b] == 1
                s_a = int(np.nonzero((st[a] == q[a]) & others)[0][0]) + 1
                x = np.ones(T, np.int16)
                x[lo:hi] = s_a
                got = plan.spike_confidence(torch.from_numpy(x).cuda(), 0)[a]
                assert np.array_equal(got[0], np.arange(lo + 1, hi + 1))
                rows.append(got[1])
            wtr.append(np.stack(rows))
    finally:
        plan.close()
    blk = info["block"]
    if H.get_option("halo") == 0:
        assert blk == 512 and info["nchains"] == (T + 511) // 512
    straddle = [(hi - 1) // blk > lo // blk for lo, hi in c["win"]]
    assert any(straddle), ("no window holds a block boundary", blk, c["win"])
    S, KN = sm.nstates, K * N
    nsrc1 = int((tr["src"] == 1).sum())
    mu = o[:KN].reshape((K, N), order="F")
    sig, lp = o[KN], o[KN + 1:KN + nsrc1]
    assert len(lp) == len(r["lp_new"])
    worst = dict(onset=0.0, occ=0.0, trough=0.0, silent=0.0)
    differ = close = total = 0
    for i, (lo, hi) in enumerate(c["win"]):
        worst["onset"] = max(worst["onset"], float(np.abs(p.onset[:, lo:hi] - r["w%d_onset" % i]).max()))
        worst["occ"] = max(worst["occ"], float(np.abs(p.occ[:, lo:hi] - r["w%d_occ" % i]).max()))
        worst["silent"] = max(worst["silent"], float(np.abs(p.silent[lo:hi] - r["w%d_silent" % i]).max()))
        worst["trough"] = max(worst["trough"], float(np.abs(wtr[i] - np.minimum(r["w%d_trough" % i], 1.0)).max()))
        clear = r["w%d_gap" % i] > 1e-6
        differ += int((p.xm[lo:hi][clear] != r["w%d_xm" % i][clear]).sum())
        close += int((~clear).sum())
        total += clear.size
    errs = dict(G0=rel(s[:S], r["sg"]), sigma=abs(sig - r["sigma_new"]) / r["sigma_new"], lp=rel(lp, r["lp_new"]),
                mu_abs=float(np.abs(mu - r["mu_new"]).max()), logz=abs(p.logz - r["loglik"]) / abs(r["loglik"]))
    print("%s (%d states, block %d, halo %d, %d blocks, workspace %.2f GB; %d of %d windows hold a boundary): " % (
        name, S, blk, info["halo"], info["nchains"], info["workspace_bytes"] / 1e9, sum(straddle), len(straddle))
        + "  ".join("%s %.3g" % kv for kv in list(errs.items()) + list(worst.items()))
        + "  decode differs at %d of %d clear samples (%d within 1e-6)  certificates %s" % (
            differ, total - close, close, diag[3:7]), flush=True)
    assert errs["G0"] <= RTOL and errs["sigma"] <= RTOL and errs["mu_abs"] <= 1e-8, errs
    assert np.allclose(lp, r["lp_new"], rtol=RTOL, atol=1e-12), errs
    assert errs["logz"] <= 1e-10, errs
    assert max(worst.values()) <= 1e-8, worst
    assert close / total <= 1e-3 and float(r["close_share"]) <= 1e-3
    assert differ == 0
    assert diag[3] == 0 and diag[5] == 0, diag


# ------------------------------------------------------------------------------------------------ host entries

def test_host_entries_follow_the_option(H):
    import torch
    c = small_case(3, 60)
    y, sm, mu, sigma, N, T = c["y"], c["sm"], c["mu"], c["sigma"], 3, T_SMALL
    KN = 60 * N
    # option off: AUTO builds a blocked plan, finds no blocked E-step and goes to the strict engine, as before
    sm_s, mu_s, sig_s = H.train_step(y, sm, mu.copy(order="F"), sigma)
    assert H.get_option("last_escalations") == 0
    H.set_option("engine", H.ENGINE_BLOCKED)
    p_s = H.posteriors(y, sm, mu, sigma)                      # no blocked posteriors either: strict
    H.set_option("engine", H.ENGINE_AUTO)
    H.shutdown()
    # option on
    H.set_option(KEY, 1)
    sm_b, mu_b, sig_b = H.train_step(y, sm, mu.copy(order="F"), sigma)
    esc = H.get_option("last_escalations")
    H.set_option("engine", H.ENGINE_BLOCKED)
    p_b = H.posteriors(y, sm, mu, sigma)
    esc_p = H.get_option("last_escalations")
    xm_b = H.posterior_decode(y, sm, mu, sigma)
    # the plan path under the geometry the host entry ended at
    dy = torch.from_numpy(y).cuda()
    es = estep_mstep(dy)
    plan, (stats, out), _ = plan_with_certificates(H, T, sm, mu, sigma, es)
    o = out.cpu().numpy()
    post = Post(plan, dy, N, T)
    plan.close()
    print("em_step: %d escalations, posteriors: %d; plan warm-up option %d" % (esc, esc_p, H.get_option("halo")))
    # which path the host entries took: this input certifies at the default warm-up (test_estep_matches_oracle
    # asserts that on the same case), so nothing escalates and the blocked path returns the plan's numbers bit for
    # bit -- the strict engine's log-domain sums agree with them to 1e-12, never to the last bit
    assert esc == 0 and esc_p == 0 and H.get_option("halo") == 0
    assert np.array_equal(mu_b, o[:KN].reshape((60, N), order="F")) and sig_b == o[KN]
    assert np.array_equal(p_b.onset, post.onset) and np.array_equal(p_b.occ, post.occ)
    assert np.array_equal(p_b.silent, post.silent) and p_b.logz == post.logz and np.array_equal(xm_b, post.xm)
    assert not np.array_equal(mu_b, mu_s) and not np.array_equal(p_b.onset, p_s.onset)
    d = dict(mu=float(np.abs(mu_b - mu_s).max()), sigma=abs(sig_b - sig_s) / sig_s,
             lp=rel(sm_b.transitions["lp"], sm_s.transitions["lp"]),
             plan_mu=float(np.abs(mu_b - o[:KN].reshape((60, N), order="F")).max()),
             onset=float(np.abs(p_b.onset - p_s.onset).max()), occ=float(np.abs(p_b.occ - p_s.occ).max()),
             silent=float(np.abs(p_b.silent - p_s.silent).max()), logz=abs(p_b.logz - p_s.logz) / abs(p_s.logz),
             plan_onset=float(np.abs(p_b.onset - post.onset).max()))
    print("3 x 60 host entries, option on against off (strict): " + "  ".join("%s %.3g" % kv for kv in d.items()),
          flush=True)
    assert np.allclose(mu_b, mu_s, rtol=RTOL, atol=1e-11) and d["sigma"] <= 1e-9, d
    assert np.allclose(sm_b.transitions["lp"], sm_s.transitions["lp"], rtol=RTOL, atol=1e-11), d
    assert max(d["onset"], d["occ"], d["silent"], d["plan_mu"], d["plan_onset"]) <= 1e-8 and d["logz"] <= 1e-10, d


def test_sort_data_confidence_takes_the_blocked_path(H, monkeypatch):
    import test_gpu_posteriors as TP
    import hmmsort_amd.api as api
    K, N, T = 60, 3, 20_000
    temps = TP.make_templates(H, N, K)
    pp = [0.004, 0.003, 0.002]
    y = H.create_signal(T, 0.5, pp, temps, seed=97)
    forms = temps[:, None, :]
    engines = []
    inner = api._posterior_plan

    def spy(*a, **k):
        plan = inner(*a, **k)
        engines.append(plan.info()["engine"])
        return plan
    monkeypatch.setattr(api, "_posterior_plan", spy)
    base = H.sort_data(forms, [1 / 0.25], pp, y, dosave=False, chunksize=20_000, confidence=True)
    assert engines == [H.ENGINE_STRICT], engines                # one chunk, 3.4 GB of alpha and beta
    H.shutdown()
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option(KEY, 1)
    out = H.sort_data(forms, [1 / 0.25], pp, y, dosave=False, chunksize=20_000, confidence=True)
    assert engines == [H.ENGINE_STRICT, H.ENGINE_BLOCKED], engines
    assert np.array_equal(out["mlseq"], base["mlseq"])
    worst, n = 0.0, 0
    for a in range(N):
        assert np.array_equal(out["spiketimes"][a], base["spiketimes"][a])
        n += len(out["spiketimes"][a])
        worst = max(worst, float(np.abs(out["confidence"][a] - base["confidence"][a]).max(initial=0.0)))
    print("sort_data, 3 x 60, one chunk of 20 000: %d spikes, confidences blocked against strict: max |d| %.3g"
          % (n, worst), flush=True)
    assert n > 50 and worst <= 1e-8


def test_off_by_default(H):
    import torch
    import test_gpu_posteriors as TP
    assert H.get_option(KEY) == 0
    H.set_option("engine", H.ENGINE_BLOCKED)
    yb, smb, mub = TP.make_case(H, 2, 100, 4_000, 0.3, 132, overlaps=True)
    assert smb.nstates == 10_000
    big = H.Plan(len(yb), smb, mub, 0.3)
    try:
        assert big.info()["engine"] == H.ENGINE_BLOCKED and big.stats_len() == 0
        lz = torch.zeros(1, dtype=torch.float64, device="cuda")
        with pytest.raises(H.HmmsortError) as e:
            big.posteriors(torch.from_numpy(yb).cuda(), None, None, None, lz)
        assert e.value.code == H._lib.EUNSUP and "156 KB" in str(e.value) and "strict" in str(e.value), str(e.value)
        with pytest.raises(H.HmmsortError) as e:
            big.estep(torch.from_numpy(yb).cuda(), torch.zeros(8, dtype=torch.float64, device="cuda"))
        assert e.value.code == H._lib.EUNSUP
        # the option is read when a plan is created: this plan stays what it is
        H.set_option(KEY, 1)
        assert big.stats_len() == 0
        on = H.Plan(len(yb), smb, mub, 0.3)
        assert on.stats_len() == 2 * 10_000 + int((smb.transitions["src"] == 1).sum()) + 2
        on.close()
        # 2 x 20 fits the LDS: option 1 leaves it on the LDS kernels (same workspace), option 2 moves it
        ys, sms, mus = TP.make_case(H, 2, 20, 4_000, 0.3, 133, overlaps=True)
        ws = {}
        for mode in (0, 1, 2):
            H.set_option(KEY, mode)
            pl = H.Plan(len(ys), sms, mus, 0.3)
            st = torch.zeros(pl.stats_len(), dtype=torch.float64, device="cuda")
            pl.estep(torch.from_numpy(ys).cuda(), st)
            torch.cuda.synchronize()
            ws[mode] = (pl.info()["workspace_bytes"], st.cpu().numpy())
            pl.close()
        assert ws[0][0] == ws[1][0] and ws[0][1].tobytes() == ws[1][1].tobytes()
        assert ws[2][0] > ws[0][0] and np.allclose(ws[2][1], ws[0][1], rtol=1e-9, atol=1e-12)
    finally:
        big.close()
