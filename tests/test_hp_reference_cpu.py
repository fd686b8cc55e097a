"""Pins the extended-precision E-step reference (oracle/hp_estep.c, oracle/hp.py) on the CPU, and with it
gives the fp64 oracle its first check against an independent implementation.

1. Exact enumeration: on tiny models every path is enumerated with `decimal` at 50 digits; gamma, xi, the
   log-likelihood and the M-step follow from their definitions.  The reference's outputs are long-double
   results rounded once to double: they must sit within 2 ulp (4.5e-16 relative; 1e-300 absolute where the
   exact value is 0).
2. Oracle against reference on the shapes the device tests use: the project's bar, 1e-8 relative (atol 1e-11
   on mu, 1e-8 on pp); gamma on every state and sample, 1e-8 absolute.  The largest difference per quantity
   and case is printed; DESIGN.md section 2 records them as the measured fp64 floor per T.
3. Invariances: block length and emission threads change no bit; sum gamma = T to 1e-14 T; windows equal the
   columns of a full run.
"""
import decimal
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

D = decimal.Decimal
BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]


@pytest.fixture(scope="module")
def HP():
    from oracle import hp
    hp.build()
    return hp


# ---------------------------------------------------------------- 1. exact enumeration

def enumerate_exact(y, sm, mu, sigma):
    """gamma (T x S), xi sums per transition, log P, and the M-step, from the definitions, in Decimal"""
    T, S, N, K = len(y), sm.nstates, sm.N, sm.K
    yd = [D(float(v)) for v in y]
    sig = D(float(sigma))
    pi = D("3.14159265358979323846264338327950288419716939937510582097494")
    norm = sig * (2 * pi).sqrt()
    # the model's per-state means are doubles, added in template order by every implementation
    mean = []
    for j in range(S):
        m = 0.0
        for l in range(N):
            m += float(mu[sm.states[l, j] - 1, l])
        mean.append(D(m))
    b = [[(-(yd[t] - mean[j]) ** 2 / (2 * sig * sig)).exp() / norm for j in range(S)] for t in range(T)]
    A = {}
    for r, (i, j, v) in enumerate(zip(sm.src, sm.dst, sm.val)):
        A[(int(i) - 1, int(j) - 1)] = (r, D(float(v)).exp())
    P = D(0)
    gam = [[D(0)] * S for _ in range(T)]
    xi = [D(0)] * len(sm.src)
    for path in itertools.product(range(S), repeat=T):
        w = b[0][path[0]]                       # alpha_0 = b(y_0): no initial distribution
        rs = []
        for t in range(1, T):
            e = A.get((path[t - 1], path[t]))
            if e is None:
                w = None
                break
            rs.append(e[0])
            w = w * e[1] * b[t][path[t]]
        if w is None:
            continue
        P += w
        for t in range(T):
            gam[t][path[t]] += w
        for r in rs:
            xi[r] += w
    gam = [[g / P for g in row] for row in gam]
    xi = [x / P for x in xi]
    sg = [sum(gam[t][j] for t in range(T)) for j in range(S)]
    sgy = [sum(gam[t][j] * yd[t] for t in range(T)) for j in range(S)]
    first = [r for r in range(len(sm.src)) if sm.src[r] == 1]
    den0 = sum(gam[t][0] for t in range(T - 1))
    lp_new = [(xi[r] / den0).ln() for r in first[1:]] if T > 1 else []      # T = 1 has no transition
    pp = [g.ln() for g in gam[0]]
    mu_new = [[D(0)] * N for _ in range(K)]
    for l in range(N):
        for k in range(2, K + 1):
            js = [j for j in range(S) if sm.states[l, j] == k and sum(sm.states[:, j] >= 2) == 1]
            mu_new[k - 1][l] = sum(sgy[j] for j in js) / sum(sg[j] for j in js)
    m_new = [sum((mu_new[sm.states[l, j] - 1][l] for l in range(N)), D(0)) for j in range(S)]
    x2 = sum(gam[t][j] * (yd[t] - m_new[j]) ** 2 for t in range(T) for j in range(S))
    sigma_new = (x2 / sum(sg)).sqrt()
    return dict(gam=gam, xi=xi, loglik=P.ln(), sg=sg, sgy=sgy, lp_new=lp_new, pp=pp, mu=mu_new, sigma=sigma_new)


def ulp_err(got, exact):
    """largest error relative to the exact value (absolute / 1e-300 where the exact value is 0, scaled to 4.5e-16)"""
    worst = 0.0
    for g, e in zip(np.ravel(got), exact):
        if e == 0:
            worst = max(worst, abs(float(g)) / 1e-300 * 4.5e-16)
        else:
            worst = max(worst, float(abs((D(float(g)) - e) / e)))
    return worst


@pytest.mark.parametrize("N,overlaps,T,sigma,seed", [
    (1, False, 5, 1.0, 1), (1, False, 5, 0.6, 2), (2, False, 5, 1.0, 3), (2, False, 4, 0.7, 4),
    (2, True, 5, 1.0, 5), (2, True, 4, 0.8, 6), (2, True, 1, 1.0, 7), (1, False, 2, 1.0, 8),
    (2, False, 5, 1.0, -9),       # negative seed: template 1 can no longer start (its transitions leave the list)
])
def test_exact_enumeration(O, HP, N, overlaps, T, sigma, seed):
    decimal.getcontext().prec = 50
    K = 3
    rng = np.random.default_rng(abs(seed))
    pp = rng.uniform(0.1, 0.3, N)
    lp = np.log(pp)
    if seed < 0:
        lp[1] = -np.inf
    sm = O.state_matrix(N, K, lp, overlaps)
    assert sm.nstates == {(1, False): 3, (2, False): 5, (2, True): 9}[(N, overlaps)]
    assert (len(sm.src) < len(O.state_matrix(N, K, np.log(pp), overlaps).src)) == (seed < 0)
    mu = np.asfortranarray(rng.uniform(-1.2, 1.2, (K, N)))
    mu[0, :] = 0
    y = rng.standard_normal(T) * 1.3
    ex = enumerate_exact(y, sm, mu, sigma)
    E, M = HP.train_step(y, sm, mu, sigma, block=2, windows=[(0, T)])
    errs = dict(gamma=ulp_err(E.windows[0], [g for row in ex["gam"] for g in row]),
                sg=ulp_err(E.sg.astype(np.float64), ex["sg"]), sgy=ulp_err(E.sgy.astype(np.float64), ex["sgy"]),
                xi=ulp_err(E.sxi.astype(np.float64), ex["xi"]), loglik=ulp_err([np.float64(E.loglik)], [ex["loglik"]]),
                pp=ulp_err(M.pp, ex["pp"]), sigma=ulp_err([M.sigma], [ex["sigma"]]))
    if T > 1:
        errs["lp_new"] = ulp_err(M.lp_new, ex["lp_new"])
    errs["mu"] = ulp_err(M.mu[1:].ravel(order="C"), [ex["mu"][k][l] for k in range(1, K) for l in range(N)])
    print("enumeration N=%d ov=%d T=%d sigma=%g (S=%d): " % (N, overlaps, T, sigma, sm.nstates)
          + "  ".join("%s %.2g" % kv for kv in errs.items()))
    assert np.all(M.mu[0] == 0)
    for k, v in errs.items():
        assert v <= 4.5e-16, (k, v)


# ---------------------------------------------------------------- 2. the fp64 oracle against the reference

def ring_case(H, N, K, T, sigma, seed):
    rng = np.random.default_rng(seed)
    amps = [(BASE[i % 4][0] * (1 + 0.13 * (i // 4)), BASE[i % 4][1] + 0.03 * (i // 4), BASE[i % 4][2])
            for i in range(N)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *a) for a in amps], 1))
    pp = rng.uniform(1e-3, 4e-3, N) * min(1.0, 60.0 / K) * min(1.0, 4.0 / N)
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    mu = np.asfortranarray(temps * rng.uniform(0.7, 1.2, N)[None, :])
    mu[0, :] = 0
    return y, np.log(pp), mu, 1.15 * sigma, False


def overlap_case(H, N, K, T, sigma, seed):
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *BASE[i][:3]) for i in range(N)], 1))
    pp = [0.012, 0.008, 0.006][:N]
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    mu = np.asfortranarray(temps * 0.85)
    mu[0, :] = 0
    return y, np.log(pp), mu, 1.15 * sigma, True


def random_init_case(H, N, K, T, sigma, seed):
    """the reference's own start (baumwelch.jl:311-322): p0 = 2^(-3K/2), sigma = std(y), random templates"""
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                        H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    y = H.create_signal(T, sigma, [0.004, 0.002], temps, seed=seed)
    rng = np.random.default_rng(3)
    s = float(np.std(y, ddof=1))
    mu = np.ones((K, N), order="F")
    for i in range(N):
        mu[:, i] = H.create_spike_template(K, 3 * s * rng.random(), 0.5 + 0.1 * rng.standard_normal(), 1.5 * rng.random())
    mu[0, :] = 0
    return y, np.log(np.full(N, 2.0 ** (-3 * K / 2))), mu, s, False


def dying_case(H, N, K, T, sigma, seed):
    """template 1's entry probability is zero: its transitions leave the list (types.jl:121)"""
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *BASE[i]) for i in range(N)], 1))
    pp = [0.004, 0.002, 0.003]
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    lp = np.log(pp)
    lp[1] = -np.inf
    mu = np.asfortranarray(temps * 0.95)
    mu[0, :] = 0
    return y, lp, mu, 1.15 * sigma, False


ORACLE_CASES = [(ring_case, N, K, T, s, 40 + i) for i, (N, K, T) in enumerate([
    (1, 40, 9_000), (2, 30, 6_000), (4, 60, 30_000), (4, 60, 40_001), (8, 33, 12_000), (16, 40, 10_000),
    (8, 128, 9_000), (10, 180, 9_000)]) for s in (0.3, 1.0)]
ORACLE_CASES += [(overlap_case, 2, 20, 20_000, s, 60) for s in (0.3, 1.0)]
ORACLE_CASES += [(overlap_case, 3, 12, 12_000, s, 61) for s in (0.3, 1.0)]
ORACLE_CASES += [(random_init_case, 3, 40, 12_000, s, 8) for s in (0.3, 1.0)]
ORACLE_CASES += [(ring_case, 4, 60, 200_000, s, 70) for s in (0.3, 1.0)]


def compare_with_oracle(name, O, HP, y, sm, mu, sigma, full_gamma=True):
    T = len(y)
    a = O.forward(y, sm, mu, sigma)
    b = O.backward(y, sm, mu, sigma)
    _, omu, osig, olp, opp = O.update(a, b, sm, mu, sigma, y)
    E, M = HP.train_step(y, sm, mu, sigma, threads=4, windows=[(0, T)] if full_gamma else ())
    fin = np.isfinite(omu) & np.isfinite(M.mu)
    errs = dict(mu_abs=np.abs(omu - M.mu)[fin].max(),
                mu_rel=(np.abs(omu - M.mu)[fin] / np.maximum(np.abs(M.mu[fin]), 1e-300)).max(),
                sigma=abs(osig - M.sigma) / M.sigma, lp=np.abs(olp / M.lp_new - 1).max(),
                pp=(np.abs(opp - M.pp) / (1e-8 + 1e-8 * np.abs(M.pp))).max() * 1e-8,
                mass=abs(float(E.sg.sum() - T)) / T)
    if full_gamma:
        # the oracle's gamma is normalised per column (baumwelch.jl:216-224, hmm_oracle_update); the posterior
        # tests' restatement PM.gamma divides by the one global z instead and inherits the O(t) magnitude of
        # the unscaled log alpha/beta: its error grows with T and is printed, not asserted
        ab = a + b
        m = ab.max(0)
        col = m + np.log(np.exp(ab - m).sum(0))
        errs["gamma"] = np.abs(np.exp(ab - col) - E.windows[0].T).max()
        m = a[:, -1].max()
        z = m + np.log(np.exp(a[:, -1] - m).sum())
        errs["gamma_global_z"] = np.abs(np.exp(ab - z) - E.windows[0].T).max()
        errs["loglik"] = abs(z - float(E.loglik)) / abs(z)
        del ab
    print("oracle vs reference %-34s T=%-7d S=%-5d " % (name, T, sm.nstates)
          + "  ".join("%s %.2g" % kv for kv in errs.items()), flush=True)
    assert np.all(np.isfinite(omu[1:])) and np.all(np.isfinite(M.mu))
    assert np.allclose(omu[fin], M.mu[fin], rtol=1e-8, atol=1e-11), errs
    assert errs["sigma"] <= 1e-8 and errs["lp"] <= 1e-8, errs
    assert np.allclose(opp, M.pp, rtol=1e-8, atol=1e-8), errs
    assert errs["mass"] <= 1e-14
    if full_gamma:
        assert errs["gamma"] <= 1e-8 and errs["loglik"] <= 1e-10, errs
    return errs


@pytest.mark.parametrize("make,N,K,T,sigma,seed", ORACLE_CASES,
                         ids=["%s-%dx%d-T%d-s%g" % (c[0].__name__[:-5], c[1], c[2], c[3], c[4]) for c in ORACLE_CASES])
def test_oracle_against_reference(O, H, HP, make, N, K, T, sigma, seed):
    """Measured differences: DESIGN.md section 2 (table 'fp64 floor')."""
    y, lp, mu, sig, ov = make(H, N, K, T, sigma, seed)
    sm = O.state_matrix(N, K, lp, ov)
    compare_with_oracle("%s %dx%d sigma=%g" % (make.__name__[:-5], N, K, sigma), O, HP, y, sm, mu, sig)


def test_template_that_can_no_longer_start(O, H, HP):
    """log p = -Inf for template 1 (as in test_gpu_em_loops): its transitions leave the list, its ring only holds
    what alpha_0 put there and is empty after K - 1 samples.  On that list the reference's logsumexpl(-Inf, -Inf)
    is NaN (utils.jl:24-32) and the oracle restates that; the yardstick is, as in test_gpu_em_loops, the oracle on
    the same model with log p = -600 in place of -Inf: the same posteriors up to e^-600.  Bars as everywhere in
    this file: mu of the live and of the dead template (the latter from the posterior mass of the first K - 1
    samples only, where the oracle's is finite), sigma, lp_new of the live templates, pp."""
    for sigma in (0.3, 1.0):
        y, lp, mu, sig, _ = dying_case(H, 3, 30, 40_000, sigma, 6)
        sm = O.state_matrix(3, 30, lp, False)
        _, nmu, nsig, _, _ = O.train_step(y, sm, mu.copy(order="F"), sig)
        assert np.isnan(nsig) and np.all(np.isnan(nmu[1:]))
        lp6 = lp.copy()
        lp6[1] = -600.0
        _, omu, osig, olp, opp = O.train_step(y, O.state_matrix(3, 30, lp6, False), mu.copy(order="F"), sig)
        E, M = HP.train_step(y, sm, mu, sig, threads=4)
        assert np.all(np.isfinite(M.mu)) and len(M.lp_new) == 2 and len(olp) == 3
        live, fin = [0, 2], np.isfinite(omu[:, 1])
        errs = dict(mu_live=np.abs(omu[:, live] - M.mu[:, live]).max(),
                    mu_dead=np.abs(omu[fin, 1] - M.mu[fin, 1]).max(), dead_finite=int(fin.sum()),
                    sigma=abs(osig - M.sigma) / M.sigma, lp=np.abs(olp[live] / M.lp_new - 1).max(),
                    pp=np.abs(opp - M.pp).max(), mass=abs(float(E.sg.sum() - len(y))) / len(y))
        print("oracle (lp = -600) vs reference (dropped list) dying 3x30 sigma=%g T=40000  " % sigma
              + "  ".join("%s %.2g" % kv for kv in errs.items()) + "  mass of the dead ring %.3g" % float(E.sg[30:59].sum()))
        assert np.allclose(omu[:, live], M.mu[:, live], rtol=1e-8, atol=1e-11), errs
        assert np.allclose(omu[fin, 1], M.mu[fin, 1], rtol=1e-8, atol=1e-11) and fin.sum() == 30, errs
        assert errs["sigma"] <= 1e-8 and errs["lp"] <= 1e-8 and errs["mass"] <= 1e-14, errs
        assert np.allclose(opp, M.pp, rtol=1e-8, atol=1e-8), errs


# ---------------------------------------------------------------- 3. invariances of the reference

def test_block_length_and_threads_change_no_bit(O, H, HP):
    y, lp, mu, sig, _ = ring_case(H, 4, 60, 20_011, 1.0, 5)
    sm = O.state_matrix(4, 60, lp, False)
    win = [(0, 300), (9_000, 9_700), (20_011 - 77, 20_011)]
    runs = [HP.train_step(y, sm, mu, sig, block=blk, threads=th, windows=win)
            for blk, th in ((1024, 1), (64, 1), (8192, 1), (1024, 16), (64, 16), (1, 3), (20_011, 2), (50_000, 1))]
    E0, M0 = runs[0]
    for E, M in runs[1:]:
        for f in ("sg", "sgy", "sgd", "sgd2", "sxi", "g0", "gl"):
            assert np.array_equal(getattr(E, f), getattr(E0, f)), f
        assert E.loglik == E0.loglik and E.defect == E0.defect
        assert all(np.array_equal(a, b) for a, b in zip(E.windows, E0.windows))
        assert np.array_equal(M.mu, M0.mu) and M.sigma == M0.sigma
        assert np.array_equal(M.lp_new, M0.lp_new) and np.array_equal(M.pp, M0.pp)
    # windows are the columns of a full run
    Ef, _ = HP.train_step(y, sm, mu, sig, windows=[(0, len(y))])
    for (lo, hi), g in zip(win, E0.windows):
        assert np.array_equal(Ef.windows[0][lo:hi], g)
    assert abs(float(E0.sg.sum() - len(y))) <= 1e-14 * len(y)
    assert float(E0.defect) <= 1e-16


def test_bad_arguments_are_refused(O, H, HP):
    y, lp, mu, sig, _ = ring_case(H, 1, 20, 600, 0.3, 5)
    sm = O.state_matrix(1, 20, lp, False)
    mean = HP.state_means(sm.states, mu)
    for kw in (dict(block=0), dict(threads=0), dict(windows=[(10, 601)]), dict(windows=[(-1, 5)])):
        with pytest.raises(RuntimeError):
            HP.estep(y, sm.src, sm.dst, sm.val, mean, sig, **kw)
    with pytest.raises(RuntimeError):
        HP.estep(y, sm.src + sm.nstates, sm.dst, sm.val, mean, sig)       # a state id outside the model
    with pytest.raises(RuntimeError):
        HP.estep(y, sm.src, sm.dst, sm.val, mean, 0.0)


def test_committed_fixtures_match_their_inputs(HP):
    """every committed fixture was made from the inputs its case regenerates today (seeded numpy stream, oracle
    state space): the device tests compare against it only then, and recompute the reference live otherwise"""
    import make_estep_at_size as G
    for name in G.CASES:
        if name in G.LIVE:
            continue
        old = G.load(name)
        y, sm, mu, sigma, temps, pp, win = G.inputs(name)
        h = G.hashes(y, sm, mu, sigma)
        assert h["sha_y"] == str(old["sha_y"]) and h["sha_model"] == str(old["sha_model"]), name
        assert old["sg"].shape == (sm.nstates,) and int(old["T"]) == len(y)
        assert abs(float(old["mass_minus_T"])) <= 1e-14 * len(y) and float(old["defect"]) <= 1e-14, name
        assert os.path.getsize(os.path.join(G.OUT, name + ".npz")) < 1 << 20
