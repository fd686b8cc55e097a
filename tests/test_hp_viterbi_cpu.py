"""Pins the extended-precision MAP-path reference (oracle/hp_viterbi.c, oracle/hp.py) on the CPU, and with it asks
for the first time whether the fp64 oracle's decode (a restatement of viterbi.jl:44-98) is the maximum-a-posteriori
path.

1. Exact enumeration: on tiny models every path is scored with `decimal` at 50 digits from the same doubles.  The
   reference's path is an arg-max; its score and ll, long-double results rounded once to double, sit within 2 ulp
   (4.5e-16 relative); where the enumeration has an exact tie (duplicate templates) the path is the one an exact
   recursion with the list-order rule (first maximum, strict >) picks.
2. Invariances: block lengths 1 .. 50 000 and the thread count change no bit; the cumulative scores are the scores of
   the path's prefixes; path_score refuses a path that is not one.
3. The fp64 oracle against the reference on the shapes the device tests use, under the acceptance rule of
   oracle/hp.py (compare_paths) with the oracle in the device's place.  Differing samples and ll errors are printed;
   DESIGN.md section 2b records them.
4. Negative control: the smallest wrong decodes there are (one onset moved by one sample; one spike left out) are
   rejected by the rule.
"""
import decimal
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import test_hp_reference_cpu as R  # noqa: E402  (the case makers of the E-step reference's tests)
import viterbi_rule as VR  # noqa: E402

D = decimal.Decimal
PI = D("3.14159265358979323846264338327950288419716939937510582097494")


@pytest.fixture(scope="module")
def HP():
    from oracle import hp
    hp.build()
    hp.vlib()
    return hp


# ---------------------------------------------------------------- 1. exact enumeration

def exact_model(y, sm, mu, sigma):
    """q[t][j] and the transition list in Decimal, from the doubles every implementation is given"""
    S, N = sm.nstates, sm.N
    sig = D(float(sigma))
    c0 = -(2 * PI).ln() / 2 - sig.ln()
    q = []
    for t in range(len(y)):
        row = []
        for j in range(S):
            m = 0.0
            for l in range(N):
                m += float(mu[sm.states[l, j] - 1, l])       # the model's mean: doubles added in template order
            row.append(c0 - (D(float(y[t])) - D(m)) ** 2 / (2 * sig * sig))
        q.append(row)
    q[0][0] = D(0)                                           # the silent state does not emit at sample 0
    trans = [(int(a) - 1, int(b) - 1, D(float(v))) for a, b, v in zip(sm.src, sm.dst, sm.val) if np.isfinite(v)]
    return q, trans


def enumerate_paths(q, trans, S):
    """score of every valid path, by brute force: {path: (score, ll)}"""
    T = len(q)
    A = {}
    for a, b, v in trans:
        A[(a, b)] = max(v, A.get((a, b), v))
    out = {}
    for path in itertools.product(range(S), repeat=T):
        s, ll, ok = q[0][path[0]], D(0), True
        for t in range(1, T):
            v = A.get((path[t - 1], path[t]))
            if v is None:
                ok = False
                break
            s += v + q[t][path[t]]
            ll += s
        if ok:
            out[path] = (s, ll)
    return out


def exact_recursion(q, trans, S):
    """the recursion with the list-order rule in exact arithmetic: what decides where the enumeration ties"""
    T = len(q)
    ninf = D("-Infinity")
    d = list(q[0])
    bp = []
    for t in range(1, T):
        best, arg = [ninf] * S, [0] * S
        for a, b, v in trans:
            if d[a] + v > best[b]:
                best[b], arg[b] = d[a] + v, a
        d = [best[j] + q[t][j] for j in range(S)]
        bp.append(arg)
    x = [max(range(S), key=lambda j: (d[j], -j))]
    for arg in reversed(bp):
        x.append(arg[x[-1]])
    return tuple(reversed(x))


def tiny(O, kind, seed, T):
    """(y, sm, mu, sigma) of an enumeration case, K = 3"""
    K = 3
    rng = np.random.default_rng(seed)
    N = 1 if kind == "ring1" else 2
    pp = rng.uniform(0.1, 0.3, N)
    lp = np.log(pp)
    if kind == "dropped":
        lp[1] = -np.inf                                     # template 1 can no longer start: its transitions leave the list
    mu = np.asfortranarray(rng.uniform(-1.2, 1.2, (K, N)))
    if kind == "twins":
        mu[:, 1] = mu[:, 0]
        lp[1] = lp[0]
    mu[0, :] = 0
    sigma = float(rng.uniform(0.5, 1.0))
    y = rng.standard_normal(T) * 1.3
    if kind in ("twins", "starts_in_ring", "ends_in_spike"):
        mu[1:, :] *= 3.0                                    # spikes that stand out: the path has to contain them
        y = rng.standard_normal(T) * 0.2
        if kind == "starts_in_ring":
            y[0:2] += mu[1:3, 0]                            # the recording starts with a spike's first phase: at sample
            sigma = 0.3                                     # 0 the silent state scores 0, the ring state its emission
        elif kind == "ends_in_spike":
            y[T - 1] += mu[1, 1]                            # ... and ends at a spike's first
        else:
            y[1:3] += mu[1:3, 0]
    sm = O.state_matrix(N, K, lp, kind == "overlap")
    return y, sm, mu, sigma


@pytest.mark.parametrize("kind,seed,T", [
    ("ring1", 1, 6), ("ring1", 2, 5), ("ring2", 3, 6), ("ring2", 4, 5), ("overlap", 5, 5), ("overlap", 6, 4),
    ("dropped", 7, 6), ("twins", 8, 6), ("twins", 9, 5), ("starts_in_ring", 10, 6), ("ends_in_spike", 11, 6),
    ("ring2", 12, 1), ("overlap", 13, 2),
])
def test_exact_enumeration(O, HP, kind, seed, T):
    decimal.getcontext().prec = 50
    y, sm, mu, sigma = tiny(O, kind, seed, T)
    S = sm.nstates
    assert S == {"ring1": 3, "overlap": 9}.get(kind, 5)
    q, trans = exact_model(y, sm, mu, sigma)
    paths = enumerate_paths(q, trans, S)
    best = max(s for s, _ in paths.values())
    winners = [p for p, (s, _) in paths.items() if s == best]
    M = HP.viterbi(y, sm, mu, sigma, block=2, idx=np.arange(T))
    got = tuple(int(v) - 1 for v in M.x)
    score, ll = paths[got]
    e_s, e_l = rel_err(M.score, score), rel_err(M.ll, ll)
    e_c = max(float(abs(D(float(M.cum[t])) - paths_prefix(q, trans, got, t))) for t in range(T))
    print("enumeration %-14s T=%d S=%d: %d valid paths, %d arg-max, path %s  score err %.2g  ll err %.2g  cum err %.2g"
          % (kind, T, S, len(paths), len(winners), got, e_s, e_l, e_c))
    assert got in winners, (got, winners)
    assert got == exact_recursion(q, trans, S)              # the list-order rule where there is a tie
    assert e_s <= 4.5e-16 and e_l <= 4.5e-16 and e_c <= 4.5e-16 * max(1.0, abs(float(score)))
    if kind == "twins":
        assert len(winners) > 1 and any(v > 0 for v in got)     # an exact tie, and a spike on the path
    if kind == "starts_in_ring":
        assert got[0] != 0
    if kind == "ends_in_spike":
        assert got[-1] != 0
    # the fp64 oracle on the same input: identical path
    xo, llo = O.viterbi(y, sm, mu, sigma)
    assert tuple(int(v) - 1 for v in xo) == got
    assert abs(llo - float(M.ll)) <= 1e-12 * max(1.0, abs(float(M.ll)))
    # and path_score is the enumeration's score
    assert rel_err(HP.path_score(y, sm, mu, sigma, M.x, 0, T), score) <= 4.5e-16


def rel_err(got, exact):
    """of a long double rounded once to double; absolute where the exact value is 0"""
    e = abs(D(float(got)) - exact)
    return float(e / abs(exact)) if exact != 0 else float(e)


def paths_prefix(q, trans, path, t):
    A = {}
    for a, b, v in trans:
        A[(a, b)] = max(v, A.get((a, b), v))
    s = q[0][path[0]]
    for u in range(1, t + 1):
        s += A[(path[u - 1], path[u])] + q[u][path[u]]
    return s


# ---------------------------------------------------------------- 2. invariances

def same(a, b):
    return (np.array_equal(a.x, b.x) and a.score == b.score and a.ll == b.ll and np.array_equal(a.cum, b.cum)
            and a.dmax == b.dmax)


def test_block_length_and_threads_change_no_bit(O, H, HP):
    y, lp, mu, sig, _ = R.ring_case(H, 4, 60, 20_011, 1.0, 5)
    sm = O.state_matrix(4, 60, lp, False)
    idx = [0, 1, 63, 64, 4095, 4096, 10_000, 20_010]
    runs = [HP.viterbi(y, sm, mu, sig, block=blk, threads=th, idx=idx)
            for blk, th in ((1024, 1), (1, 1), (2, 3), (63, 1), (64, 16), (8192, 1), (20_010, 1), (20_011, 2), (50_000, 1))]
    for r in runs[1:]:
        assert same(r, runs[0])
    # the states of a column are spread over threads only from 1 024 states on: an overlap model
    y, lp, mu, sig, _ = R.overlap_case(H, 2, 40, 3_001, 0.3, 3)
    sm = O.state_matrix(2, 40, lp, True)
    assert sm.nstates >= 1024
    runs = [HP.viterbi(y, sm, mu, sig, block=blk, threads=th, idx=[0, 1500, 3000])
            for blk, th in ((1024, 1), (1024, 4), (7, 16), (50_000, 3))]
    for r in runs[1:]:
        assert same(r, runs[0])


def test_cumulative_scores_are_prefix_scores(O, H, HP):
    y, lp, mu, sig, _ = R.ring_case(H, 4, 60, 30_000, 0.3, 6)
    sm = O.state_matrix(4, 60, lp, False)
    idx = [0, 1, 2, 59, 60, 1000, 1023, 1024, 1025, 17_321, 29_999]
    M = HP.viterbi(y, sm, mu, sig, idx=idx)
    for t, c in zip(M.idx, M.cum):
        p = HP.path_score(y, sm, mu, sig, M.x, 0, int(t) + 1)
        # both are sums of the same t + 1 ... 2 t + 1 long doubles in another order
        assert abs(float(c - p)) <= (2 * t + 2) * 2.0 ** -64 * max(1.0, abs(float(p))), (t, float(c), float(p))
    assert M.cum[-1] == M.score
    # ll is the sum of the cumulative scores from sample 1 on
    full = HP.viterbi(y, sm, mu, sig, idx=np.arange(len(y)))
    assert same(HP.viterbi(y, sm, mu, sig, idx=idx), M) and np.array_equal(full.x, M.x)
    assert abs(float(full.cum[1:].sum() - M.ll)) <= len(y) * 2.0 ** -64 * abs(float(M.ll))
    # a range's score is the difference of two prefixes
    a, b = 1000, 17_322
    mid = HP.path_score(y, sm, mu, sig, M.x, a, b)
    e0 = HP.path_score(y, sm, mu, sig, M.x, a, a + 1)
    assert abs(float((M.cum[9] - M.cum[5]) - (mid - e0))) <= 1e-15 * abs(float(mid))


def test_bad_arguments_and_invalid_paths_are_refused(O, H, HP):
    y, lp, mu, sig, _ = R.ring_case(H, 2, 20, 600, 0.3, 5)
    sm = O.state_matrix(2, 20, lp, False)
    mean = HP.state_means(sm.states, mu)
    for kw in (dict(block=0), dict(threads=0), dict(idx=[600]), dict(idx=[-1])):
        with pytest.raises(RuntimeError):
            HP.viterbi_mean(y, sm.src, sm.dst, sm.val, mean, sig, **kw)
    with pytest.raises(RuntimeError):
        HP.viterbi_mean(y, sm.src + sm.nstates, sm.dst, sm.val, mean, sig)
    with pytest.raises(RuntimeError):
        HP.viterbi_mean(y, sm.src, sm.dst, sm.val, mean, 0.0)
    M = HP.viterbi(y, sm, mu, sig)
    x = M.x.copy()
    t = int(np.nonzero(x > 1)[0][3])
    x[t] += 1                                               # skips a phase
    with pytest.raises(ValueError):
        HP.path_score(y, sm, mu, sig, x, 0, len(y))
    assert not HP.path_is_valid(HP._Model(sm, mu, sig), x)
    x = M.x.copy()
    x[5] = sm.nstates + 1
    with pytest.raises(ValueError):
        HP.path_score(y, sm, mu, sig, x, 0, len(y))


# ---------------------------------------------------------------- 3. the fp64 oracle against the reference

def cut_case(H, N, K, T, sigma, seed):
    """a recording cut by both edges: it starts 25 samples into a spike and ends 30 samples into one"""
    import make_estep_at_size as E
    temps, pp = E.ring_model(N, K)
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    y[:K - 25] += temps[25:, 0]
    y[T - 30:] += temps[:30, 2]
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    return y, np.log(pp), mu, 1.15 * sigma, False


def twin_case(H, N, K, T, sigma, seed):
    """templates 1 = 2 with the same entry probability: every spike of theirs is an exact tie"""
    amps = [R.BASE[i % 4] for i in range(N)]
    amps[1] = amps[0]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *a) for a in amps], 1))
    pp = np.array([0.002, 0.002, 0.001, 0.0015][:N])
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    return y, np.log(pp), temps, sigma, False


def p60_case(H, N, K, T, sigma, seed):
    """the reference's own Viterbi-test model (test/runtests.jl:17-34: N = 2, K = 60, overlaps on, 3 600 states)"""
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                        H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
    pp = [0.003, 0.001]
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    rng = np.random.default_rng(5)
    for t0 in rng.integers(1000, T - 1000, 8):
        y[t0:t0 + K] += temps[:, 0]
        y[t0 + 17:t0 + 17 + K] += temps[:, 1]
    return y, np.log(pp), temps, sigma, True


DECODE_CASES = [(R.ring_case, N, K, T, s, 40 + i) for i, (N, K, T) in enumerate([
    (1, 40, 9_000), (2, 30, 6_000), (4, 60, 40_001), (16, 40, 10_000), (8, 128, 9_000), (10, 180, 9_000)])
    for s in (0.3, 1.0)]
DECODE_CASES += [(R.overlap_case, 2, 20, 20_000, s, 60) for s in (0.3, 1.0)]
DECODE_CASES += [(R.overlap_case, 3, 12, 12_000, s, 61) for s in (0.3, 1.0)]
DECODE_CASES += [(R.random_init_case, 3, 40, 12_000, s, 8) for s in (0.3, 1.0)]
DECODE_CASES += [(cut_case, 4, 60, 30_000, s, 71) for s in (0.3, 1.0)]
DECODE_CASES += [(twin_case, 4, 60, 200_000, 0.3, 72), (p60_case, 2, 60, 20_000, 0.3, 77)]
DECODE_CASES += [(R.ring_case, 4, 60, 200_000, s, 70) for s in (0.3, 1.0)]
DECODE_CASES += [(R.ring_case, 4, 60, 2_000_000, 0.3, 73)]


@pytest.mark.parametrize("make,N,K,T,sigma,seed", DECODE_CASES,
                         ids=["%s-%dx%d-T%d-s%g" % (c[0].__name__[:-5], c[1], c[2], c[3], c[4]) for c in DECODE_CASES])
def test_oracle_decode_against_reference(O, H, HP, make, N, K, T, sigma, seed):
    """Measured: DESIGN.md section 2b (table 'fp64 oracle's decode against the MAP reference')."""
    y, lp, mu, sig, ov = make(H, N, K, T, sigma, seed)
    sm = O.state_matrix(N, K, lp, ov)
    xo, llo = O.viterbi(y, sm, mu, sig)
    ref = VR.Ref.live(y, sm, mu, sig, threads=4)
    tag = "oracle vs reference %s %dx%d s=%g" % (make.__name__[:-5], N, K, sigma)
    VR.accept(tag, y, sm, mu, sig, ref, xo, llo, duplicates=make is twin_case)
    assert (xo > 1).sum() > 0                               # spikes were decoded at all
    if make is cut_case:
        assert xo[0] > 1 and xo[-1] > 1, (xo[0], xo[-1])    # first-sample rule and final arg-max inside spikes
    if ov:
        assert (xo > 1 + N * (K - 1)).sum() > 0 or make is R.overlap_case


# ---------------------------------------------------------------- 4. negative control

def test_rule_rejects_the_smallest_wrong_decodes(O, H, HP):
    import make_viterbi_at_size as G
    y, sm, mu, sigma, pp = G.inputs("G03")
    ref = VR.Ref.live(y, sm, mu, sigma)
    L = sm.K - 1
    x = ref.x
    heads = np.nonzero((x[1:] > 1) & (x[:-1] == 1))[0] + 1
    t = int([h for h in heads if h + L + 1 < len(x) and x[h + L] == 1 and x[h + L + 1] == 1][10])
    model = HP._Model(sm, mu, sigma)
    # one onset, one sample late
    late = x.copy()
    late[t] = 1
    late[t + 1:t + 1 + L] = x[t:t + L]
    # one spike left out
    gone = x.copy()
    gone[t:t + L] = 1
    for name, bad in (("onset one sample late", late), ("one spike replaced by silence", gone)):
        assert HP.path_is_valid(model, bad)
        runs = HP.compare_paths(y, model, None, None, x, bad, ref.idx, ref.cum, ref.dmax)
        assert len(runs) == 1 and runs[0].s == t
        r = runs[0]
        print("negative control, %s: run [%d, %d]  Delta %.6g  tau %.3g  Delta/tau %.3g" % (
            name, r.s, r.e, r.delta, r.tau, r.ratio))
        assert r.delta > r.tau and r.delta > 1e6 * r.tau
        ll_bad = float(ref.ll) - r.delta * (len(y) - r.e)   # every later cumulative value carries the loss
        with pytest.raises(AssertionError, match="score worse than fp64 rounding allows"):
            VR.accept(name, y, sm, mu, sigma, ref, bad, ll_bad, model=model)


def test_committed_fixtures_match_their_inputs(O, HP):
    """every committed fixture was made from the inputs its case regenerates today, decodes to a valid path whose
    score is the stored one, and is smaller than 1 MiB.  (The 10 M cases' full check is the generator's --check.)"""
    import make_viterbi_at_size as G
    for name in G.CASES:
        p = os.path.join(G.OUT, name + ".npz")
        assert os.path.exists(p) and os.path.getsize(p) < 1 << 20, name
        z = G.unpack(G.load(name))
        N, K, ov, T = G.shape(name)
        assert (int(z["N"]), int(z["K"]), int(z["overlaps"]), int(z["T"])) == (N, K, int(ov), T)
        if T > 2_000_000 or name == "CLI":
            continue                                        # inputs take too long to regenerate here; the GPU test hashes them
        y, sm, mu, sigma, pp = G.inputs(name)
        h = G.hashes(y, sm, mu, sigma)
        assert h["sha_y"] == str(z["sha_y"]) and h["sha_model"] == str(z["sha_model"]), name
        x = G.decode(z["idx"], z["state"], T, sm)
        score = HP.path_score(y, sm, mu, sigma, x, 0, T)
        # the stored score is a serial long-double sum rounded once to double, this one a pairwise sum
        assert abs(float(score - HP.LD(z["score"]))) <= (2.0 ** -53 + 2 * T * 2.0 ** -64) * abs(float(score)), name
