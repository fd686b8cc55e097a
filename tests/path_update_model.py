"""Numpy model of Viterbi training's update (hmmsort_plan_path_update), written as loops: the model
re-estimated from a decoded path.  It is update() of baumwelch.jl:205-309 with gamma and xi the indicators of the
path.  Test infrastructure: the CPU test checks it against the reference restatement, the GPU tests check the
library against it.  Also the shared shapes and signal generators of both test files."""
import math

import numpy as np

NEG_INF = float("-inf")


def single_table(states):
    """state (0-based column) -> (l, k) when exactly one row l has states[l, j] >= 2 (k = that value), else None"""
    N, S = states.shape
    tab = []
    for j in range(S):
        act = [l for l in range(N) if states[l, j] >= 2]
        tab.append((act[0], int(states[act[0], j])) if len(act) == 1 else None)
    return tab


def path_update(y, x, states, transitions, mu, by_template=False, exact=False):
    """y: T floats; x: T 1-based ids; states: N x S (1-based rows of mu); transitions: records with src, dst in list
    order; mu: K x N, the current model.  by_template: lp' in N slots by template (wave and ring plans), else one
    entry per transition out of state 1 but the first, in list order.  exact: sums with math.fsum (the reference
    for the library, whose order of summing differs); else serially in time order (what update() does).
    Returns a dict: mu, sigma, lp, pp, counts [3], c (K x N visit counts), n."""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x).astype(np.int64)
    states = np.asarray(states)
    mu = np.asarray(mu, dtype=np.float64)
    T, (N, S), K = len(y), states.shape, mu.shape[0]
    single = single_table(states)
    valid = lambda s: 1 <= s <= S  # noqa: E731
    counts = [0, 0, 0]
    # templates
    terms = [[[] for _ in range(N)] for _ in range(K)]
    for t in range(T):
        if not valid(x[t]):
            counts[0] += 1
            continue
        e = single[x[t] - 1]
        if e is not None:
            terms[e[1] - 1][e[0]].append(float(y[t]))
    mu_n = np.zeros((K, N), order="F")
    c = np.zeros((K, N), dtype=np.int64)
    for l in range(N):
        for k in range(1, K):
            q = terms[k][l]
            c[k, l] = len(q)
            if q:
                s = math.fsum(q) if exact else sum(q, 0.0)
                mu_n[k, l] = s / len(q)
            else:
                mu_n[k, l] = mu[k, l]   # 0/0: the row keeps its value
                counts[2] += 1
    # sigma with the new means
    mean = np.zeros(S)
    for j in range(S):
        a = 0.0
        for l in range(N):
            a += mu_n[states[l, j] - 1, l]
        mean[j] = a
    sq = []
    for t in range(T):
        if valid(x[t]):
            d = float(y[t]) - float(mean[x[t] - 1])
            sq.append(d * d)
    n = len(sq)
    tot = math.fsum(sq) if exact else sum(sq, 0.0)
    sigma = math.sqrt(tot / n) if n else float("nan")
    # entry probabilities
    src = [int(r["src"]) for r in transitions]
    dst = [int(r["dst"]) for r in transitions]
    pairs = set(zip(src, dst))
    out1 = [d for s_, d in zip(src, dst) if s_ == 1]
    n_i = [0] * len(out1)
    b = 0
    for t in range(T - 1):
        if valid(x[t]) and valid(x[t + 1]) and (int(x[t]), int(x[t + 1])) not in pairs:
            counts[1] += 1
        if x[t] == 1:
            b += 1
            for i, d in enumerate(out1):
                if x[t + 1] == d:
                    n_i[i] += 1
    lg = lambda ni: NEG_INF if ni == 0 or b == 0 else math.log(ni) - math.log(b)  # noqa: E731
    if by_template:
        lp = [NEG_INF] * N
        for i, d in enumerate(out1):
            e = single[d - 1]
            if e is not None and e[1] == 2:
                lp[e[0]] = lg(n_i[i])
    else:
        lp = [lg(n_i[i]) for i in range(1, len(out1))]
    pp = np.full(S, NEG_INF)
    if T and valid(x[0]):
        pp[x[0] - 1] = 0.0
    return dict(mu=mu_n, sigma=sigma, lp=np.array(lp, dtype=np.float64), pp=pp, counts=counts, c=c, n=n)


# ---- the shapes both test files use ----------------------------------------------------------------------------
BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25)]
SIGMA = 0.3


def templates(H, N, K):
    t = np.asfortranarray(np.stack([H.create_spike_template(K, *BASE[i]) for i in range(N)], 1))
    t[0, :] = 0.0
    return t


def overlap_signal(T, sigma, pp, temps, seed):
    """independent spike trains, one per template (a template cannot restart before it has finished and passed
    through one silent sample; no two start in the same sample), summed over Gaussian noise: spikes of different
    templates overlap"""
    K, N = temps.shape
    rng = np.random.default_rng(seed)
    y = sigma * rng.standard_normal(T)
    u = rng.random((T, N))
    free = [0] * N                      # first sample at which template j may start again
    for t in range(T):
        for j in range(N):
            if t >= free[j] and u[t, j] < pp[j]:
                m = min(K - 1, T - t)
                y[t:t + m] += temps[1:1 + m, j]   # rows 2..K of mu: the K-1 phases of the ring
                free[j] = t + K
                break                   # one onset per sample: two templates never start together
    return y


def shape(H, name):
    """(y, StateMatrix, true templates, sigma) of the three shapes: '2x12o' two templates of 12 rows with overlaps,
    6 000 samples; '3x20' ring, 8 000 samples; '2x70' ring, 20 000 samples"""
    if name == "2x12o":
        temps, pp = templates(H, 2, 12), [0.02, 0.015]
        return overlap_signal(6000, SIGMA, pp, temps, 11), H.StateMatrix.create(2, 12, np.log(pp), True), temps, SIGMA
    if name == "3x20":
        temps, pp = templates(H, 3, 20), [0.012, 0.008, 0.006]
        return H.create_signal(8000, SIGMA, pp, temps, seed=12), H.StateMatrix.create(3, 20, np.log(pp), False), temps, SIGMA
    if name == "2x70":
        temps, pp = templates(H, 2, 70), [0.004, 0.003]
        return H.create_signal(20000, SIGMA, pp, temps, seed=13), H.StateMatrix.create(2, 70, np.log(pp), False), temps, SIGMA
    raise KeyError(name)


SHAPES = ("2x12o", "3x20", "2x70")
