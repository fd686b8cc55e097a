"""Numpy / math.fsum model of Viterbi training from additive path statistics (hmmsort_plan_path_stats,
hmmsort_plan_path_finish), written from the definitions as loops.  Test infrastructure: the CPU test ties
it to path_update_model.path_update, the GPU tests check the library against it.

The vector of a range [own_lo, own_hi) of a path x of y, with NE = N (K-1) and entry e = l (K-1) + (k-2):
  c, s   count and sum of y over owned samples whose state has template l alone active, at phase k
  sm     sum of y over owned samples in states with two or more active templates, once per active template
  nj     owned samples in each such state
  ent, b the counts behind lp': pairs (1 -> dst_i) and (1 -> anything) with t owned and t + 1 < T
  sum_y2, n  over owned samples with a valid id; bad0 / bad1: invalid ids / valid pairs that are no transition
  x0     the id x[0] when first, own_lo == 0 and the id is valid, else 0
and the finish:  sigma'^2 n = sum y^2 - 2 sum_e mu'_e (s_e + sm_e) + sum_e c_e mu'_e^2 + sum_j nj_j M_j^2."""
import math

import numpy as np

import path_update_model as PU

INT_SLOTS = ("c", "nj", "ent", "b", "n", "x0", "bad0", "bad1")
FLOAT_SLOTS = ("s", "sm", "sum_y2")
ORDER = ("c", "s", "sm", "nj", "ent", "b", "sum_y2", "n", "x0", "bad0", "bad1")


def multi_table(states):
    """state (0-based column) -> [(l, k), ...] of its active rows in neuron order when there are two or more"""
    N, S = states.shape
    tab = []
    for j in range(S):
        act = [(l, int(states[l, j])) for l in range(N) if states[l, j] >= 2]
        tab.append(act if len(act) >= 2 else None)
    return tab


def slots(states, transitions, by_template):
    """(number of lp' slots, {1-based destination id: slot}) of the transitions out of state 1"""
    N = states.shape[0]
    single = PU.single_table(states)
    out1 = [int(r["dst"]) for r in transitions if int(r["src"]) == 1]
    tab = {}
    for i, d in enumerate(out1):
        if by_template:
            e = single[d - 1]
            if e is not None and e[1] == 2:
                tab[d] = e[0]
        elif i >= 1:
            tab[d] = i - 1
    return (N if by_template else len(out1) - 1), tab


def path_stats(y, x, states, transitions, K, by_template=False, own_lo=0, own_hi=None, first=True):
    """the statistics of samples [own_lo, own_hi) of (y, x) as a dict of the slots above (integer slots as Python
    ints / int64 arrays, float slots by math.fsum), plus `abs`: sum of |y| over what entered s_e + sm_e"""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x).astype(np.int64)
    states = np.asarray(states)
    T, (N, S), L = len(y), states.shape, K - 1
    own_hi = T if own_hi is None else own_hi
    assert 0 <= own_lo <= own_hi <= T
    single, multi = PU.single_table(states), multi_table(states)
    nslot, slot = slots(states, transitions, by_template)
    pairs = set((int(r["src"]), int(r["dst"])) for r in transitions)
    valid = lambda s: 1 <= s <= S  # noqa: E731
    NE = N * L
    c, nj, ent = np.zeros(NE, dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(nslot, dtype=np.int64)
    ts, tm, sq = [[] for _ in range(NE)], [[] for _ in range(NE)], []
    b = bad0 = bad1 = 0
    for t in range(own_lo, own_hi):
        xt, yt = int(x[t]), float(y[t])
        if not valid(xt):
            bad0 += 1
        else:
            sq.append(yt * yt)
            e = single[xt - 1]
            if e is not None:
                c[e[0] * L + e[1] - 2] += 1
                ts[e[0] * L + e[1] - 2].append(yt)
            elif multi[xt - 1] is not None:
                nj[xt - 1] += 1
                for l, k in multi[xt - 1]:
                    tm[l * L + k - 2].append(yt)
        if t + 1 < T:
            xn = int(x[t + 1])
            if valid(xt) and valid(xn) and (xt, xn) not in pairs:
                bad1 += 1
            if xt == 1:
                b += 1
                if xn in slot:
                    ent[slot[xn]] += 1
    x0 = int(x[0]) if first and own_lo == 0 and own_hi > 0 and valid(int(x[0])) else 0
    return dict(c=c, s=np.array([math.fsum(q) for q in ts]), sm=np.array([math.fsum(q) for q in tm]), nj=nj, ent=ent,
                b=b, sum_y2=math.fsum(sq), n=len(sq), x0=x0, bad0=bad0, bad1=bad1,
                abs=np.array([math.fsum(abs(v) for v in p + q) for p, q in zip(ts, tm)]))


def add(parts):
    """the slot-wise sum of statistics dicts: integers exactly, floats by math.fsum"""
    out = {}
    for k in ORDER + ("abs",):
        v = [p[k] for p in parts]
        if k in INT_SLOTS:
            out[k] = sum(v[1:], v[0])
        elif np.ndim(v[0]):
            out[k] = np.array([math.fsum(col) for col in zip(*v)])
        else:
            out[k] = math.fsum(v)
    return out


def vector(st):
    """the statistics dict in the library's layout, as float64"""
    return np.concatenate([np.atleast_1d(np.asarray(st[k], dtype=np.float64)) for k in ORDER])


def split_vector(v, N, K, S):
    """the library's vector -> dict of slots (all float64)"""
    NE = N * (K - 1)
    nslot = len(v) - 3 * NE - S - 6
    cuts = np.cumsum([NE, NE, NE, S, nslot, 1, 1, 1, 1, 1])
    parts = np.split(np.asarray(v), cuts)
    return {k: (p if k in ("c", "s", "sm", "nj", "ent") else float(p[0])) for k, p in zip(ORDER, parts)}


def finish(st, states, mu, T=None):
    """statistics dict and the current model mu (K x N) -> dict like path_update's: mu, sigma, lp, pp, counts, c
    (K x N), n; and tot_terms, the sum of the absolute values behind the four sums of sigma'^2 n (for the bound)"""
    states = np.asarray(states)
    mu = np.asarray(mu, dtype=np.float64)
    (N, S), K = states.shape, mu.shape[0]
    L = K - 1
    mu_n = np.zeros((K, N), order="F")
    c2 = np.zeros((K, N), dtype=np.int64)
    kept = 0
    t1, t2, a1 = [], [], []
    for l in range(N):
        for k in range(1, K):
            e = l * L + k - 1
            c2[k, l] = st["c"][e]
            if st["c"][e] > 0:
                mu_n[k, l] = st["s"][e] / float(st["c"][e])
            else:
                mu_n[k, l] = mu[k, l]
                kept += 1
            m = float(mu_n[k, l])
            t1.append(-2.0 * m * (float(st["s"][e]) + float(st["sm"][e])))
            a1.append(2.0 * abs(m) * float(st["abs"][e]) if "abs" in st else abs(t1[-1]))
            t2.append(float(st["c"][e]) * m * m)
    t3 = []
    for j in range(S):
        if st["nj"][j] > 0:
            a = 0.0
            for l in range(N):
                a += mu_n[states[l, j] - 1, l]
            t3.append(float(st["nj"][j]) * a * a)
    n = int(st["n"])
    tot = math.fsum([float(st["sum_y2"])] + t1 + t2 + t3)
    sigma = math.sqrt(max(tot, 0.0) / n) if n else float("nan")
    b = int(st["b"])
    lp = np.array([PU.NEG_INF if ni == 0 or b == 0 else math.log(int(ni)) - math.log(b) for ni in st["ent"]],
                  dtype=np.float64)
    pp = np.full(S, PU.NEG_INF)
    if 1 <= int(st["x0"]) <= S:
        pp[int(st["x0"]) - 1] = 0.0
    return dict(mu=mu_n, sigma=sigma, lp=lp, pp=pp, counts=[int(st["bad0"]), int(st["bad1"]), kept], c=c2, n=n, tot=tot,
                tot_terms=math.fsum([float(st["sum_y2"])] + a1 + t2 + t3))


def sigma_bound(m, T):
    """relative bound on sigma' of the library against the model's finish m, for T samples in all: each of the four
    sums carries at most T 2^-52 of its absolute sum in any order, so |d tot| <= 4 T 2^-52 tot_terms and sigma'
    takes half of that relative error, plus the 4 T 2^-52 of the two-pass form"""
    return 0.5 * 4 * T * 2.0 ** -52 * m["tot_terms"] / m["tot"] + 4 * T * 2.0 ** -52


def pooled(pairs, states, transitions, mu, by_template=False):
    """one step from several channels' (y, x): the channels' whole-recording statistics added in the order given,
    finished with the model mu.  Returns (finish dict, summed statistics)."""
    K = np.asarray(mu).shape[0]
    st = add([path_stats(y, x, states, transitions, K, by_template) for y, x in pairs])
    return finish(st, states, mu), st
