"""The numpy model of hmmsort_correlograms (definitions in include/hmmsort.h), in two independent forms: `brute`, a
double loop over pairs straight from the definitions, and `fast`, a searchsorted form for the larger cases.  Both take
a list of ascending 1-based int64 time arrays and return (ccg [U, U, 2H], viol [U], coinc [U, U], n [U]), all int64."""
import numpy as np


def brute(lists, b, H, r, c):
    U = len(lists)
    ccg = np.zeros((U, U, 2 * H), dtype=np.int64)
    viol = np.zeros(U, dtype=np.int64)
    coinc = np.zeros((U, U), dtype=np.int64)
    n = np.array([len(t) for t in lists], dtype=np.int64)
    for u in range(U):
        tu = [int(x) for x in lists[u]]
        for i in range(1, len(tu)):
            if tu[i] - tu[i - 1] < r:
                viol[u] += 1
        for v in range(U):
            tv = [int(x) for x in lists[v]]
            for i, a in enumerate(tu):
                partner = False
                for j, q in enumerate(tv):
                    if u == v and i == j:
                        continue
                    d = q - a
                    if -H * b <= d < H * b:
                        ccg[u, v, d // b + H] += 1          # Python's // is the floor
                    if abs(d) <= c:
                        partner = True
                coinc[u, v] += partner
    return ccg, viol, coinc, n


def fast(lists, b, H, r, c):
    lists = [np.asarray(t, dtype=np.int64) for t in lists]
    U = len(lists)
    ccg = np.zeros((U, U, 2 * H), dtype=np.int64)
    viol = np.array([int(np.sum(np.diff(t) < r)) for t in lists], dtype=np.int64)
    coinc = np.zeros((U, U), dtype=np.int64)
    n = np.array([len(t) for t in lists], dtype=np.int64)
    edges = (np.arange(2 * H + 1, dtype=np.int64) - H) * b
    for u in range(U):
        tu = lists[u]
        for v in range(U):
            tv = lists[v]
            if len(tu) == 0 or len(tv) == 0:
                continue
            # targets below each bin edge, per source: the differences are the bin counts
            below = np.searchsorted(tv, tu[:, None] + edges[None, :], side="left")
            ccg[u, v] = np.diff(below, axis=1).sum(0)
            near = np.searchsorted(tv, tu + c, side="right") - np.searchsorted(tv, tu - c, side="left")
            if u == v:
                ccg[u, v, H] -= len(tu)                     # d = 0 with itself
                near = near - 1
            coinc[u, v] = int(np.sum(near > 0))
    return ccg, viol, coinc, n


def pairs_in_window(lists, u, v, W):
    """number of pairs (i, j), (u, i) != (v, j), with -W <= t_v[j] - t_u[i] < W"""
    tu, tv = np.asarray(lists[u], dtype=np.int64), np.asarray(lists[v], dtype=np.int64)
    d = tv[None, :] - tu[:, None]
    return int(np.sum((d >= -W) & (d < W))) - (len(tu) if u == v else 0)


def random_lists(rng, U, nmax, span):
    """U ascending lists of 0..nmax distinct times in 1..span"""
    return [np.sort(rng.choice(span, size=int(rng.integers(0, min(nmax, span) + 1)), replace=False)).astype(np.int64) + 1
            for _ in range(U)]
