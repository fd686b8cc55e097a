"""The numpy model of hmmsort_footprints (include/hmmsort.h), stated literally: a loop over tiles of 256
list entries, inside it a loop over the used spikes, vectorised over (slot, k) only, s * s formed as an array product
before the add.  `brute` is written straight from the definition (math.fsum per entry).  `cases` are the inputs the CPU
and the GPU tests share.  Test infrastructure; no GPU."""
import math

import numpy as np

TILE = 256


def table_of(U, C, chan):
    """the [U][M] table of block channels: `chan` as given, or every channel in order"""
    if chan is None:
        return np.tile(np.arange(C, dtype=np.int32), (U, 1))
    return np.asarray(chan, dtype=np.int32).reshape(U, -1)


def used(t, pre, W, T):
    a = int(t) - 1 - pre
    return a >= 0 and a + W <= T


def model(y, lists, pre, W, chan=None, cut_by_used=False):
    """-> (sum [U][M][W], sumsq, nused [U], n [U]).  cut_by_used: the WRONG tiling (256 used spikes per tile instead of
    256 list entries), for the test that shows the order matters."""
    y = np.asarray(y, dtype=np.float64)
    C, T = y.shape
    U = len(lists)
    table = table_of(U, C, chan)
    M = table.shape[1]
    s, q = np.zeros((U, M, W)), np.zeros((U, M, W))
    nused, n = np.zeros(U, dtype=np.int64), np.zeros(U, dtype=np.int64)
    for u in range(U):
        t = [int(v) for v in lists[u]]
        n[u] = len(t)
        live = table[u] >= 0
        rows = table[u][live]
        if cut_by_used:
            t = [v for v in t if used(v, pre, W, T)]
        acc_s, acc_q = np.zeros((M, W)), np.zeros((M, W))
        for b0 in range(0, len(t), TILE):
            ps, pq = np.zeros((M, W)), np.zeros((M, W))
            for v in t[b0:b0 + TILE]:
                if not used(v, pre, W, T):
                    continue
                a = v - 1 - pre
                snip = y[rows, a:a + W]
                sq = snip * snip
                ps[live] = ps[live] + snip
                pq[live] = pq[live] + sq
                nused[u] += 1
            acc_s = acc_s + ps
            acc_q = acc_q + pq
        s[u], q[u] = acc_s, acc_q
    return s, q, nused, n


def brute(y, lists, pre, W, chan=None):
    """-> (sum, sumsq, nused, n, sumabs): every entry from the definition with math.fsum; sumabs is the sum of the
    addends' magnitudes, the scale a summation error is measured against"""
    y = np.asarray(y, dtype=np.float64)
    C, T = y.shape
    U = len(lists)
    table = table_of(U, C, chan)
    M = table.shape[1]
    s, q, sa = np.zeros((U, M, W)), np.zeros((U, M, W)), np.zeros((U, M, W))
    nused, n = np.zeros(U, dtype=np.int64), np.zeros(U, dtype=np.int64)
    for u in range(U):
        n[u] = len(lists[u])
        starts = [int(t) - 1 - pre for t in lists[u] if int(t) - 1 - pre >= 0 and int(t) - 1 - pre + W <= T]
        nused[u] = len(starts)
        idx = np.asarray(starts, dtype=np.int64)
        for m in range(M):
            c = int(table[u, m])
            if c < 0 or not starts:
                continue
            for k in range(W):
                vals = y[c, idx + k].tolist()
                s[u, m, k] = math.fsum(vals)
                q[u, m, k] = math.fsum(v * v for v in vals)
                sa[u, m, k] = math.fsum(abs(v) for v in vals)
    return s, q, nused, n, sa


def wide_block(rng, C, T):
    """normal x 10^uniform(-3, 3): six decades, so that the order of the adds shows in the low bits"""
    return rng.standard_normal((C, T)) * 10.0 ** rng.uniform(-3.0, 3.0, (C, T))


def seam_list(rng, n, T, pre, W):
    """n ascending times in 1..T: the first has its window start at sample -1 and the last has its window cross the end
    of the recording (both unused; needs pre >= 1 and W - pre >= 2), the others are used"""
    assert pre >= 1 and W - pre >= 2 and n >= 2
    inner = np.sort(rng.choice(np.arange(pre + 1, T - W + pre + 2), n - 2, replace=False))
    t = np.concatenate([[pre], inner, [T]]).astype(np.int64)
    assert np.all(np.diff(t) > 0)
    return t


SEAM_W = (7, 60, 64, 65, 200)
SEAM_N = (255, 256, 257, 513)


def seam_case(W, chan=None, seed=0):
    """C = 3, T = 40 000, lists of 255, 256, 257 and 513 spikes with an unused spike at either end"""
    rng = np.random.default_rng(1000 + W + seed)
    C, T, pre = 3, 40_000, W // 3
    y = wide_block(rng, C, T)
    lists = [seam_list(rng, n, T, pre, W) for n in SEAM_N]
    return y, lists, pre, W, chan


def degenerate_cases():
    """C = 2, T = 50: an empty unit and a one-spike unit; the window's edges; a window longer than the recording"""
    rng = np.random.default_rng(5)
    y = wide_block(rng, 2, 50)
    empty, one = np.zeros(0, dtype=np.int64), np.array([17], dtype=np.int64)
    edges = np.array([3, 4, 44, 45, 1 << 40], dtype=np.int64)
    return {"w1": (y, [empty, one], 0, 1, None),
            "edges": (y, [empty, one, edges], 3, 10, None),
            "w51": (y, [empty, one, edges], 3, 51, None)}


def cases():
    """name -> (y, lists, pre, W, chan): every input of the GPU tests that is compared with the model"""
    out = {"degenerate_" + k: v for k, v in degenerate_cases().items()}
    for W in SEAM_W:
        out["seam_W%d" % W] = seam_case(W)
    out["seam_M5_W60"] = seam_case(60, np.tile(np.array([2, 0, 1, 1, 0], dtype=np.int32), (len(SEAM_N), 1)), seed=7)
    y, lists, pre, W, _ = seam_case(60, seed=11)
    out["channel_table"] = (y, lists, pre, W, np.array([[2, 1, 0, -1], [1, 1, -1, 1], [-1, -1, -1, -1],
                                                       [0, 2, 2, 0]], dtype=np.int32))
    return out
