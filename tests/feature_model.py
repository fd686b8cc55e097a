"""The numpy model of hmmsort_snippet_features and hmmsort_cluster_isolation (include/hmmsort.h), stated
literally: loops over tiles of 256 list entries, over entries, over k, a and b; array operations run across rows only
(or, in the moments, where the entries are the serial direction, across the independent (a, b) entries), and every
product is formed as an array of its own before the add, so nothing is fused.  `cases` builds the inputs the CPU and
the GPU tests share.  Test infrastructure; no GPU."""
import numpy as np
from scipy.special import erfc

import footprint_model as FM

TILE = 256
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def used_mask(t, pre, W, T):
    a = np.asarray(t, dtype=np.int64) - 1 - pre
    return (a >= 0) & (a + W <= T)


def features(y, lists, pre, W, chan=None, basis=None, centre=None):
    """-> (feat [n_total][F], used [n_total] uint8, n [U], nused [U]).  Rows in unit order."""
    y = np.asarray(y, dtype=np.float64)
    C, T = y.shape
    chan = np.arange(C) if chan is None else np.asarray(chan, dtype=np.int64)
    M = len(chan)
    t = np.concatenate([np.asarray(v, dtype=np.int64) for v in lists] + [np.zeros(0, dtype=np.int64)])
    n = np.array([len(v) for v in lists], dtype=np.int64)
    use = used_mask(t, pre, W, T)
    start = np.where(use, t - 1 - pre, 0)
    offs = np.concatenate([[0], np.cumsum(n)])
    nused = np.array([int(use[offs[u]:offs[u + 1]].sum()) for u in range(len(lists))], dtype=np.int64)
    P = W if basis is None else np.asarray(basis).shape[1]
    feat = np.zeros((len(t), M * P))
    if W <= T:
        for m in range(M):
            row = y[chan[m]]
            if basis is None:
                for k in range(W):
                    s = row[start + k]
                    feat[:, m * W + k] = s if centre is None else s - centre[m][k]
            else:
                for p in range(P):
                    acc = np.zeros(len(t))
                    for k in range(W):
                        d = row[start + k] - (0.0 if centre is None else centre[m][k])
                        prod = basis[m][p][k] * d
                        acc = acc + prod
                    feat[:, m * P + p] = acc
    feat[~use] = 0.0
    return feat, use.astype(np.uint8), n, nused


def moments(feat, used, n, groups, cut_by_used=False):
    """-> (m1 [U][groups][G], m2 [U][groups][G][G]), G = F / groups: mode 1 is groups = M, mode 2 is groups = 1.
    cut_by_used: the WRONG tiling (256 used entries per tile), for the test that shows the order matters."""
    feat = np.asarray(feat, dtype=np.float64)
    U, F = len(n), feat.shape[1]
    G = F // groups
    offs = np.concatenate([[0], np.cumsum(n)])
    m1, m2 = np.zeros((U, groups, G)), np.zeros((U, groups, G, G))
    for u in range(U):
        rows = list(range(offs[u], offs[u + 1]))
        if cut_by_used:
            rows = [r for r in rows if used[r]]
        a1, a2 = np.zeros((groups, G)), np.zeros((groups, G, G))
        for b0 in range(0, len(rows), TILE):
            p1, p2 = np.zeros((groups, G)), np.zeros((groups, G, G))
            for r in rows[b0:b0 + TILE]:
                if not used[r]:
                    continue
                f = feat[r].reshape(groups, G)
                prod = f[:, :, None] * f[:, None, :]
                p1 = p1 + f
                p2 = p2 + prod
            a1 = a1 + p1
            a2 = a2 + p2
        m1[u], m2[u] = a1, a2
    return m1, m2


def d2_rows(feat, mu_u, vinv_u):
    """d2[u][.] of every row against one unit, by the stated loops"""
    feat = np.asarray(feat, dtype=np.float64)
    F = feat.shape[1]
    d = feat - mu_u[None, :]
    q = np.zeros(len(feat))
    for a in range(F):
        rr = np.zeros(len(feat))
        for b in range(F):
            prod = vinv_u[a, b] * d[:, b]
            rr = rr + prod
        prod = d[:, a] * rr
        q = q + prod
    return np.where(q > 0, q, 0.0)


def chi2_sf(x, F):
    """Q_F(x), the chi-square survival function in the stated form, elementwise"""
    x = np.asarray(x, dtype=np.float64)
    h = 0.5 * x
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        eh = np.exp(-h)
        if F % 2 == 0:
            t, s = np.ones_like(h), np.ones_like(h)
            for j in range(1, F // 2):
                t = t * h / float(j)
                s = s + t
            res = eh * s
        else:
            sh = np.sqrt(h)
            res = erfc(sh)
            if F >= 3:
                t, s = np.ones_like(h), np.ones_like(h)
                for j in range(1, (F - 3) // 2 + 1):
                    t = t * h / (float(j) + 0.5)
                    s = s + t
                res = res + eh * sh * 1.1283791670955126 * s
    return np.where(eh == 0.0, 0.0, res)


def isolation(feat, offs, used, mu, vinv):
    """-> (iso_d2 [U], closer [U][U] int64, lpair [U][U], d2 [U][n])"""
    feat = np.asarray(feat, dtype=np.float64)
    n, F = feat.shape
    offs = np.asarray(offs, dtype=np.int64) - int(offs[0])
    U = len(offs) - 1
    use = np.ones(n, dtype=bool) if used is None else np.asarray(used).astype(bool)
    scored = np.array([not np.isnan(vinv[u][0][0]) for u in range(U)])
    unit = np.repeat(np.arange(U), np.diff(offs))
    d2 = np.full((U, n), np.nan)
    for u in range(U):
        if scored[u]:
            d2[u] = d2_rows(feat, mu[u], vinv[u])
    iso = np.full(U, np.nan)
    closer = np.zeros((U, U), dtype=np.int64)
    lpair = np.zeros((U, U))
    for u in range(U):
        if not scored[u]:
            closer[u, :], closer[:, u] = -1, -1
            lpair[u, :] = np.nan
    for u in range(U):
        closer[u, u], lpair[u, u] = 0, 0.0
        if not scored[u]:
            continue
        member = unit == u
        n_u, other = int((member & use).sum()), np.sort(d2[u][~member & use])
        if n_u >= 1 and len(other) >= n_u:
            iso[u] = other[n_u - 1]
        for v in range(U):
            if v == u:
                continue
            if scored[v]:
                rows = np.arange(offs[v], offs[v + 1])
                closer[u, v] = int(np.sum(use[rows] & (d2[u][rows] < d2[v][rows])))
            acc = 0.0
            for b0 in range(offs[v], offs[v + 1], TILE):
                b1 = min(b0 + TILE, offs[v + 1])
                q = chi2_sf(d2[u][b0:b1], F)
                p = np.float64(0.0)
                for e in range(b1 - b0):
                    if use[b0 + e]:
                        p = p + q[e]
                acc = acc + p
            lpair[u, v] = acc
    return iso, closer, lpair, d2


def gaussians(g1, g2, nused):
    """mu and the inverse sample covariance per unit, as api.unit_gaussians states them"""
    U, F = g1.shape
    mu, vinv = np.zeros((U, F)), np.zeros((U, F, F))
    for u in range(U):
        n = float(nused[u])
        if n <= F:
            vinv[u, 0, 0] = np.nan
            continue
        mu[u] = g1[u] / n
        vinv[u] = np.linalg.inv((g2[u] / n - np.outer(mu[u], mu[u])) * (n / (n - 1.0)))
    return mu, vinv


def l_ratio(lpair, nused):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(np.asarray(nused) > 0, lpair.sum(axis=1) / np.asarray(nused, dtype=np.float64), np.nan)


def pca(b1, b2, nused, P):
    """the rule of api.pca_basis"""
    n = float(np.sum(nused))
    _, M, W = b1.shape
    centre = b1.sum(axis=0) / n
    basis = np.zeros((M, P, W))
    for m in range(M):
        cov = b2[:, m].sum(axis=0) / n - np.outer(centre[m], centre[m])
        _, vec = np.linalg.eigh(0.5 * (cov + cov.T))
        for p in range(P):
            v = vec[:, W - 1 - p]
            basis[m, p] = v if v[np.argmax(np.abs(v))] > 0 else -v
    return basis, centre


# ---- inputs ----------------------------------------------------------------------------------------------------------

def seam_case(W, seed=0):
    """footprint_model.seam_case (C = 3, T = 40 000, lists of 255, 256, 257 and 513 entries, the first and the last of
    each unused); W = 1 cannot have a window that starts before the block AND one that crosses its end under the
    footprints' generator, so it gets pre = 1: the first time (1) starts at sample -1, a time T + 1 ends past T."""
    if W >= 3 and W - W // 3 >= 2 and W // 3 >= 1:
        y, lists, pre, W, _ = FM.seam_case(W, seed=seed)
        return y, lists, pre, W
    rng = np.random.default_rng(2000 + W + seed)
    C, T, pre = 3, 40_000, 1
    y = FM.wide_block(rng, C, T)
    lists = []
    for n in FM.SEAM_N:
        inner = np.sort(rng.choice(np.arange(pre + 1, T - W + pre + 2), n - 2, replace=False))
        lists.append(np.concatenate([[pre], inner, [T + pre + 1]]).astype(np.int64))
    return y, lists, pre, W


def random_basis(rng, M, P, W, wide=True):
    b = rng.standard_normal((M, P, W))
    c = rng.standard_normal((M, W))
    if wide:
        b = b * 10.0 ** rng.uniform(-3.0, 3.0, b.shape)
        c = c * 10.0 ** rng.uniform(-3.0, 3.0, c.shape)
    return b, c


def iso_case(F, counts=(255, 256, 257, 513), seed=0, unused=True, dup=False):
    """Gaussian clusters in F dimensions with overlapping supports: -> (feat, offs, used, mu, vinv).  vinv is a
    generic (non-symmetric) perturbation of the inverse covariance; dup repeats rows so that distances tie."""
    rng = np.random.default_rng(3000 + F + seed)
    U = len(counts)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = int(offs[-1])
    feat = np.zeros((n, F))
    mu, vinv = np.zeros((U, F)), np.zeros((U, F, F))
    for u in range(U):
        centre = rng.standard_normal(F) * 1.5
        A = rng.standard_normal((F, F)) / np.sqrt(F) + np.eye(F)
        feat[offs[u]:offs[u + 1]] = centre + rng.standard_normal((counts[u], F)) @ A.T
        mu[u] = centre + 0.01 * rng.standard_normal(F)
        vinv[u] = np.linalg.inv(A @ A.T) + 1e-3 * rng.standard_normal((F, F))
    if dup:
        feat[1::2] = feat[0:n - 1:2][:len(feat[1::2])]
    used = None
    if unused:
        used = (rng.uniform(size=n) > 0.05).astype(np.uint8)
        used[0], used[-1] = 0, 0
    return feat, offs, used, mu, vinv


def science_case(M, noise_list=False, seed=0):
    """Three synthetic units on two channels: A and B have similar templates on channel 0 and differ on channel 1, C
    is well separated on both.  -> (y, lists, pre, W, chan, events): the block, the three lists (and, with
    noise_list, nothing more: the caller appends api-style unassigned events), the window, chan of M channels, and
    every event put into the block (units' spikes and small noise events no unit owns)."""
    rng = np.random.default_rng(4000 + seed)
    T, W, pre = 60_000, 24, 8
    k = np.arange(W)
    bump = lambda c, w, a: a * np.exp(-0.5 * ((k - c) / w) ** 2)
    tmpl = {0: (bump(8, 2.0, -6.0), bump(8, 2.0, -1.0)),
            1: (bump(8, 2.2, -5.6), bump(9, 2.5, -5.0)),
            2: (bump(8, 1.5, -20.0) + bump(14, 3.0, 6.0), bump(8, 1.5, -15.0) + bump(15, 3.0, 5.0))}
    y = rng.standard_normal((2, T))
    slots = rng.permutation(np.arange(1, T // 40 - 1))[:520] * 40
    owner = np.concatenate([np.full(150, 0), np.full(150, 1), np.full(150, 2), np.full(70, 3)])
    lists = [[], [], []]
    events = []
    for t0, o in zip(slots, owner):
        t = int(t0) + 1 + pre
        events.append(t)
        if o == 3:
            amp = rng.uniform(3.0, 6.5)
            y[0, t0:t0 + W] += bump(8, 2.0, -amp)
            y[1, t0:t0 + W] += bump(8, 2.0, -amp * rng.uniform(0.0, 1.0))
            continue
        g = 1.0 + 0.03 * rng.standard_normal()
        y[0, t0:t0 + W] += g * tmpl[o][0]
        y[1, t0:t0 + W] += g * tmpl[o][1]
        lists[o].append(t)
    lists = [np.sort(np.asarray(v, dtype=np.int64)) for v in lists]
    return y, lists, pre, W, list(range(M)), np.sort(np.asarray(events, dtype=np.int64))


def pipeline(y, lists, pre, W, chan, P, space=None):
    """cluster_isolation in the model alone: -> (iso_d2, l_ratio, closer, lpair, nused, (basis, centre)).  `space`: a
    (basis, centre) to use instead of the lists' own pooled PCA"""
    if space is None:
        f0, use, n, nused = features(y, lists, pre, W, chan)
        b1, b2 = moments(f0, use, n, len(chan))
        space = pca(b1, b2, nused, P)
    f, use, n, nused = features(y, lists, pre, W, chan, *space)
    g1, g2 = moments(f, use, n, 1)
    mu, vinv = gaussians(g1[:, 0], g2[:, 0], nused)
    iso, closer, lpair, _ = isolation(f, np.concatenate([[0], np.cumsum(n)]), use, mu, vinv)
    return iso, l_ratio(lpair, nused), closer, lpair, nused, space
