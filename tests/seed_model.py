"""Numpy model of the template seed (DESIGN "Template seed"): robust noise scale, threshold crossings that are the
extremum of their +-R window, snippets read in place, centres started at amplitude quantiles, Lloyd iterations.
Written for reading, not speed; the GPU tests compare hmmsort_seed_templates with it.  All indices 0-based except
the returned event times, which are 1-based like extract_spiketimes."""
import numpy as np

MAD_TO_SIGMA = 0.6744897501960817   # the normal distribution's upper quartile


def noise_scale(y):
    """lower median of |y| (order statistic (T-1)//2, exact) over the quartile constant: one division"""
    a = np.abs(np.asarray(y, dtype=np.float64))
    r = (len(a) - 1) // 2
    return float(np.partition(a, r)[r]) / MAD_TO_SIGMA


def detect(y, K, threshold, sigma_n, polarity, align, refractory):
    """ascending 0-based event samples"""
    T, D, R, a = len(y), K - 1, refractory, align
    v = -y if polarity < 0 else (np.abs(y) if polarity == 0 else y)
    thr = threshold * sigma_n
    ev = []
    for t in np.nonzero(v > thr)[0].tolist():
        if t - a < 0 or t - a + D - 1 > T - 1:
            continue
        if np.all(v[max(0, t - R):t] < v[t]) and np.all(v[t + 1:min(T - 1, t + R) + 1] <= v[t]):
            ev.append(t)
    return np.array(ev, dtype=np.int64), v


def distances(S, c):
    """d[e, i] = sum_j (S[e, j] - c[i, j])^2, accumulated in ascending j, multiply and add rounded separately"""
    d = np.zeros((S.shape[0], c.shape[0]))
    for j in range(S.shape[1]):
        diff = S[:, j, None] - c[None, :, j]
        d = d + diff * diff
    return d


def seed_model(y, N, K, threshold=4.0, sigma=0.0, polarity=0, align=None, refractory=None, max_iters=20):
    """-> dict(mu K x N, sigma, lp, counts, n_events, iters, times (1-based), labels, margin).
    margin: the smallest (second best - best) / second best distance any assignment saw (inf when N == 1 or no
    event): exact label comparison with another implementation is fair only when this is far above rounding."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    T, D = len(y), K - 1
    a = D // 3 if align is None or align < 0 else int(align)
    R = K - 1 if refractory is None or refractory < 0 else int(refractory)
    if max_iters is None or max_iters <= 0:
        max_iters = 20
    if threshold is None or threshold != threshold:
        threshold = 4.0
    sigma_n = float(sigma) if sigma > 0 else noise_scale(y)
    ev, v = detect(y, K, threshold, sigma_n, polarity, a, R)
    E = len(ev)
    mu = np.zeros((K, N), order="F")
    counts = np.zeros(N, dtype=np.int64)
    labels = np.full(E, -1, dtype=np.int64)
    iters, margin = 0, np.inf
    if E > 0:
        S = np.stack([y[t - a:t - a + D] for t in ev])
        order = np.lexsort((ev, v[ev]))                       # by (v[t_e], t_e) ascending
        c = np.stack([S[order[min(E - 1, ((2 * i + 1) * E) // (2 * N))]] for i in range(N)])
        while True:
            d = distances(S, c)
            new = np.argmin(d, axis=1)                         # first minimum: ties to the lower i
            if N > 1:
                two = np.sort(d, axis=1)[:, :2]
                with np.errstate(invalid="ignore", divide="ignore"):
                    m = np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / two[:, 1], 0.0)
                margin = min(margin, float(m.min()))
            iters += 1
            changed = bool(np.any(new != labels))
            labels = new
            if not changed:
                break
            for i in range(N):
                if np.any(labels == i):
                    c[i] = S[labels == i].sum(axis=0) / np.count_nonzero(labels == i)
            if iters == max_iters:
                break
        counts = np.bincount(labels, minlength=N).astype(np.int64)
        mu[1:, :] = c.T
    with np.errstate(divide="ignore"):
        lp = np.log(counts / T)
    return dict(mu=mu, sigma=sigma_n, lp=lp, counts=counts, n_events=E, iters=iters, times=ev + 1,
                labels=labels.astype(np.int16), margin=margin, align=a)


def best_shift_error(mu_col, truth_col, max_shift=None):
    """relative RMS error of a template against the generating one at the best integer shift, over the rows the
    two share at that shift (a seed is aligned to its extremum, not to the generating template's first row)"""
    K = len(truth_col)
    max_shift = K // 2 if max_shift is None else max_shift
    best = np.inf
    for s in range(-max_shift, max_shift + 1):
        a, b = (mu_col[:K - s], truth_col[s:]) if s >= 0 else (mu_col[-s:], truth_col[:K + s])
        best = min(best, float(np.sqrt(np.sum((a - b) ** 2) / np.sum(b ** 2))))
    return best


def match_errors(mu, truth):
    """each generating template's error against its best column of mu: (errors, columns)"""
    err = np.array([[best_shift_error(mu[:, i], truth[:, k]) for i in range(mu.shape[1])]
                    for k in range(truth.shape[1])])
    return err.min(axis=1), err.argmin(axis=1)
