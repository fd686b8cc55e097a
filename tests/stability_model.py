"""Numpy model of hmmsort_unit_stability (include/hmmsort.h): the authority the device code is compared
with, byte for byte, and of the host-side finishers of api.UnitStability.  Written for clarity, not speed.

Times are 1-based samples; everything else is 0-based.  A NaN value means "no value"."""
from types import SimpleNamespace

import numpy as np

TILE = 256
SIGN = np.uint64(1 << 63)


def keys(v):
    """order-preserving unsigned keys of doubles: -Inf < ... < -0.0 < +0.0 < ... < +Inf"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where((b & SIGN) != 0, ~b, b | SIGN)


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where((k & SIGN) != 0, k ^ SIGN, ~k).view(np.float64)


def rank(num, den, m):
    """0-based rank of quantile num / den among m values, in integers"""
    return (int(num) * (int(m) - 1)) // int(den)


def order_stats(valid, q_num, q_den):
    """the quantiles of the valid (non-NaN) values: inputs picked by rank among the sorted integer keys; NaN when
    there is none"""
    if len(valid) == 0:
        return np.full(len(q_num), np.nan)
    k = np.sort(keys(valid))
    return unkeys(np.array([k[rank(q, q_den, len(k))] for q in q_num], dtype=np.uint64)).reshape(len(q_num))


def fold(xs):
    """serial sum from +0.0, every addition rounded (Python floats are IEEE doubles, and nothing is fused)"""
    s = 0.0
    for x in xs:
        s = s + float(x)
    return s


def tiled_sums(valid):
    """(sum, sum of squares) of the valid values in event order: tiles of 256, a serial fold from +0.0 inside a tile
    with the square rounded on its own, and a serial fold from +0.0 of the tile partials"""
    ps, pq = [], []
    for i in range(0, len(valid), TILE):
        tile = [float(x) for x in valid[i:i + TILE]]
        ps.append(fold(tile))
        pq.append(fold([x * x for x in tile]))
    return fold(ps), fold(pq)


def time_bins(T, bin):
    return (int(T) + int(bin) - 1) // int(bin)


def bin_of(t, bin):
    """time bin of 1-based sample numbers"""
    return (np.asarray(t, dtype=np.int64) - 1) // int(bin)


def histogram(valid, HB, lo, scale):
    """(hist[HB], under, over): p = (v - lo) * scale, subtraction and product rounded separately"""
    h = np.zeros(HB, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (np.asarray(valid, dtype=np.float64) - np.float64(lo)) * np.float64(scale)
    under, over = int(np.sum(p < 0.0)), int(np.sum(p >= float(HB)))
    inside = p[(p >= 0.0) & (p < float(HB))]
    np.add.at(h, np.floor(inside).astype(np.int64), 1)
    return h, under, over


def unit_stability(times, values, T, bin, q_num=(), q_den=1, hist=None):
    """The tables of hmmsort_unit_stability for U lists of times (and values, or None: counts only).
    hist: None or (HB, hist_lo, hist_scale).  Returns a SimpleNamespace with the fields of hmmsort_stab_out."""
    U, B, nq = len(times), time_bins(T, bin), len(q_num)
    HB, lo, scale = hist if hist is not None else (0, 0.0, 1.0)
    r = SimpleNamespace(T=int(T), bin=int(bin), q_num=tuple(int(q) for q in q_num), q_den=int(q_den), HB=int(HB),
                        hist_lo=float(lo), hist_scale=float(scale))
    r.n = np.array([len(t) for t in times], dtype=np.int64)
    r.count = np.zeros((U, B), dtype=np.int64)
    for u, t in enumerate(times):
        np.add.at(r.count[u], bin_of(t, bin), 1)
    if values is None:
        for k in ("valid", "quant", "sum", "sumsq", "uvalid", "uquant", "umin", "umax", "usum", "usumsq", "hist",
                  "under", "over"):
            setattr(r, k, None)
        return r
    r.valid = np.zeros((U, B), dtype=np.int64)
    r.quant = np.full((U, B, nq), np.nan)
    r.sum, r.sumsq = np.zeros((U, B)), np.zeros((U, B))
    r.uvalid = np.zeros(U, dtype=np.int64)
    r.uquant = np.full((U, nq), np.nan)
    r.umin, r.umax = np.full(U, np.nan), np.full(U, np.nan)
    r.usum, r.usumsq = np.zeros(U), np.zeros(U)
    r.hist = np.zeros((U, HB), dtype=np.int64)
    r.under, r.over = np.zeros(U, dtype=np.int64), np.zeros(U, dtype=np.int64)
    for u in range(U):
        v = np.asarray(values[u], dtype=np.float64)
        b = bin_of(times[u], bin)
        ok = ~np.isnan(v)
        for bb in np.unique(b):
            seg = v[(b == bb) & ok]
            r.valid[u, bb] = len(seg)
            r.quant[u, bb] = order_stats(seg, q_num, q_den)
            r.sum[u, bb], r.sumsq[u, bb] = tiled_sums(seg)
        allv = v[ok]
        r.uvalid[u] = len(allv)
        r.uquant[u] = order_stats(allv, q_num, q_den)
        r.umin[u], r.umax[u] = order_stats(allv, (0, 1), 1)
        r.usum[u], r.usumsq[u] = fold(r.sum[u]), fold(r.sumsq[u])   # the bin sums, not the events again
        if HB > 0:
            r.hist[u], r.under[u], r.over[u] = histogram(allv, HB, lo, scale)
    return r


# ---- finishers (api.UnitStability states the same) -------------------------------------------------------------------

def bin_samples(r):
    """[B]: samples per time bin; the last one may be short"""
    B = time_bins(r.T, r.bin)
    return np.minimum(r.bin, r.T - np.arange(B, dtype=np.int64) * r.bin)


def firing_rate(r, fs):
    """[U, B]: spikes per second in every time bin"""
    return r.count / (bin_samples(r) / float(fs))


def presence_ratio(r, min_count=1):
    """[U]: the share of full-length bins with at least min_count spikes; the short last bin is left out unless it is
    the only bin"""
    full = bin_samples(r) == r.bin
    if not full.any():
        full[:] = True
    return np.sum(r.count[:, full] >= int(min_count), axis=1) / float(np.sum(full))


def median_index(r):
    for k, q in enumerate(r.q_num):
        if 2 * q == r.q_den:
            return k
    raise ValueError("amplitude_drift needs the quantile 1/2 among the quantiles")


def amplitude_drift(r, min_valid=20):
    """[U]: (largest - smallest per-bin median) / overall median, over the bins with at least min_valid values; NaN
    for a unit without such a bin"""
    k = median_index(r)
    out = np.full(len(r.n), np.nan)
    for u in range(len(r.n)):
        med = r.quant[u, r.valid[u] >= int(min_valid), k]
        if len(med):
            with np.errstate(divide="ignore", invalid="ignore"):
                out[u] = (med.max() - med.min()) / r.uquant[u, k]
    return out


SMOOTH = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def amplitude_cutoff(r):
    """[U]: the estimated share of spikes lost below the detection floor (Hill et al. 2011), from the histogram: the
    counts smoothed with the binomial kernel (1, 4, 6, 4, 1) / 16 (zero padded), the peak at the first largest smoothed
    bin, the low edge at the first non-empty bin (bin 0 when `under` counts anything); the mass of the smoothed bins at
    or above the mirror image of the low edge about the peak, plus `over`, over the total count, capped at 0.5.  NaN for
    a unit without a value."""
    HB = r.hist.shape[1]
    out = np.full(len(r.n), np.nan)
    for u in range(len(r.n)):
        h = r.hist[u].astype(np.float64)
        total = float(r.under[u] + r.hist[u].sum() + r.over[u])
        if total == 0 or HB == 0:
            continue
        sm = np.convolve(h, SMOOTH, mode="same") if HB >= len(SMOOTH) else h
        peak = int(np.argmax(sm))
        nz = np.nonzero(r.hist[u])[0]
        low = 0 if r.under[u] > 0 or len(nz) == 0 else int(nz[0])
        mirror = 2 * peak - low
        mass = float(sm[mirror:].sum()) if mirror < HB else 0.0
        out[u] = min(0.5, (mass + float(r.over[u])) / total)
    return out
