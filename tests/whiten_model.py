"""The rules of the whitening stages (include/hmmsort.h, "Spatial whitening"; csrc/whiten.hip) in numpy: every
operation in the order and with the rounding the contract fixes, so that the device result can be compared with ==.
numpy rounds every elementwise product and sum on its own (no fused multiply-add), which is what the contract asks.
All functions take the fp64 channel-major block Y of shape (C, T)."""
import numpy as np

from seed_model import MAD_TO_SIGMA, noise_scale as row_noise_scale  # noqa: F401 (MAD_TO_SIGMA: for the tests)

TILE = 256


def noise_scale(Y):
    """sigma[c]: order statistic (T - 1) // 2 of |Y[c]| over MAD_TO_SIGMA, the seed's rule row by row"""
    return np.array([row_noise_scale(row) for row in np.asarray(Y, dtype=np.float64)])


def loud_mask(Y, thr):
    """loud[t] iff some channel has not (|Y[c][t]| <= thr[c]); NaN and Inf samples are loud"""
    with np.errstate(invalid="ignore"):
        return (~(np.abs(Y) <= np.asarray(thr, dtype=np.float64)[:, None])).any(axis=0)


def quiet_mask(Y, thr, guard=30):
    """quiet[t] iff no sample of [max(0, t - guard), min(T - 1, t + guard)] is loud"""
    loud = loud_mask(Y, thr)
    T = len(loud)
    cs = np.concatenate([[0], np.cumsum(loud)])
    t = np.arange(T)
    lo, hi = np.maximum(0, t - guard), np.minimum(T - 1, t + guard)
    return cs[hi + 1] - cs[lo] == 0


def sums(Y, quiet, tile=TILE, by_quiet_index=False):
    """(s1, s2): per tile of `tile` consecutive samples a serial fold from +0.0 over its quiet samples in ascending t,
    p1 = p1 + y, p2 = p2 + outer(y, y) with the products rounded on their own; the tile partials folded serially from
    +0.0 in tile order.  by_quiet_index cuts the tiles by position among the quiet samples instead (NOT the rule:
    the tests show that it differs)."""
    Y = np.asarray(Y, dtype=np.float64)
    nC, T = Y.shape
    s1, s2 = np.zeros(nC), np.zeros((nC, nC))
    if by_quiet_index:
        Y, T = Y[:, quiet], int(np.count_nonzero(quiet))
        quiet = np.ones(T, dtype=bool)
    for t0 in range(0, T, tile):
        p1, p2 = np.zeros(nC), np.zeros((nC, nC))
        for t in np.nonzero(quiet[t0:t0 + tile])[0] + t0:
            y = Y[:, t]
            p1 = p1 + y
            p2 = p2 + np.multiply.outer(y, y)
        s1 = s1 + p1
        s2 = s2 + p2
    return s1, s2


def noise_cov(Y, threshold=4.0, guard=30, thr=None):
    """(sigma or None, thr, quiet, n_quiet, s1, s2) as hmmsort_noise_cov computes them"""
    Y = np.asarray(Y, dtype=np.float64)
    sigma = None
    if thr is None:
        sigma = noise_scale(Y)
        thr = threshold * sigma
    thr = np.broadcast_to(np.asarray(thr, dtype=np.float64), (Y.shape[0],))
    quiet = quiet_mask(Y, thr, guard)
    s1, s2 = sums(Y, quiet)
    return sigma, thr, quiet, int(np.count_nonzero(quiet)), s1, s2


def mix(Y, nbr, w):
    """out[r] = fold over m ascending, empty slots (nbr = -1) skipped: acc = acc + w[r][m] * Y[nbr[r][m]]"""
    Y = np.asarray(Y, dtype=np.float64)
    nbr, w = np.asarray(nbr), np.asarray(w, dtype=np.float64)
    R, M = nbr.shape
    acc = np.zeros((R, Y.shape[1]))
    for m in range(M):
        rows = np.nonzero(nbr[:, m] >= 0)[0]
        if len(rows):
            acc[rows] = acc[rows] + w[rows, m][:, None] * Y[nbr[rows, m]]
    return acc


def heavy_tailed(rng, C, T):
    """normal x 10^uniform(-3, 3): magnitudes over six decades, so that the order and the tiling of a sum show"""
    return rng.standard_normal((C, T)) * 10.0 ** rng.uniform(-3.0, 3.0, size=(C, T))
