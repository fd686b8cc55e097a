/*
 * hp_viterbi.c -- TEST INFRASTRUCTURE ONLY.  Extended-precision maximum-a-posteriori path of a
 * Gaussian HMM given as a transition list, written from the equations (Rabiner 1989, section
 * III.B, max-sum form) and not from hmm_oracle.c: another number format (long double, x87, 64-bit
 * mantissa), another formulation (delta renormalised at every sample, gather over the incoming
 * transitions of a state instead of a scatter over the list, no back-pointer array), another memory
 * scheme (checkpointed delta, O(S*(T/C + C)) memory).  The fp64 oracle's decode and every device
 * engine's are compared with it.
 *
 * Model (the definitions that belong to the model; reference viterbi.jl:44-98, utils.jl:1-4):
 *   q_j(y)     = -1/2 log(2 pi) - log(sigma) - (y - m_j)^2 / (2 sigma^2)   (utils.jl:1 `log2pi` is
 *                1/2 log 2 pi; utils.jl:4), m_j = per-state mean handed in by the caller
 *   delta_0(1) = 0, delta_0(j) = q_j(y_0) otherwise        (viterbi.jl:55-63: no initial distribution,
 *                                                           the silent state does not emit at sample 0)
 *   delta_t(j) = max_r { delta_{t-1}(src_r) + lp_r : dst_r = j } + q_j(y_t)          (viterbi.jl:74-87)
 *                the maximum is the first one in list order (strict >, :80); a state that no finite
 *                candidate reaches keeps -inf and points at state 1 (:52-53)
 *   x_{T-1}    = first arg max_j delta_{T-1}(j)  (:90),   x_{t-1} = the maximiser of delta_t(x_t)  (:94)
 *   ll         = sum_{t >= 1} delta_t(x_t), the reference's sum of cumulative values  (:92-96)
 *   score      = delta_{T-1}(x_{T-1}), the log-probability of the path itself
 *
 * Formulation.  dh_t = delta_t - G_t with G_t = sum_{s <= t} c_s, c_s = the column maximum before
 * it is subtracted: every stored value has the magnitude of a difference between explanations of the
 * last few samples (a few hundred at most), never the O(t) magnitude whose fp64 rounding decides the
 * reference implementation's near-ties.  G_t is accumulated apart, in one serial order.
 *
 * The forward pass keeps dh_t and G_t at t = C-1, 2C-1, ...; the backward pass recomputes a block's dh
 * rows from its checkpoint (the same operations on the same values, hence the same bits), and finds
 * x_{t-1} by repeating the maximisation of the one state x_t over its incoming transitions in list
 * order.  ll is summed for t descending, whatever the block length, so C cannot change a bit of any
 * output.  The states of a column are spread over `threads` threads (only when S >= 1024); each dh_t(j)
 * is computed by exactly one thread from dh_{t-1}, y_t, m_j, sigma and the column maximum is exact in
 * any order, so the thread count cannot either.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if LDBL_MANT_DIG < 64
#error "hp_viterbi.c needs a long double with at least a 64-bit mantissa; there is no fallback"
#endif

typedef long double ld;

int hpv_mant_dig(void) { return LDBL_MANT_DIG; }

typedef struct {
    int64_t S;
    const int64_t *off;     /* S+1: incoming transitions of state j are in[off[j] .. off[j+1]) */
    const int64_t *isrc;    /* source state, list order kept within a destination */
    const ld *ilp;
    const ld *m;
    ld c0, two_s2;
    int threads;
} model_t;

/* the maximiser of one state: first maximum in list order; state 0 (the model's state 1) if none is finite */
static inline int64_t best_in(const model_t *M, const ld *prev, int64_t j, ld *val)
{
    ld best = -INFINITY;
    int64_t k = 0;
    for (int64_t e = M->off[j]; e < M->off[j + 1]; e++) {
        ld t = prev[M->isrc[e]] + M->ilp[e];
        if (t > best) { best = t; k = M->isrc[e]; }
    }
    *val = best;
    return k;
}

/* one column: out = dh_t from prev = dh_{t-1} (prev == NULL: sample 0); returns c_t, the subtracted maximum */
static ld column(const model_t *M, const ld *prev, double yt, ld *out)
{
    const int64_t S = M->S;
    const ld v = (ld)yt;
#pragma omp parallel for num_threads(M->threads) schedule(static) if (M->threads > 1 && S >= 1024)
    for (int64_t j = 0; j < S; j++) {
        ld d = v - M->m[j];
        ld q = M->c0 - d * d / M->two_s2;
        if (prev) {
            ld b;
            best_in(M, prev, j, &b);
            out[j] = b + q;
        } else {
            out[j] = j == 0 ? 0.0L : q;
        }
    }
    ld c = -INFINITY;
    for (int64_t j = 0; j < S; j++) if (out[j] > c) c = out[j];
    if (!isfinite(c)) return c;
    for (int64_t j = 0; j < S; j++) out[j] -= c;
    return c;
}

/*
 * y[T]; transitions (src, dst 0-based, lp) x R; mean[S]; sigma; block = C; threads.
 * idx[nidx]: sample indices, ascending, at which cum receives delta_t(x_t), the score of the path up to
 * and including sample t.
 * Outputs: x[T] (1-based states), *score, *ll, cum[nidx], *dmax = max_t |dh_t(x_t)| (how far below the
 * column maximum the path ever runs: the magnitude whose long-double rounding decides this routine's ties).
 * Returns 0, -1 out of memory, -2 bad argument, -3 a column without a finite value.
 */
int hp_viterbi(const double *y, int64_t T, int64_t S, int64_t R, const int64_t *src, const int64_t *dst,
               const double *lp, const double *mean, double sigma, int64_t block, int threads,
               int64_t nidx, const int64_t *idx, int32_t *x, ld *score, ld *ll, ld *cum, ld *dmax)
{
    if (T < 1 || S < 1 || R < 0 || block < 1 || threads < 1 || !(sigma > 0) || nidx < 0) return -2;
    for (int64_t r = 0; r < R; r++)
        if (src[r] < 0 || src[r] >= S || dst[r] < 0 || dst[r] >= S) return -2;
    for (int64_t i = 0; i < nidx; i++)
        if (idx[i] < 0 || idx[i] >= T || (i > 0 && idx[i] < idx[i - 1])) return -2;
    int rc = 0;
    const int64_t C = block < T ? block : T;
    const int64_t nb = (T + C - 1) / C;
    int64_t *off = calloc((size_t)(S + 1), sizeof(int64_t));
    int64_t *fill = malloc(sizeof(int64_t) * (size_t)S);
    int64_t *isrc = malloc(sizeof(int64_t) * (size_t)(R > 0 ? R : 1));
    ld *ilp = malloc(sizeof(ld) * (size_t)(R > 0 ? R : 1));
    ld *m = malloc(sizeof(ld) * (size_t)S);
    ld *ck = malloc(sizeof(ld) * (size_t)(nb * S));       /* ck[k] = dh at t = k*C - 1, k >= 1 */
    ld *gck = malloc(sizeof(ld) * (size_t)nb);            /* G at the same samples */
    ld *buf = malloc(sizeof(ld) * (size_t)((C + 1) * S)); /* row u+1 = dh at t0 + u, row 0 = the checkpoint */
    ld *g = malloc(sizeof(ld) * (size_t)(C + 1));
    if (!off || !fill || !isrc || !ilp || !m || !ck || !gck || !buf || !g) { rc = -1; goto done; }

    for (int64_t r = 0; r < R; r++) off[dst[r] + 1]++;
    for (int64_t j = 0; j < S; j++) { off[j + 1] += off[j]; fill[j] = off[j]; }
    for (int64_t r = 0; r < R; r++) {
        int64_t e = fill[dst[r]]++;
        isrc[e] = src[r];
        ilp[e] = (ld)lp[r];
    }
    for (int64_t j = 0; j < S; j++) m[j] = (ld)mean[j];
    const ld s = (ld)sigma;
    model_t M = { S, off, isrc, ilp, m, -0.5L * logl(2.0L * acosl(-1.0L)) - logl(s), 2.0L * s * s, threads };

    /* ---- forward: checkpoints only ---- */
    ld *prev = buf, *cur = buf + S, G = 0.0L;
    for (int64_t t = 0; t < T; t++) {
        ld c = column(&M, t == 0 ? NULL : prev, y[t], cur);
        if (!isfinite(c)) { rc = -3; goto done; }
        G += c;
        if ((t + 1) % C == 0 && (t + 1) / C < nb) {
            memcpy(ck + ((t + 1) / C) * S, cur, sizeof(ld) * (size_t)S);
            gck[(t + 1) / C] = G;
        }
        ld *sw = prev; prev = cur; cur = sw;
    }
    {
        int64_t jm = 0;                                 /* first arg-max of the last column */
        for (int64_t j = 1; j < S; j++) if (prev[j] > prev[jm]) jm = j;
        x[T - 1] = (int32_t)(jm + 1);
        *score = prev[jm] + G;
    }

    /* ---- backward, block by block from the end ---- */
    ld L = 0.0L, dm = 0.0L;
    int64_t p = nidx - 1;
    for (int64_t k = nb - 1; k >= 0; k--) {
        int64_t t0 = k * C, n = (t0 + C <= T) ? C : T - t0;
        if (k > 0) {
            memcpy(buf, ck + k * S, sizeof(ld) * (size_t)S);
            g[0] = gck[k];
        } else {
            g[0] = 0.0L;
        }
        for (int64_t u = 0; u < n; u++) {
            ld c = column(&M, t0 + u == 0 ? NULL : buf + u * S, y[t0 + u], buf + (u + 1) * S);
            g[u + 1] = g[u] + c;
        }
        for (int64_t u = n - 1; u >= 0; u--) {
            int64_t t = t0 + u, j = x[t] - 1;
            ld dh = buf[(u + 1) * S + j], val = dh + g[u + 1];
            if (fabsl(dh) > dm) dm = fabsl(dh);
            while (p >= 0 && idx[p] == t) cum[p--] = val;
            if (t >= 1) {
                ld b;
                L += val;
                x[t - 1] = (int32_t)(best_in(&M, buf + u * S, j, &b) + 1);
            }
        }
    }
    *ll = L;
    *dmax = dm;
done:
    free(off); free(fill); free(isrc); free(ilp); free(m); free(ck); free(gck); free(buf); free(g);
    return rc;
}
