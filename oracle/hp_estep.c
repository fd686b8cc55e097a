/*
 * hp_estep.c -- TEST INFRASTRUCTURE ONLY.  Extended-precision Baum-Welch E-step of a Gaussian
 * HMM given as a transition list, written from the equations (Rabiner 1989, section V.A,
 * scaled forward-backward) and not from hmm_oracle.c: another number format (long double, x87,
 * 64-bit mantissa), another formulation (linear domain with per-sample scaling instead of
 * unscaled log domain), another memory scheme (checkpointed alpha, O(S*(T/C + C)) memory).
 * It is the checker of the checkers: the fp64 oracle and every device engine are compared with it.
 *
 * Model (the definitions that belong to the model, reference baumwelch.jl:25-98, 205-309):
 *   b_j(y)        = N(y; m_j, sigma^2),  m_j = per-state mean handed in by the caller
 *   alpha_0(j)    = b_j(y_0)                      (no initial distribution: uniform, dropped)
 *   alpha_t(j)    = b_j(y_t) * sum_i alpha_{t-1}(i) a_ij
 *   beta_{T-1}(i) = 1
 *   beta_t(i)     = sum_j a_ij b_j(y_{t+1}) beta_{t+1}(j)
 *   gamma_t(j)    = alpha_t(j) beta_t(j) / P(y)
 *   xi_t(i,j)     = alpha_t(i) a_ij b_j(y_{t+1}) beta_{t+1}(j) / P(y),   t = 0 .. T-2
 *
 * Scaling.  With e_t = min_j (y_t - m_j)^2 the emission is factored as
 *   b_j(y_t) = k_t * bt_j(t),   bt_j(t) = exp(-((y_t - m_j)^2 - e_t) / (2 sigma^2)) in (0, 1],
 *   log k_t  = -e_t / (2 sigma^2) - log(sigma sqrt(2 pi)),
 * and the recursions run on ah_t = alpha_t / (alpha_t summed over states), i.e.
 *   ah_t(j) = bt_j(t) * sum_i ah_{t-1}(i) a_ij / c_t,   c_t = the sum over j of the numerators,
 *   bh_t(i) = sum_j a_ij w_{t+1}(j),   w_{t+1}(j) = bt_j(t+1) bh_{t+1}(j) / c_{t+1},  bh_{T-1} = 1,
 * so that gamma_t(j) = ah_t(j) bh_t(j), xi_t(i,j) = ah_t(i) a_ij w_{t+1}(j) with no further
 * normalisation (neither is renormalised here: sum_j gamma_t(j) = 1 is a checked property), and
 *   log P(y) = sum_t (log c_t + log k_t).
 *
 * The forward pass keeps ah_t and c_t at t = 0, C, 2C, ...; the backward pass recomputes the block's ah
 * from its checkpoint (the same operations on the same values, hence the same bits) and walks it
 * downwards.  Every accumulation runs in one fixed serial order (t descending, states/transitions
 * ascending), so the block length cannot change a bit of the result.  The emission table of a
 * block is filled by `threads` threads; each entry is computed by exactly one of them from y_t,
 * m_j, sigma alone, so the thread count cannot either.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#if LDBL_MANT_DIG < 64
#error "hp_estep.c needs a long double with at least a 64-bit mantissa; there is no fallback"
#endif

typedef long double ld;

int hp_mant_dig(void) { return LDBL_MANT_DIG; }

/* bt (n x S, row per sample) and log k_t for samples [t0, t0+n) */
static void emissions(const double *y, int64_t t0, int64_t n, int64_t S, const ld *m, ld inv2s2,
                      ld logsig, ld *bt, ld *logk, int threads)
{
#pragma omp parallel for num_threads(threads) schedule(static)
    for (int64_t u = 0; u < n; u++) {
        ld v = (ld)y[t0 + u];
        ld *row = bt + u * S;
        ld e = INFINITY;
        for (int64_t j = 0; j < S; j++) {
            ld d = v - m[j];
            row[j] = d * d;
            if (row[j] < e) e = row[j];
        }
        for (int64_t j = 0; j < S; j++)
            row[j] = expl(-(row[j] - e) * inv2s2);
        logk[u] = -e * inv2s2 - logsig;
    }
}

/* one scaled forward step: an <- bt .* (A' ap) / c ; returns c */
static ld fwd_step(int64_t S, int64_t R, const int64_t *src, const int64_t *dst, const ld *a,
                   const ld *ap, const ld *bt, ld *an)
{
    for (int64_t j = 0; j < S; j++) an[j] = 0.0L;
    for (int64_t r = 0; r < R; r++) an[dst[r]] += ap[src[r]] * a[r];
    ld c = 0.0L;
    for (int64_t j = 0; j < S; j++) {
        an[j] *= bt[j];
        c += an[j];
    }
    for (int64_t j = 0; j < S; j++) an[j] /= c;
    return c;
}

/*
 * y[T]; transitions (src, dst 0-based, lp = log a) x R; mean[S]; sigma; block = C; threads.
 * win[2*nwin] = sample windows [lo, hi); gwin receives gamma (row per window sample, S columns,
 * windows concatenated in the order given), rounded once to double.
 * Outputs (long double): sg[S] = sum_t gamma_t(j), sgd[S] = sum_t gamma_t(j)(y_t - m_j),
 * sgd2[S] = sum_t gamma_t(j)(y_t - m_j)^2, sxi[R] = sum_{t<T-1} xi_t(r), g0[S] = gamma_0,
 * gl[S] = gamma_{T-1}, *loglik, *defect = max_t |sum_j gamma_t(j) - 1|.
 * Returns 0, -1 out of memory, -2 bad argument, -3 a scale c_t that is not positive and finite.
 */
int hp_estep(const double *y, int64_t T, int64_t S, int64_t R, const int64_t *src,
             const int64_t *dst, const double *lp, const double *mean, double sigma, int64_t block,
             int threads, int64_t nwin, const int64_t *win, double *gwin, ld *sg, ld *sgd, ld *sgd2,
             ld *sxi, ld *g0, ld *gl, ld *loglik, ld *defect)
{
    if (T < 1 || S < 1 || R < 0 || block < 1 || threads < 1 || !(sigma > 0)) return -2;
    for (int64_t r = 0; r < R; r++)
        if (src[r] < 0 || src[r] >= S || dst[r] < 0 || dst[r] >= S) return -2;
    for (int64_t w = 0; w < nwin; w++) {
        if (win[2 * w] < 0 || win[2 * w + 1] > T || win[2 * w] > win[2 * w + 1]) return -2;
    }
    int rc = 0;
    int64_t C = block < T ? block : T;
    int64_t nb = (T + C - 1) / C;
    ld *a = malloc(sizeof(ld) * (size_t)(R > 0 ? R : 1));
    ld *m = malloc(sizeof(ld) * (size_t)S);
    ld *ck = malloc(sizeof(ld) * (size_t)(nb * S));      /* ah at t = k*C */
    ld *cck = malloc(sizeof(ld) * (size_t)nb);           /* c at t = k*C */
    ld *bt = malloc(sizeof(ld) * (size_t)(C * S));       /* emissions of one block */
    ld *ah = malloc(sizeof(ld) * (size_t)(C * S));       /* ah of one block */
    ld *cs = malloc(sizeof(ld) * (size_t)C);             /* c_t of one block */
    ld *logk = malloc(sizeof(ld) * (size_t)C);
    ld *bh = malloc(sizeof(ld) * (size_t)S);
    ld *w = malloc(sizeof(ld) * (size_t)S);
    int64_t *woff = malloc(sizeof(int64_t) * (size_t)(nwin > 0 ? nwin : 1));
    if (!a || !m || !ck || !cck || !bt || !ah || !cs || !logk || !bh || !w || !woff) { rc = -1; goto done; }
    for (int64_t r = 0; r < R; r++) a[r] = expl((ld)lp[r]);
    for (int64_t j = 0; j < S; j++) m[j] = (ld)mean[j];
    {
        int64_t o = 0;
        for (int64_t q = 0; q < nwin; q++) { woff[q] = o; o += win[2 * q + 1] - win[2 * q]; }
    }
    const ld s = (ld)sigma;
    const ld inv2s2 = 1.0L / (2.0L * s * s);
    const ld logsig = logl(s * sqrtl(2.0L * acosl(-1.0L)));

    /* ---- forward: log-likelihood, checkpoints ah_{kC} and their scales c_{kC} ---- */
    ld ll = 0.0L;
    ld *prev = w, *cur = bh;                                /* two rows, swapped every sample */
    for (int64_t k = 0; k < nb; k++) {
        int64_t t0 = k * C, n = (t0 + C <= T) ? C : T - t0;
        emissions(y, t0, n, S, m, inv2s2, logsig, bt, logk, threads);
        for (int64_t u = 0; u < n; u++) {
            ld c;
            if (t0 + u == 0) {
                /* alpha_0(j) = b_j(y_0): no initial distribution */
                c = 0.0L;
                for (int64_t j = 0; j < S; j++) c += bt[j];
                for (int64_t j = 0; j < S; j++) cur[j] = bt[j] / c;
            } else {
                c = fwd_step(S, R, src, dst, a, prev, bt + u * S, cur);
            }
            if (!(c > 0.0L) || !isfinite(c)) { rc = -3; goto done; }
            ll += logl(c) + logk[u];
            if (u == 0) {
                memcpy(ck + k * S, cur, sizeof(ld) * (size_t)S);
                cck[k] = c;
            }
            ld *sw = prev; prev = cur; cur = sw;
        }
    }
    *loglik = ll;

    /* ---- backward, block by block from the end ---- */
    for (int64_t j = 0; j < S; j++) sg[j] = sgd[j] = sgd2[j] = 0.0L;
    for (int64_t r = 0; r < R; r++) sxi[r] = 0.0L;
    ld dmax = 0.0L;
    for (int64_t k = nb - 1; k >= 0; k--) {
        int64_t t0 = k * C, n = (t0 + C <= T) ? C : T - t0;
        emissions(y, t0, n, S, m, inv2s2, logsig, bt, logk, threads);
        memcpy(ah, ck + k * S, sizeof(ld) * (size_t)S);
        cs[0] = cck[k];
        for (int64_t u = 1; u < n; u++)
            cs[u] = fwd_step(S, R, src, dst, a, ah + (u - 1) * S, bt + u * S, ah + u * S);
        for (int64_t u = n - 1; u >= 0; u--) {
            int64_t t = t0 + u;
            const ld *au = ah + u * S;
            if (t == T - 1) {
                for (int64_t j = 0; j < S; j++) bh[j] = 1.0L;       /* beta_{T-1} = 1 */
            } else {
                /* w holds w_{t+1}; xi_t(r) = ah_t(src) a_r w_{t+1}(dst), bh_t(i) = sum_j a_ij w_{t+1}(j) */
                for (int64_t j = 0; j < S; j++) bh[j] = 0.0L;
                for (int64_t r = 0; r < R; r++) {
                    ld aw = a[r] * w[dst[r]];
                    bh[src[r]] += aw;
                    sxi[r] += au[src[r]] * aw;
                }
            }
            ld v = (ld)y[t], gs = 0.0L;
            for (int64_t j = 0; j < S; j++) {
                ld g = au[j] * bh[j];
                ld d = v - m[j];
                gs += g;
                sg[j] += g;
                sgd[j] += g * d;
                sgd2[j] += g * (d * d);
            }
            gs = fabsl(gs - 1.0L);
            if (gs > dmax) dmax = gs;
            if (t == 0) for (int64_t j = 0; j < S; j++) g0[j] = au[j] * bh[j];
            if (t == T - 1) for (int64_t j = 0; j < S; j++) gl[j] = au[j] * bh[j];
            for (int64_t q = 0; q < nwin; q++)
                if (t >= win[2 * q] && t < win[2 * q + 1]) {
                    double *o = gwin + (woff[q] + (t - win[2 * q])) * S;
                    for (int64_t j = 0; j < S; j++) o[j] = (double)(au[j] * bh[j]);
                }
            /* w_t(j) = bt_j(t) bh_t(j) / c_t for the step below */
            for (int64_t j = 0; j < S; j++) w[j] = bt[u * S + j] * bh[j] / cs[u];
        }
    }
    *defect = dmax;
done:
    free(a); free(m); free(ck); free(cck); free(bt); free(ah); free(cs); free(logk); free(bh); free(w);
    free(woff);
    return rc;
}
