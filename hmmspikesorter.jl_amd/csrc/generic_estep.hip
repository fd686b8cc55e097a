// Time-parallel E-step for an ARBITRARY transition list (overlap models, reference types.jl:78-90):
// forward (baumwelch.jl:25-51), backward (:73-98) and the sufficient statistics of update (:205-309)
// without materialising alpha/beta/gamma for the whole signal.
//
// The signal is cut into the blocked engine's blocks of B samples (generic_blocked.hip).  One
// workgroup takes one block at a time: a forward sweep over [lo-H, hi) from a flat column (emissions
// only), keeping the scaled alpha of its OWN samples in a per-workgroup HBM window of S x B doubles,
// then a backward sweep from hi+H down to lo which, on the owned samples, turns alpha*beta into gamma
// and adds it to the block's statistics in registers.  Workspace = (resident workgroups) x S x B
// doubles, whatever T is; the reference's S x T arrays (28.8 GB each at S = 3600, T = 10^6) never exist.
//
// Arithmetic: the recursions run in the linear domain with one scale per column (alpha_hat = alpha /
// sum, beta likewise) instead of the reference's log-sum-exp per transition; gamma is normalised per
// sample, so the scales (and the unknown constant of a warmed-up block) cancel exactly as the `- g`
// of baumwelch.jl:222 cancels them.  Emissions are shifted by the largest exponent of the column
// (exp(e_j - max_j e_j)), so a sample far from every state mean does not underflow the column.
// Differences to the log-domain sweep: 1e-13 relative (tests: 1e-8 against the strict engine).
//
// Whether H samples of warm-up were enough is CERTIFIED per boundary (bes_check): the posterior
// gamma at the boundary sample must not move (L1 distance <= tol) when the neighbour's exact column
// is replaced by the warmed-up one.  Failures are counted in diag[3] (forward) / diag[5] (backward);
// hmmsort_em_step then retries with a longer warm-up and finally with the strict engine.
//
// Statistics (per state j, summed over t):  G0_j = sum gamma_j(t),  G1_j = sum gamma_j(t) y_t;
// X_i = sum_{t<T-1} xi_i(t) for the transitions i leaving the silent state (:229-261, normalised by the
// all-transition total, which equals the gamma normaliser);  Gamma0 = sum_{t<T-1} gamma_1(t);  sum y^2.
// sigma follows from  sum_t sum_j (y_t - m_j)^2 gamma_j(t) = sum y^2 - 2 sum_j m_j G1_j + sum_j m_j^2 G0_j.
//
// Posteriors (hmmsort_plan_posteriors on a blocked plan, DESIGN 3.5 "Blocked path"): the same sweep in a second
// instantiation, bes_block_post, reduces the gamma of every owned sample over the workgroup into per-template
// onset / occupancy / trough mass, the silent state's gamma and the arg-max state, and sums the log-likelihood in
// the forward sweep.  The kernel body is generic_estep_block.inc, included once for each of the two kernels.
#include <cmath>

#include "fastmath.h"
#include "generic_dev.h"
#include "hmmsort_internal.h"
#include "generic_estep_common.h"

namespace hmmsort {

namespace {

#define BES_POST 0
#include "generic_estep_block.inc"
#undef BES_POST
#define BES_POST 1
#include "generic_estep_block.inc"
#undef BES_POST

// logz = sum of the blocks' terms in block order + T (-log(sigma sqrt(2 pi)))
__global__ __launch_bounds__(64) void bes_logz(int nblk, const double *__restrict__ partL, double c0T,
                                               double *__restrict__ logz)
{
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 64) acc += partL[b];
    acc = wsum(acc);
    if (threadIdx.x == 0) logz[0] = acc + c0T;
}

// Boundary certificates.  Boundary c (between blocks c and c+1, samples hi-1 | hi):
//   forward : gamma(hi-1) of block c, with its exact alpha(hi-1) replaced by block c+1's warmed-up one;
//   backward: gamma(hi) of block c+1, with its exact beta(hi) replaced by block c's warmed-up one.
// err = sum_j | gamma_j r_j / sum(gamma r) - gamma_j |, r = warm / exact.  diag: [0] fwd failures,
// [1] bwd failures, [2], [3] largest errors (double bit patterns).
__global__ __launch_bounds__(256) void bes_check(int S, int nblk, double tol, const double *__restrict__ rec,
                                                 unsigned long long *__restrict__ diag)
{
    __shared__ double red[8];
    const int c = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
    const double *ra = rec + (size_t)c * 6 * S, *rb = rec + (size_t)(c + 1) * 6 * S;
    const double *gam = dir == 0 ? ra + 2 * S : rb + 5 * S;
    const double *exact = dir == 0 ? ra + 1 * S : rb + 4 * S;
    const double *warm = dir == 0 ? rb + 0 * S : ra + 3 * S;
    double sw = 0.0;
    for (int j = tid; j < S; j += 256) {
        const double gm = gam[j];
        if (gm > 0.0) sw += gm * (warm[j] / exact[j]);
    }
    sw = wsum(sw);
    if ((tid & 63) == 0) red[tid >> 6] = sw;
    __syncthreads();
    sw = (red[0] + red[1]) + (red[2] + red[3]);
    double err = 0.0;
    for (int j = tid; j < S; j += 256) {
        const double gm = gam[j];
        if (gm > 0.0) err += fabs(gm * (warm[j] / exact[j]) / sw - gm);
    }
    err = wsum(err);
    if ((tid & 63) == 0) red[4 + (tid >> 6)] = err;
    __syncthreads();
    if (tid == 0) {
        err = (red[4] + red[5]) + (red[6] + red[7]);
        if (!(err <= tol)) atomicAdd(&diag[dir], 1ull);
        if (!(err == err)) err = INFINITY;
        atomicMax(&diag[2 + dir], (unsigned long long)__double_as_longlong(err));
    }
}

// stats = [G0 (S) | G1 (S) | X (nsrc1) | Gamma0 | sum y^2], summed over the blocks in block order
__global__ __launch_bounds__(64) void bes_reduce(int S, int nblk, int nsrc1, const double *__restrict__ partG,
                                                 const double *__restrict__ partX, double *__restrict__ stats)
{
    const int i = blockIdx.x, lane = threadIdx.x, n1 = 2 * S;
    double acc = 0.0;
    if (i < n1) for (int b = lane; b < nblk; b += 64) acc += partG[(size_t)b * n1 + i];
    else for (int b = lane; b < nblk; b += 64) acc += partX[(size_t)b * (nsrc1 + 2) + (i - n1)];
    acc = wsum(acc);
    if (lane == 0) stats[i] = acc;
}

// M-step finish from the statistics (baumwelch.jl:262-307): out = [mu (K x N) | sigma | xb[2:end] | pp]
__global__ __launch_bounds__(256) void bes_mstep(const int16_t *__restrict__ states, int N, int K, int S, int nsrc1,
                                                 const double *__restrict__ stats, const double *__restrict__ pp,
                                                 double *__restrict__ gg, double *__restrict__ mean_new,
                                                 double *__restrict__ out)
{
    __shared__ double red[12];
    const int tid = threadIdx.x, KN = K * N;
    const double *G0 = stats, *G1 = stats + S, *X = stats + 2 * S;
    double *mu = out;
    for (int i = tid; i < KN; i += 256) { mu[i] = 0.0; gg[i] = 0.0; }
    __syncthreads();
    if (tid == 0) {                                   // :266-287, states with exactly one active neuron
        for (int j = 0; j < S; j++) {
            int nact = 0;
            for (int l = 0; l < N; l++) nact += (states[l + N * j] >= 2);
            if (nact != 1) continue;
            for (int l = 0; l < N; l++) {
                const int ss = states[l + N * j];
                if (ss > 1) { mu[(ss - 1) + K * l] += G1[j]; gg[(ss - 1) + K * l] += G0[j]; }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < KN; i += 256)
        if (i % K != 0) mu[i] /= gg[i];
    __syncthreads();
    double x2 = 0.0, qq = 0.0;
    for (int j = tid; j < S; j += 256) {              // :288-305 with the NEW means
        double mj = 0.0;
        for (int l = 0; l < N; l++) mj += mu[(states[l + N * j] - 1) + K * l];
        mean_new[j] = mj;
        x2 += (mj * mj) * G0[j] - (2.0 * mj) * G1[j];
        qq += G0[j];
    }
    x2 = wsum(x2); qq = wsum(qq);
    if ((tid & 63) == 0) { red[tid >> 6] = x2; red[4 + (tid >> 6)] = qq; }
    __syncthreads();
    if (tid == 0) {
        const double X2 = ((red[0] + red[1]) + (red[2] + red[3])) + X[nsrc1 + 1];
        const double QQ = (red[4] + red[5]) + (red[6] + red[7]);
        out[KN] = sqrt(X2 / QQ);                      // :306-307
    }
    for (int i = 1 + tid; i < nsrc1; i += 256) out[KN + i] = log(X[i]) - log(X[nsrc1]);   // :264 xb[2:end]
    for (int j = tid; j < S; j += 256) out[KN + nsrc1 + j] = log(pp[j]);                  // :263
}

__global__ void bes_weights(const double *__restrict__ lp, int n, double *__restrict__ w)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[i] = exp(lp[i]);
}

}  // namespace

// two columns of S doubles + reduction scratch in LDS; 16 states per thread at 1024 threads
static bool lds_columns_fit(const GenericDev *g)
{
    return g->blocked && g->nsrc1 >= 1 && g->nsrc1 <= 256 && g->T >= 2 &&
           (2 * (size_t)g->S + 2 * 3 * kRedW + 4 * (size_t)g->nsrc1) * 8 <= 156 * 1024 && g->S <= 16 * 1024;
}

// option "blocked_hbm_columns" as the plan saw it when it was created: 1 sends a model the LDS test refuses to the
// device-memory-column kernels (generic_estep_big.hip), 2 every model
bool blocked_estep_big(const GenericDev *g)
{
    return g->blocked && g->nsrc1 >= 1 && g->nsrc1 <= 256 && g->T >= 2 &&
           (g->hbm_cols == 2 || (g->hbm_cols == 1 && !lds_columns_fit(g)));
}

void blocked_set_hbm_columns(GenericDev *g, int64_t v) { g->hbm_cols = (int)v; }

bool blocked_estep_supported(const GenericDev *g) { return lds_columns_fit(g) || blocked_estep_big(g); }

int64_t blocked_stats_len(const GenericDev *g) { return 2 * g->S + g->nsrc1 + 2; }

// LDS of the posterior instantiation: the E-step's plus 3 N + 3 reduction slots per parity.  The E-step's bound of
// 156 KB leaves 4 KB of the CU's 160 KB: enough for 4 templates (3 840 B more)
static size_t post_lds_bytes(const GenericDev *g)
{
    return (2 * (size_t)g->S + 2 * (size_t)(3 + 3 * g->N + 3) * kRedW + 4 * (size_t)g->nsrc1) * sizeof(double);
}

bool blocked_post_supported(const GenericDev *g)
{
    if (blocked_estep_big(g)) return g->N <= kPostMaxN;
    return blocked_estep_supported(g) && g->N <= kPostMaxN && post_lds_bytes(g) <= 160 * 1024;
}

// buffers every variant of the sweep needs, the weights and the cleared certificates; grid = resident workgroups
static int bes_prepare(GenericDev *g, int grid, bool post, hipStream_t st)
{
    const size_t S = (size_t)g->S, nb = (size_t)g->nblk;
    int rc;
    if ((rc = balloc(&g->d_es_win, (size_t)grid * g->B * S, &g->bytes)) ||
        (rc = balloc(&g->d_es_rec, nb * 6 * S, &g->bytes)) ||
        (rc = balloc(&g->d_es_partG, nb * 2 * S, &g->bytes)) ||
        (rc = balloc(&g->d_es_partX, nb * (g->nsrc1 + 2), &g->bytes)) ||
        (rc = balloc(&g->d_es_inw, (size_t)g->R, &g->bytes)) || (rc = balloc(&g->d_es_outw, (size_t)g->R, &g->bytes)) ||
        (rc = balloc(&g->d_es_diag, 4, &g->bytes)) || (rc = balloc(&g->d_es_tmp, 2 * S + g->K * g->N, &g->bytes)))
        return rc;
    if (post && ((rc = balloc(&g->d_es_lls, (size_t)grid * g->B, &g->bytes)) ||
                 (rc = balloc(&g->d_es_partL, nb + 1, &g->bytes))))
        return rc;
    g->es_grid = grid;
    hipLaunchKernelGGL(bes_weights, dim3((unsigned)((g->R + 255) / 256)), dim3(256), 0, st, g->d_in_lp, (int)g->R, g->d_es_inw);
    hipLaunchKernelGGL(bes_weights, dim3((unsigned)((g->R + 255) / 256)), dim3(256), 0, st, g->d_out_lp, (int)g->R, g->d_es_outw);
    HS_HIP(hipMemsetAsync(g->d_es_diag, 0, 4 * sizeof(unsigned long long), st));
    HS_HIP(hipMemsetAsync(g->d_es_rec, 0, nb * 6 * S * sizeof(double), st));
    return HMMSORT_OK;
}

// certificates of the sweep just launched and, for the E-step, the sum of the block statistics
static int bes_finish(GenericDev *g, double *d_stats, bool post, hipStream_t st)
{
    const size_t nb = (size_t)g->nblk;
    HS_HIP(hipGetLastError());
    if (nb > 1)
        hipLaunchKernelGGL(bes_check, dim3((unsigned)(nb - 1), 2), dim3(256), 0, st, (int)g->S, (int)nb, 1e-9, g->d_es_rec,
                           g->d_es_diag);
    if (!post)
        hipLaunchKernelGGL(bes_reduce, dim3((unsigned)blocked_stats_len(g)), dim3(64), 0, st, (int)g->S, (int)nb, g->nsrc1,
                           g->d_es_partG, g->d_es_partX, d_stats);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

// the E-step (pp == nullptr) or the posterior sweep over the same blocks
static int bes_run(GenericDev *g, const double *d_y, double *d_stats, BesPost *pp, hipStream_t st)
{
    HS_CHECK(g->hbm_cols != 0 || blocked_estep_supported(g), HMMSORT_EUNSUP,
             "blocked E-step: model too large for the LDS columns");
    HS_CHECK(blocked_estep_supported(g), HMMSORT_EUNSUP,
             "blocked E-step: not a blocked plan of at least 2 samples whose silent state has 1 to 256 transitions");
    int rc;
    if (blocked_estep_big(g)) {
        // columns in device memory (generic_estep_big.hip): its own grid, window, column scratch and block kernel.
        // BesPost is a type of this translation unit, so the outputs cross in a BigPost
        BigPost bp;
        if (pp) {
            for (int l = 0; l < kPostMaxN; l++) bp.qv[l] = pp->qv[l];
            bp.onset = pp->onset; bp.occ = pp->occ; bp.tq = pp->tq; bp.silent = pp->silent; bp.xm = pp->xm;
        }
        if ((rc = blocked_big_prepare(g)) || (rc = bes_prepare(g, g->es_grid, pp != nullptr, st)) ||
            (rc = blocked_big_launch(g, d_y, pp ? &bp : nullptr, st)))
            return rc;
        return bes_finish(g, d_stats, pp != nullptr, st);
    }
    const size_t S = (size_t)g->S, nb = (size_t)g->nblk;
    const int nt = g->S <= 256 ? 256 : (g->S <= 4096 ? 512 : 1024);
    const int spt = (int)((S + nt - 1) / nt);
    int dev = 0, ncu = 256;
    HS_HIP(hipGetDevice(&dev));
    HS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    const size_t lds = pp ? post_lds_bytes(g) : (2 * S + 2 * 3 * kRedW + 4 * (size_t)g->nsrc1) * sizeof(double);
    const int per_cu = lds <= 76 * 1024 && nt <= 512 ? 2 : 1;
    const int grid = (int)std::min<size_t>(nb, (size_t)ncu * per_cu);
    if ((rc = bes_prepare(g, grid, pp != nullptr, st))) return rc;
    BesArgs a;
    bes_fill_args(a, g, d_y);
    auto launch = [&](auto kern) -> int {
        if (lds > 64 * 1024)
            HS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, st, a);
        return HMMSORT_OK;
    };
    // register budget by launch bound: 1-2 states per thread fit 128 VGPRs (bound 1024: more waves per SIMD,
    // S = 900: 15.5 against 22 ms per 10^6 samples); 4-8 states per thread need the 256 of a 512-thread bound
    // (S = 3600: 54 against 96 ms)
    if (pp) {
        BesPost po = *pp;
        po.lls = g->d_es_lls; po.partL = g->d_es_partL;
        auto launch_post = [&](auto kern) -> int {
            if (lds > 64 * 1024)
                HS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, st, a, po);
            return HMMSORT_OK;
        };
        // the same thread counts and launch bounds as the E-step; partial sums for 2 or 4 templates
#define BES_LAUNCH_POST(NP)                                                                                              \
    (nt <= 512 ? (spt <= 1 ? launch_post(bes_block_post<1, 1024, NP>) : spt <= 2 ? launch_post(bes_block_post<2, 1024, NP>) \
                  : spt <= 4 ? launch_post(bes_block_post<4, 512, NP>) : launch_post(bes_block_post<8, 512, NP>))  \
               : (spt <= 8 ? launch_post(bes_block_post<8, 1024, NP>) : launch_post(bes_block_post<16, 1024, NP>)))
        rc = po.N <= 2 ? BES_LAUNCH_POST(2) : BES_LAUNCH_POST(4);
#undef BES_LAUNCH_POST
    } else if (nt <= 512) rc = spt <= 1 ? launch(bes_block<1, 1024>) : spt <= 2 ? launch(bes_block<2, 1024>)
                        : spt <= 4 ? launch(bes_block<4, 512>) : launch(bes_block<8, 512>);
    else rc = spt <= 8 ? launch(bes_block<8, 1024>) : launch(bes_block<16, 1024>);
    if (rc) return rc;
    return bes_finish(g, d_stats, pp != nullptr, st);
}

int blocked_estep(GenericDev *g, const double *d_y, double *d_stats, hipStream_t st)
{
    return bes_run(g, d_y, d_stats, nullptr, st);
}

int blocked_posteriors(GenericDev *g, const double *d_y, const int32_t *trough, double *d_onset, double *d_occ,
                       double *d_silent, double *d_tq, int16_t *d_xm, double *d_logz, hipStream_t st)
{
    HS_CHECK(blocked_estep_supported(g), HMMSORT_EUNSUP,
             "plan_posteriors: the blocked path holds two columns of S doubles in LDS (156 KB: %d states at most, this "
             "model has %lld); use the strict engine (option \"engine\" = HMMSORT_ENGINE_STRICT)",
             (int)((156 * 1024 / 8 - 2 * 3 * kRedW - 4 * g->nsrc1) / 2), (long long)g->S);
    HS_CHECK(!blocked_estep_big(g) || g->N <= kPostMaxN, HMMSORT_EUNSUP,
             "plan_posteriors: the blocked path takes up to %d templates (this model: %lld); use the strict engine",
             kPostMaxN, (long long)g->N);
    HS_CHECK(blocked_post_supported(g), HMMSORT_EUNSUP,
             "plan_posteriors: the blocked path takes up to %d templates within 160 KB of LDS (this model: %lld templates, "
             "%zu bytes); use the strict engine", kPostMaxN, (long long)g->N, post_lds_bytes(g));
    BesPost po;
    po.states = g->d_states;
    for (int l = 0; l < kPostMaxN; l++) po.qv[l] = l < g->N ? trough[l] : 0;
    po.N = (int)g->N; po.nred = 3 + 3 * (int)g->N + 3;
    po.onset = d_onset; po.occ = d_occ; po.tq = d_tq; po.silent = d_silent; po.xm = d_xm;
    po.lls = nullptr; po.partL = nullptr;
    int rc = bes_run(g, d_y, nullptr, &po, st);
    if (rc) return rc;
    if (d_logz) {
        hipLaunchKernelGGL(bes_logz, dim3(1), dim3(64), 0, st, (int)g->nblk, g->d_es_partL,
                           (double)g->T * (-kLog2Pi - g->lsig), d_logz);
        HS_HIP(hipGetLastError());
    }
    return HMMSORT_OK;
}

int blocked_mstep(GenericDev *g, const double *d_stats, double *d_out, hipStream_t st)
{
    HS_CHECK(g->d_es_rec, HMMSORT_EINVAL, "blocked M-step: no E-step has run on this plan");
    // pp = gamma[:,1] (:263): the first block's posterior on the first sample
    hipLaunchKernelGGL(bes_mstep, dim3(1), dim3(256), 0, st, g->d_states, (int)g->N, (int)g->K, (int)g->S, g->nsrc1,
                       d_stats, g->d_es_rec + 5 * (size_t)g->S, g->d_es_tmp + 2 * g->S, g->d_es_tmp, d_out);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int blocked_estep_diagnostics(GenericDev *g, hipStream_t st, int64_t diag[8])
{
    if (!g->d_es_diag) return HMMSORT_OK;
    unsigned long long h[4];
    HS_HIP(hipMemcpyAsync(h, g->d_es_diag, sizeof(h), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    diag[3] = (int64_t)h[0];
    diag[5] = (int64_t)h[1];
    diag[4] = (int64_t)h[2];
    diag[6] = (int64_t)h[3];
    return HMMSORT_OK;
}

void blocked_estep_destroy(GenericDev *g)
{
    void *ptrs[] = {g->d_es_win, g->d_es_rec, g->d_es_partG, g->d_es_partX, g->d_es_inw, g->d_es_outw,
                    g->d_es_diag, g->d_es_tmp, g->d_es_lls, g->d_es_partL, g->d_es_cols, g->d_es_srec};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
}

}  // namespace hmmsort
