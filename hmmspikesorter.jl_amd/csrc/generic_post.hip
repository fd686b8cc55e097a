// Smoothed state posteriors of an ARBITRARY transition list from the strict engine's materialised alpha/beta
// (reference src/baumwelch.jl:25-51, :73-98): gamma_t(s) = exp(alpha_t(s) + beta_t(s) - z_t), z_t = logsumexp_s
// (alpha_t(s) + beta_t(s)) -- every column normalised by its own sum, as the reference's update does
// (baumwelch.jl:216-224).  z_t equals z = logsumexp_s alpha_{T-1}(s) (the logz output) in exact arithmetic, but the
// unscaled log alpha/beta have magnitude O(t) and their rounding reaches 1e-7 of z at 200 000 samples: dividing by
// the one global z put that error into every probability.  Reduced per sample over the state table into the
// outputs of hmmsort_plan_posteriors.  Serves
// the models the wave engine does not take (overlap models) and is the second, independent implementation the
// wave path is checked against.  Slow by design: it reads S x T doubles twice.
#include <cmath>

#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

__device__ __forceinline__ double pw_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void kg_post_logz(const double *__restrict__ alpha, int64_t T, int S,
                                                    double *__restrict__ logz)
{
    __shared__ double red[4];
    const double *a = alpha + (int64_t)S * (T - 1);
    double m = -INFINITY;
    for (int j = threadIdx.x; j < S; j += 256) m = fmax(m, a[j]);
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    double s = 0.0;
    for (int j = threadIdx.x; j < S; j += 256) s += exp(a[j] - m);
    s = pw_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) logz[0] = m + log((red[0] + red[1]) + (red[2] + red[3]));
}

constexpr int kPostMaxN = 16;

// one wavefront per sample; states: N x S (1-based phases, 1 = silent), qv[a] = trough phase of template a
__global__ __launch_bounds__(64) void kg_post(const double *__restrict__ alpha, const double *__restrict__ beta,
                                              int64_t T, int S, int N, const int16_t *__restrict__ states,
                                              const int32_t *__restrict__ qv, double *__restrict__ onset,
                                              double *__restrict__ occ, double *__restrict__ silent,
                                              double *__restrict__ tq, int16_t *__restrict__ xm)
{
    const int lane = threadIdx.x;
    int q[kPostMaxN];
#pragma unroll
    for (int a = 0; a < kPostMaxN; a++) q[a] = a < N ? qv[a] : 0;
    for (int64_t t = blockIdx.x; t < T; t += gridDim.x) {
        const double *al = alpha + (int64_t)S * t, *be = beta + (int64_t)S * t;
        double on[kPostMaxN], oc[kPostMaxN], tr[kPostMaxN];
#pragma unroll
        for (int a = 0; a < kPostMaxN; a++) { on[a] = 0.0; oc[a] = 0.0; tr[a] = 0.0; }
        double m = -INFINITY, sum = 0.0;
        for (int s = lane; s < S; s += 64) m = fmax(m, al[s] + be[s]);
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
        for (int s = lane; s < S; s += 64) {
            const double v = al[s] + be[s];
            // a state the reference's logsumexpl(-Inf, -Inf) left NaN stays out of the normaliser only: below, its
            // NaN still goes into the marginals of the templates that own it, as it did with the global z
            if (v == v) sum += exp(v - m);
        }
        const double z = m + log(pw_sum(sum));
        double bv = -1.0;
        int bs = 0;
        for (int s = lane; s < S; s += 64) {
            const double gm = exp((al[s] + be[s]) - z);
            if (gm > bv) { bv = gm; bs = s; }               // s rises: the lower state number keeps a tie
#pragma unroll
            for (int a = 0; a < kPostMaxN; a++)
                if (a < N) {
                    const int v = states[a + (int64_t)N * s];
                    on[a] += v == 2 ? gm : 0.0;
                    oc[a] += v > 1 ? gm : 0.0;
                    tr[a] += v == q[a] ? gm : 0.0;
                }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int os = __shfl_xor(bs, o);
            if (ov > bv || (ov == bv && os < bs)) { bv = ov; bs = os; }
        }
#pragma unroll
        for (int a = 0; a < kPostMaxN; a++)
            if (a < N) {
                const double v1 = pw_sum(on[a]), v2 = pw_sum(oc[a]), v3 = pw_sum(tr[a]);
                if (lane == 0) {
                    onset[(int64_t)a * T + t] = v1;
                    occ[(int64_t)a * T + t] = v2;
                    tq[(int64_t)a * T + t] = v3;
                }
            }
        if (lane == 0) {
            silent[t] = exp((al[0] + be[0]) - z);
            xm[t] = (int16_t)(bs + 1);
        }
    }
}

}  // namespace

int generic_posteriors(const double *d_alpha, const double *d_beta, int64_t T, int64_t S, int64_t N,
                       const int16_t *d_states, const int32_t *d_qv, double *d_logz, double *d_onset,
                       double *d_occ, double *d_silent, double *d_tq, int16_t *d_xm, hipStream_t st)
{
    HS_CHECK(N <= kPostMaxN, HMMSORT_EUNSUP, "posteriors (strict path): more than %d templates", kPostMaxN);
    hipLaunchKernelGGL(kg_post_logz, dim3(1), dim3(256), 0, st, d_alpha, T, (int)S, d_logz);
    const unsigned nb = (unsigned)(T < 65536 ? T : 65536);
    hipLaunchKernelGGL(kg_post, dim3(nb), dim3(64), 0, st, d_alpha, d_beta, T, (int)S, (int)N, d_states, d_qv,
                       d_onset, d_occ, d_silent, d_tq, d_xm);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

}  // namespace hmmsort
