// The stitch rule of the reference's chunked decode (fit.jl:24-36) on a decoded chunk in device memory
// (hmmsort_chunk_stitch, include/hmmsort.h): where the chunk's leading non-silent run ends (l), where its last
// silent sample is (kk), and the copy of x[l..kk] into the recording's path.  Three launches on the caller's stream
// with no host round trip between them: the trim points live in d_lk, the copy reads them from there, and the host
// reads the same two integers when it next waits for the stream.  Plain loads, stores and 64-bit atomics.
// k_chunk_ll gives a decoded chunk the reference's own log-likelihood, rounded as the reference rounds it.
#include <algorithm>
#include <cmath>

#include "hmmsort_internal.h"

namespace hmmsort {
namespace {

constexpr int kStitchThreads = 256;
constexpr int kStitchMaxBlocks = 2048;

// grid-stride blocks for n elements; n >= 1
inline int stitch_blocks(int64_t n)
{
    return (int)std::min<int64_t>((n + kStitchThreads - 1) / kStitchThreads, kStitchMaxBlocks);
}

// what the reductions start from: "no silent sample" (l = k + 1, kk = 0), or the fixed ends of a chunk that
// begins / ends the recording
__global__ void k_stitch_init(int64_t k, int lead, int trail, long long *__restrict__ lk)
{
    lk[0] = lead ? (long long)k + 1 : 1;
    lk[1] = trail ? 0 : (long long)k;
}

// first and last silent sample (1-based) of x[0..k): lk[0] = min, lk[1] = max over the samples with x <= 1.
// Every sample is looked at, so a run of any length is found; one atomic pair per workgroup that saw a silent one.
__global__ __launch_bounds__(kStitchThreads) void k_stitch_scan(const int16_t *__restrict__ x, int64_t k, int lead,
                                                                int trail, long long *__restrict__ lk)
{
    __shared__ long long s_lo[kStitchThreads / 64], s_hi[kStitchThreads / 64];
    long long lo = (long long)k + 1, hi = 0;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < k; t += step)
        if (!(x[t] > 1)) {
            lo = lo < t + 1 ? lo : t + 1;
            hi = t + 1;   // t ascends within a thread
        }
    for (int d = 32; d > 0; d >>= 1) {
        const long long olo = __shfl_down(lo, d, 64), ohi = __shfl_down(hi, d, 64);
        lo = olo < lo ? olo : lo;
        hi = ohi > hi ? ohi : hi;
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[wave] = lo;
        s_hi[wave] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStitchThreads / 64; w++) {
            lo = s_lo[w] < lo ? s_lo[w] : lo;
            hi = s_hi[w] > hi ? s_hi[w] : hi;
        }
        if (hi > 0) {   // the workgroup saw a silent sample
            if (lead) atomicMin(&lk[0], lo);
            if (trail) atomicMax(&lk[1], hi);
        }
    }
}

// dst[l-1 .. kk-1] = x[l-1 .. kk-1] with l, kk read from device memory; nothing when l > kk.  1 <= l and kk <= k
// by construction (k_stitch_init / k_stitch_scan), so no index leaves [0, k).
__global__ __launch_bounds__(kStitchThreads) void k_stitch_copy(const int16_t *__restrict__ x, int64_t k,
                                                                const long long *__restrict__ lk,
                                                                int16_t *__restrict__ dst)
{
    const int64_t lo = lk[0] - 1;
    int64_t hi = lk[1];
    hi = hi < k ? hi : k;
    if (lo < 0) return;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < hi; t += step) dst[t] = x[t];
}

__global__ void k_fill_i16(int16_t *__restrict__ p, int64_t n, int16_t v)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += step) p[t] = v;
}

// The chunk's ll exactly as viterbi.jl:92-96 rounds it: the values T1[x_t, t] along the decoded path, accumulated
// forward in the reference's operation order ((T1 + lp) + q, as gen_viterbi_ll does), then summed from the last
// sample down to the second.  Both folds are serial by definition -- any other grouping of the additions differs
// in the last bits, and the chunk sum of fit.jl:37 is compared with == -- so one workgroup walks the chunk in
// tiles: all threads look up lp(x_{t-1} -> x_t) and the emission term of a tile into LDS, thread 0 folds the tile,
// all threads store the tile's path values to pv.  The second pass reads pv back tile by tile from the end.
// Thread 0 folds in batches of kLlBatch held in registers, the next batch loaded while the current one is added, so
// the chain of dependent additions is what the fold waits for, not LDS.  A tile is padded to whole batches with
// +0.0 terms, which change no sum.
// A state outside 1..S (no engine writes one) reads as the silent state's mean and a missing transition.
constexpr int kLlThreads = 256;
constexpr int kLlTile = 2048;
constexpr int kLlBatch = 16;   // divides kLlTile

__global__ __launch_bounds__(kLlThreads) void k_chunk_ll(const double *__restrict__ y, const int16_t *__restrict__ x,
                                                         int64_t k, int S, const double *__restrict__ mean,
                                                         const int32_t *__restrict__ in_ptr,
                                                         const int32_t *__restrict__ in_src,
                                                         const double *__restrict__ in_lp, double c0, double den,
                                                         double *pv, double *__restrict__ ll_out)
{
    __shared__ double s_lp[kLlTile], s_q[kLlTile];
    __shared__ double s_acc;
    const int tid = threadIdx.x;
    auto state = [&](int64_t t) {
        const int s = (int)x[t] - 1;
        return (s >= 0 && s < S) ? s : -1;
    };
    if (tid == 0) {
        const int s0 = state(0);
        double p = 0.0;   // T1[1,1] = 0 for the silent state (viterbi.jl:63)
        if (s0 > 0) {
            const double dd = y[0] - mean[s0];
            p = c0 - (dd * dd) / den;
        }
        pv[0] = p;
        s_acc = p;
    }
    for (int64_t t0 = 1; t0 < k; t0 += kLlTile) {
        const int n = (int)(k - t0 < kLlTile ? k - t0 : kLlTile);
        __syncthreads();
        for (int u = tid; u < n; u += kLlThreads) {
            const int xp = state(t0 + u - 1), xc = state(t0 + u);
            double lp = -INFINITY;
            if (xp >= 0 && xc >= 0) {
                const int e1 = in_ptr[xc + 1];
                for (int e = in_ptr[xc]; e < e1; e++)
                    if (in_src[e] == xp) { lp = in_lp[e]; break; }
            }
            const double dd = y[t0 + u] - mean[xc >= 0 ? xc : 0];
            s_lp[u] = lp;
            s_q[u] = c0 - (dd * dd) / den;
        }
        const int npad = (n + kLlBatch - 1) / kLlBatch * kLlBatch;
        for (int u = n + tid; u < npad; u += kLlThreads) s_lp[u] = 0.0, s_q[u] = 0.0;
        __syncthreads();
        if (tid == 0) {
            double p = s_acc;
            double a[kLlBatch], b[kLlBatch], an[kLlBatch], bn[kLlBatch];
#pragma unroll
            for (int j = 0; j < kLlBatch; j++) a[j] = s_lp[j], b[j] = s_q[j];
            for (int u0 = 0; u0 < npad; u0 += kLlBatch) {
                const int nx = u0 + kLlBatch < npad ? u0 + kLlBatch : u0;   // the last batch reloads itself
#pragma unroll
                for (int j = 0; j < kLlBatch; j++) an[j] = s_lp[nx + j], bn[j] = s_q[nx + j];
#pragma unroll
                for (int j = 0; j < kLlBatch; j++) {
                    p = (p + a[j]) + b[j];
                    b[j] = p;
                }
#pragma unroll
                for (int j = 0; j < kLlBatch; j++) s_q[u0 + j] = b[j], a[j] = an[j], b[j] = bn[j];
            }
            s_acc = p;
        }
        __syncthreads();
        for (int u = tid; u < n; u += kLlThreads) pv[t0 + u] = s_q[u];
    }
    __syncthreads();
    if (tid == 0) s_acc = 0.0;
    for (int64_t hi = k; hi > 1; hi -= kLlTile) {   // samples [lo, hi), from the end; sample 0 is not summed
        const int64_t lo = hi - kLlTile > 1 ? hi - kLlTile : 1;
        const int n = (int)(hi - lo);
        __syncthreads();
        const int npad = (n + kLlBatch - 1) / kLlBatch * kLlBatch;
        for (int u = tid; u < npad; u += kLlThreads) s_q[u] = u < n ? pv[lo + u] : 0.0;
        __syncthreads();
        if (tid == 0) {
            double ll = s_acc;
            double b[kLlBatch], bn[kLlBatch];
#pragma unroll
            for (int j = 0; j < kLlBatch; j++) b[j] = s_q[npad - kLlBatch + j];
            for (int u0 = npad - kLlBatch; u0 >= 0; u0 -= kLlBatch) {
                const int nx = u0 >= kLlBatch ? u0 - kLlBatch : u0;
#pragma unroll
                for (int j = 0; j < kLlBatch; j++) bn[j] = s_q[nx + j];
#pragma unroll
                for (int j = kLlBatch - 1; j >= 0; j--) ll += b[j];
#pragma unroll
                for (int j = 0; j < kLlBatch; j++) b[j] = bn[j];
            }
            s_acc = ll;
        }
    }
    __syncthreads();
    if (tid == 0) *ll_out = s_acc;
}

}  // namespace

int dev_chunk_ll(const double *d_y, const int16_t *d_x, int64_t k, int64_t S, const double *d_mean,
                 const int32_t *d_in_ptr, const int32_t *d_in_src, const double *d_in_lp, double sigma, double *d_pv,
                 double *d_ll, hipStream_t st)
{
    if (k < 1) return HMMSORT_OK;
    const double c0 = -kLog2Pi - std::log(sigma), den = 2.0 * (sigma * sigma);   // funcl, as the strict engine hoists it
    hipLaunchKernelGGL(k_chunk_ll, dim3(1), dim3(kLlThreads), 0, st, d_y, d_x, k, (int)S, d_mean, d_in_ptr, d_in_src,
                       d_in_lp, c0, den, d_pv, d_ll);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int dev_fill_i16(int16_t *d_p, int64_t n, int16_t v, hipStream_t st)
{
    if (n <= 0) return HMMSORT_OK;
    hipLaunchKernelGGL(k_fill_i16, dim3(stitch_blocks(n)), dim3(kStitchThreads), 0, st, d_p, n, v);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int dev_chunk_stitch(const int16_t *d_x, int64_t k, bool lead, bool trail, int16_t *d_dst, int64_t *d_lk,
                     hipStream_t st)
{
    long long *lk = reinterpret_cast<long long *>(d_lk);
    const int blocks = stitch_blocks(k);
    hipLaunchKernelGGL(k_stitch_init, dim3(1), dim3(1), 0, st, k, (int)lead, (int)trail, lk);
    if (lead || trail)
        hipLaunchKernelGGL(k_stitch_scan, dim3(blocks), dim3(kStitchThreads), 0, st, d_x, k, (int)lead, (int)trail, lk);
    hipLaunchKernelGGL(k_stitch_copy, dim3(blocks), dim3(kStitchThreads), 0, st, d_x, k, lk, d_dst);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

}  // namespace hmmsort

extern "C" int hmmsort_chunk_stitch(const int16_t *d_x, int64_t k, int lead, int trail, int16_t *d_dst,
                                    int64_t *d_lk, void *stream)
{
    using namespace hmmsort;
    HS_CHECK(d_x && d_dst && d_lk, HMMSORT_EINVAL, "chunk_stitch: null argument");
    HS_CHECK(k >= 1 && k <= 2147483647LL, HMMSORT_EINVAL, "chunk_stitch: chunk length %lld outside 1 .. 2^31 - 1",
             (long long)k);
    int rc = need_device();
    if (rc) return rc;
    return dev_chunk_stitch(d_x, k, lead != 0, trail != 0, d_dst, d_lk, (hipStream_t)stream);
}
