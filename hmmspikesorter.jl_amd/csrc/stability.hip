// Unit stability over time (hmmsort_unit_stability and its device and plan forms, include/hmmsort.h):
// per unit and time bin the spike count, and of one fp64 value per spike the number of valid (non-NaN) values, exact
// order statistics, the sum and the sum of squares; the same per unit over the whole recording, and a histogram of
// the values per unit.  Every result is a fixed function of the input: counts are differences of searched boundaries,
// order statistics are inputs selected by integer keys, sums run in one stated order without fused multiply-add, and
// the only atomics are integer ones.  The numpy model tests/stability_model.py states the same rules.
//
// The U lists sit concatenated in device memory behind U + 1 host offsets (times and values alike).
//   k_stab_bounds    one thread per (unit, boundary): the first entry of the unit's list at or after b bin + 1, by binary
//                    search; segment (u, b) is the range between two neighbouring boundaries.
//   k_stab_tcount, k_stab_scan, k_stab_compact
//                    the values mapped to order-preserving 64-bit keys with the NaNs set aside, in the same order:
//                    valid counts per tile of 256 entries, one exclusive scan of them by one workgroup, then every tile
//                    writes its keys and, per entry, the number of valid entries before it (d_pre), so that a boundary
//                    in the list is a boundary in the keys (k_stab_gather).
// The host reads both boundary tables (they are the count and valid outputs), and from them lists the work: a job per
// non-empty segment and per unit, and the tiles of 256 keys of every non-empty segment.
//   k_stab_sel_wave  jobs of at most 64 keys, one wave each and four per workgroup: a lane holds a key, counts the keys
//                    that sort before it (equal keys by position) and the lane whose count is a wanted rank writes it.
//   k_stab_sel_block longer jobs, one workgroup each: most-significant-digit radix select with the 11-bit digits and
//                    kSelBins counters of radix_select.hip, up to kStabGroup ranks per sweep with a prefix and an LDS
//                    histogram each.  A job of at most kStabLdsKeys keys is read from memory once and swept in LDS; a
//                    longer one (a unit's whole recording) re-reads its range in every sweep.
//   k_stab_tile_sums one thread per tile of 256 keys: the serial fold from +0.0, the square rounded on its own.
//   k_stab_seg_fold  one thread per non-empty segment folds its tile partials in tile order; k_stab_unit_fold one thread
//                    per unit folds the bin sums in bin order.
//   k_stab_hist      grid (blocks, unit): 32-bit LDS counters, one 64-bit integer atomic per non-zero bin and block.
#include <algorithm>
#include <cmath>

#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

constexpr int kStabThreads = 256;
constexpr int kStabTile = 256;          // valid values of one sum tile; entries of one compaction tile
constexpr int kStabWaveKeys = 64;       // the longest job one wave serves
constexpr int kStabLdsKeys = 2048;      // the longest job that is swept in LDS: 16 KB of keys
constexpr int kStabGroup = 4;           // ranks of one sweep: 4 x 8 KB of counters
constexpr int kStabMaxRanks = HMMSORT_STAB_MAX_Q + 2;   // a unit's quantiles, minimum and maximum
constexpr int kStabPasses = 6;          // 5 x 11 bits + 9 bits = 64
constexpr int kStabHistBlocks = 64;
constexpr unsigned long long kSign = 0x8000000000000000ULL;

// -Inf < ... < -0.0 < +0.0 < ... < +Inf as unsigned integers, and back
__device__ __forceinline__ unsigned long long stab_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double stab_val(unsigned long long k)
{
    return __longlong_as_double((long long)((k & kSign) ? (k ^ kSign) : ~k));
}

// first index in [lo, hi) whose entry is >= key (hi when none)
__device__ __forceinline__ int64_t stab_lower_bound(const int64_t *__restrict__ a, int64_t lo, int64_t hi, int64_t key)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// bnd[u (B + 1) + b]: position in the concatenated lists of unit u's first time in bin b or later; b == B: its end
__global__ __launch_bounds__(kStabThreads) void k_stab_bounds(const int64_t *__restrict__ t,
                                                              const int64_t *__restrict__ off, int64_t U, int64_t B,
                                                              int64_t bin, int64_t *__restrict__ bnd)
{
    const int64_t i = (int64_t)blockIdx.x * kStabThreads + threadIdx.x;
    if (i >= U * (B + 1)) return;
    const int64_t u = i / (B + 1), b = i - u * (B + 1);
    const int64_t lo = off[u], hi = off[u + 1];
    bnd[i] = b == B ? hi : stab_lower_bound(t, lo, hi, b * bin + 1);
}

// this thread's entry of tile blockIdx.x of v[0 .. n): is it a value, and how many of the tile's earlier entries are;
// *total: the tile's count
__device__ __forceinline__ int stab_tile_prefix(bool valid, int *s_w, int *total)
{
    const unsigned long long bm = __ballot(valid);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_w[w] = __popcll(bm);
    __syncthreads();
    int before = __popcll(bm & ((1ULL << lane) - 1ULL));
    for (int q = 0; q < w; q++) before += s_w[q];
    *total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return before;
}

__global__ __launch_bounds__(kStabThreads) void k_stab_tcount(const double *__restrict__ v, int64_t n,
                                                              int64_t *__restrict__ tcnt)
{
    __shared__ int s_w[4];
    const int64_t i = (int64_t)blockIdx.x * kStabTile + threadIdx.x;
    const double x = i < n ? v[i] : 0.0;
    int total;
    (void)stab_tile_prefix(i < n && x == x, s_w, &total);
    if (threadIdx.x == 0) tcnt[blockIdx.x] = total;
}

// tbase[0 .. ntile]: exclusive prefix sums of tcnt; one workgroup
__global__ __launch_bounds__(kStabThreads) void k_stab_scan(const int64_t *__restrict__ tcnt, int64_t ntile,
                                                            int64_t *__restrict__ tbase)
{
    __shared__ int64_t s[kStabThreads];
    const int tid = threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < ntile; base += kStabThreads) {
        const int64_t i = base + tid;
        const int64_t x = i < ntile ? tcnt[i] : 0;
        s[tid] = x;
        __syncthreads();
        for (int d = 1; d < kStabThreads; d <<= 1) {
            const int64_t y = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += y;
            __syncthreads();
        }
        if (i < ntile) tbase[i] = carry + s[tid] - x;
        carry += s[kStabThreads - 1];
        __syncthreads();
    }
    if (tid == 0) tbase[ntile] = carry;
}

// keys of the values in their order, pre[i] = values among v[0 .. i), pre[n] = all of them
__global__ __launch_bounds__(kStabThreads) void k_stab_compact(const double *__restrict__ v, int64_t n, int64_t ntile,
                                                               const int64_t *__restrict__ tbase,
                                                               unsigned long long *__restrict__ kv,
                                                               int64_t *__restrict__ pre)
{
    __shared__ int s_w[4];
    const int64_t i = (int64_t)blockIdx.x * kStabTile + threadIdx.x;
    const double x = i < n ? v[i] : 0.0;
    const bool valid = i < n && x == x;
    int total;
    const int64_t at = tbase[blockIdx.x] + stab_tile_prefix(valid, s_w, &total);
    if (i < n) pre[i] = at;
    if (valid) kv[at] = stab_key(x);
    if (blockIdx.x == 0 && threadIdx.x == 0) pre[n] = tbase[ntile];
}

// vb[i] = pre[bnd[i] - o0]: the boundary in the keys
__global__ __launch_bounds__(kStabThreads) void k_stab_gather(const int64_t *__restrict__ bnd, int64_t nb, int64_t o0,
                                                              const int64_t *__restrict__ pre, int64_t *__restrict__ vb)
{
    const int64_t i = (int64_t)blockIdx.x * kStabThreads + threadIdx.x;
    if (i < nb) vb[i] = pre[bnd[i] - o0];
}

__global__ __launch_bounds__(kStabThreads) void k_stab_fill(double *__restrict__ p, int64_t n, double x)
{
    const int64_t i = (int64_t)blockIdx.x * kStabThreads + threadIdx.x;
    if (i < n) p[i] = x;
}

// ---- exact select of R ranks per job ---------------------------------------------------------------------------------

struct StabSel {
    const unsigned long long *kv;
    const int64_t *jstart, *jm, *jout;   // [njobs] first key, keys (>= 1), row of `out`
    int64_t njobs;
    int R;                               // ranks per job: rank r of m keys is num[r] (m - 1) / den
    long long den, num[kStabMaxRanks];
    double *out;                         // rows of R
};

__global__ __launch_bounds__(kStabThreads) void k_stab_sel_wave(const StabSel A)
{
    const int lane = threadIdx.x & 63;
    const int64_t job = (int64_t)blockIdx.x * (kStabThreads / 64) + (threadIdx.x >> 6);
    if (job >= A.njobs) return;   // the whole wave
    const int m = (int)A.jm[job];
    const unsigned long long k = lane < m ? A.kv[A.jstart[job] + lane] : 0ULL;
    int before = 0;
    for (int j = 0; j < m; j++) {
        const unsigned long long kj = __shfl(k, j);
        before += (kj < k || (kj == k && j < lane)) ? 1 : 0;
    }
    double *out = A.out + A.jout[job] * A.R;
    for (int r = 0; r < A.R; r++) {
        const long long rank = A.num[r] * (long long)(m - 1) / A.den;
        if (lane < m && before == rank) out[r] = stab_val(k);
    }
}

__global__ __launch_bounds__(kStabThreads) void k_stab_sel_block(const StabSel A)
{
    constexpr int kPer = kSelBins / kStabThreads;
    __shared__ unsigned long long s_key[kStabLdsKeys];
    __shared__ unsigned int s_h[kStabGroup][kSelBins];
    __shared__ unsigned int s_part[kStabGroup][kStabThreads];
    __shared__ unsigned long long s_prefix[kStabGroup];
    __shared__ long long s_rank[kStabGroup];
    const int tid = threadIdx.x;
    const int64_t job = blockIdx.x, m = A.jm[job];
    const unsigned long long *__restrict__ src = A.kv + A.jstart[job];
    const bool fits = m <= kStabLdsKeys;
    if (fits)
        for (int64_t i = tid; i < m; i += kStabThreads) s_key[i] = src[i];
    for (int g0 = 0; g0 < A.R; g0 += kStabGroup) {
        const int G = A.R - g0 < kStabGroup ? A.R - g0 : kStabGroup;
        if (tid < G) {
            s_prefix[tid] = 0ULL;
            s_rank[tid] = A.num[g0 + tid] * (long long)(m - 1) / A.den;
        }
        for (int p = 0; p < kStabPasses; p++) {
            const int shift = 64 - 11 * (p + 1) > 0 ? 64 - 11 * (p + 1) : 0;
            const int bits = p + 1 < kStabPasses ? 11 : 64 - 11 * (kStabPasses - 1);
            const int hs = shift + bits;   // 64 in the first pass: no higher bits, and no shift by 64
            const unsigned int mask = (1u << bits) - 1u;
            for (int i = tid; i < G * kSelBins; i += kStabThreads) (&s_h[0][0])[i] = 0u;
            __syncthreads();   // also: s_key, s_prefix and s_rank are written
            for (int64_t i = tid; i < m; i += kStabThreads) {
                const unsigned long long k = fits ? s_key[i] : src[i];
                const unsigned int d = (unsigned int)(k >> shift) & mask;
                for (int g = 0; g < G; g++)
                    if (p == 0 || (k >> hs) == (s_prefix[g] >> hs)) atomicAdd(&s_h[g][d], 1u);
            }
            __syncthreads();
            for (int g = 0; g < G; g++) {
                unsigned int sum = 0;
                for (int q = 0; q < kPer; q++) sum += s_h[g][tid * kPer + q];
                s_part[g][tid] = sum;
            }
            __syncthreads();
            if (tid < G) {   // the digit that holds the rank; the rank becomes the rank within it
                unsigned long long r = (unsigned long long)s_rank[tid];
                int w = 0;
                while (w < kStabThreads - 1 && r >= s_part[tid][w]) r -= s_part[tid][w++];
                int b = w * kPer;
                while (b < w * kPer + kPer - 1 && r >= s_h[tid][b]) r -= s_h[tid][b++];
                s_prefix[tid] |= (unsigned long long)b << shift;
                s_rank[tid] = (long long)r;
            }
            __syncthreads();
        }
        if (tid < G) A.out[A.jout[job] * A.R + g0 + tid] = stab_val(s_prefix[tid]);
        __syncthreads();
    }
}

// ---- sums ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kStabThreads) void k_stab_tile_sums(const unsigned long long *__restrict__ kv,
                                                                 const int64_t *__restrict__ tstart,
                                                                 const int32_t *__restrict__ tlen, int64_t nt,
                                                                 double *__restrict__ ps, double *__restrict__ pq)
{
    const int64_t i = (int64_t)blockIdx.x * kStabThreads + threadIdx.x;
    if (i >= nt) return;
    const unsigned long long *__restrict__ k = kv + tstart[i];
    const int n = tlen[i];
    double s = 0.0, q = 0.0;
    for (int j = 0; j < n; j++) {
        const double v = stab_val(k[j]);
        s = __dadd_rn(s, v);
        q = __dadd_rn(q, __dmul_rn(v, v));
    }
    ps[i] = s, pq[i] = q;
}

// segment j (row jout[j] of the outputs) owns the tile partials tfirst[j] .. tfirst[j + 1]
__global__ __launch_bounds__(kStabThreads) void k_stab_seg_fold(const double *__restrict__ ps,
                                                                const double *__restrict__ pq,
                                                                const int64_t *__restrict__ tfirst,
                                                                const int64_t *__restrict__ jout, int64_t nseg,
                                                                double *__restrict__ sum, double *__restrict__ sumsq)
{
    const int64_t j = (int64_t)blockIdx.x * kStabThreads + threadIdx.x;
    if (j >= nseg) return;
    double s = 0.0, q = 0.0;
    for (int64_t k = tfirst[j]; k < tfirst[j + 1]; k++) {
        s = __dadd_rn(s, ps[k]);
        q = __dadd_rn(q, pq[k]);
    }
    sum[jout[j]] = s, sumsq[jout[j]] = q;
}

__global__ __launch_bounds__(kStabThreads) void k_stab_unit_fold(const double *__restrict__ sum,
                                                                 const double *__restrict__ sumsq, int64_t U, int64_t B,
                                                                 double *__restrict__ usum, double *__restrict__ usumsq)
{
    const int64_t u = (int64_t)blockIdx.x * kStabThreads + threadIdx.x;
    if (u >= U) return;
    double s = 0.0, q = 0.0;
    for (int64_t b = 0; b < B; b++) {
        s = __dadd_rn(s, sum[u * B + b]);
        q = __dadd_rn(q, sumsq[u * B + b]);
    }
    usum[u] = s, usumsq[u] = q;
}

// ---- histogram -----------------------------------------------------------------------------------------------------

// counters [HB | under | over] of unit blockIdx.y, over its keys vb[u (B + 1)] .. vb[u (B + 1) + B]
__global__ __launch_bounds__(kStabThreads) void k_stab_hist(const unsigned long long *__restrict__ kv,
                                                            const int64_t *__restrict__ vb, int64_t B, int HB, double lo,
                                                            double scale, unsigned long long *__restrict__ hist,
                                                            unsigned long long *__restrict__ under,
                                                            unsigned long long *__restrict__ over)
{
    __shared__ unsigned int s_h[HMMSORT_STAB_MAX_HIST + 2];
    const int u = blockIdx.y;
    const int64_t first = vb[(int64_t)u * (B + 1)], end = vb[(int64_t)u * (B + 1) + B];
    for (int k = threadIdx.x; k < HB + 2; k += kStabThreads) s_h[k] = 0u;
    __syncthreads();
    const double top = (double)HB;
    for (int64_t i = first + (int64_t)blockIdx.x * kStabThreads + threadIdx.x; i < end;
         i += (int64_t)gridDim.x * kStabThreads) {
        const double p = __dmul_rn(__dsub_rn(stab_val(kv[i]), lo), scale);   // never NaN: lo is finite, scale > 0
        const int k = p < 0.0 ? HB : (p >= top ? HB + 1 : (int)p);
        atomicAdd(&s_h[k], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < HB + 2; k += kStabThreads) {
        const unsigned int h = s_h[k];
        if (!h) continue;
        unsigned long long *dst = k < HB ? &hist[(int64_t)u * HB + k] : (k == HB ? &under[u] : &over[u]);
        atomicAdd(dst, (unsigned long long)h);
    }
}

inline unsigned stab_blocks(int64_t n) { return (unsigned)((n + kStabThreads - 1) / kStabThreads); }

}  // namespace

int stab_check(const char *who, int64_t U, const hmmsort_stab_opt *opt, const hmmsort_stab_out *out, int64_t *B_out)
{
    HS_CHECK(opt && out && out->n, HMMSORT_EINVAL, "%s: null argument (the options, the output record and its n are "
             "required)", who);
    HS_CHECK(U >= 1 && U <= HMMSORT_STAB_MAX_UNITS, HMMSORT_EINVAL, "%s: U = %lld units (1..%d)", who, (long long)U,
             HMMSORT_STAB_MAX_UNITS);
    HS_CHECK(opt->T >= 1 && opt->T <= (1ll << 40), HMMSORT_EINVAL, "%s: T = %lld (1..2^40)", who, (long long)opt->T);
    HS_CHECK(opt->bin >= 1, HMMSORT_EINVAL, "%s: bin = %lld (at least 1 sample)", who, (long long)opt->bin);
    HS_CHECK(opt->nq >= 0 && opt->nq <= HMMSORT_STAB_MAX_Q, HMMSORT_EINVAL, "%s: nq = %lld quantiles (0..%d)", who,
             (long long)opt->nq, HMMSORT_STAB_MAX_Q);
    HS_CHECK(opt->q_den >= 1 && opt->q_den <= HMMSORT_STAB_MAX_QDEN, HMMSORT_EINVAL, "%s: q_den = %lld (1..%lld)", who,
             (long long)opt->q_den, (long long)HMMSORT_STAB_MAX_QDEN);
    for (int64_t k = 0; k < opt->nq; k++)
        HS_CHECK(opt->q_num[k] >= 0 && opt->q_num[k] <= opt->q_den, HMMSORT_EINVAL, "%s: q_num[%lld] = %lld outside "
                 "0..q_den = %lld", who, (long long)k, (long long)opt->q_num[k], (long long)opt->q_den);
    HS_CHECK(opt->HB >= 0 && opt->HB <= HMMSORT_STAB_MAX_HIST, HMMSORT_EINVAL, "%s: HB = %lld histogram bins (0..%d)",
             who, (long long)opt->HB, HMMSORT_STAB_MAX_HIST);
    if (opt->HB > 0) {
        HS_CHECK(std::isfinite(opt->hist_scale) && opt->hist_scale > 0.0, HMMSORT_EINVAL, "%s: hist_scale = %g (finite "
                 "and positive)", who, opt->hist_scale);
        HS_CHECK(std::isfinite(opt->hist_lo), HMMSORT_EINVAL, "%s: hist_lo = %g (finite)", who, opt->hist_lo);
    }
    const int64_t B = (opt->T + opt->bin - 1) / opt->bin;
    HS_CHECK(B <= HMMSORT_STAB_MAX_BINS, HMMSORT_EUNSUP, "%s: B = %lld time bins (ceil(T / bin) = ceil(%lld / %lld); at "
             "most 2^24)", who, (long long)B, (long long)opt->T, (long long)opt->bin);
    HS_CHECK(U * B <= HMMSORT_STAB_MAX_BINS, HMMSORT_EUNSUP, "%s: %lld segments (U * B = %lld * %lld; at most 2^24)", who,
             (long long)(U * B), (long long)U, (long long)B);
    *B_out = B;
    return HMMSORT_OK;
}

int dev_unit_stability(int64_t U, const int64_t *d_times, const double *d_vals, const int64_t *offs,
                       const hmmsort_stab_opt *opt, const hmmsort_stab_out *out, int64_t B, hipStream_t st)
{
    const int64_t o0 = offs[0], n = offs[U] - o0, nb = U * (B + 1), nseg = U * B, nq = opt->nq, HB = opt->HB;
    for (int64_t u = 0; u < U; u++) {
        HS_CHECK(offs[u + 1] >= offs[u], HMMSORT_EINVAL, "unit_stability: unit %lld has %lld entries", (long long)u,
                 (long long)(offs[u + 1] - offs[u]));
        out->n[u] = offs[u + 1] - offs[u];
    }
    HS_CHECK(n < (1ll << 31), HMMSORT_EUNSUP, "unit_stability: %lld spikes in all (below 2^31)", (long long)n);
    int rc;
    DevBuf doff, dbnd, dvb, dtcnt, dtbase, dkv, dpre;
    std::vector<int64_t> bnd((size_t)nb), vb;
    if ((rc = doff.alloc((U + 1) * sizeof(int64_t))) || (rc = dbnd.alloc(nb * sizeof(int64_t)))) return rc;
    HS_HIP(hipMemcpyAsync(doff.p, offs, (U + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_stab_bounds, dim3(stab_blocks(nb)), dim3(kStabThreads), 0, st, d_times, doff.as<int64_t>(), U,
                       B, opt->bin, dbnd.as<int64_t>());
    HS_HIP(hipGetLastError());
    HS_HIP(hipMemcpyAsync(bnd.data(), dbnd.p, nb * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    const bool vals = d_vals && n > 0;
    if (d_vals) vb.assign((size_t)nb, 0);
    if (vals) {
        const int64_t ntile = (n + kStabTile - 1) / kStabTile;
        if ((rc = dvb.alloc(nb * sizeof(int64_t))) || (rc = dtcnt.alloc(ntile * sizeof(int64_t))) ||
            (rc = dtbase.alloc((ntile + 1) * sizeof(int64_t))) || (rc = dkv.alloc(n * sizeof(unsigned long long))) ||
            (rc = dpre.alloc((n + 1) * sizeof(int64_t))))
            return rc;
        hipLaunchKernelGGL(k_stab_tcount, dim3((unsigned)ntile), dim3(kStabThreads), 0, st, d_vals + o0, n,
                           dtcnt.as<int64_t>());
        hipLaunchKernelGGL(k_stab_scan, dim3(1), dim3(kStabThreads), 0, st, dtcnt.as<int64_t>(), ntile,
                           dtbase.as<int64_t>());
        hipLaunchKernelGGL(k_stab_compact, dim3((unsigned)ntile), dim3(kStabThreads), 0, st, d_vals + o0, n, ntile,
                           dtbase.as<int64_t>(), dkv.as<unsigned long long>(), dpre.as<int64_t>());
        hipLaunchKernelGGL(k_stab_gather, dim3(stab_blocks(nb)), dim3(kStabThreads), 0, st, dbnd.as<int64_t>(), nb, o0,
                           dpre.as<int64_t>(), dvb.as<int64_t>());
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(vb.data(), dvb.p, nb * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    HS_HIP(hipStreamSynchronize(st));
    // the boundaries of a list that ascends never step back; the device forms cannot check their lists before
    for (int64_t u = 0; u < U; u++)
        for (int64_t b = 0; b < B; b++)
            HS_CHECK(bnd[u * (B + 1) + b + 1] >= bnd[u * (B + 1) + b], HMMSORT_EINVAL, "unit_stability: times: the list "
                     "of unit %lld is not ascending (bin %lld)", (long long)u, (long long)b);
    if (out->count)
        for (int64_t u = 0; u < U; u++)
            for (int64_t b = 0; b < B; b++) out->count[u * B + b] = bnd[u * (B + 1) + b + 1] - bnd[u * (B + 1) + b];
    if (!d_vals) return HMMSORT_OK;   // counts only
    if (out->valid)
        for (int64_t u = 0; u < U; u++)
            for (int64_t b = 0; b < B; b++) out->valid[u * B + b] = vb[u * (B + 1) + b + 1] - vb[u * (B + 1) + b];
    if (out->uvalid)
        for (int64_t u = 0; u < U; u++) out->uvalid[u] = vb[u * (B + 1) + B] - vb[u * (B + 1)];
    const bool want_q = out->quant && nq > 0, want_s = out->sum || out->sumsq || out->usum || out->usumsq;
    const bool want_u = (out->uquant && nq > 0) || out->umin || out->umax;
    const bool want_h = HB > 0 && (out->hist || out->under || out->over);
    const double nan = std::nan("");
    if (!vals) {   // no spike at all: nothing more is launched
        if (want_q) std::fill(out->quant, out->quant + nseg * nq, nan);
        if (out->sum) std::fill(out->sum, out->sum + nseg, 0.0);
        if (out->sumsq) std::fill(out->sumsq, out->sumsq + nseg, 0.0);
        for (int64_t u = 0; u < U; u++) {
            for (int64_t k = 0; out->uquant && k < nq; k++) out->uquant[u * nq + k] = nan;
            if (out->umin) out->umin[u] = nan;
            if (out->umax) out->umax[u] = nan;
            if (out->usum) out->usum[u] = 0.0;
            if (out->usumsq) out->usumsq[u] = 0.0;
        }
        if (HB > 0 && out->hist) std::fill(out->hist, out->hist + U * HB, (int64_t)0);
        if (HB > 0 && out->under) std::fill(out->under, out->under + U, (int64_t)0);
        if (HB > 0 && out->over) std::fill(out->over, out->over + U, (int64_t)0);
        return HMMSORT_OK;
    }

    // the work: [0, nw) segment jobs of one wave, [nw, njs) of one workgroup; then the same for the units
    std::vector<int64_t> jstart, jm, jout, tfirst, tstart;
    std::vector<int32_t> tlen;
    for (int pass = 0; pass < 2; pass++)   // short jobs first
        for (int64_t s = 0; s < nseg; s++) {
            const int64_t i = s / B * (B + 1) + s % B, m = vb[i + 1] - vb[i];
            if (m > 0 && (m <= kStabWaveKeys) == (pass == 0)) jstart.push_back(vb[i]), jm.push_back(m), jout.push_back(s);
        }
    const int64_t njs = (int64_t)jm.size();
    int64_t nw = 0;
    while (nw < njs && jm[nw] <= kStabWaveKeys) nw++;
    if (want_s) {
        tfirst.push_back(0);
        for (int64_t j = 0; j < njs; j++) {
            for (int64_t k = 0; k < jm[j]; k += kStabTile)
                tstart.push_back(jstart[j] + k), tlen.push_back((int32_t)std::min<int64_t>(kStabTile, jm[j] - k));
            tfirst.push_back((int64_t)tstart.size());
        }
    }
    for (int pass = 0; pass < 2; pass++)
        for (int64_t u = 0; u < U; u++) {
            const int64_t i = u * (B + 1), m = vb[i + B] - vb[i];
            if (m > 0 && (m <= kStabWaveKeys) == (pass == 0)) jstart.push_back(vb[i]), jm.push_back(m), jout.push_back(u);
        }
    const int64_t nj = (int64_t)jm.size(), nju = nj - njs, nt = (int64_t)tstart.size();
    int64_t nwu = 0;
    while (nwu < nju && jm[njs + nwu] <= kStabWaveKeys) nwu++;

    const int Ru = (int)nq + 2;
    DevBuf djs, djm, djo, dtf, dts, dtl, dps, dpq, dq, duq, dsum, dsq, dus, duss, dh;
    if ((rc = djs.alloc(nj * sizeof(int64_t))) || (rc = djm.alloc(nj * sizeof(int64_t))) ||
        (rc = djo.alloc(nj * sizeof(int64_t))))
        return rc;
    HS_HIP(hipMemcpyAsync(djs.p, jstart.data(), nj * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemcpyAsync(djm.p, jm.data(), nj * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemcpyAsync(djo.p, jout.data(), nj * sizeof(int64_t), hipMemcpyHostToDevice, st));
    StabSel A;
    A.kv = dkv.as<unsigned long long>();
    A.den = opt->q_den;
    for (int64_t k = 0; k < nq; k++) A.num[k] = opt->q_num[k];
    A.num[nq] = 0, A.num[nq + 1] = opt->q_den;   // a unit's minimum and maximum
    for (int64_t k = nq + 2; k < kStabMaxRanks; k++) A.num[k] = 0;
    // ranks of a slice [j0, j1) of the job list into rows of R
    auto select = [&](int64_t j0, int64_t jw, int64_t j1, int R, double *d_out) {
        A.jstart = djs.as<int64_t>() + j0, A.jm = djm.as<int64_t>() + j0, A.jout = djo.as<int64_t>() + j0;
        A.R = R, A.out = d_out;
        if (jw > j0) {
            A.njobs = jw - j0;
            hipLaunchKernelGGL(k_stab_sel_wave, dim3((unsigned)((A.njobs + 3) / 4)), dim3(kStabThreads), 0, st, A);
        }
        if (j1 > jw) {
            A.jstart += jw - j0, A.jm += jw - j0, A.jout += jw - j0, A.njobs = j1 - jw;
            hipLaunchKernelGGL(k_stab_sel_block, dim3((unsigned)A.njobs), dim3(kStabThreads), 0, st, A);
        }
    };
    if (want_q) {
        if ((rc = dq.alloc(nseg * nq * sizeof(double)))) return rc;
        hipLaunchKernelGGL(k_stab_fill, dim3(stab_blocks(nseg * nq)), dim3(kStabThreads), 0, st, dq.as<double>(),
                           nseg * nq, nan);
        select(0, nw, njs, (int)nq, dq.as<double>());
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(out->quant, dq.p, nseg * nq * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    std::vector<double> uq;
    if (want_u) {
        uq.assign((size_t)(U * Ru), 0.0);
        if ((rc = duq.alloc(U * Ru * sizeof(double)))) return rc;
        hipLaunchKernelGGL(k_stab_fill, dim3(stab_blocks(U * Ru)), dim3(kStabThreads), 0, st, duq.as<double>(), U * Ru,
                           nan);
        select(njs, njs + nwu, nj, Ru, duq.as<double>());
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(uq.data(), duq.p, U * Ru * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (want_s) {
        if ((rc = dtf.alloc((njs + 1) * sizeof(int64_t))) || (rc = dts.alloc(nt * sizeof(int64_t))) ||
            (rc = dtl.alloc(nt * sizeof(int32_t))) || (rc = dps.alloc(nt * sizeof(double))) ||
            (rc = dpq.alloc(nt * sizeof(double))) || (rc = dsum.alloc(nseg * sizeof(double))) ||
            (rc = dsq.alloc(nseg * sizeof(double))) || (rc = dus.alloc(U * sizeof(double))) ||
            (rc = duss.alloc(U * sizeof(double))))
            return rc;
        HS_HIP(hipMemcpyAsync(dtf.p, tfirst.data(), (njs + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(dts.p, tstart.data(), nt * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(dtl.p, tlen.data(), nt * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemsetAsync(dsum.p, 0, nseg * sizeof(double), st));   // +0.0 for a segment without a value
        HS_HIP(hipMemsetAsync(dsq.p, 0, nseg * sizeof(double), st));
        if (njs > 0) {   // else every value is a NaN
            hipLaunchKernelGGL(k_stab_tile_sums, dim3(stab_blocks(nt)), dim3(kStabThreads), 0, st,
                               dkv.as<unsigned long long>(), dts.as<int64_t>(), dtl.as<int32_t>(), nt, dps.as<double>(),
                               dpq.as<double>());
            hipLaunchKernelGGL(k_stab_seg_fold, dim3(stab_blocks(njs)), dim3(kStabThreads), 0, st, dps.as<double>(),
                               dpq.as<double>(), dtf.as<int64_t>(), djo.as<int64_t>(), njs, dsum.as<double>(),
                               dsq.as<double>());
        }
        hipLaunchKernelGGL(k_stab_unit_fold, dim3(stab_blocks(U)), dim3(kStabThreads), 0, st, dsum.as<double>(),
                           dsq.as<double>(), U, B, dus.as<double>(), duss.as<double>());
        HS_HIP(hipGetLastError());
        if (out->sum) HS_HIP(hipMemcpyAsync(out->sum, dsum.p, nseg * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out->sumsq) HS_HIP(hipMemcpyAsync(out->sumsq, dsq.p, nseg * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out->usum) HS_HIP(hipMemcpyAsync(out->usum, dus.p, U * sizeof(double), hipMemcpyDeviceToHost, st));
        if (out->usumsq) HS_HIP(hipMemcpyAsync(out->usumsq, duss.p, U * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    std::vector<int64_t> h;
    if (want_h) {
        int64_t most = 0;
        for (int64_t u = 0; u < U; u++) most = std::max(most, vb[u * (B + 1) + B] - vb[u * (B + 1)]);
        const unsigned blocks = (unsigned)std::min<int64_t>(kStabHistBlocks, std::max<int64_t>(1, (most + 4095) / 4096));
        h.assign((size_t)(U * (HB + 2)), 0);
        if ((rc = dh.alloc(U * (HB + 2) * sizeof(int64_t)))) return rc;
        HS_HIP(hipMemsetAsync(dh.p, 0, U * (HB + 2) * sizeof(int64_t), st));
        unsigned long long *d_h = dh.as<unsigned long long>();
        hipLaunchKernelGGL(k_stab_hist, dim3(blocks, (unsigned)U), dim3(kStabThreads), 0, st,
                           dkv.as<unsigned long long>(), dvb.as<int64_t>(), B, (int)HB, opt->hist_lo, opt->hist_scale, d_h,
                           d_h + U * HB, d_h + U * HB + U);
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(h.data(), dh.p, U * (HB + 2) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    HS_HIP(hipStreamSynchronize(st));   // the tables die with this frame
    for (int64_t u = 0; want_u && u < U; u++) {
        for (int64_t k = 0; out->uquant && k < nq; k++) out->uquant[u * nq + k] = uq[u * Ru + k];
        if (out->umin) out->umin[u] = uq[u * Ru + nq];
        if (out->umax) out->umax[u] = uq[u * Ru + nq + 1];
    }
    if (want_h) {
        if (out->hist) std::copy(h.begin(), h.begin() + U * HB, out->hist);
        if (out->under) std::copy(h.begin() + U * HB, h.begin() + U * HB + U, out->under);
        if (out->over) std::copy(h.begin() + U * HB + U, h.end(), out->over);
    }
    return HMMSORT_OK;
}

}  // namespace hmmsort
