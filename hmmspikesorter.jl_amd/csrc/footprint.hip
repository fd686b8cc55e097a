// Footprints: the spike-triggered sum and sum of squares of every unit on every listed channel of a resident block
// (hmmsort_footprints / _device / hmmsort_plan_footprints, include/hmmsort.h).  The work is a gather; the
// only arithmetic is a fold in a fixed order, so the same input gives the same bits and the numpy model
// tests/footprint_model.py states the same rule.
//
// The U lists sit concatenated in device memory behind U + 1 offsets, as for the correlograms.  Every list is cut into
// tiles of 256 consecutive entries (host tables: first entry, entries, unit per tile; first tile per unit).
//   k_fp_gather  grid (tile, groups of 4 wave items).  The block stages the tile once in LDS: per entry the window's
//                first sample t - 1 - pre, or -1 for an entry that is not used.  A wave item is one slot and one run
//                of 64 window samples of it, so a wave reads, per spike, one contiguous run of its channel's row: the
//                address is a scalar origin (row + window start, both the same for the whole wave) plus the lane's k
//                as a 32-bit offset.  (hipcc hoists row + k into a lane pointer and adds the scalar window start with
//                one 64-bit VALU add per load; the bytes, not that add, bound the kernel.)  Each lane folds the tile's spikes serially, eight loads issued ahead of the eight
//                adds that consume them; the adds stay in list order.  An unused entry loads the window at sample 0
//                (inside the block, since W <= T when anything is launched) and contributes +0.0: ps + 0.0 == ps to
//                the bit, because a sum that started at +0.0 is never -0.0.  The tile's partials go to [tile][M W].
//   k_fp_fold    one lane per (u, slot, k): the unit's tile partials folded from 0.0 in tile order; lane (u, 0, 0) also
//                adds up the tiles' used counts.  Empty slots are written as zeros here and never gathered.
#include <algorithm>

#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

constexpr int kFpTile = 256;        // list entries of one tile = threads of a block (spike_fit's summary constant)
constexpr int kFpWaves = kFpTile / 64;
constexpr int kFpAhead = 8;         // loads in flight per lane
constexpr int64_t kFpMaxEntries = 1ll << 28;

struct FpArgs {
    const double *y;          // [C][T]
    const int64_t *t;         // the lists, concatenated
    const int64_t *tile_e;    // [ntiles] index into t of the tile's first entry
    const int32_t *tile_n;    // [ntiles] its entries, 1..256
    const int32_t *tile_u;    // [ntiles] its unit
    const int64_t *first;     // [U + 1] first tile of a unit
    const int32_t *chan;      // [U][M] or null
    int64_t T, lo, hi;        // an entry t is used iff lo <= t <= hi (lo = 1 + pre, hi = T - W + 1 + pre)
    int U, M, W, nchunk, MW;  // nchunk = ceil(W / 64)
    double *psum, *psq;       // [ntiles][M W]
    int32_t *tused;           // [ntiles]
    double *sum, *sumsq;      // [U][M W]
    int64_t *nused;           // [U]
};

// a 64-bit value every lane of the wave holds, moved to scalar registers
__device__ __forceinline__ int64_t fp_uniform(int64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ __launch_bounds__(kFpTile) void k_fp_gather(const FpArgs A)
{
    __shared__ int64_t s_base[kFpTile];
    __shared__ int s_w[kFpWaves];
    const int64_t tile = blockIdx.x;
    const int n = A.tile_n[tile];
    int64_t b = -1;
    if ((int)threadIdx.x < n) {
        const int64_t t = A.t[A.tile_e[tile] + threadIdx.x];
        if (t >= A.lo && t <= A.hi) b = t - A.lo;   // 0 <= b <= T - W
    }
    s_base[threadIdx.x] = b;
    if (blockIdx.y == 0) {
        const unsigned long long bm = __ballot(b >= 0);
        if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(bm);
    }
    __syncthreads();
    if (blockIdx.y == 0 && threadIdx.x == 0) A.tused[tile] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * kFpWaves + (threadIdx.x >> 6)));
    if (item >= A.M * A.nchunk) return;
    const int m = item / A.nchunk, k = (item - m * A.nchunk) * 64 + (int)(threadIdx.x & 63);
    const int ch = A.chan ? A.chan[(int64_t)A.tile_u[tile] * A.M + m] : m;
    if (ch < 0 || k >= A.W) return;
    // the row is the same for the whole wave: a scalar origin, and the lane's k as a 32-bit byte offset (k < 1024)
    const char *row = (const char *)fp_uniform((int64_t)(A.y + (int64_t)ch * A.T));
    const uint32_t kb = (uint32_t)k * (uint32_t)sizeof(double);
    double ps = 0.0, pq = 0.0;
    for (int i0 = 0; i0 < n; i0 += kFpAhead) {   // entries n .. 255 of s_base are -1
        double s[kFpAhead];
#pragma unroll
        for (int j = 0; j < kFpAhead; j++) {
            const int64_t bj = fp_uniform(s_base[i0 + j]);
            const double v = *(const double *)(row + (bj < 0 ? 0 : bj) * (int64_t)sizeof(double) + kb);
            s[j] = bj < 0 ? 0.0 : v;
        }
#pragma unroll
        for (int j = 0; j < kFpAhead; j++) {
            const double q = s[j] * s[j];   // rounded on its own (-ffp-contract=off)
            ps = ps + s[j];
            pq = pq + q;
        }
    }
    const int64_t o = tile * A.MW + (int64_t)m * A.W + k;
    A.psum[o] = ps;
    A.psq[o] = pq;
}

__global__ __launch_bounds__(kFpTile) void k_fp_fold(const FpArgs A)
{
    const int64_t idx = (int64_t)blockIdx.x * kFpTile + threadIdx.x;
    if (idx >= (int64_t)A.U * A.MW) return;
    const int u = (int)(idx / A.MW), j = (int)(idx - (int64_t)u * A.MW), m = j / A.W;
    const int ch = A.chan ? A.chan[(int64_t)u * A.M + m] : m;
    const int64_t t0 = A.first[u], t1 = A.first[u + 1];
    double a = 0.0, q = 0.0;
    if (ch >= 0)
        for (int64_t tile = t0; tile < t1; tile++) {
            a = a + A.psum[tile * A.MW + j];
            q = q + A.psq[tile * A.MW + j];
        }
    A.sum[idx] = a;
    A.sumsq[idx] = q;
    if (j == 0) {
        int64_t c = 0;
        for (int64_t tile = t0; tile < t1; tile++) c += A.tused[tile];
        A.nused[u] = c;
    }
}

}  // namespace

int fp_check(const char *who, int64_t C, int64_t T, int64_t U, const hmmsort_fp_opt *opt, const hmmsort_fp_out *out,
             int64_t *M_out)
{
    HS_CHECK(opt && out && out->n, HMMSORT_EINVAL, "%s: null argument (the options, the output record and its n are "
             "required)", who);
    HS_CHECK(C >= 1 && C <= HMMSORT_PRE_MAX_CHANNELS, HMMSORT_EINVAL, "%s: C = %lld channels (1..%d)", who,
             (long long)C, HMMSORT_PRE_MAX_CHANNELS);
    HS_CHECK(T >= 1 && T <= (1ll << 36), HMMSORT_EINVAL, "%s: T = %lld samples (1..2^36)", who, (long long)T);
    HS_CHECK(U >= 1 && U <= HMMSORT_FP_MAX_UNITS, HMMSORT_EINVAL, "%s: U = %lld units (1..%d)", who, (long long)U,
             HMMSORT_FP_MAX_UNITS);
    HS_CHECK(opt->W >= 1 && opt->W <= HMMSORT_FP_MAX_W, HMMSORT_EINVAL, "%s: W = %lld window samples (1..%d)", who,
             (long long)opt->W, HMMSORT_FP_MAX_W);
    HS_CHECK(opt->pre >= 0 && opt->pre <= (1ll << 20), HMMSORT_EINVAL, "%s: pre = %lld (0..2^20)", who,
             (long long)opt->pre);
    int64_t M = C;
    if (opt->chan) {
        M = opt->M;
        HS_CHECK(M >= 1 && M <= HMMSORT_FP_MAX_SLOTS, HMMSORT_EINVAL, "%s: M = %lld slots per unit (1..%d)", who,
                 (long long)M, HMMSORT_FP_MAX_SLOTS);
        for (int64_t i = 0; i < U * M; i++)
            HS_CHECK(opt->chan[i] >= -1 && opt->chan[i] < C, HMMSORT_EINVAL, "%s: chan: unit %lld, slot %lld: channel "
                     "%d outside -1..%lld", who, (long long)(i / M), (long long)(i % M), (int)opt->chan[i],
                     (long long)(C - 1));
    }
    const int64_t entries = U * M * opt->W;
    HS_CHECK(entries <= kFpMaxEntries, HMMSORT_EUNSUP, "%s: %lld footprint entries (U * M * W = %lld * %lld * %lld; at "
             "most 2^28)", who, (long long)entries, (long long)U, (long long)M, (long long)opt->W);
    *M_out = M;
    return HMMSORT_OK;
}

int dev_footprints(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times, const int64_t *offs,
                   const hmmsort_fp_opt *opt, const hmmsort_fp_out *out, hipStream_t st)
{
    const int64_t W = opt->W, M = opt->chan ? opt->M : C, MW = M * W;
    int64_t ntiles = 0;
    for (int64_t u = 0; u < U; u++) {
        out->n[u] = offs[u + 1] - offs[u];
        ntiles += (out->n[u] + kFpTile - 1) / kFpTile;
    }
    if (ntiles == 0 || W > T) {   // no spike, or no window fits: zeros, nothing is launched
        if (out->sum) std::fill(out->sum, out->sum + U * MW, 0.0);
        if (out->sumsq) std::fill(out->sumsq, out->sumsq + U * MW, 0.0);
        if (out->nused) std::fill(out->nused, out->nused + U, (int64_t)0);
        HS_HIP(hipStreamSynchronize(st));   // what the caller enqueued for d_times
        return HMMSORT_OK;
    }
    if (!(out->sum || out->sumsq || out->nused)) return HMMSORT_OK;
    HS_CHECK(ntiles <= 0x7fffffffll, HMMSORT_EUNSUP, "footprints: %lld tiles of %d spikes", (long long)ntiles, kFpTile);
    // one workspace in 8-byte words: the tables (built in `tab`, one upload), then partials, results and tile counts
    const int64_t half = (ntiles + 1) / 2, nchan = opt->chan ? (U * M + 1) / 2 : 0;   // int32 tables, in words
    const int64_t o_first = ntiles, o_tn = o_first + U + 1, o_tu = o_tn + half, o_chan = o_tu + half;
    const int64_t o_ps = o_chan + nchan, o_pq = o_ps + ntiles * MW, o_sum = o_pq + ntiles * MW, o_sq = o_sum + U * MW;
    const int64_t o_nu = o_sq + U * MW, o_tused = o_nu + U, words = o_tused + half;
    std::vector<int64_t> tab((size_t)o_ps, 0);
    int64_t *tile_e = tab.data(), *first = tab.data() + o_first;
    int32_t *tile_n = (int32_t *)(tab.data() + o_tn), *tile_u = (int32_t *)(tab.data() + o_tu);
    for (int64_t u = 0, k = 0; u < U; u++) {
        first[u] = k;
        for (int64_t e = 0; e < out->n[u]; e += kFpTile, k++) {
            tile_e[k] = offs[u] + e;
            tile_n[k] = (int32_t)std::min<int64_t>(kFpTile, out->n[u] - e);
            tile_u[k] = (int32_t)u;
        }
        first[u + 1] = k;
    }
    if (opt->chan) std::copy(opt->chan, opt->chan + U * M, (int32_t *)(tab.data() + o_chan));
    DevBuf ws;
    int rc;
    if ((rc = ws.alloc((size_t)words * sizeof(int64_t)))) return rc;
    int64_t *w = ws.as<int64_t>();
    HS_HIP(hipMemcpyAsync(w, tab.data(), (size_t)o_ps * sizeof(int64_t), hipMemcpyHostToDevice, st));
    FpArgs A;
    A.y = d_y, A.t = d_times, A.tile_e = w, A.first = w + o_first;
    A.tile_n = (const int32_t *)(w + o_tn), A.tile_u = (const int32_t *)(w + o_tu);
    A.chan = opt->chan ? (const int32_t *)(w + o_chan) : nullptr;
    A.T = T, A.lo = 1 + opt->pre, A.hi = T - W + 1 + opt->pre;
    A.U = (int)U, A.M = (int)M, A.W = (int)W, A.nchunk = (int)((W + 63) / 64), A.MW = (int)MW;
    A.psum = (double *)(w + o_ps), A.psq = (double *)(w + o_pq), A.tused = (int32_t *)(w + o_tused);
    A.sum = (double *)(w + o_sum), A.sumsq = (double *)(w + o_sq), A.nused = w + o_nu;
    const int64_t items = M * A.nchunk;   // at most 1024 * 16
    hipLaunchKernelGGL(k_fp_gather, dim3((unsigned)ntiles, (unsigned)((items + kFpWaves - 1) / kFpWaves)),
                       dim3(kFpTile), 0, st, A);
    HS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_fp_fold, dim3((unsigned)((U * MW + kFpTile - 1) / kFpTile)), dim3(kFpTile), 0, st, A);
    HS_HIP(hipGetLastError());
    if (out->sum) HS_HIP(hipMemcpyAsync(out->sum, A.sum, U * MW * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out->sumsq) HS_HIP(hipMemcpyAsync(out->sumsq, A.sumsq, U * MW * sizeof(double), hipMemcpyDeviceToHost, st));
    if (out->nused) HS_HIP(hipMemcpyAsync(out->nused, A.nused, U * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));   // the workspace and `tab` die with this frame
    return HMMSORT_OK;
}

}  // namespace hmmsort
