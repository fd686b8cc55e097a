// Correlograms, refractory violations and coincident spikes of sorted units (hmmsort_correlograms /
// hmmsort_plan_correlograms, include/hmmsort.h).  Integers only: every output is a count, the global sums
// are 64-bit integer atomics, and integer adds commute, so the same input gives the same bits whatever the arrival
// order.  The numpy model tests/correlogram_model.py states the same rules.
//
// The U lists sit concatenated in device memory behind U + 1 offsets.  Sources are cut into tiles of 256 consecutive
// spikes of one unit (a host table of (unit, first spike) per tile); a tile's spikes span a short stretch of time, so
// the targets any of them can reach in a unit v are one short run of v's list.
//   k_ccg_hist   grid (tile, v).  Two lanes find that run by binary search over v's whole list (the targets in
//                [t_first - H b, t_last + H b)); a block whose run is empty leaves.  Each lane then takes one source
//                spike: lower bound of t - H b inside the run, walk while t_v[j] < t + H b, d in 64 bits, bin =
//                (d + H b) / b on a non-negative 32-bit value (a shift for a power of two, else a multiply-high
//                reciprocal with a correction), one LDS atomic per pair.  Non-zero bins go to ccg[u][v][.] with one
//                64-bit atomic per bin and tile.  Work: two searches per (tile, v), one short search per source with a
//                non-empty run, and the pairs inside the window.
//                The LDS counters are 32-bit: the times of a list are strictly ascending, so one source finds at most
//                min(b, targets walked) targets in one bin; the run is walked in chunks of 2^23 targets with a flush
//                between chunks, so a tile adds at most 256 * 2^23 = 2^31 to a counter before it is flushed.
//   k_ccg_coinc  grid (tile, v): the same run for the window |d| <= c, per lane one lower bound and one compare (two
//                when the entry found is the spike itself); a block count, one atomic per (tile, v).
//   k_ccg_viol   grid (tile): a neighbour compare per lane, one atomic per tile.
#include <algorithm>

#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

constexpr int kCcgTile = 256;                  // source spikes of one tile = threads of a block
constexpr int kCcgMaxBins = 4096;              // 2 H at most: 16 KB of LDS counters
constexpr int64_t kCcgChunk = 1ll << 23;       // targets walked between two flushes of the LDS counters
constexpr int64_t kCcgMaxTime = 1ll << 40;

struct CcgArgs {
    const int64_t *t;        // the lists, concatenated
    const int64_t *off;      // [U + 1]
    const int32_t *tile_u;   // [ntiles] unit of the tile
    const int64_t *tile_s;   // [ntiles] its first spike, counted inside the unit
    int U, nbins;            // nbins = 2 H
    uint32_t b, W;           // W = H b < 2^31
    int shift;               // log2 b for a power of two, else -1
    uint32_t recip;          // floor(2^32 / b) otherwise
    int64_t r, c;            // clamped to 2^41: no time difference is larger
    unsigned long long *ccg, *viol, *coinc;
};

// first index in [lo, hi) whose entry is >= key (hi when none)
__device__ __forceinline__ int64_t lower_bound(const int64_t *__restrict__ a, int64_t lo, int64_t hi, int64_t key)
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

// the tile a block works on: unit, list, this lane's spike
struct CcgTile {
    int u;
    const int64_t *tu;
    int64_t nu, s0, i, last;   // s0, last: the tile's first and last spike
    bool live;
    int64_t t;
};

__device__ __forceinline__ CcgTile ccg_tile(const CcgArgs &A, int tile)
{
    CcgTile q;
    q.u = A.tile_u[tile];
    const int64_t s0 = q.s0 = A.tile_s[tile], ou = A.off[q.u];
    q.tu = A.t + ou;
    q.nu = A.off[q.u + 1] - ou;
    q.last = (s0 + kCcgTile < q.nu ? s0 + kCcgTile : q.nu) - 1;
    q.i = s0 + threadIdx.x;
    q.live = q.i <= q.last;
    q.t = q.live ? q.tu[q.i] : 0;
    return q;
}

// [*lo, *hi): the entries of tv[0..nv) in [kmin, kend), found by lanes 0 and 1; false (for the whole block) when empty
__device__ __forceinline__ bool ccg_run(const int64_t *__restrict__ tv, int64_t nv, int64_t kmin, int64_t kend,
                                        int64_t *s_run, int64_t *lo, int64_t *hi)
{
    if (threadIdx.x < 2) s_run[threadIdx.x] = lower_bound(tv, 0, nv, threadIdx.x == 0 ? kmin : kend);
    __syncthreads();
    *lo = s_run[0], *hi = s_run[1];
    return *lo < *hi;
}

// number of threads of the block for which hit holds, in thread 0
__device__ __forceinline__ int ccg_block_count(bool hit, int *s_w)
{
    const unsigned long long bm = __ballot(hit);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = __popcll(bm);
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ __launch_bounds__(kCcgTile) void k_ccg_hist(const CcgArgs A)
{
    __shared__ uint32_t s_h[kCcgMaxBins];
    __shared__ int64_t s_run[2];
    const int v = blockIdx.y;
    const int64_t ov = A.off[v], nv = A.off[v + 1] - ov;
    if (nv == 0) return;
    const int64_t *__restrict__ tv = A.t + ov;
    const CcgTile q = ccg_tile(A, blockIdx.x);
    const int64_t W = A.W;
    int64_t lo, hi;
    if (!ccg_run(tv, nv, q.tu[q.s0] - W, q.tu[q.last] + W, s_run, &lo, &hi)) return;
    const int64_t j0 = q.live ? lower_bound(tv, lo, hi, q.t - W) : hi;
    const bool same = q.u == v;
    unsigned long long *out = A.ccg + ((int64_t)q.u * A.U + v) * A.nbins;
    for (int64_t c0 = lo; c0 < hi; c0 += kCcgChunk) {
        const int64_t c1 = hi - c0 < kCcgChunk ? hi : c0 + kCcgChunk;
        for (int k = threadIdx.x; k < A.nbins; k += kCcgTile) s_h[k] = 0u;
        __syncthreads();
        for (int64_t j = j0 > c0 ? j0 : c0; j < c1; j++) {
            const int64_t d = tv[j] - q.t;   // >= -W by the lower bound
            if (d >= W) break;
            if (same && j == q.i) continue;  // the self pair
            const uint32_t x = (uint32_t)(d + W);   // 0 <= x < 2 W < 2^32
            uint32_t k;
            if (A.shift >= 0) {
                k = x >> A.shift;
            } else {
                k = __umulhi(x, A.recip);            // floor(x / b) or one less
                if (x - k * A.b >= A.b) k++;
            }
            atomicAdd(&s_h[k], 1u);
        }
        __syncthreads();
        for (int k = threadIdx.x; k < A.nbins; k += kCcgTile) {
            const uint32_t h = s_h[k];
            if (h) atomicAdd(&out[k], (unsigned long long)h);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kCcgTile) void k_ccg_coinc(const CcgArgs A)
{
    __shared__ int64_t s_run[2];
    __shared__ int s_w[4];
    const int v = blockIdx.y;
    const int64_t ov = A.off[v], nv = A.off[v + 1] - ov;
    if (nv == 0) return;
    const int64_t *__restrict__ tv = A.t + ov;
    const CcgTile q = ccg_tile(A, blockIdx.x);
    int64_t lo, hi;
    if (!ccg_run(tv, nv, q.tu[q.s0] - A.c, q.tu[q.last] + A.c + 1, s_run, &lo, &hi)) return;
    bool hit = false;
    if (q.live) {
        int64_t j = lower_bound(tv, lo, hi, q.t - A.c);
        // Its own entry: everything before it is earlier than t - c, so the next entry is the only candidate left.
        if (q.u == v && j == q.i) j++;
        hit = j < hi && tv[j] <= q.t + A.c;
    }
    const int cnt = ccg_block_count(hit, s_w);
    if (threadIdx.x == 0 && cnt) atomicAdd(&A.coinc[(int64_t)q.u * A.U + v], (unsigned long long)cnt);
}

__global__ __launch_bounds__(kCcgTile) void k_ccg_viol(const CcgArgs A)
{
    __shared__ int s_w[4];
    const CcgTile q = ccg_tile(A, blockIdx.x);
    const bool hit = q.live && q.i >= 1 && q.t - q.tu[q.i - 1] < A.r;
    const int cnt = ccg_block_count(hit, s_w);
    if (threadIdx.x == 0 && cnt) atomicAdd(&A.viol[q.u], (unsigned long long)cnt);
}

}  // namespace

int ccg_check(const char *who, int64_t U, const hmmsort_ccg_opt *opt, const hmmsort_ccg_out *out)
{
    HS_CHECK(opt && out && out->n, HMMSORT_EINVAL, "%s: null argument (the options, the output record and its n are "
             "required)", who);
    HS_CHECK(U >= 1 && U <= 4096, HMMSORT_EINVAL, "%s: U = %lld units (1..4096)", who, (long long)U);
    HS_CHECK(opt->bin >= 1, HMMSORT_EINVAL, "%s: bin = %lld (at least 1 sample)", who, (long long)opt->bin);
    HS_CHECK(opt->half_bins >= 1 && opt->half_bins <= kCcgMaxBins / 2, HMMSORT_EINVAL, "%s: half_bins = %lld (1..%d)",
             who, (long long)opt->half_bins, kCcgMaxBins / 2);
    HS_CHECK(opt->bin < (1ll << 31) && opt->half_bins * opt->bin < (1ll << 31), HMMSORT_EINVAL,
             "%s: half_bins * bin = %lld * %lld samples on each side (below 2^31)", who, (long long)opt->half_bins,
             (long long)opt->bin);
    HS_CHECK(opt->refractory >= 0, HMMSORT_EINVAL, "%s: refractory = %lld", who, (long long)opt->refractory);
    HS_CHECK(opt->coincidence >= 0, HMMSORT_EINVAL, "%s: coincidence = %lld", who, (long long)opt->coincidence);
    const int64_t entries = U * U * 2 * opt->half_bins;
    HS_CHECK(entries <= (1ll << 28), HMMSORT_EUNSUP, "%s: %lld correlogram entries (U * U * 2 * half_bins = %lld * %lld "
             "* %lld; at most 2^28)", who, (long long)entries, (long long)U, (long long)U,
             (long long)(2 * opt->half_bins));
    return HMMSORT_OK;
}

int dev_correlograms(int64_t U, const int64_t *d_times, const int64_t *offs, const hmmsort_ccg_opt *opt,
                     const hmmsort_ccg_out *out, hipStream_t st)
{
    const int64_t nb = 2 * opt->half_bins;
    std::vector<int32_t> tile_u;
    std::vector<int64_t> tile_s;
    for (int64_t u = 0; u < U; u++) {
        const int64_t n = offs[u + 1] - offs[u];
        HS_CHECK(n >= 0, HMMSORT_EINVAL, "correlograms: unit %lld has %lld entries", (long long)u, (long long)n);
        out->n[u] = n;
        for (int64_t s = 0; s < n; s += kCcgTile) tile_u.push_back((int32_t)u), tile_s.push_back(s);
    }
    const int64_t ntiles = (int64_t)tile_u.size();
    if (ntiles == 0) {   // no spike at all: nothing is launched
        if (out->ccg) std::fill(out->ccg, out->ccg + U * U * nb, (int64_t)0);
        if (out->viol) std::fill(out->viol, out->viol + U, (int64_t)0);
        if (out->coinc) std::fill(out->coinc, out->coinc + U * U, (int64_t)0);
        return HMMSORT_OK;
    }
    if (!(out->ccg || out->viol || out->coinc)) return HMMSORT_OK;
    HS_CHECK(ntiles <= 0x7fffffffll, HMMSORT_EUNSUP, "correlograms: %lld tiles of %d spikes", (long long)ntiles,
             kCcgTile);
    DevBuf doff, dtu, dts, dccg, dviol, dcoinc;
    int rc;
    if ((rc = doff.alloc((U + 1) * sizeof(int64_t))) || (rc = dtu.alloc(ntiles * sizeof(int32_t))) ||
        (rc = dts.alloc(ntiles * sizeof(int64_t))) || (out->ccg && (rc = dccg.alloc(U * U * nb * sizeof(int64_t)))) ||
        (out->viol && (rc = dviol.alloc(U * sizeof(int64_t)))) ||
        (out->coinc && (rc = dcoinc.alloc(U * U * sizeof(int64_t)))))
        return rc;
    HS_HIP(hipMemcpyAsync(doff.p, offs, (U + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemcpyAsync(dtu.p, tile_u.data(), ntiles * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemcpyAsync(dts.p, tile_s.data(), ntiles * sizeof(int64_t), hipMemcpyHostToDevice, st));
    CcgArgs A;
    A.t = d_times, A.off = doff.as<int64_t>(), A.tile_u = dtu.as<int32_t>(), A.tile_s = dts.as<int64_t>();
    A.U = (int)U, A.nbins = (int)nb;
    A.b = (uint32_t)opt->bin, A.W = (uint32_t)(opt->half_bins * opt->bin);
    A.shift = -1, A.recip = 0;
    if ((A.b & (A.b - 1)) == 0) {
        A.shift = 0;
        while ((1u << A.shift) < A.b) A.shift++;
    } else {
        A.recip = (uint32_t)((1ull << 32) / A.b);
    }
    A.r = std::min<int64_t>(opt->refractory, 2 * kCcgMaxTime), A.c = std::min<int64_t>(opt->coincidence, 2 * kCcgMaxTime);
    A.ccg = dccg.as<unsigned long long>(), A.viol = dviol.as<unsigned long long>();
    A.coinc = dcoinc.as<unsigned long long>();
    const dim3 pairs((unsigned)ntiles, (unsigned)U);
    if (out->ccg) {
        HS_HIP(hipMemsetAsync(dccg.p, 0, U * U * nb * sizeof(int64_t), st));
        hipLaunchKernelGGL(k_ccg_hist, pairs, dim3(kCcgTile), 0, st, A);
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(out->ccg, dccg.p, U * U * nb * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (out->coinc) {
        HS_HIP(hipMemsetAsync(dcoinc.p, 0, U * U * sizeof(int64_t), st));
        hipLaunchKernelGGL(k_ccg_coinc, pairs, dim3(kCcgTile), 0, st, A);
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(out->coinc, dcoinc.p, U * U * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (out->viol) {
        HS_HIP(hipMemsetAsync(dviol.p, 0, U * sizeof(int64_t), st));
        hipLaunchKernelGGL(k_ccg_viol, dim3((unsigned)ntiles), dim3(kCcgTile), 0, st, A);
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(out->viol, dviol.p, U * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    HS_HIP(hipStreamSynchronize(st));   // the tables die with this frame
    return HMMSORT_OK;
}

}  // namespace hmmsort
