// Template seed (hmmsort_seed_templates, include/hmmsort.h; DESIGN "Template seed"): approximate templates from the
// recording alone, so that training can start on the device.  Four stages, all on the caller's stream:
//   1. noise scale: the exact lower median of |y| by the radix select of radix_select.hip over the 63-bit patterns.
//   2. detection: a sample above threshold that is the extremum of its +-R window (earliest sample of a plateau).
//      One streaming pass, a tile plus R halo samples each side in LDS; per-tile counts, a scan, a compaction into
//      the ascending event list.
//   3. initial centres: the snippets at N amplitude quantiles, found by the same radix select over the events' keys
//      (N selects side by side, ties resolved by event order, i.e. by time).
//   4. Lloyd iterations: arg-min assignment, then centre sums over fixed tiles of events in time order, partials
//      folded in tile order.  No floating-point atomics: the same input gives the same bits whatever the launch
//      geometry.
// The file is compiled with -ffp-contract=off like the rest of the library: a distance is accumulated as a separate
// multiply and add per snippet sample, in ascending sample order, as the numpy model of the tests does.
#include <algorithm>
#include <cmath>
#include <limits>

#include "hmmsort_internal.h"

namespace hmmsort {
namespace {

constexpr int kSeedThreads = 256;
constexpr int kSeedWaves = kSeedThreads / 64;
constexpr int kSeedMaxBlocks = 2048;
constexpr int kDetTile = 1024;      // samples a detection workgroup owns
constexpr int kSumTile = kSeedThreads;   // events per partial centre sum: fixed, so the sum order is

static_assert(kDetTile % kSeedThreads == 0, "detection rounds");

__device__ __forceinline__ double seed_polar(double y, int pol) { return pol < 0 ? -y : (pol == 0 ? fabs(y) : y); }

// position of a flagged thread among the flagged threads of its workgroup, in thread order, and their number.
// Two barriers; s_w is kSeedWaves ints the caller provides.
__device__ __forceinline__ int block_rank(bool flag, int *s_w, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < kSeedWaves; w++) {
        if (w < wave) off += s_w[w];
        tot += s_w[w];
    }
    __syncthreads();
    *total = tot;
    return off + __popcll(b & ((1ULL << lane) - 1ULL));
}

// ---- detection -------------------------------------------------------------------------------------------------
// Workgroup b owns samples [b * kDetTile, (b + 1) * kDetTile).  v of the tile and of R samples either side goes to
// LDS; a sample is an event iff v > thr, its snippet fits the recording, every v in [t - R, t) is smaller and every
// v in (t, t + R] is no larger (windows clipped to the recording).  The threshold test comes first; only what passes
// it and its two neighbours has its window scanned, by the whole wavefront.  Two events are more than R apart, so a tile holds
// at most per_tile = (kDetTile - 1) / (R + 1) + 1 of them: tile_ev[b * per_tile ..] receives them in ascending order.
__global__ __launch_bounds__(kSeedThreads) void k_detect(const double *__restrict__ y, int64_t T, int pol, double thr,
                                                         int R, int a, int D, int per_tile,
                                                         int *__restrict__ tile_cnt, int64_t *__restrict__ tile_ev)
{
    __shared__ double s_v[kDetTile + 2 * HMMSORT_SEED_MAX_R];
    __shared__ int s_w[kSeedWaves];
    const int64_t t0 = (int64_t)blockIdx.x * kDetTile;
    for (int l = threadIdx.x; l < kDetTile + 2 * R; l += kSeedThreads) {
        const int64_t g = t0 - R + l;
        s_v[l] = (g >= 0 && g < T) ? seed_polar(y[g], pol) : 0.0;   // outside the recording: never compared
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int base = 0;
    for (int u = threadIdx.x; u < kDetTile; u += kSeedThreads) {   // same trip count for every thread
        const int64_t t = t0 + u;
        // candidates: above threshold, snippet inside the recording, and the two neighbours already agree -- a sample
        // on a flank stops here
        bool cand = false;
        if (t < T) {
            const double vt = s_v[R + u];
            cand = vt > thr && t - a >= 0 && t - a + D - 1 <= T - 1 && (t < 1 || s_v[R + u - 1] < vt) &&
                   (t + 1 > T - 1 || s_v[R + u + 1] <= vt);
        }
        // the wavefront scans each candidate's window together, 64 samples a step, instead of one lane walking it
        bool ev = false;
        unsigned long long todo = __ballot(cand);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int uc = u - lane + src;   // a wavefront's samples are consecutive
            const int64_t tc = t0 + uc;
            const double vc = s_v[R + uc];
            const int nb = (int)(tc < R ? tc : R), nf = (int)(T - 1 - tc < R ? T - 1 - tc : R);
            bool bad = false;
            for (int d = lane + 1; d <= nb; d += 64) bad |= !(s_v[R + uc - d] < vc);
            for (int d = lane + 1; d <= nf; d += 64) bad |= !(s_v[R + uc + d] <= vc);
            const bool ok = __ballot(bad) == 0;
            if (lane == src) ev = ok;
        }
        int tot;
        const int pos = base + block_rank(ev, s_w, &tot);
        if (ev && pos < per_tile) tile_ev[(int64_t)blockIdx.x * per_tile + pos] = t;
        base += tot;
    }
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = base < per_tile ? base : per_tile;
}

// exclusive scan of the tile counts by one workgroup; n_events[0] = their sum
__global__ __launch_bounds__(kSeedThreads) void k_tile_scan(const int *__restrict__ tile_cnt, int64_t ntiles,
                                                            int64_t *__restrict__ tile_off,
                                                            int64_t *__restrict__ n_events)
{
    __shared__ long long s_w[kSeedWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long base = 0;
    for (int64_t b0 = 0; b0 < ntiles; b0 += kSeedThreads) {
        const int64_t b = b0 + threadIdx.x;
        const long long c = b < ntiles ? tile_cnt[b] : 0;
        long long x = c;
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(x, d, 64);
            if (lane >= d) x += o;
        }
        if (lane == 63) s_w[wave] = x;
        __syncthreads();
        long long off = base, tot = 0;
        for (int w = 0; w < kSeedWaves; w++) {
            if (w < wave) off += s_w[w];
            tot += s_w[w];
        }
        if (b < ntiles) tile_off[b] = off + x - c;
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) n_events[0] = base;
}

// the ascending event list and the events' keys (pattern of v[t] > 0): one thread per tile
__global__ __launch_bounds__(kSeedThreads) void k_compact(const double *__restrict__ y, int pol, int64_t ntiles,
                                                          int per_tile, const int *__restrict__ tile_cnt,
                                                          const int64_t *__restrict__ tile_off,
                                                          const int64_t *__restrict__ tile_ev, int64_t E,
                                                          int64_t *__restrict__ ev_t,
                                                          unsigned long long *__restrict__ ev_key)
{
    const int64_t step = (int64_t)gridDim.x * kSeedThreads;
    for (int64_t b = (int64_t)blockIdx.x * kSeedThreads + threadIdx.x; b < ntiles; b += step) {
        const int n = tile_cnt[b];
        const int64_t off = tile_off[b];
        for (int q = 0; q < n && off + q < E; q++) {
            const int64_t t = tile_ev[b * per_tile + q];
            ev_t[off + q] = t;
            ev_key[off + q] = sel_key(seed_polar(y[t], pol));
        }
    }
}

// ---- clustering ------------------------------------------------------------------------------------------------
// centre i = the snippet of the event whose key is the slot's selected key and that has `rank` equal keys before it
// in event (= time) order.  One workgroup per centre.
__global__ __launch_bounds__(kSeedThreads) void k_seed_centres(const double *__restrict__ y,
                                                               const int64_t *__restrict__ ev_t,
                                                               const unsigned long long *__restrict__ ev_key,
                                                               int64_t E, const RadixSel *__restrict__ st, int a,
                                                               int D, double *__restrict__ c)
{
    __shared__ int s_w[kSeedWaves];
    __shared__ long long s_found;
    const unsigned long long want_key = st[blockIdx.x].prefix;
    const long long want = st[blockIdx.x].rank;
    if (threadIdx.x == 0) s_found = 0;
    long long base = 0;
    for (int64_t e0 = 0; e0 < E; e0 += kSeedThreads) {
        const int64_t e = e0 + threadIdx.x;
        const bool f = e < E && ev_key[e] == want_key;
        int tot;
        const long long pos = base + block_rank(f, s_w, &tot);
        if (f && pos == want) s_found = e;
        base += tot;
    }
    __syncthreads();
    const int64_t t = ev_t[s_found];
    for (int j = threadIdx.x; j < D; j += kSeedThreads) c[(size_t)blockIdx.x * D + j] = y[t - a + j];
}

// label[e] = arg min_i sum_j (y[t_e - a + j] - c[i][j])^2, ties to the lower i; *changed |= 1 when a label moved.
// One thread per event.  The sum runs over j in chunks of kAssignChunk: a thread issues the loads of its snippet's
// chunk together (a launch holds about one wavefront per SIMD, so nothing else hides their latency), the workgroup
// stages the centres' chunk in LDS (read back at wave-uniform addresses), then every thread accumulates in ascending
// j: the rounding is that of one plain loop over j.
constexpr int kAssignChunk = 64;

__global__ __launch_bounds__(kSeedThreads) void k_assign(const double *__restrict__ y,
                                                         const int64_t *__restrict__ ev_t, int64_t E, int N, int D,
                                                         int a, const double *__restrict__ c,
                                                         int16_t *__restrict__ labels, int *__restrict__ changed)
{
    __shared__ double s_c[HMMSORT_SEED_MAX_N * kAssignChunk];
    const int64_t e = (int64_t)blockIdx.x * kSeedThreads + threadIdx.x;
    const bool live = e < E;
    const double *s = y + (live ? ev_t[e] - a : 0);   // a dead thread loads nothing
    double acc[HMMSORT_SEED_MAX_N];
#pragma unroll
    for (int i = 0; i < HMMSORT_SEED_MAX_N; i++) acc[i] = 0.0;
    for (int j0 = 0; j0 < D; j0 += kAssignChunk) {
        const int nj = D - j0 < kAssignChunk ? D - j0 : kAssignChunk;
        double sv[kAssignChunk];
#pragma unroll
        for (int q = 0; q < kAssignChunk; q++) sv[q] = (live && q < nj) ? s[j0 + q] : 0.0;
        __syncthreads();   // the previous chunk's centres have been read
        for (int q = threadIdx.x; q < N * kAssignChunk; q += kSeedThreads) {
            const int i = q / kAssignChunk, jj = q - i * kAssignChunk;
            s_c[q] = jj < nj ? c[(size_t)i * D + j0 + jj] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kAssignChunk; q++)
            if (q < nj) {
#pragma unroll
                for (int i = 0; i < HMMSORT_SEED_MAX_N; i++)
                    if (i < N) {
                        const double d = sv[q] - s_c[i * kAssignChunk + q];
                        acc[i] = acc[i] + d * d;
                    }
            }
    }
    if (!live) return;
    double bd = acc[0];
    int bi = 0;
#pragma unroll
    for (int i = 1; i < HMMSORT_SEED_MAX_N; i++)
        if (i < N && acc[i] < bd) {
            bd = acc[i];
            bi = i;
        }
    if (labels[e] != (int16_t)bi) {
        labels[e] = (int16_t)bi;
        atomicOr(changed, 1);
    }
}

// part[tile][i][j] = sum of y[t_e - a + j] over the events e of the tile with label i, in ascending e;
// pcnt[tile][i] = how many.  grid = (event tiles, N).
__global__ __launch_bounds__(kSeedThreads) void k_centre_partial(const double *__restrict__ y,
                                                                 const int64_t *__restrict__ ev_t,
                                                                 const int16_t *__restrict__ labels, int64_t E, int D,
                                                                 int a, double *__restrict__ part,
                                                                 int *__restrict__ pcnt)
{
    __shared__ int64_t s_t[kSumTile];
    __shared__ int s_w[kSeedWaves];
    const int i = blockIdx.y, N = gridDim.y;
    const int64_t e = (int64_t)blockIdx.x * kSumTile + threadIdx.x;
    const bool f = e < E && labels[e] == (int16_t)i;
    int n;
    const int pos = block_rank(f, s_w, &n);
    if (f) s_t[pos] = ev_t[e] - a;
    __syncthreads();
    double *out = part + ((size_t)blockIdx.x * N + i) * D;
    for (int j = threadIdx.x; j < D; j += kSeedThreads) {
        double acc = 0.0;
        for (int q = 0; q < n; q++) acc = acc + y[s_t[q] + j];
        out[j] = acc;
    }
    if (threadIdx.x == 0) pcnt[(size_t)blockIdx.x * N + i] = n;
}

// the partials folded in tile order; a cluster with events gets their mean, an empty one keeps its centre.
// grid = (ceil(D / kFoldJ), N): a workgroup owns kFoldJ consecutive snippet samples of one cluster.  It brings the
// partials of kFoldTiles tiles into LDS with every load in flight at once (sixteen lanes of tiles by kFoldJ samples),
// then kFoldJ threads add them in tile order -- the order, and so the bits, of a single loop over the tiles.
constexpr int kFoldJ = 16, kFoldTiles = kSeedThreads, kFoldLanes = kSeedThreads / kFoldJ;

__global__ __launch_bounds__(kSeedThreads) void k_centre_fold(const double *__restrict__ part,
                                                              const int *__restrict__ pcnt, int64_t ntiles, int N,
                                                              int D, double *__restrict__ c,
                                                              int64_t *__restrict__ counts)
{
    __shared__ double s_p[kFoldTiles][kFoldJ];
    __shared__ int s_n[kFoldTiles];
    const int i = blockIdx.y, jj = threadIdx.x % kFoldJ, tq = threadIdx.x / kFoldJ;
    const int j = blockIdx.x * kFoldJ + jj;
    double acc = 0.0;
    long long n = 0;
    for (int64_t b0 = 0; b0 < ntiles; b0 += kFoldTiles) {
        const int nb = (int)(ntiles - b0 < kFoldTiles ? ntiles - b0 : kFoldTiles);
        double v[kFoldTiles / kFoldLanes];
#pragma unroll
        for (int q = 0; q < kFoldTiles / kFoldLanes; q++) {
            const int b = tq + kFoldLanes * q;
            v[q] = (b < nb && j < D) ? part[((size_t)(b0 + b) * N + i) * D + j] : 0.0;
        }
        const int m = (int)threadIdx.x < nb ? pcnt[(size_t)(b0 + threadIdx.x) * N + i] : 0;
        __syncthreads();   // the previous chunk has been added
#pragma unroll
        for (int q = 0; q < kFoldTiles / kFoldLanes; q++) s_p[tq + kFoldLanes * q][jj] = v[q];
        s_n[threadIdx.x] = m;
        __syncthreads();
        if (threadIdx.x < kFoldJ)
            for (int b = 0; b < nb; b++) {
                acc = acc + s_p[b][threadIdx.x];
                n += s_n[b];
            }
    }
    if (threadIdx.x < kFoldJ && j < D) {   // here jj == threadIdx.x
        if (n > 0) c[(size_t)i * D + j] = acc / (double)n;
        if (j == 0) counts[i] = n;
    }
}

inline int seed_blocks(int64_t n)
{
    return (int)std::max<int64_t>(1, std::min<int64_t>((n + kSeedThreads - 1) / kSeedThreads, kSeedMaxBlocks));
}

}  // namespace

int seed_resolve(int64_t T, int64_t N, int64_t K, const hmmsort_seed_opt *opt, const hmmsort_seed_out *out,
                 SeedParams *p)
{
    HS_CHECK(out && out->mu && out->sigma && out->lp && out->counts, HMMSORT_EINVAL,
             "seed_templates: mu, sigma, lp and counts are required");
    HS_CHECK(K >= 2 && K <= HMMSORT_SEED_MAX_K, HMMSORT_EINVAL, "seed_templates: K = %lld outside 2 .. %d",
             (long long)K, HMMSORT_SEED_MAX_K);
    HS_CHECK(N >= 1 && N <= HMMSORT_SEED_MAX_N, HMMSORT_EINVAL, "seed_templates: N = %lld outside 1 .. %d",
             (long long)N, HMMSORT_SEED_MAX_N);
    HS_CHECK(T >= K && T <= (1LL << 40), HMMSORT_EINVAL, "seed_templates: T = %lld outside K .. 2^40", (long long)T);
    HS_CHECK(out->cap >= 0, HMMSORT_EINVAL, "seed_templates: cap = %lld", (long long)out->cap);
    const int64_t D = K - 1;
    p->threshold = (opt && opt->threshold == opt->threshold) ? opt->threshold : 4.0;
    p->sigma = opt ? opt->sigma : 0.0;
    p->polarity = opt ? opt->polarity : 0;
    p->align = (opt && opt->align >= 0) ? opt->align : D / 3;
    p->refractory = (opt && opt->refractory >= 0) ? opt->refractory : K - 1;
    p->max_iters = (opt && opt->max_iters > 0) ? opt->max_iters : 20;
    HS_CHECK(p->polarity >= -1 && p->polarity <= 1, HMMSORT_EINVAL, "seed_templates: polarity %d outside -1 .. 1",
             p->polarity);
    HS_CHECK(p->align < D, HMMSORT_EINVAL, "seed_templates: align = %lld must be below K - 1 = %lld",
             (long long)p->align, (long long)D);
    HS_CHECK(p->refractory >= 1 && p->refractory <= HMMSORT_SEED_MAX_R, HMMSORT_EINVAL,
             "seed_templates: refractory = %lld outside 1 .. %d", (long long)p->refractory, HMMSORT_SEED_MAX_R);
    return HMMSORT_OK;
}

int dev_seed_templates(const double *d_y, int64_t T, int64_t N, int64_t K, const SeedParams &p, hmmsort_seed_out *out,
                       hipStream_t st)
{
    const int D = (int)(K - 1), R = (int)p.refractory, a = (int)p.align, n = (int)N;
    int rc;
    // E = 0 until shown otherwise
    for (int64_t i = 0; i < K * N; i++) out->mu[i] = 0.0;
    for (int64_t i = 0; i < N; i++) {
        out->counts[i] = 0;
        out->lp[i] = -std::numeric_limits<double>::infinity();
    }
    if (out->n_events) *out->n_events = 0;
    if (out->iters) *out->iters = 0;

    DevBuf b_st, b_hist;
    if ((rc = b_st.alloc(sizeof(RadixSel) * HMMSORT_SEED_MAX_N))) return rc;
    if ((rc = b_hist.alloc(sizeof(unsigned long long) * kSelBins * HMMSORT_SEED_MAX_N))) return rc;
    RadixSel *d_st = b_st.as<RadixSel>();
    unsigned long long *d_hist = b_hist.as<unsigned long long>();
    HS_HIP(hipMemsetAsync(d_hist, 0, b_hist.cap, st));
    RadixSel h_st[HMMSORT_SEED_MAX_N];

    // 1. noise scale
    double sigma_n = p.sigma;
    if (!(sigma_n > 0)) {
        h_st[0].prefix = 0;
        h_st[0].rank = (T - 1) / 2;
        HS_HIP(hipMemcpyAsync(d_st, h_st, sizeof(RadixSel), hipMemcpyHostToDevice, st));
        if ((rc = dev_radix_select(d_y, nullptr, 0, T, 1, seed_blocks(T), d_st, d_hist, st))) return rc;
        HS_HIP(hipMemcpyAsync(h_st, d_st, sizeof(RadixSel), hipMemcpyDeviceToHost, st));
        HS_HIP(hipStreamSynchronize(st));
        sel_sigmas(h_st, 1, &sigma_n);
    }
    *out->sigma = sigma_n;
    const double thr = p.threshold * sigma_n;

    // 2. detection
    const int64_t ntiles = (T + kDetTile - 1) / kDetTile;
    const int per_tile = (kDetTile - 1) / (R + 1) + 1;
    DevBuf b_cnt, b_off, b_tev, b_ne;
    if ((rc = b_cnt.alloc(sizeof(int) * ntiles))) return rc;
    if ((rc = b_off.alloc(sizeof(int64_t) * ntiles))) return rc;
    if ((rc = b_tev.alloc(sizeof(int64_t) * ntiles * per_tile))) return rc;
    if ((rc = b_ne.alloc(sizeof(int64_t)))) return rc;
    hipLaunchKernelGGL(k_detect, dim3((unsigned)ntiles), dim3(kSeedThreads), 0, st, d_y, T, p.polarity, thr, R, a, D,
                       per_tile, b_cnt.as<int>(), b_tev.as<int64_t>());
    hipLaunchKernelGGL(k_tile_scan, dim3(1), dim3(kSeedThreads), 0, st, b_cnt.as<int>(), ntiles, b_off.as<int64_t>(),
                       b_ne.as<int64_t>());
    HS_HIP(hipGetLastError());
    int64_t E = 0;
    HS_HIP(hipMemcpyAsync(&E, b_ne.p, sizeof E, hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    HS_CHECK(E >= 0 && E <= T / (R + 1) + 1, HMMSORT_EHIP, "seed_templates: %lld events exceed the bound",
             (long long)E);
    if (out->n_events) *out->n_events = E;
    if (E == 0) return HMMSORT_OK;

    DevBuf b_evt, b_key, b_lab, b_c, b_counts, b_chg, b_part, b_pcnt;
    const int64_t etiles = (E + kSumTile - 1) / kSumTile;
    if ((rc = b_evt.alloc(sizeof(int64_t) * E))) return rc;
    if ((rc = b_key.alloc(sizeof(unsigned long long) * E))) return rc;
    if ((rc = b_lab.alloc(sizeof(int16_t) * E))) return rc;
    if ((rc = b_c.alloc(sizeof(double) * N * D))) return rc;
    if ((rc = b_counts.alloc(sizeof(int64_t) * N))) return rc;
    if ((rc = b_chg.alloc(sizeof(int)))) return rc;
    if ((rc = b_part.alloc(sizeof(double) * etiles * N * D))) return rc;
    if ((rc = b_pcnt.alloc(sizeof(int) * etiles * N))) return rc;
    int64_t *d_evt = b_evt.as<int64_t>();
    unsigned long long *d_key = b_key.as<unsigned long long>();
    int16_t *d_lab = b_lab.as<int16_t>();
    double *d_c = b_c.as<double>();
    hipLaunchKernelGGL(k_compact, dim3(seed_blocks(ntiles)), dim3(kSeedThreads), 0, st, d_y, p.polarity, ntiles,
                       per_tile, b_cnt.as<int>(), b_off.as<int64_t>(), b_tev.as<int64_t>(), E, d_evt, d_key);

    // 3. initial centres: the snippets at ranks ((2i + 1) E) / (2N) of the order by (v, t)
    for (int i = 0; i < n; i++) {
        h_st[i].prefix = 0;
        h_st[i].rank = std::min<int64_t>(E - 1, ((2 * (int64_t)i + 1) * E) / (2 * N));
    }
    HS_HIP(hipMemcpyAsync(d_st, h_st, sizeof(RadixSel) * n, hipMemcpyHostToDevice, st));
    if ((rc = dev_radix_select(nullptr, d_key, 0, E, n, seed_blocks(E), d_st, d_hist, st))) return rc;
    hipLaunchKernelGGL(k_seed_centres, dim3(n), dim3(kSeedThreads), 0, st, d_y, d_evt, d_key, E, d_st, a, D, d_c);

    // 4. Lloyd iterations; no event carries label -1, so the first assignment changes every label
    HS_HIP(hipMemsetAsync(d_lab, 0xff, sizeof(int16_t) * E, st));
    int64_t iters = 0;
    for (;;) {
        int changed = 0;
        HS_HIP(hipMemsetAsync(b_chg.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_assign, dim3((unsigned)etiles), dim3(kSeedThreads), 0, st, d_y, d_evt, E, n, D, a, d_c,
                           d_lab, b_chg.as<int>());
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(&changed, b_chg.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HS_HIP(hipStreamSynchronize(st));
        iters++;
        if (!changed) break;
        hipLaunchKernelGGL(k_centre_partial, dim3((unsigned)etiles, n), dim3(kSeedThreads), 0, st, d_y, d_evt, d_lab,
                           E, D, a, b_part.as<double>(), b_pcnt.as<int>());
        hipLaunchKernelGGL(k_centre_fold, dim3((D + kFoldJ - 1) / kFoldJ, n), dim3(kSeedThreads), 0, st,
                           b_part.as<double>(), b_pcnt.as<int>(), etiles, n, D, d_c, b_counts.as<int64_t>());
        HS_HIP(hipGetLastError());
        if (iters == p.max_iters) break;
    }
    if (out->iters) *out->iters = iters;

    // 5. results
    std::vector<double> c((size_t)N * D);
    HS_HIP(hipMemcpyAsync(c.data(), d_c, sizeof(double) * N * D, hipMemcpyDeviceToHost, st));
    HS_HIP(hipMemcpyAsync(out->counts, b_counts.p, sizeof(int64_t) * N, hipMemcpyDeviceToHost, st));
    const int64_t ncopy = std::min<int64_t>(E, out->cap);
    if (out->times && ncopy > 0)
        HS_HIP(hipMemcpyAsync(out->times, d_evt, sizeof(int64_t) * ncopy, hipMemcpyDeviceToHost, st));
    if (out->labels && ncopy > 0)
        HS_HIP(hipMemcpyAsync(out->labels, d_lab, sizeof(int16_t) * ncopy, hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < N; i++) {
        for (int64_t j = 0; j < D; j++) out->mu[i * K + 1 + j] = c[i * D + j];
        out->lp[i] = out->counts[i] > 0 ? std::log((double)out->counts[i] / (double)T)
                                        : -std::numeric_limits<double>::infinity();
    }
    if (out->times)
        for (int64_t e = 0; e < ncopy; e++) out->times[e] += 1;   // 1-based, like extract_spiketimes
    return HMMSORT_OK;
}

}  // namespace hmmsort
