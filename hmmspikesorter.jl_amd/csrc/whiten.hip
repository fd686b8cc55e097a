// Spatial whitening (hmmsort_noise_scale_device / hmmsort_noise_cov / hmmsort_channel_mix, include/hmmsort.h; DESIGN
// 3.16) on the fp64 channel-major block [C][T] the front end writes: the noise scale of every channel, the mask of
// quiet samples, the raw first and second moments over them, and a mix of the channels through a sparse [R][M] matrix.
// The matrix itself is the host's work (api.whitening_matrix).
//
// Every floating-point result is the work of one thread in a fixed order, every multiplication and addition rounded
// on its own (no fused multiply-add, no floating-point atomics, no matrix-core instructions), so the result is a fixed
// function of the input that tests/whiten_model.py reproduces bit for bit, whatever the launch geometry.  The only
// atomics are on integers (the histogram counters of the noise scale's select, radix_select.hip).
#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "hmmsort_internal.h"

#pragma clang fp contract(off)

namespace hmmsort {
namespace {

constexpr int kWhThreads = 256;
constexpr int kMaskPer = 4, kMaskTile = kWhThreads * kMaskPer;   // samples a mask workgroup owns
constexpr int kSumTile = 256;       // samples of one partial sum: fixed, it is part of the result
constexpr int kNoLoud = 1 << 30;    // in-tile index of "no loud sample to the right"
constexpr int64_t kNoLoud64 = INT64_MAX;
constexpr size_t kPartBudget = 32u << 20;    // bytes of tile partials in flight: what a call allocates and frees
constexpr int kMixRows = 4;         // output rows a thread of the dense mix shares an LDS read among

// ---- 2. quiet mask -----------------------------------------------------------------------------------------------
// The mask is the dilation of the loud samples by `guard` either side, for any guard, from the nearest loud sample on
// each side: within the tile by scans across the lanes of a wave, beyond it from the tile records (the last loud
// sample before the tile, the first one after it).  k_wh_loud reads the block once; k_wh_scan, k_wh_quiet and
// k_wh_count touch only the records and T bytes.

// flag[t] = 1 iff some channel has !(|y[c][t]| <= thr[c]); first / last: the tile's first and last loud sample
// (kNoLoud64 / -1: none).  A thread owns samples tid + 256 q of the tile, so every read is a full row segment.
__global__ __launch_bounds__(kWhThreads) void k_wh_loud(const double *__restrict__ y, int64_t T, int C,
                                                        const double *__restrict__ thr, uint8_t *__restrict__ flag,
                                                        int64_t *__restrict__ first, int64_t *__restrict__ last)
{
    __shared__ int s_lo, s_hi;
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kMaskTile;
    if (tid == 0) {
        s_lo = kNoLoud;
        s_hi = -1;
    }
    __syncthreads();
    bool loud[kMaskPer];
#pragma unroll
    for (int q = 0; q < kMaskPer; q++) loud[q] = false;
#pragma unroll 2
    for (int c = 0; c < C; c++) {
        const double th = thr[c];
        const double *row = y + (int64_t)c * T;
#pragma unroll
        for (int q = 0; q < kMaskPer; q++) {
            const int64_t t = t0 + tid + q * kWhThreads;
            const double v = row[t < T ? t : T - 1];   // clamped: unconditional load, unused beyond the end
            loud[q] = loud[q] || !(fabs(v) <= th);
        }
    }
    int lo = kNoLoud, hi = -1;
#pragma unroll
    for (int q = 0; q < kMaskPer; q++) {
        const int i = tid + q * kWhThreads;
        if (t0 + i < T) {
            flag[t0 + i] = loud[q] ? 1 : 0;
            if (loud[q]) {
                lo = i < lo ? i : lo;
                hi = i > hi ? i : hi;
            }
        }
    }
    if (hi >= 0) {
        atomicMin(&s_lo, lo);
        atomicMax(&s_hi, hi);
    }
    __syncthreads();
    if (tid == 0) {
        first[blockIdx.x] = s_hi >= 0 ? t0 + s_lo : kNoLoud64;
        last[blockIdx.x] = s_hi >= 0 ? t0 + s_hi : (int64_t)-1;
    }
}

// in place: last[b] becomes the last loud sample before tile b, first[b] the first one after it.  One workgroup; a
// thread owns a run of consecutive tiles.
__global__ __launch_bounds__(kWhThreads) void k_wh_scan(int64_t *__restrict__ first, int64_t *__restrict__ last,
                                                        int64_t nb)
{
    __shared__ int64_t s_mx[kWhThreads], s_mn[kWhThreads];
    const int tid = threadIdx.x;
    const int64_t chunk = (nb + kWhThreads - 1) / kWhThreads;
    const int64_t b0 = tid * chunk < nb ? tid * chunk : nb, b1 = b0 + chunk < nb ? b0 + chunk : nb;
    int64_t mx = -1, mn = kNoLoud64;
    for (int64_t b = b0; b < b1; b++) {
        mx = last[b] > mx ? last[b] : mx;
        mn = first[b] < mn ? first[b] : mn;
    }
    s_mx[tid] = mx;
    s_mn[tid] = mn;
    __syncthreads();
    int64_t pre = -1, suf = kNoLoud64;
    for (int k = 0; k < tid; k++) pre = s_mx[k] > pre ? s_mx[k] : pre;
    for (int k = tid + 1; k < kWhThreads; k++) suf = s_mn[k] < suf ? s_mn[k] : suf;
    for (int64_t b = b0; b < b1; b++) {
        const int64_t v = last[b];
        last[b] = pre;
        pre = v > pre ? v : pre;
    }
    for (int64_t b = b1 - 1; b >= b0; b--) {
        const int64_t v = first[b];
        first[b] = suf;
        suf = v < suf ? v : suf;
    }
}

// flag[t]: loud on entry, quiet on return.  A workgroup reads and writes the bytes and the records of its own tile
// only; before[b] becomes the tile's number of quiet samples (one atomic counter for all tiles would serialise them).
__global__ __launch_bounds__(kWhThreads) void k_wh_quiet(uint8_t *__restrict__ flag, int64_t T, int64_t guard,
                                                         const int64_t *__restrict__ after, int64_t *before)
{
    constexpr int kWaves = kWhThreads / 64;
    __shared__ int s_wl[kWaves], s_wr[kWaves];
    __shared__ unsigned int s_cnt[kWaves];
    const int64_t pl = before[blockIdx.x], nf = after[blockIdx.x];   // read by all before the barrier below
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * kMaskTile;
    // a thread owns kMaskPer consecutive samples; the nearest loud in-tile index at or before / at or after a sample
    // comes from the thread's own samples, the lanes before / after it (wave scans) and the waves before / after
    const int base = tid * kMaskPer;
    bool f[kMaskPer];
    int tl = -1, tr = kNoLoud;   // the thread's last and first loud sample
#pragma unroll
    for (int q = 0; q < kMaskPer; q++) {
        f[q] = t0 + base + q < T && flag[t0 + base + q] != 0;
        tl = f[q] ? base + q : tl;
        tr = (f[q] && tr == kNoLoud) ? base + q : tr;
    }
    int sl = tl, sr = tr;        // inclusive over the lanes up to / from this one
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int a = __shfl_up(sl, off), b = __shfl_down(sr, off);
        sl = (lane >= off && a > sl) ? a : sl;
        sr = (lane + off < 64 && b < sr) ? b : sr;
    }
    if (lane == 63) s_wl[wave] = sl;
    if (lane == 0) s_wr[wave] = sr;
    int left = __shfl_up(sl, 1), right = __shfl_down(sr, 1);   // exclusive: the lanes before / after this one
    left = lane == 0 ? -1 : left;
    right = lane == 63 ? kNoLoud : right;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        left = (w < wave && s_wl[w] > left) ? s_wl[w] : left;
        right = (w > wave && s_wr[w] < right) ? s_wr[w] : right;
    }
    int li[kMaskPer], ri[kMaskPer];
#pragma unroll
    for (int q = 0; q < kMaskPer; q++) {
        left = f[q] ? base + q : left;
        li[q] = left;
    }
#pragma unroll
    for (int q = kMaskPer - 1; q >= 0; q--) {
        right = f[q] ? base + q : right;
        ri[q] = right;
    }
    unsigned int cnt = 0;
#pragma unroll
    for (int q = 0; q < kMaskPer; q++) {
        const int64_t t = t0 + base + q;
        if (t < T) {
            const int64_t L = li[q] >= 0 ? t0 + li[q] : pl;
            const int64_t R = ri[q] < kNoLoud ? t0 + ri[q] : nf;
            const bool quiet = (L < 0 || t - L > guard) && (R == kNoLoud64 || R - t > guard);
            flag[t] = quiet ? 1 : 0;
            cnt += quiet ? 1u : 0u;
        }
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
        unsigned int tot = 0;
        for (int w = 0; w < kWaves; w++) tot += s_cnt[w];
        before[blockIdx.x] = (int64_t)tot;
    }
}

// n_quiet = the sum of the tiles' counts (integers: any order).  One workgroup.
__global__ __launch_bounds__(kWhThreads) void k_wh_count(const int64_t *__restrict__ counts, int64_t nb,
                                                         unsigned long long *__restrict__ n_quiet)
{
    __shared__ unsigned long long s_sum[kWhThreads];
    unsigned long long sum = 0;
    for (int64_t b = threadIdx.x; b < nb; b += kWhThreads) sum += (unsigned long long)counts[b];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int off = kWhThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) s_sum[threadIdx.x] += s_sum[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_quiet = s_sum[0];
}

// ---- 3. sums -----------------------------------------------------------------------------------------------------
// A workgroup owns one tile of kSumTile samples and one pair (bi <= bj) of blocks of B = 16 RB channels; its 16 x 16
// threads keep RB x RB entries each.  The rows are staged in LDS sample-major, TS samples at a time, so that a thread's
// RB values of a sample are contiguous and all lanes read the same sample (no bank conflict; the 16 j-groups are
// distinct, the i-groups broadcast).  The quiet flags of 64 samples become one wave-uniform 64-bit mask: the loop
// visits quiet samples only, so a loud sample contributes nothing, not +0.0 * y.  part: per tile C C + C doubles,
// [s2 | s1]; entries with j >= i are complete (a diagonal block writes its lower half too, the same bits mirrored).
template <int RB>
__global__ __launch_bounds__(kWhThreads) void k_wh_sums(const double *__restrict__ y, int64_t T, int C,
                                                        const uint8_t *__restrict__ quiet, int64_t tile0,
                                                        double *__restrict__ part)
{
    constexpr int B = 16 * RB, TS = 2048 / B, LD = B + 2, NB = RB == 4 ? 2 : 4;
    __shared__ __attribute__((aligned(16))) double s_a[TS * LD];
    __shared__ __attribute__((aligned(16))) double s_b[TS * LD];
    __shared__ uint8_t s_q[kSumTile];
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15, lane = tid & 63;
    const int nb = (C + B - 1) / B;
    int bi = 0, rem = blockIdx.y;
    while (rem >= nb - bi) {
        rem -= nb - bi;
        bi++;
    }
    const int bj = bi + rem;
    const bool diag = bi == bj;
    const int64_t t0 = (tile0 + blockIdx.x) * kSumTile;
    const uint8_t myq = t0 + tid < T ? quiet[t0 + tid] : 0;
    s_q[tid] = myq;
    const int any = __syncthreads_or(myq);

    double acc[RB][RB], p1[RB];
#pragma unroll
    for (int a = 0; a < RB; a++) {
        p1[a] = 0.0;
#pragma unroll
        for (int b = 0; b < RB; b++) acc[a][b] = 0.0;
    }
    const double *sb = diag ? s_a : s_b;
    if (any) {
        for (int sub = 0; sub < kSumTile / TS; sub++) {
            if (sub) __syncthreads();   // the previous samples are consumed
#pragma unroll 4
            for (int e = tid; e < B * TS; e += kWhThreads) {
                const int row = e / TS, ts = e - row * TS;
                const int64_t t = t0 + sub * TS + ts;
                const int ci = bi * B + row, cj = bj * B + row;
                s_a[ts * LD + row] = (ci < C && t < T) ? y[(int64_t)ci * T + t] : 0.0;
                if (!diag) s_b[ts * LD + row] = (cj < C && t < T) ? y[(int64_t)cj * T + t] : 0.0;
            }
            __syncthreads();
            for (int g0 = 0; g0 < TS; g0 += 64) {
                const int n = TS - g0 < 64 ? TS - g0 : 64;
                unsigned long long m = __ballot(lane < n && s_q[sub * TS + g0 + (lane < n ? lane : 0)] != 0);
                // NB quiet samples at a time, in ascending order: their LDS reads leave together, ahead of the arithmetic
                while (m) {
                    int ts[NB], k = 0;
#pragma unroll
                    for (int q = 0; q < NB; q++) {
                        ts[q] = m ? g0 + __builtin_ctzll(m) : ts[0];
                        k += m ? 1 : 0;
                        m &= m - 1;   // 0 stays 0
                    }
                    double va[NB][RB], vb[NB][RB];
#pragma unroll
                    for (int q = 0; q < NB; q++) {
#pragma unroll
                        for (int a = 0; a < RB; a++) va[q][a] = s_a[ts[q] * LD + ti * RB + a];
#pragma unroll
                        for (int b = 0; b < RB; b++) vb[q][b] = sb[ts[q] * LD + tj * RB + b];
                    }
#pragma unroll
                    for (int q = 0; q < NB; q++) {
                        if (q < k) {
#pragma unroll
                            for (int a = 0; a < RB; a++)
#pragma unroll
                                for (int b = 0; b < RB; b++) acc[a][b] = acc[a][b] + va[q][a] * vb[q][b];
                            if (diag && tj == 0) {
#pragma unroll
                                for (int a = 0; a < RB; a++) p1[a] = p1[a] + va[q][a];
                            }
                        }
                    }
                }
            }
        }
    }
    double *rec = part + (size_t)blockIdx.x * ((size_t)C * C + C);
#pragma unroll
    for (int a = 0; a < RB; a++) {
        const int i = bi * B + ti * RB + a;
        if (i >= C) continue;
#pragma unroll
        for (int b = 0; b < RB; b++) {
            const int j = bj * B + tj * RB + b;
            if (j < C) rec[(size_t)i * C + j] = acc[a][b];
        }
        if (diag && tj == 0) rec[(size_t)C * C + i] = p1[a];
    }
}

// one lane per entry (j >= i of s2, all of s1): acc = acc + part[g] for the G tiles of this round, in tile order;
// first: acc starts from +0.0.  The chain of G dependent additions is the stage's serial part, so everything else is
// kept off it: a workgroup owns kFoldEnt consecutive entries, all its threads fetch kFoldTiles tiles of them at a time
// (128-byte segments, the next batch in flight in registers while this one is folded), and the first kFoldEnt lanes
// fold the batch out of LDS.
constexpr int kFoldEnt = 16, kFoldTiles = 256, kFoldPer = kFoldEnt * kFoldTiles / kWhThreads;

__global__ __launch_bounds__(kWhThreads) void k_wh_fold(const double *__restrict__ part, int C, int64_t G, int first,
                                                        double *__restrict__ acc)
{
    __shared__ double s_p[kFoldTiles * kFoldEnt];
    const int64_t rec = (int64_t)C * C + C;
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kFoldEnt;
    const int64_t e = e0 + tid;                                       // the entry of a folding lane
    const bool folds = tid < kFoldEnt && e < rec && !(e < (int64_t)C * C && e % C < e / C);
    double s = (folds && !first) ? acc[e] : 0.0;
    double v[kFoldPer];
    auto fetch = [&](int64_t g0) {
#pragma unroll
        for (int q = 0; q < kFoldPer; q++) {
            const int idx = tid + q * kWhThreads;
            const int64_t g = g0 + idx / kFoldEnt, ee = e0 + idx % kFoldEnt;
            v[q] = part[(g < G ? g : G - 1) * rec + (ee < rec ? ee : rec - 1)];   // clamped, unused beyond the ends
        }
    };
    fetch(0);
    for (int64_t g0 = 0; g0 < G; g0 += kFoldTiles) {
#pragma unroll
        for (int q = 0; q < kFoldPer; q++) s_p[tid + q * kWhThreads] = v[q];
        __syncthreads();
        if (g0 + kFoldTiles < G) fetch(g0 + kFoldTiles);
        if (folds) {
            // 16 partials at a time into registers, the next 16 on their way while these are added
            constexpr int U = 16;
            const int n = G - g0 < kFoldTiles ? (int)(G - g0) : kFoldTiles;
            double cur[U], nxt[U];
#pragma unroll
            for (int q = 0; q < U; q++) cur[q] = s_p[q * kFoldEnt + tid];
            for (int g = 0; g < n; g += U) {
                const int gn = g + U < kFoldTiles ? g + U : g;   // the batch after this one (any batch at the end)
#pragma unroll
                for (int q = 0; q < U; q++) nxt[q] = s_p[(gn + q) * kFoldEnt + tid];
#pragma unroll
                for (int q = 0; q < U; q++)
                    if (g + q < n) s = s + cur[q];
#pragma unroll
                for (int q = 0; q < U; q++) cur[q] = nxt[q];
            }
        }
        __syncthreads();
    }
    if (folds) acc[e] = s;
}

// ---- 4. channel mix --------------------------------------------------------------------------------------------
// A workgroup owns TT consecutive samples (a power of two, 16 .. 256) of all rows: the column tile in[.][t0 .. t0 + TT)
// is staged in LDS before the first output is written, which is what makes d_out == d_in safe.  Thread tid works on
// sample tid % TT; the 256 / TT threads of a sample share out the output rows.  WAVEROW (TT >= 64): a wave covers 64
// consecutive t of one row, so its row number is made a scalar and nbr[r][m] and w[r][m] are scalar loads; every
// global access is a full row segment.  DENSE (M == C and nbr[r][m] == m throughout): kMixRows rows per thread share
// each LDS read.
template <bool DENSE, bool WAVEROW>
__global__ __launch_bounds__(kWhThreads) void k_wh_mix(const double *in, int64_t T, int C, int R, int M, int TT,
                                                       const int32_t *__restrict__ nbr, const double *__restrict__ w,
                                                       double *out)
{
    extern __shared__ __attribute__((aligned(16))) double s_x[];   // [C][TT]
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * TT;
    const int sh = __builtin_ctz(TT);
    {
        // S loads of a thread leave before the first one is waited for; unconditional, from a clamped sample
        constexpr int S = 8;
        const int total = C * TT;
        for (int e0 = tid; e0 < total; e0 += S * kWhThreads) {
            double v[S];
#pragma unroll
            for (int q = 0; q < S; q++) {
                const int e = e0 + q * kWhThreads < total ? e0 + q * kWhThreads : total - 1;
                const int64_t t = t0 + (e & (TT - 1));
                v[q] = in[(int64_t)(e >> sh) * T + (t < T ? t : T - 1)];
            }
#pragma unroll
            for (int q = 0; q < S; q++)
                if (e0 + q * kWhThreads < total) s_x[e0 + q * kWhThreads] = v[q];
        }
    }
    __syncthreads();
    const int l = tid & (TT - 1), ng = kWhThreads >> sh;
    const int rg = WAVEROW ? __builtin_amdgcn_readfirstlane(tid >> sh) : tid >> sh;
    const int64_t t = t0 + l;
    if (DENSE) {
        for (int r0 = rg * kMixRows; r0 < R; r0 += ng * kMixRows) {
            double acc[kMixRows];
            const double *wr[kMixRows];
#pragma unroll
            for (int q = 0; q < kMixRows; q++) {
                acc[q] = 0.0;
                wr[q] = w + (size_t)(r0 + q < R ? r0 + q : R - 1) * M;
            }
            for (int m = 0; m < C; m++) {
                const double x = s_x[(m << sh) + l];
#pragma unroll
                for (int q = 0; q < kMixRows; q++) acc[q] = acc[q] + wr[q][m] * x;
            }
#pragma unroll
            for (int q = 0; q < kMixRows; q++)
                if (r0 + q < R && t < T) out[(int64_t)(r0 + q) * T + t] = acc[q];
        }
    } else {
        for (int r = rg; r < R; r += ng) {
            double acc = 0.0;
            for (int m = 0; m < M; m++) {
                const int c = nbr[(size_t)r * M + m];
                if (c >= 0) acc = acc + w[(size_t)r * M + m] * s_x[(c << sh) + l];
            }
            if (t < T) out[(int64_t)r * T + t] = acc;
        }
    }
}

// sigma of every channel into the host array (synchronises st): the lower median of |y[c][.]| by the radix select
// of radix_select.hip, all channels in one grid, slot c on row c
int run_noise_scale(const double *d_y, int64_t C, int64_t T, double *sigma, hipStream_t st)
{
    int rc;
    DevBuf b_st, b_hist;
    if ((rc = b_st.alloc(sizeof(RadixSel) * C))) return rc;
    if ((rc = b_hist.alloc(sizeof(unsigned long long) * kSelBins * C))) return rc;
    std::vector<RadixSel> h_st((size_t)C);
    for (auto &s : h_st) {
        s.prefix = 0;
        s.rank = (T - 1) / 2;
    }
    HS_HIP(hipMemsetAsync(b_hist.p, 0, b_hist.cap, st));
    HS_HIP(hipMemcpyAsync(b_st.p, h_st.data(), sizeof(RadixSel) * C, hipMemcpyHostToDevice, st));
    const int64_t per = std::max<int64_t>(1, 8192 / C);
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>((T + 8 * kWhThreads - 1) / (8 * kWhThreads), per));
    if ((rc = dev_radix_select(d_y, nullptr, T, T, (int)C, blocks, b_st.as<RadixSel>(),
                               b_hist.as<unsigned long long>(), st)))
        return rc;
    HS_HIP(hipMemcpyAsync(h_st.data(), b_st.p, sizeof(RadixSel) * C, hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    sel_sigmas(h_st.data(), C, sigma);
    return HMMSORT_OK;
}

int check_block(const char *who, const double *y, int64_t C, int64_t T)
{
    HS_CHECK(y, HMMSORT_EINVAL, "%s: null block (y)", who);
    HS_CHECK(C >= 1 && C <= HMMSORT_WHITEN_MAX_CHANNELS, HMMSORT_EINVAL, "%s: C = %lld outside 1 .. %d", who,
             (long long)C, HMMSORT_WHITEN_MAX_CHANNELS);
    HS_CHECK(T >= 1 && T <= (1LL << 36), HMMSORT_EINVAL, "%s: T = %lld outside 1 .. 2^36", who, (long long)T);
    return HMMSORT_OK;
}

}  // namespace

int wh_scale_check(const char *who, const double *y, int64_t C, int64_t T, const double *sigma)
{
    int rc = check_block(who, y, C, T);
    if (rc) return rc;
    HS_CHECK(sigma, HMMSORT_EINVAL, "%s: null output array (sigma)", who);
    return HMMSORT_OK;
}

int wh_noise_check(const char *who, const double *y, int64_t C, int64_t T, const hmmsort_noise_opt *opt,
                   const hmmsort_noise_out *out, bool host_form, NoiseParams *p)
{
    int rc = check_block(who, y, C, T);
    if (rc) return rc;
    HS_CHECK(out, HMMSORT_EINVAL, "%s: null output record (out)", who);
    HS_CHECK(out->n_quiet, HMMSORT_EINVAL, "%s: null output (out->n_quiet)", who);
    HS_CHECK(out->s1, HMMSORT_EINVAL, "%s: null output array (out->s1)", who);
    HS_CHECK(out->s2, HMMSORT_EINVAL, "%s: null output array (out->s2)", who);
    HS_CHECK(!host_form || !out->d_quiet, HMMSORT_EINVAL, "%s: out->d_quiet is device memory; the host form takes "
             "none", who);
    *p = NoiseParams();
    if (opt) {
        HS_CHECK(opt->guard <= HMMSORT_WHITEN_MAX_GUARD, HMMSORT_EINVAL, "%s: guard = %lld above %d", who,
                 (long long)opt->guard, HMMSORT_WHITEN_MAX_GUARD);
        if (opt->guard >= 0) p->guard = opt->guard;
        if (opt->thr) {
            for (int64_t c = 0; c < C; c++)
                HS_CHECK(opt->thr[c] > 0, HMMSORT_EINVAL, "%s: thr[%lld] = %g is not positive", who, (long long)c,
                         opt->thr[c]);
            p->thr = opt->thr;
        } else {
            HS_CHECK(!(opt->threshold < 0), HMMSORT_EINVAL, "%s: threshold = %g is negative", who, opt->threshold);
            if (opt->threshold == opt->threshold) p->threshold = opt->threshold;
        }
    }
    return HMMSORT_OK;
}

int wh_mix_check(const char *who, const double *in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                 const double *w, const double *out)
{
    HS_CHECK(in, HMMSORT_EINVAL, "%s: null input block (in)", who);
    HS_CHECK(out, HMMSORT_EINVAL, "%s: null output block (out)", who);
    HS_CHECK(nbr, HMMSORT_EINVAL, "%s: null channel table (nbr)", who);
    HS_CHECK(w, HMMSORT_EINVAL, "%s: null weights (w)", who);
    HS_CHECK(C >= 1 && C <= HMMSORT_WHITEN_MAX_CHANNELS, HMMSORT_EINVAL, "%s: C = %lld outside 1 .. %d", who,
             (long long)C, HMMSORT_WHITEN_MAX_CHANNELS);
    HS_CHECK(R >= 1 && R <= HMMSORT_WHITEN_MAX_CHANNELS, HMMSORT_EINVAL, "%s: R = %lld outside 1 .. %d", who,
             (long long)R, HMMSORT_WHITEN_MAX_CHANNELS);
    HS_CHECK(M >= 1 && M <= HMMSORT_WHITEN_MAX_CHANNELS, HMMSORT_EINVAL, "%s: M = %lld outside 1 .. %d", who,
             (long long)M, HMMSORT_WHITEN_MAX_CHANNELS);
    HS_CHECK(T >= 1 && T <= (1LL << 36), HMMSORT_EINVAL, "%s: T = %lld outside 1 .. 2^36", who, (long long)T);
    for (int64_t i = 0; i < R * M; i++)
        HS_CHECK(nbr[i] >= -1 && nbr[i] < C, HMMSORT_EINVAL, "%s: nbr[%lld][%lld] = %d outside -1 .. C - 1 = %lld", who,
                 (long long)(i / M), (long long)(i % M), (int)nbr[i], (long long)C - 1);
    if (in == out) {
        HS_CHECK(R == C, HMMSORT_EINVAL, "%s: in place (out == in) needs R == C (R = %lld, C = %lld)", who,
                 (long long)R, (long long)C);
    } else {
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
        const size_t na = (size_t)C * T * sizeof(double), nb = (size_t)R * T * sizeof(double);
        HS_CHECK(a + na <= b || b + nb <= a, HMMSORT_EINVAL, "%s: the input and output blocks (in, out) overlap in "
                 "part; only out == in is allowed", who);
    }
    return HMMSORT_OK;
}

int dev_noise_scale(const double *d_y, int64_t C, int64_t T, double *sigma, hipStream_t st)
{
    std::vector<double> s((size_t)C);
    int rc = run_noise_scale(d_y, C, T, s.data(), st);
    if (rc) return rc;
    std::copy(s.begin(), s.end(), sigma);
    return HMMSORT_OK;
}

int dev_noise_cov(const double *d_y, int64_t C, int64_t T, const NoiseParams &p, const hmmsort_noise_out *out,
                  hipStream_t st)
{
    int rc;
    const int nC = (int)C;
    // thresholds
    std::vector<double> sigma, thr((size_t)C);
    if (p.thr) {
        std::copy(p.thr, p.thr + C, thr.begin());
    } else {
        sigma.resize((size_t)C);
        if ((rc = run_noise_scale(d_y, C, T, sigma.data(), st))) return rc;
        for (int64_t c = 0; c < C; c++) thr[c] = p.threshold * sigma[c];
    }
    // mask
    const int64_t nmask = (T + kMaskTile - 1) / kMaskTile;
    DevBuf b_thr, b_first, b_last, b_nq, b_mask;
    if ((rc = b_thr.alloc(sizeof(double) * C))) return rc;
    if ((rc = b_first.alloc(sizeof(int64_t) * nmask))) return rc;
    if ((rc = b_last.alloc(sizeof(int64_t) * nmask))) return rc;
    if ((rc = b_nq.alloc(sizeof(unsigned long long)))) return rc;
    uint8_t *d_mask = out->d_quiet;
    if (!d_mask) {
        if ((rc = b_mask.alloc((size_t)T))) return rc;
        d_mask = b_mask.as<uint8_t>();
    }
    HS_HIP(hipMemcpyAsync(b_thr.p, thr.data(), sizeof(double) * C, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_wh_loud, dim3((unsigned)nmask), dim3(kWhThreads), 0, st, d_y, T, nC, b_thr.as<double>(), d_mask,
                       b_first.as<int64_t>(), b_last.as<int64_t>());
    hipLaunchKernelGGL(k_wh_scan, dim3(1), dim3(kWhThreads), 0, st, b_first.as<int64_t>(), b_last.as<int64_t>(), nmask);
    hipLaunchKernelGGL(k_wh_quiet, dim3((unsigned)nmask), dim3(kWhThreads), 0, st, d_mask, T, p.guard,
                       b_first.as<int64_t>(), b_last.as<int64_t>());
    hipLaunchKernelGGL(k_wh_count, dim3(1), dim3(kWhThreads), 0, st, b_last.as<int64_t>(), nmask,
                       b_nq.as<unsigned long long>());
    HS_HIP(hipGetLastError());
    // sums: rounds of G tiles, so that the partials in flight stay within kPartBudget whatever T is
    const int64_t ntiles = (T + kSumTile - 1) / kSumTile;
    const size_t rec = (size_t)C * C + C;
    const int64_t G = std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)(kPartBudget / (rec * sizeof(double)))));
    DevBuf b_part, b_acc;
    if ((rc = b_part.alloc((size_t)G * rec * sizeof(double)))) return rc;
    if ((rc = b_acc.alloc(rec * sizeof(double)))) return rc;
    const int B = C <= 16 ? 16 : (C <= 32 ? 32 : 64);
    const int nb = (int)((C + B - 1) / B);
    const unsigned npairs = (unsigned)(nb * (nb + 1) / 2);
    for (int64_t g0 = 0; g0 < ntiles; g0 += G) {
        const int64_t g = std::min<int64_t>(G, ntiles - g0);
        const dim3 grid((unsigned)g, npairs);
        if (B == 16)
            hipLaunchKernelGGL(k_wh_sums<1>, grid, dim3(kWhThreads), 0, st, d_y, T, nC, d_mask, g0, b_part.as<double>());
        else if (B == 32)
            hipLaunchKernelGGL(k_wh_sums<2>, grid, dim3(kWhThreads), 0, st, d_y, T, nC, d_mask, g0, b_part.as<double>());
        else
            hipLaunchKernelGGL(k_wh_sums<4>, grid, dim3(kWhThreads), 0, st, d_y, T, nC, d_mask, g0, b_part.as<double>());
        hipLaunchKernelGGL(k_wh_fold, dim3((unsigned)((rec + kFoldEnt - 1) / kFoldEnt)), dim3(kWhThreads), 0, st,
                           b_part.as<double>(), nC, g, (int)(g0 == 0), b_acc.as<double>());
    }
    HS_HIP(hipGetLastError());
    std::vector<double> h((size_t)rec);
    unsigned long long nq = 0;
    HS_HIP(hipMemcpyAsync(h.data(), b_acc.p, rec * sizeof(double), hipMemcpyDeviceToHost, st));
    HS_HIP(hipMemcpyAsync(&nq, b_nq.p, sizeof nq, hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < C; i++)
        for (int64_t j = i; j < C; j++) {
            out->s2[i * C + j] = h[(size_t)(i * C + j)];
            out->s2[j * C + i] = h[(size_t)(i * C + j)];
        }
    for (int64_t i = 0; i < C; i++) out->s1[i] = h[(size_t)(C * C + i)];
    *out->n_quiet = (int64_t)nq;
    if (out->sigma && !p.thr) std::copy(sigma.begin(), sigma.end(), out->sigma);
    return HMMSORT_OK;
}

int dev_channel_mix(const double *d_in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                    const double *w, double *d_out, hipStream_t st)
{
    int rc;
    DevBuf b_nbr, b_w;
    if ((rc = b_nbr.alloc(sizeof(int32_t) * R * M))) return rc;
    if ((rc = b_w.alloc(sizeof(double) * R * M))) return rc;
    // blocking copies of at most a few megabytes, so that the host arrays need not outlive the call
    HS_HIP(hipMemcpy(b_nbr.p, nbr, sizeof(int32_t) * R * M, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(b_w.p, w, sizeof(double) * R * M, hipMemcpyHostToDevice));
    bool dense = M == C;
    for (int64_t i = 0; dense && i < R * M; i++) dense = nbr[i] == (int32_t)(i % M);
    // the column tile, a power of two of samples: C rows within 32 KB (several workgroups per CU, so that one stages
    // while another computes) as long as a wave still covers one row, then within 64 KB, 16 samples at the least
    int TT = 256;
    while (TT > 64 && (size_t)C * TT * sizeof(double) > 32 * 1024) TT >>= 1;
    while (TT > 16 && (size_t)C * TT * sizeof(double) > 64 * 1024) TT >>= 1;
    const size_t lds = (size_t)C * TT * sizeof(double);
    const int64_t nt = (T + TT - 1) / TT;
    HS_CHECK(nt <= INT_MAX, HMMSORT_EUNSUP, "channel_mix: %lld sample tiles exceed a grid", (long long)nt);
    auto go = [&](auto kern) -> int {
        if (lds > 64 * 1024)
            HS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3((unsigned)nt), dim3(kWhThreads), lds, st, d_in, T, (int)C, (int)R, (int)M, TT,
                           b_nbr.as<int32_t>(), b_w.as<double>(), d_out);
        HS_HIP(hipGetLastError());
        return HMMSORT_OK;
    };
    if (TT >= 64)
        rc = dense ? go(k_wh_mix<true, true>) : go(k_wh_mix<false, true>);
    else
        rc = dense ? go(k_wh_mix<true, false>) : go(k_wh_mix<false, false>);
    if (rc) return rc;
    HS_HIP(hipStreamSynchronize(st));
    return HMMSORT_OK;
}

}  // namespace hmmsort
