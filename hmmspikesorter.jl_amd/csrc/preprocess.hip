// Front end for raw recordings (hmmsort_preprocess / hmmsort_preprocess_device, include/hmmsort.h): a
// zero-phase linear-phase FIR filter per channel, then a common reference (median or mean) per sample across a group
// of channels.  The raw block is read once from device memory in its own type and layout; the result is the fp64
// channel-major [C][T] array the batched plans, fit_channels and the template seed take.
//
// Every output is the work of one thread in a fixed order, with every multiplication and addition rounded on its own
// (no fused multiply-add, no floating-point atomics), so the result is a fixed function of the input that
// tests/preprocess_model.py reproduces bit for bit, whatever the launch geometry.
//
//   acc = taps[0] * x[t];  for j = 1..P ascending:  acc = acc + taps[j] * (x[t-j] + x[t+j]);   x mirrored about its
//   end samples without repeating them (x[-i] = x[i], x[T-1+i] = x[T-1-i]; T >= P + 1).
#include <algorithm>
#include <map>
#include <vector>

#include "wave_common.h"   // wave_lds_order

#pragma clang fp contract(off)

namespace hmmsort {
namespace {

constexpr int kPreThreads = 256, kPreR = 4, kPreTile = kPreThreads * kPreR;
constexpr int kPreMaxCB = 16;                    // channels of a sample-major slab
constexpr size_t kPreLdsBudget = 64 * 1024;      // what a slab may take while one channel's tile needs less
constexpr int kRefThreads = 256, kRefLdsThreads = 64;

// halo rounded up to whole groups of R samples, so that a thread's samples start a padded group
inline int pre_halo(int P) { return (P + kPreR - 1) / kPreR * kPreR; }
// doubles of one channel's staged tile: n = tile + 2 halo samples, one pad slot per R (p(i) = i + i / R); odd, so
// that the rows of a slab start on different banks
inline int pre_npad(int P)
{
    const int n = kPreTile + 2 * pre_halo(P);
    return (n + n / kPreR + 2) | 1;
}
inline size_t pre_lds(int P, int CB)
{
    return ((size_t)CB * pre_npad(P) + kPreTile + kPreTile / kPreR + 1) * sizeof(double);
}

// k_pre_fir: 256 threads x R consecutive outputs of one channel; grid (tiles, channel blocks).  The tile with its
// halo is staged in LDS already widened, mirror indices resolved there, so the tap loop has no branch and no clamp.
// A thread keeps two sliding windows in registers, one moving right (a) and one moving left (b): per block of R lags
// it reads R new samples for each (one LDS read per window and lag), and the R taps of the block are wave-uniform
// scalar loads; both are fetched one block ahead of their use.  `taps` holds P + 1 values and zeros up to a whole
// block beyond.  LAYOUT 1 (sample-major) stages a slab of CB channels with consecutive lanes on consecutive
// addresses and then filters the channels one after the other; LAYOUT 0 has CB = 1.  Loads are of single elements:
// nothing is assumed about alignment beyond the element size.  Results leave through LDS, wave by wave, so that every
// global store is a full row segment.  Row c of `out` is channel c of `in`, for c < nch <= C.
template <typename SRC, int LAYOUT>
__global__ __launch_bounds__(kPreThreads) void k_pre_fir(const SRC *__restrict__ in, int64_t T, int64_t C, int nch,
                                                         const double *__restrict__ taps, int P, int CB,
                                                         double *__restrict__ out)
{
    constexpr int R = kPreR, TILE = kPreTile;
    extern __shared__ __attribute__((aligned(16))) double ly[];
    const int tid = threadIdx.x;
    const int Ph = (P + R - 1) / R * R, n = TILE + 2 * Ph, npad = (n + n / R + 2) | 1;
    const int64_t t0 = (int64_t)blockIdx.x * TILE;
    const int c0 = blockIdx.y * CB;
    const int cbn = nch - c0 < CB ? nch - c0 : CB;
    double *lo = ly + (size_t)CB * npad;   // TILE results, padded
    auto pad = [](int i) { return i + i / R; };
    // sample of the recording behind slot i; slots beyond the true halo (never used in arithmetic) are clamped
    auto src = [&](int i) {
        int64_t u = t0 - Ph + i;
        u = u < 0 ? -u : u;
        u = u >= T ? 2 * (T - 1) - u : u;
        return u < 0 ? (int64_t)0 : u;
    };
    {
        // S loads of a thread leave before the first one is waited for; unconditional, from a clamped slot
        constexpr int S = 8;
        const int total = n * cbn;
        for (int e0 = tid; e0 < total; e0 += S * kPreThreads) {
            SRC v[S];
            int slot[S];
#pragma unroll
            for (int q = 0; q < S; q++) {
                const int e = e0 + q * kPreThreads < total ? e0 + q * kPreThreads : total - 1;
                if (LAYOUT == 0) {
                    v[q] = in[(int64_t)c0 * T + src(e)];
                    slot[q] = pad(e);
                } else {
                    const int i = e / cbn, cb = e - i * cbn;
                    v[q] = in[src(i) * C + (c0 + cb)];
                    slot[q] = cb * npad + pad(i);
                }
            }
#pragma unroll
            for (int q = 0; q < S; q++)
                if (e0 + q * kPreThreads < total) ly[slot[q]] = (double)v[q];
        }
    }
    __syncthreads();

    const int nblk = Ph / R, nfull = P / R, rem = P - nfull * R;
    const int lane = tid & 63, seg = (tid >> 6) * (64 * R);
    const double h0 = taps[0];
    for (int cb = 0; cb < cbn; cb++) {
        // group g holds samples R g .. R g + R - 1 of the staged row at slots (R + 1) g ..; the thread's own is g0
        const double *x = ly + cb * npad + (R + 1) * (Ph / R + tid);
        double acc[R], a[2 * R - 1], b[2 * R - 1], na[R], nb[R], tn[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double xr = x[r];
            acc[r] = h0 * xr;
            if (r > 0) a[r - 1] = xr;            // a[i] = x[c0 + j0 + 1 + i]
            if (r < R - 1) b[R + r] = xr;        // b[i] = x[c0 - j0 - R + i]
        }
        if (nblk > 0) {
#pragma unroll
            for (int q = 0; q < R; q++) {
                na[q] = x[(R + 1) + q];
                nb[q] = x[-(R + 1) + q];
                tn[q] = taps[1 + q];
            }
        }
        for (int m = 0; m < nfull; m++) {
            double tj[R];
#pragma unroll
            for (int q = 0; q < R; q++) {
                a[R - 1 + q] = na[q];
                b[q] = nb[q];
                tj[q] = tn[q];
            }
            const int mp = m + 1 < nblk ? m + 1 : m;   // the block after this one, fetched now
#pragma unroll
            for (int q = 0; q < R; q++) {
                na[q] = x[(R + 1) * (mp + 1) + q];
                nb[q] = x[-(R + 1) * (mp + 1) + q];
                tn[q] = taps[R * mp + 1 + q];
            }
#pragma unroll
            for (int q = 0; q < R; q++)
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] = acc[r] + tj[q] * (b[r + R - 1 - q] + a[r + q]);
#pragma unroll
            for (int i = 0; i < R - 1; i++) {
                a[i] = a[R + i];
                b[R + i] = b[i];
            }
        }
        if (rem > 0) {   // the last P mod R lags
#pragma unroll
            for (int q = 0; q < R; q++) {
                a[R - 1 + q] = na[q];
                b[q] = nb[q];
            }
#pragma unroll
            for (int q = 0; q < R - 1; q++)
                if (q < rem) {
#pragma unroll
                    for (int r = 0; r < R; r++) acc[r] = acc[r] + tn[q] * (b[r + R - 1 - q] + a[r + q]);
                }
        }
        // thread-major in, time-major out: a wave's 64 R results are one contiguous segment, staged in the slots its
        // own lanes own, so the order of the wave's own LDS accesses is all that is needed
        wave_lds_order();
#pragma unroll
        for (int r = 0; r < R; r++) lo[(R + 1) * tid + r] = acc[r];
        wave_lds_order();
        double *dst = out + (int64_t)(c0 + cb) * T;
#pragma unroll
        for (int q = 0; q < R; q++) {
            const int i = seg + lane + 64 * q;
            const double o = lo[pad(i)];
            if (t0 + i < T) dst[t0 + i] = o;
        }
    }
}

constexpr int kRefMedian = HMMSORT_REF_MEDIAN, kRefMean = HMMSORT_REF_MEAN;

// middle value of v[0..G) by rank: v_i has rank #{j : v_j < v_i or (v_j == v_i and j < i)}, a permutation of 0..G-1
// for ordered values, so exactly one entry has each middle rank, ties included
template <int GT, typename Get>
__device__ __forceinline__ double pre_median(Get get, int G)
{
    const int k1 = (G - 1) / 2, k2 = G / 2;
    double lo = 0.0, hi = 0.0;
#pragma unroll
    for (int i = 0; i < GT; i++) {
        if (i < G) {
            const double vi = get(i);
            int rank = 0;
#pragma unroll
            for (int j = 0; j < GT; j++)
                if (j < G) {
                    const double vj = get(j);
                    rank += (j < i ? vj <= vi : vj < vi) ? 1 : 0;
                }
            lo = rank == k1 ? vi : lo;
            hi = rank == k2 ? vi : hi;
        }
    }
    return (G & 1) ? lo : (lo + hi) * 0.5;
}

// k_pre_ref: one thread per sample; the column of the group's G <= GT channels (mem, ascending) is read completely
// into registers before any of it is written, which is what makes running in place safe.  Reads and writes are
// coalesced along t for every channel.
template <int MODE, int GT>
__global__ __launch_bounds__(kRefThreads) void k_pre_ref(double *__restrict__ out, int64_t T,
                                                         const int32_t *__restrict__ mem, int G)
{
    const int64_t t = (int64_t)blockIdx.x * kRefThreads + threadIdx.x;
    if (t >= T) return;
    double v[GT];
#pragma unroll
    for (int i = 0; i < GT; i++) v[i] = i < G ? out[(int64_t)mem[i] * T + t] : 0.0;
    double m;
    if (MODE == kRefMedian) {
        m = pre_median<GT>([&](int i) { return v[i]; }, G);
    } else {
        double s = 0.0;
#pragma unroll
        for (int i = 0; i < GT; i++)
            if (i < G) s = s + v[i];
        m = s / (double)G;
    }
#pragma unroll
    for (int i = 0; i < GT; i++)
        if (i < G) out[(int64_t)mem[i] * T + t] = v[i] - m;
}

// the median of a group of up to HMMSORT_PRE_MAX_GROUP channels: the column in LDS, value i of thread l at
// s[i * 64 + l] (no bank conflict), 64 threads per workgroup so that 64 x 64 doubles fit several times per CU.  Ranks
// are counted for kRefBlock values at a time, so that a value read from LDS meets kRefBlock candidates: values before
// the block count when <=, values after it when <, and the block against itself in registers.
constexpr int kRefBlock = 8;

__global__ __launch_bounds__(kRefLdsThreads) void k_pre_ref_lds(double *__restrict__ out, int64_t T,
                                                                const int32_t *__restrict__ mem, int G)
{
    extern __shared__ __attribute__((aligned(16))) double s[];
    constexpr int B = kRefBlock;
    const int l = threadIdx.x;
    const int64_t t = (int64_t)blockIdx.x * kRefLdsThreads + l;
    if (t >= T) return;   // no barrier below: a thread reads only what it wrote
    for (int i = 0; i < G; i++) s[i * kRefLdsThreads + l] = out[(int64_t)mem[i] * T + t];
    const int k1 = (G - 1) / 2, k2 = G / 2;
    double lo = 0.0, hi = 0.0;
    for (int i0 = 0; i0 < G; i0 += B) {
        double vi[B];
        int rank[B];
#pragma unroll
        for (int q = 0; q < B; q++) {
            vi[q] = s[(i0 + q < G ? i0 + q : G - 1) * kRefLdsThreads + l];
            rank[q] = 0;
        }
        for (int j = 0; j < i0; j++) {
            const double vj = s[j * kRefLdsThreads + l];
#pragma unroll
            for (int q = 0; q < B; q++) rank[q] += vj <= vi[q] ? 1 : 0;
        }
#pragma unroll
        for (int p = 0; p < B; p++)
            if (i0 + p < G) {
#pragma unroll
                for (int q = 0; q < B; q++)
                    if (p != q) rank[q] += (p < q ? vi[p] <= vi[q] : vi[p] < vi[q]) ? 1 : 0;
            }
        for (int j = i0 + B; j < G; j++) {
            const double vj = s[j * kRefLdsThreads + l];
#pragma unroll
            for (int q = 0; q < B; q++) rank[q] += vj < vi[q] ? 1 : 0;
        }
#pragma unroll
        for (int q = 0; q < B; q++)
            if (i0 + q < G) {
                lo = rank[q] == k1 ? vi[q] : lo;
                hi = rank[q] == k2 ? vi[q] : hi;
            }
    }
    const double m = (G & 1) ? lo : (lo + hi) * 0.5;
    for (int i = 0; i < G; i++) out[(int64_t)mem[i] * T + t] = s[i * kRefLdsThreads + l] - m;
}

// the mean of a group of any size: the column is summed in channel order, then read again and written
__global__ __launch_bounds__(kRefThreads) void k_pre_mean_any(double *__restrict__ out, int64_t T,
                                                              const int32_t *__restrict__ mem, int G)
{
    const int64_t t = (int64_t)blockIdx.x * kRefThreads + threadIdx.x;
    if (t >= T) return;
    double s = 0.0;
    for (int i = 0; i < G; i++) s = s + out[(int64_t)mem[i] * T + t];
    const double m = s / (double)G;
    for (int i = 0; i < G; i++) {
        double *p = out + (int64_t)mem[i] * T + t;
        *p = *p - m;
    }
}

template <typename SRC>
int launch_fir(const SRC *d_in, int layout, int64_t C, int64_t T, int nch, const double *d_taps, int P, double *d_out,
               hipStream_t st)
{
    int CB = 1;
    if (layout == HMMSORT_LAYOUT_SAMPLE_MAJOR) {
        const size_t one = pre_lds(P, 1), row = (size_t)pre_npad(P) * sizeof(double);
        if (one < kPreLdsBudget) CB = 1 + (int)((kPreLdsBudget - one) / row);
        CB = std::min(std::min(CB, kPreMaxCB), nch);
    }
    const size_t lds = pre_lds(P, CB);
    const dim3 grid((unsigned)((T + kPreTile - 1) / kPreTile), (unsigned)((nch + CB - 1) / CB));
    auto go = [&](auto kern) -> int {
        if (lds > 64 * 1024)
            HS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, grid, dim3(kPreThreads), lds, st, d_in, T, C, nch, d_taps, P, CB, d_out);
        HS_HIP(hipGetLastError());
        return HMMSORT_OK;
    };
    return layout == HMMSORT_LAYOUT_SAMPLE_MAJOR ? go(k_pre_fir<SRC, 1>) : go(k_pre_fir<SRC, 0>);
}

template <int MODE>
int launch_ref(double *d_out, int64_t T, const int32_t *d_mem, int G, hipStream_t st)
{
    const dim3 grid((unsigned)((T + kRefThreads - 1) / kRefThreads));
    if (G <= 4)
        hipLaunchKernelGGL((k_pre_ref<MODE, 4>), grid, dim3(kRefThreads), 0, st, d_out, T, d_mem, G);
    else if (G <= 8)
        hipLaunchKernelGGL((k_pre_ref<MODE, 8>), grid, dim3(kRefThreads), 0, st, d_out, T, d_mem, G);
    else if (G <= 16)
        hipLaunchKernelGGL((k_pre_ref<MODE, 16>), grid, dim3(kRefThreads), 0, st, d_out, T, d_mem, G);
    else if (MODE == kRefMean)
        hipLaunchKernelGGL(k_pre_mean_any, grid, dim3(kRefThreads), 0, st, d_out, T, d_mem, G);
    else
        hipLaunchKernelGGL(k_pre_ref_lds, dim3((unsigned)((T + kRefLdsThreads - 1) / kRefLdsThreads)),
                           dim3(kRefLdsThreads), (size_t)G * kRefLdsThreads * sizeof(double), st, d_out, T, d_mem, G);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

size_t sample_bytes(int sample_type)
{
    switch (sample_type) {
    case HMMSORT_SAMPLES_I16: return 2;
    case HMMSORT_SAMPLES_I32: return 4;
    case HMMSORT_SAMPLES_F32: return 4;
    case HMMSORT_SAMPLES_F64: return 8;
    default: return 0;
    }
}

}  // namespace

int pre_resolve(const char *who, const void *in, int sample_type, int layout, int64_t C, int64_t T,
                const hmmsort_pre_opt *opt, const double *out, bool host_form, PrePlan *p)
{
    HS_CHECK(in, HMMSORT_EINVAL, "%s: null input block (in)", who);
    HS_CHECK(out, HMMSORT_EINVAL, "%s: null output array (out)", who);
    HS_CHECK(C >= 1 && C <= HMMSORT_PRE_MAX_CHANNELS, HMMSORT_EINVAL, "%s: C = %lld outside 1 .. %d", who, (long long)C,
             HMMSORT_PRE_MAX_CHANNELS);
    HS_CHECK(T >= 1 && T <= (1LL << 36), HMMSORT_EINVAL, "%s: T = %lld outside 1 .. 2^36", who, (long long)T);
    HS_CHECK(sample_bytes(sample_type) > 0, HMMSORT_EINVAL, "%s: unknown sample_type %d", who, sample_type);
    HS_CHECK(layout == HMMSORT_LAYOUT_CHANNEL_MAJOR || layout == HMMSORT_LAYOUT_SAMPLE_MAJOR, HMMSORT_EINVAL,
             "%s: unknown layout %d", who, layout);
    p->half = 0;
    p->taps = nullptr;
    p->reference = opt ? opt->reference : HMMSORT_REF_NONE;
    p->groups.clear();
    p->keep.clear();
    HS_CHECK(p->reference == HMMSORT_REF_NONE || p->reference == HMMSORT_REF_MEDIAN ||
             p->reference == HMMSORT_REF_MEAN, HMMSORT_EINVAL, "%s: unknown reference mode %d", who, p->reference);
    if (opt && opt->taps) {
        HS_CHECK(opt->half >= 0 && opt->half <= HMMSORT_PRE_MAX_HALF, HMMSORT_EINVAL, "%s: half = %lld outside 0 .. %d",
                 who, (long long)opt->half, HMMSORT_PRE_MAX_HALF);
        HS_CHECK(T >= opt->half + 1, HMMSORT_EINVAL, "%s: T = %lld is shorter than half + 1 = %lld (the mirrored "
                 "ends need that many samples)", who, (long long)T, (long long)opt->half + 1);
        p->half = opt->half;
        p->taps = opt->taps;
    }
    int64_t rows = C;
    if (host_form && opt && (opt->keep || opt->nkeep != 0)) {
        HS_CHECK(opt->keep && opt->nkeep >= 1, HMMSORT_EINVAL, "%s: keep / nkeep = %lld: a list needs at least one "
                 "entry", who, (long long)opt->nkeep);
        for (int64_t i = 0; i < opt->nkeep; i++)
            HS_CHECK(opt->keep[i] >= 0 && opt->keep[i] < C, HMMSORT_EINVAL, "%s: keep[%lld] = %d outside 0 .. C - 1 = "
                     "%lld", who, (long long)i, (int)opt->keep[i], (long long)C - 1);
        p->keep.assign(opt->keep, opt->keep + opt->nkeep);
        rows = opt->nkeep;
    }
    {
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
        const size_t na = (size_t)C * T * sample_bytes(sample_type), nb = (size_t)rows * T * sizeof(double);
        HS_CHECK(a + na <= b || b + nb <= a, HMMSORT_EINVAL, "%s: the input block and the output array (in, out) "
                 "overlap", who);
    }
    if (p->reference != HMMSORT_REF_NONE) {
        std::map<int32_t, std::vector<int32_t>> byid;
        for (int64_t c = 0; c < C; c++) {
            const int32_t id = (opt && opt->group) ? opt->group[c] : 0;
            if (id >= 0) byid[id].push_back((int32_t)c);
        }
        for (auto &kv : byid) {
            HS_CHECK(p->reference != HMMSORT_REF_MEDIAN || kv.second.size() <= HMMSORT_PRE_MAX_GROUP, HMMSORT_EUNSUP,
                     "%s: group %d has %zu channels; the median reference takes at most %d (the mean takes any "
                     "size)", who, (int)kv.first, kv.second.size(), HMMSORT_PRE_MAX_GROUP);
            p->groups.push_back(std::move(kv.second));
        }
    }
    return HMMSORT_OK;
}

int dev_preprocess(const void *d_in, int sample_type, int layout, int64_t C, int64_t T, const PrePlan &p,
                   const std::vector<int32_t> *rows, double *d_out, hipStream_t st)
{
    const int P = (int)p.half;
    int rc;
    // taps (a whole block of zeros beyond the last) and the groups' members; blocking copies of a few kilobytes, so
    // that the host arrays need not outlive the call
    std::vector<double> taps((size_t)pre_halo(P) + 2 * kPreR + 1, 0.0);
    taps[0] = 1.0;
    if (p.taps) std::copy(p.taps, p.taps + P + 1, taps.begin());
    std::vector<int32_t> mem;
    for (const auto &g : p.groups) mem.insert(mem.end(), g.begin(), g.end());
    DevBuf b_taps, b_mem;
    if ((rc = b_taps.alloc(taps.size() * sizeof(double)))) return rc;
    HS_HIP(hipMemcpy(b_taps.p, taps.data(), taps.size() * sizeof(double), hipMemcpyHostToDevice));
    if (!mem.empty()) {
        if ((rc = b_mem.alloc(mem.size() * sizeof(int32_t)))) return rc;
        HS_HIP(hipMemcpy(b_mem.p, mem.data(), mem.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    const double *d_taps = b_taps.as<double>();
    // all C channels in one launch, or one launch per listed channel: channel k of a block is a block of one channel
    // that starts k rows (channel-major) or k samples (sample-major) further on
    auto fir = [&](auto *src) -> int {
        if (!rows) return launch_fir(src, layout, C, T, (int)C, d_taps, P, d_out, st);
        for (size_t r = 0; r < rows->size(); r++) {
            const int64_t k = (*rows)[r];
            const int rc1 = launch_fir(src + (layout == HMMSORT_LAYOUT_SAMPLE_MAJOR ? k : k * T), layout, C, T, 1, d_taps,
                                       P, d_out + (int64_t)r * T, st);
            if (rc1) return rc1;
        }
        return HMMSORT_OK;
    };
    switch (sample_type) {
    case HMMSORT_SAMPLES_I16: rc = fir((const int16_t *)d_in); break;
    case HMMSORT_SAMPLES_I32: rc = fir((const int32_t *)d_in); break;
    case HMMSORT_SAMPLES_F32: rc = fir((const float *)d_in); break;
    default: rc = fir((const double *)d_in); break;
    }
    if (rc) return rc;
    size_t off = 0;
    for (const auto &g : p.groups) {
        const int32_t *d_mem = b_mem.as<int32_t>() + off;
        rc = p.reference == HMMSORT_REF_MEDIAN ? launch_ref<kRefMedian>(d_out, T, d_mem, (int)g.size(), st)
                                               : launch_ref<kRefMean>(d_out, T, d_mem, (int)g.size(), st);
        if (rc) return rc;
        off += g.size();
    }
    HS_HIP(hipStreamSynchronize(st));
    return HMMSORT_OK;
}

}  // namespace hmmsort
