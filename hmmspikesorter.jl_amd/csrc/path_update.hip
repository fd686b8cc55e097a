// Viterbi training (hard EM): the model re-estimated from a decoded path (hmmsort_plan_path_update,
// include/hmmsort.h).  It is update() of baumwelch.jl:205-309 with gamma and xi the indicators of the
// path, so it needs the plan's HostModel and nothing of its engine: two streaming passes over (y, x).
//   pass 1  k_pu_counts  per tile of samples, one wavefront: count and sum of y per (template, phase) of the
//                        single-active states, entry counts out of the silent state, the three diagnostics
//           k_pu_final   column sums of the tiles' tables in a fixed order; writes mu', lp', pp'
//   pass 2  k_pu_mean    per-state mean of the NEW templates, added in neuron order
//           k_pu_resid   squared residuals, per-workgroup partials by a fixed tree
//           k_pu_sigma   fixed-order sum of the partials, sqrt; hands the diagnostics to the caller
// No floating-point atomics anywhere: the result is a fixed function of (y, x, model).  One step of pass 1 is
// W = min(K-1, 64) consecutive samples, one per lane.  A template that is at phase k at sample t cannot be there
// again before t + K (it has to finish its ring and pass through its silent row), so within a step no two lanes
// address the same (template, phase) and the wavefront's table in LDS is updated with plain read-modify-write;
// the steps of a wavefront run in time order (its LDS instructions execute in program order).  A path that is not
// one of this model (counts[1] != 0) can break that argument: its sums are then unspecified, but every index is
// checked against its table before it is used.
#include <algorithm>
#include <cmath>

#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

constexpr int kPuGroup = 4096;     // (template, phase) entries one LDS pass holds: 48 KB of sums and counts
constexpr int kPuSlotLds = 1024;   // entry counters kept in LDS; a longer list counts in device memory
constexpr int kPuMinTile = 4096;   // samples per tile at least; grows with N (K-1)
constexpr int kPuResidThreads = 256;
constexpr int kPuResidChunk = 8192;
constexpr int kPuResidMaxBlocks = 2048;
constexpr int kPuInts = 4;         // per channel: counts[0..2], b, then the entry counters

struct PuGeom {
    int64_t T, tile;
    int S, N, K, NE, W, nslot, rstride, ntiles, rblocks;
};

__device__ inline long long wave_sum_ll(long long v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__device__ inline double wave_sum_f64(double v)
{
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

__global__ __launch_bounds__(64) void k_pu_counts(PuGeom g, const double *__restrict__ y,
                                                  const int16_t *__restrict__ x,
                                                  const int32_t *__restrict__ single,
                                                  const int32_t *__restrict__ slot,
                                                  const int32_t *__restrict__ in_ptr,
                                                  const int32_t *__restrict__ in_src,
                                                  double *__restrict__ part_sum, uint32_t *__restrict__ part_cnt,
                                                  unsigned long long *__restrict__ ints)
{
    extern __shared__ double s_pu[];
    const int lane = threadIdx.x, ch = blockIdx.y, S = g.S, NE = g.NE, W = g.W;
    const int G = NE < kPuGroup ? NE : kPuGroup;
    const int nsl = g.nslot <= kPuSlotLds ? g.nslot : 0;
    double *s_sum = s_pu;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_sum + G);
    uint32_t *s_ent = s_cnt + G;
    const int64_t T = g.T;
    const double *yc = y + (int64_t)ch * T;
    const int16_t *xc = x + (int64_t)ch * T;
    slot += (int64_t)ch * S;
    in_ptr += (int64_t)ch * (S + 1);
    in_src += (int64_t)ch * g.rstride;
    ints += (int64_t)ch * (kPuInts + g.nslot);
    const int64_t t0 = (int64_t)blockIdx.x * g.tile;
    const int64_t t1 = t0 + g.tile < T ? t0 + g.tile : T;
    const size_t row = ((size_t)ch * g.ntiles + blockIdx.x) * (size_t)NE;

    for (int e0 = 0; e0 == 0 || e0 < NE; e0 += kPuGroup) {
        const int ge = NE - e0 < G ? NE - e0 : G;
        const bool first = e0 == 0;   // the integer counts are taken in the first pass only
        for (int i = lane; i < ge; i += 64) s_sum[i] = 0.0, s_cnt[i] = 0u;
        if (first)
            for (int i = lane; i < nsl; i += 64) s_ent[i] = 0u;
        __syncthreads();
        long long bad0 = 0, bad1 = 0, nb = 0;
#pragma unroll 2
        for (int64_t ts = t0; ts < t1; ts += W) {
            const int64_t t = ts + lane;
            int e = -1;
            double yv = 0.0;
            if (lane < W && t < t1) {
                const int xs = (int)xc[t] - 1;
                const bool v = xs >= 0 && xs < S;
                yv = yc[t];
                if (v) e = single[xs];
                if (first) {
                    bad0 += !v;
                    if (t + 1 < T) {
                        const int xn = (int)xc[t + 1] - 1;
                        const bool vn = xn >= 0 && xn < S;
                        if (v && vn) {
                            bool found = false;
                            const int p1 = in_ptr[xn + 1];
                            for (int p = in_ptr[xn]; p < p1; p++)
                                if (in_src[p] == xs) { found = true; break; }
                            bad1 += !found;
                        }
                        if (v && xs == 0) {
                            nb++;
                            const int sl = vn ? slot[xn] : -1;
                            if (sl >= 0 && sl < g.nslot) {
                                if (nsl) atomicAdd(&s_ent[sl], 1u);
                                else atomicAdd(&ints[kPuInts + sl], 1ull);
                            }
                        }
                    }
                }
                e -= e0;
                if (e < 0 || e >= ge) e = -1;
            }
            if (e >= 0) {
                s_cnt[e] += 1u;
                s_sum[e] += yv;
            }
        }
        __syncthreads();
        for (int i = lane; i < ge; i += 64) {
            part_sum[row + e0 + i] = s_sum[i];
            part_cnt[row + e0 + i] = s_cnt[i];
        }
        if (first) {
            for (int i = lane; i < nsl; i += 64)
                if (s_ent[i]) atomicAdd(&ints[kPuInts + i], (unsigned long long)s_ent[i]);
            bad0 = wave_sum_ll(bad0);
            bad1 = wave_sum_ll(bad1);
            nb = wave_sum_ll(nb);
            if (lane == 0) {
                if (bad0) atomicAdd(&ints[0], (unsigned long long)bad0);
                if (bad1) atomicAdd(&ints[1], (unsigned long long)bad1);
                if (nb) atomicAdd(&ints[3], (unsigned long long)nb);
            }
        }
        __syncthreads();
    }
}

// blocks [0, NE): one (template, phase) each, the tiles' rows strided over the lanes and folded by a fixed tree;
// blocks from NE on: lp' and pp', one entry per lane, and the zero first row of mu'
__global__ __launch_bounds__(64) void k_pu_final(PuGeom g, const int16_t *__restrict__ x,
                                                 const double *__restrict__ part_sum,
                                                 const uint32_t *__restrict__ part_cnt,
                                                 const double *__restrict__ mu_cur,
                                                 unsigned long long *__restrict__ ints, double *__restrict__ out,
                                                 int64_t out_len)
{
    const int lane = threadIdx.x, ch = blockIdx.y, i = blockIdx.x, NE = g.NE, K = g.K, N = g.N, L = K - 1;
    out += (int64_t)ch * out_len;
    ints += (int64_t)ch * (kPuInts + g.nslot);
    if (i < NE) {
        const size_t base = (size_t)ch * g.ntiles * (size_t)NE + i;
        double s = 0.0;
        long long c = 0;
        for (int r = lane; r < g.ntiles; r += 64) {
            s += part_sum[base + (size_t)r * NE];
            c += (long long)part_cnt[base + (size_t)r * NE];
        }
        s = wave_sum_f64(s);
        c = wave_sum_ll(c);
        if (lane == 0) {
            const int l = i / L, k = i % L;
            const int idx = (k + 1) + K * l;
            if (c > 0) {
                out[idx] = s / (double)c;
            } else {   // 0/0: the row keeps the plan's value
                out[idx] = mu_cur[(int64_t)ch * K * N + idx];
                atomicAdd(&ints[2], 1ull);
            }
        }
        return;
    }
    if (i == NE)
        for (int l = lane; l < N; l += 64) out[(int64_t)K * l] = 0.0;
    const int64_t j = (int64_t)(i - NE) * 64 + lane;
    if (j < g.nslot) {
        const unsigned long long n = ints[kPuInts + j], b = ints[3];
        out[(int64_t)K * N + 1 + j] = (n == 0 || b == 0) ? -INFINITY : log((double)n) - log((double)b);
    } else if (j - g.nslot < g.S) {
        const int64_t s = j - g.nslot;
        const int x0 = (int)x[(int64_t)ch * g.T] - 1;
        out[(int64_t)K * N + 1 + g.nslot + s] = (s == x0) ? 0.0 : -INFINITY;
    }
}

__global__ __launch_bounds__(256) void k_pu_mean(PuGeom g, const int16_t *__restrict__ states,
                                                 const double *__restrict__ out, int64_t out_len,
                                                 double *__restrict__ mean)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x, ch = blockIdx.y;
    if (j >= g.S) return;
    const double *mu = out + (int64_t)ch * out_len;
    double a = 0.0;
    for (int l = 0; l < g.N; l++) {
        const int k = (int)states[l + (int64_t)g.N * j] - 1;   // 0 .. K-1 by build_host_model
        a += mu[k + (int64_t)g.K * l];
    }
    mean[(int64_t)ch * g.S + j] = a;
}

__global__ __launch_bounds__(kPuResidThreads) void k_pu_resid(PuGeom g, const double *__restrict__ y,
                                                              const int16_t *__restrict__ x,
                                                              const double *__restrict__ mean,
                                                              double *__restrict__ rpart)
{
    __shared__ double s_w[kPuResidThreads / 64];
    const int tid = threadIdx.x, ch = blockIdx.y;
    const int64_t T = g.T, chunk = (T + g.rblocks - 1) / g.rblocks;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = lo + chunk < T ? lo + chunk : T;
    const double *yc = y + (int64_t)ch * T, *mc = mean + (int64_t)ch * g.S;
    const int16_t *xc = x + (int64_t)ch * T;
    double acc = 0.0;
    for (int64_t t = lo + tid; t < hi; t += kPuResidThreads) {
        const int xs = (int)xc[t] - 1;
        if (xs >= 0 && xs < g.S) {
            const double d = yc[t] - mc[xs];
            acc += d * d;
        }
    }
    acc = wave_sum_f64(acc);
    if ((tid & 63) == 0) s_w[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double a = s_w[0];
        for (int w = 1; w < kPuResidThreads / 64; w++) a += s_w[w];
        rpart[(int64_t)ch * g.rblocks + blockIdx.x] = a;
    }
}

__global__ __launch_bounds__(64) void k_pu_sigma(PuGeom g, const double *__restrict__ rpart,
                                                 const unsigned long long *__restrict__ ints,
                                                 double *__restrict__ out, int64_t out_len,
                                                 long long *__restrict__ counts)
{
    const int lane = threadIdx.x, ch = blockIdx.x;
    ints += (int64_t)ch * (kPuInts + g.nslot);
    double s = 0.0;
    for (int r = lane; r < g.rblocks; r += 64) s += rpart[(int64_t)ch * g.rblocks + r];
    s = wave_sum_f64(s);
    if (lane == 0) {
        const double n = (double)(g.T - (int64_t)ints[0]);
        out[(int64_t)ch * out_len + (int64_t)g.K * g.N] = sqrt(s / n);
    }
    if (counts && lane < 3) counts[(int64_t)ch * 3 + lane] = (long long)ints[lane];
}

}  // namespace

// what a plan keeps for its path updates: the lookup tables of its current model(s) and the workspace
struct PathUpdateDev {
    PuGeom g{};
    std::vector<int32_t> h_single;                    // state -> (template, phase) entry: fixed by the state table
    std::vector<int32_t> h_slot, h_inptr, h_insrc;   // host images of the per-channel tables (source of the upload)
    std::vector<double> h_mu;
    hipEvent_t uploaded = nullptr;                    // behind the last upload: its host images are free again
    ~PathUpdateDev()
    {
        if (uploaded) (void)hipEventDestroy(uploaded);
    }
    DevBuf single, states, slot, inptr, insrc, mu, mean, part_sum, part_cnt, ints, rpart;
    int64_t bytes() const
    {
        return (int64_t)(single.cap + states.cap + slot.cap + inptr.cap + insrc.cap + mu.cap + mean.cap + part_sum.cap +
                         part_cnt.cap + ints.cap + rpart.cap);
    }
};

namespace {

// state -> l (K-1) + (k-2) when exactly one row l holds a phase k >= 2, else -1
void single_table(const HostModel &m, std::vector<int32_t> &tab)
{
    tab.assign(m.S, -1);
    for (int64_t j = 0; j < m.S; j++) {
        int64_t active = 0, l1 = 0;
        for (int64_t l = 0; l < m.N; l++)
            if (m.states[l + m.N * j] >= 2) active++, l1 = l;
        if (active == 1) tab[j] = (int32_t)(l1 * (m.K - 1) + (m.states[l1 + m.N * j] - 2));
    }
}

// state -> slot of the transition 1 -> state in lp': by template for plans that take ring models only (the slot of
// a template whose entry left the list stays, and stays -Inf), else list position among the transitions out of
// state 1, the first of which (1 -> 1) is dropped like xb[2:end]
void slot_table(const HostModel &m, bool by_template, int64_t nslot, const std::vector<int32_t> &single, int32_t *tab)
{
    std::fill(tab, tab + m.S, -1);
    for (int32_t p = m.out_ptr[0], i = 0; p < m.out_ptr[1]; p++, i++) {
        const int32_t d = m.out_dst[p];
        int64_t s = -1;
        if (by_template) {
            if (single[d] >= 0 && single[d] % (m.K - 1) == 0) s = single[d] / (m.K - 1);
        } else if (i >= 1) {
            s = i - 1;
        }
        if (s >= 0 && s < nslot) tab[d] = (int32_t)s;
    }
}

}  // namespace

int plan_path_update(hmmsort_plan *p, const double *d_y, const int16_t *d_x, double *d_out, int64_t *d_counts,
                     hipStream_t st)
{
    const HostModel &m0 = p->model;
    const int64_t C = p->C, S = m0.S, N = m0.N, K = m0.K, T = p->T;
    const int64_t nslot = p->eng->n_lp(), out_len = K * N + 1 + nslot + S;
    int rc;
    if (!p->pu) {
        std::shared_ptr<PathUpdateDev> d(new PathUpdateDev());
        PuGeom &g = d->g;
        g.T = T;
        g.S = (int)S, g.N = (int)N, g.K = (int)K;
        HS_CHECK(N * (K - 1) <= (int64_t)1 << 24, HMMSORT_EUNSUP, "plan_path_update: %lld x %lld template entries",
                 (long long)N, (long long)(K - 1));
        g.NE = (int)(N * (K - 1));
        g.W = (int)std::max<int64_t>(1, std::min<int64_t>(K - 1, 64));
        // a tile's table is 12 bytes per entry beside the tile's 10 bytes per sample: 16 samples per entry keep
        // the partials under a tenth of the signal
        g.tile = std::max<int64_t>(kPuMinTile, 16 * (int64_t)g.NE);
        const int64_t ntiles = (T + g.tile - 1) / g.tile;
        HS_CHECK(ntiles <= 2147483647LL / 64, HMMSORT_EUNSUP, "plan_path_update: signal too long");
        g.ntiles = (int)ntiles;
        g.rblocks = (int)std::max<int64_t>(1, std::min<int64_t>((T + kPuResidChunk - 1) / kPuResidChunk, kPuResidMaxBlocks));
        single_table(m0, d->h_single);
        const size_t npart = (size_t)C * g.ntiles * std::max(g.NE, 1);
        if ((rc = d->single.alloc(S * sizeof(int32_t))) || (rc = d->states.alloc(N * S * sizeof(int16_t))) ||
            (rc = d->slot.alloc(C * S * sizeof(int32_t))) || (rc = d->inptr.alloc(C * (S + 1) * sizeof(int32_t))) ||
            (rc = d->mu.alloc(C * K * N * sizeof(double))) || (rc = d->mean.alloc(C * S * sizeof(double))) ||
            (rc = d->part_sum.alloc(npart * sizeof(double))) || (rc = d->part_cnt.alloc(npart * sizeof(uint32_t))) ||
            (rc = d->rpart.alloc((size_t)C * g.rblocks * sizeof(double))))
            return rc;
        // once per plan, like plan creation: these two wait for their copy
        HS_HIP(hipMemcpy(d->single.p, d->h_single.data(), S * sizeof(int32_t), hipMemcpyHostToDevice));
        HS_HIP(hipMemcpy(d->states.p, m0.states.data(), N * S * sizeof(int16_t), hipMemcpyHostToDevice));
        HS_HIP(hipEventCreateWithFlags(&d->uploaded, hipEventDisableTiming));
        p->pu = d;
        p->pu_stale = true;
    }
    PathUpdateDev &d = *p->pu;
    PuGeom &g = d.g;
    if (p->pu_stale) {
        // the tables of the current model(s), built in host images the plan keeps: the copies below are enqueued,
        // not waited for.  Only the previous upload (long done in any loop) must have left the images.
        HS_HIP(hipEventSynchronize(d.uploaded));
        int64_t rmax = 1;
        for (int64_t ch = 0; ch < C; ch++) rmax = std::max(rmax, (C > 1 ? p->models[ch] : m0).R);
        g.nslot = (int)nslot;
        g.rstride = (int)rmax;
        d.h_slot.resize(C * S);
        d.h_inptr.assign(C * (S + 1), 0);
        d.h_insrc.assign(C * rmax, 0);
        d.h_mu.resize(C * K * N);
        for (int64_t ch = 0; ch < C; ch++) {
            const HostModel &m = C > 1 ? p->models[ch] : m0;
            slot_table(m, p->eng->ring_models_only(), nslot, d.h_single, d.h_slot.data() + ch * S);
            std::copy(m.in_ptr.begin(), m.in_ptr.end(), d.h_inptr.begin() + ch * (S + 1));
            std::copy(m.in_src.begin(), m.in_src.end(), d.h_insrc.begin() + ch * rmax);
            std::copy(m.mu.begin(), m.mu.end(), d.h_mu.begin() + ch * K * N);
        }
        if ((rc = d.insrc.ensure(C * rmax * sizeof(int32_t))) ||
            (rc = d.ints.ensure(C * (kPuInts + nslot) * sizeof(int64_t))))
            return rc;
        HS_HIP(hipMemcpyAsync(d.slot.p, d.h_slot.data(), d.h_slot.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(d.inptr.p, d.h_inptr.data(), d.h_inptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(d.insrc.p, d.h_insrc.data(), d.h_insrc.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(d.mu.p, d.h_mu.data(), d.h_mu.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HS_HIP(hipEventRecord(d.uploaded, st));
        p->pu_stale = false;
    }
    unsigned long long *ints = d.ints.as<unsigned long long>();
    HS_HIP(hipMemsetAsync(ints, 0, C * (kPuInts + nslot) * sizeof(int64_t), st));
    const int G = std::min(g.NE, kPuGroup), nsl = g.nslot <= kPuSlotLds ? g.nslot : 0;
    const size_t lds = (size_t)G * (sizeof(double) + sizeof(uint32_t)) + (size_t)nsl * sizeof(uint32_t) + 8;
    hipLaunchKernelGGL(k_pu_counts, dim3(g.ntiles, C), dim3(64), lds, st, g, d_y, d_x, d.single.as<int32_t>(),
                       d.slot.as<int32_t>(), d.inptr.as<int32_t>(), d.insrc.as<int32_t>(), d.part_sum.as<double>(),
                       d.part_cnt.as<uint32_t>(), ints);
    const int extra = (int)((nslot + S + 63) / 64);
    hipLaunchKernelGGL(k_pu_final, dim3(g.NE + extra, C), dim3(64), 0, st, g, d_x, d.part_sum.as<double>(),
                       d.part_cnt.as<uint32_t>(), d.mu.as<double>(), ints, d_out, out_len);
    hipLaunchKernelGGL(k_pu_mean, dim3((unsigned)((S + 255) / 256), C), dim3(256), 0, st, g, d.states.as<int16_t>(), d_out,
                       out_len, d.mean.as<double>());
    hipLaunchKernelGGL(k_pu_resid, dim3(g.rblocks, C), dim3(kPuResidThreads), 0, st, g, d_y, d_x, d.mean.as<double>(),
                       d.rpart.as<double>());
    hipLaunchKernelGGL(k_pu_sigma, dim3(C), dim3(64), 0, st, g, d.rpart.as<double>(), ints, d_out, out_len,
                       reinterpret_cast<long long *>(d_counts));
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

}  // namespace hmmsort
