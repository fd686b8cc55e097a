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
// The second half of the file is the same update from additive statistics (hmmsort_plan_path_stats / _finish): one
// pass, a vector that adds over time shards, chunks and channels, and a finish that does not touch the signal.
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

// ---- the same update from additive statistics (hmmsort_plan_path_stats / _finish, hmmsort_stats_sum) ----------------
// sigma' does not need the second pass.  With M_t the mean of the NEW templates in the state of sample t,
//   sum_t (y_t - M_t)^2 = sum y^2 - 2 sum_e mu'_e (s_e + sm_e) + sum_e c_e mu'_e^2 + sum_{j multi} n_j M_j^2
// where c_e, s_e are pass 1's count and sum of y per (template, phase) entry e of the single-active states, sm_e the
// sum of y over the samples of states with two or more active templates (entered once per active template) and n_j
// the number of samples in each such state j.  All are plain sums over time, so one pass over any range of (y, x)
// gives a vector that adds over time shards, chunks and pooled channels; the finish is O(S + N K).
//   k_ps_counts  k_pu_counts' tiles, steps and tables, plus sm, n_j, sum y^2; samples outside the range are masked
//   k_ps_final   the tiles' tables summed in k_pu_final's order into the statistics vector
//   k_ps_finish  a statistics vector and the plan's mu -> mu', sigma', lp', pp' in hmmsort_plan_mstep's layout
//   k_stats_sum  P vectors added in ascending order, one thread per entry
// vector, per channel:  [ c NE | s NE | sm NE | n_j S | ent nslot | b | sum_y2 | n | x0 | bad0 | bad1 ]
namespace {

constexpr int kPsGroup = 2048;     // entries one LDS pass holds: 40 KB of s, sm and c (per entry the order of adding
                                   // is time order whatever the group size, so the sums equal k_pu_counts')
constexpr int kPsTail = 6;
constexpr int kPsFinishThreads = 1024;

struct PsGeom {
    int64_t T, tile, own_lo, own_hi, tile0, len;
    int S, N, K, NE, W, nslot, rstride, nt, first;
};

// total of v over the workgroup, to every thread: lanes by the shuffle tree, then the wavefronts in order
__device__ inline double block_sum_f64(double v, double *s_w)
{
    v = wave_sum_f64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    double a = s_w[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); w++) a += s_w[w];
    return a;
}

// One wavefront per tile [tile0 + blockIdx.x] of g.tile samples, tiles anchored at sample 0 of the arrays.  The
// read-modify-write argument of k_pu_counts carries over to sm: a sample in a multi-active state updates one entry
// per active template, and "no two lanes of a step address the same (template, phase)" is a statement about one
// template l (it cannot be at phase k again before t + K), whatever the other templates do at that sample.  s/c
// and sm are separate tables, and a lane's own entries differ in l.
__global__ __launch_bounds__(64) void k_ps_counts(PsGeom g, const double *__restrict__ y,
                                                  const int16_t *__restrict__ x,
                                                  const int32_t *__restrict__ single,
                                                  const int32_t *__restrict__ multi,
                                                  const int32_t *__restrict__ slot,
                                                  const int32_t *__restrict__ in_ptr,
                                                  const int32_t *__restrict__ in_src,
                                                  double *__restrict__ part_sum, double *__restrict__ part_sm,
                                                  uint32_t *__restrict__ part_cnt, double *__restrict__ part_y2,
                                                  unsigned long long *__restrict__ ints,
                                                  unsigned long long *__restrict__ nj)
{
    extern __shared__ double s_ps[];
    const int lane = threadIdx.x, ch = blockIdx.y, S = g.S, N = g.N, NE = g.NE, W = g.W;
    const int G = NE < kPsGroup ? NE : kPsGroup;
    const int nsl = g.nslot <= kPuSlotLds ? g.nslot : 0;
    double *s_sum = s_ps, *s_sm = s_ps + G;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_sm + G);
    uint32_t *s_ent = s_cnt + G;
    const int64_t T = g.T;
    const double *yc = y + (int64_t)ch * T;
    const int16_t *xc = x + (int64_t)ch * T;
    slot += (int64_t)ch * S;
    in_ptr += (int64_t)ch * (S + 1);
    in_src += (int64_t)ch * g.rstride;
    ints += (int64_t)ch * (kPuInts + g.nslot);
    nj += (int64_t)ch * S;
    const int64_t t0 = (g.tile0 + (int64_t)blockIdx.x) * g.tile;
    const int64_t t1 = t0 + g.tile < T ? t0 + g.tile : T;
    const size_t row = ((size_t)ch * g.nt + blockIdx.x) * (size_t)NE;

    for (int e0 = 0; e0 == 0 || e0 < NE; e0 += kPsGroup) {
        const int ge = NE - e0 < G ? NE - e0 : G;
        const bool first = e0 == 0;   // the integer counts and sum y^2 are taken in the first pass only
        for (int i = lane; i < ge; i += 64) s_sum[i] = 0.0, s_sm[i] = 0.0, s_cnt[i] = 0u;
        if (first)
            for (int i = lane; i < nsl; i += 64) s_ent[i] = 0u;
        __syncthreads();
        long long bad0 = 0, bad1 = 0, nb = 0;
        double y2 = 0.0;
#pragma unroll 2
        for (int64_t ts = t0; ts < t1; ts += W) {
            const int64_t t = ts + lane;
            int e = -1;
            const int32_t *ml = nullptr;
            double yv = 0.0;
            if (lane < W && t < t1 && t >= g.own_lo && t < g.own_hi) {
                const int xs = (int)xc[t] - 1;
                const bool v = xs >= 0 && xs < S;
                yv = yc[t];
                if (v) {
                    e = single[xs];
                    if (e < 0 && multi[(int64_t)xs * N] >= 0) ml = multi + (int64_t)xs * N;
                }
                if (first) {
                    bad0 += !v;
                    if (v) y2 += yv * yv;
                    if (ml) atomicAdd(&nj[xs], 1ull);
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
            if (ml)
                for (int l = 0; l < N; l++) {
                    const int m = ml[l];
                    if (m < 0) break;
                    if (m >= e0 && m - e0 < ge) s_sm[m - e0] += yv;
                }
        }
        __syncthreads();
        for (int i = lane; i < ge; i += 64) {
            part_sum[row + e0 + i] = s_sum[i];
            part_sm[row + e0 + i] = s_sm[i];
            part_cnt[row + e0 + i] = s_cnt[i];
        }
        if (first) {
            for (int i = lane; i < nsl; i += 64)
                if (s_ent[i]) atomicAdd(&ints[kPuInts + i], (unsigned long long)s_ent[i]);
            bad0 = wave_sum_ll(bad0);
            bad1 = wave_sum_ll(bad1);
            nb = wave_sum_ll(nb);
            y2 = wave_sum_f64(y2);
            if (lane == 0) {
                if (bad0) atomicAdd(&ints[0], (unsigned long long)bad0);
                if (bad1) atomicAdd(&ints[1], (unsigned long long)bad1);
                if (nb) atomicAdd(&ints[3], (unsigned long long)nb);
                part_y2[(size_t)ch * g.nt + blockIdx.x] = y2;
            }
        }
        __syncthreads();
    }
}

// blocks [0, NE): one entry each, as k_pu_final sums it; block NE: sum y^2 and the tail; blocks after it: n_j and the
// entry counts, one slot per lane
__global__ __launch_bounds__(64) void k_ps_final(PsGeom g, const int16_t *__restrict__ x,
                                                 const double *__restrict__ part_sum,
                                                 const double *__restrict__ part_sm,
                                                 const uint32_t *__restrict__ part_cnt,
                                                 const double *__restrict__ part_y2,
                                                 const unsigned long long *__restrict__ ints,
                                                 const unsigned long long *__restrict__ nj,
                                                 double *__restrict__ stats)
{
    const int lane = threadIdx.x, ch = blockIdx.y, i = blockIdx.x, NE = g.NE, S = g.S;
    stats += (int64_t)ch * g.len;
    ints += (int64_t)ch * (kPuInts + g.nslot);
    if (i < NE) {
        const size_t base = (size_t)ch * g.nt * (size_t)NE + i;
        double s = 0.0, m = 0.0;
        long long c = 0;
        for (int r = lane; r < g.nt; r += 64) {
            s += part_sum[base + (size_t)r * NE];
            m += part_sm[base + (size_t)r * NE];
            c += (long long)part_cnt[base + (size_t)r * NE];
        }
        s = wave_sum_f64(s);
        m = wave_sum_f64(m);
        c = wave_sum_ll(c);
        if (lane == 0) {
            stats[i] = (double)c;
            stats[(int64_t)NE + i] = s;
            stats[2 * (int64_t)NE + i] = m;
        }
        return;
    }
    if (i == NE) {
        double y2 = 0.0;
        for (int r = lane; r < g.nt; r += 64) y2 += part_y2[(size_t)ch * g.nt + r];
        y2 = wave_sum_f64(y2);
        if (lane == 0) {
            double *tail = stats + 3 * (int64_t)NE + S + g.nslot;
            int x0 = 0;
            if (g.first && g.own_lo == 0) {
                x0 = (int)x[(int64_t)ch * g.T];
                if (x0 < 1 || x0 > S) x0 = 0;
            }
            tail[0] = (double)ints[3];
            tail[1] = y2;
            tail[2] = (double)(g.own_hi - g.own_lo - (int64_t)ints[0]);
            tail[3] = (double)x0;
            tail[4] = (double)ints[0];
            tail[5] = (double)ints[1];
        }
        return;
    }
    const int64_t j = (int64_t)(i - NE - 1) * 64 + lane;
    if (j < S)
        stats[3 * (int64_t)NE + j] = (double)nj[(int64_t)ch * S + j];
    else if (j - S < g.nslot)
        stats[3 * (int64_t)NE + j] = (double)ints[kPuInts + (j - S)];
}

// Workgroup 0 of a channel: mu' first (every thread's rows, then a barrier), then the four sums by the block tree.
// The workgroups after it write lp' and pp', one entry per thread: they need the integer slots only.
__global__ __launch_bounds__(kPsFinishThreads) void k_ps_finish(PsGeom g, const double *__restrict__ stats,
                                                               const int16_t *__restrict__ states,
                                                               const double *__restrict__ mu_cur, double *out,
                                                               int64_t out_len, long long *__restrict__ counts)
{
    __shared__ double s_w[kPsFinishThreads / 64];
    const int tid = threadIdx.x, ch = blockIdx.y, NE = g.NE, K = g.K, N = g.N, S = g.S, L = K - 1;
    stats += (int64_t)ch * g.len;
    out += (int64_t)ch * out_len;
    const double *c = stats, *s = stats + NE, *sm = stats + 2 * (int64_t)NE, *n_j = stats + 3 * (int64_t)NE;
    const double *ent = n_j + S, *tail = ent + g.nslot;
    if (blockIdx.x > 0) {
        const int64_t j = (int64_t)(blockIdx.x - 1) * kPsFinishThreads + tid;
        const double b = tail[0], x0 = tail[3];
        if (j < g.nslot) {
            const double n = ent[j];
            out[(int64_t)K * N + 1 + j] = (n == 0.0 || b == 0.0) ? -INFINITY : log(n) - log(b);
        } else if (j - g.nslot < S) {
            out[(int64_t)K * N + 1 + j] = ((double)(j - g.nslot + 1) == x0) ? 0.0 : -INFINITY;
        }
        return;
    }
    double a1 = 0.0, a2 = 0.0, a3 = 0.0, kept = 0.0;
    for (int e = tid; e < NE; e += kPsFinishThreads) {
        const int l = e / L, k = e % L;
        const int idx = (k + 1) + K * l;
        double m;
        if (c[e] > 0.0) {
            m = s[e] / c[e];
        } else {   // 0/0: the row keeps the plan's value
            m = mu_cur[(int64_t)ch * K * N + idx];
            kept += 1.0;
        }
        out[idx] = m;
        a1 += m * (s[e] + sm[e]);
        a2 += c[e] * (m * m);
    }
    for (int l = tid; l < N; l += kPsFinishThreads) out[(int64_t)K * l] = 0.0;
    __syncthreads();   // mu' is complete and visible to the workgroup
    for (int j = tid; j < S; j += kPsFinishThreads) {
        if (!(n_j[j] > 0.0)) continue;
        double a = 0.0;
        for (int l = 0; l < N; l++) {
            const int k = (int)states[l + (int64_t)N * j] - 1;   // 0 .. K-1 by build_host_model
            a += out[k + (int64_t)K * l];
        }
        a3 += n_j[j] * (a * a);
    }
    a1 = block_sum_f64(a1, s_w);
    a2 = block_sum_f64(a2, s_w);
    a3 = block_sum_f64(a3, s_w);
    kept = block_sum_f64(kept, s_w);
    if (tid == 0) {
        const double tot = ((tail[1] - 2.0 * a1) + a2) + a3;
        out[(int64_t)K * N] = sqrt((tot > 0.0 ? tot : 0.0) / tail[2]);
        if (counts) {
            counts[(int64_t)ch * 3] = (long long)tail[4];
            counts[(int64_t)ch * 3 + 1] = (long long)tail[5];
            counts[(int64_t)ch * 3 + 2] = (long long)kept;
        }
    }
}

__global__ __launch_bounds__(256) void k_stats_sum(const double *__restrict__ parts, int64_t nparts, int64_t len,
                                                   double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    double a = parts[i];
    for (int64_t p = 1; p < nparts; p++) a += parts[p * len + i];
    out[i] = a;
}

// acc <- w acc + new on the first nweighted entries, product and sum rounded one after the other (the file is built
// with contraction off; the intrinsics say so where it matters), acc <- acc + new on the rest
__global__ __launch_bounds__(256) void k_stats_blend(double *__restrict__ acc, double w, const double *__restrict__ nw,
                                                     int64_t len, int64_t nweighted)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const double a = acc[i], b = nw[i];
    acc[i] = i < nweighted ? __dadd_rn(__dmul_rn(w, a), b) : __dadd_rn(a, b);
}

// state -> the entries l (K-1) + (k-2) of its active rows in neuron order, -1 padded, for states with two or more;
// all -1 for the others
void multi_table(const HostModel &m, std::vector<int32_t> &tab)
{
    tab.assign(std::max<int64_t>(m.S * m.N, 1), -1);
    for (int64_t j = 0; j < m.S; j++) {
        int64_t active = 0;
        for (int64_t l = 0; l < m.N; l++) active += m.states[l + m.N * j] >= 2;
        if (active < 2) continue;
        int64_t at = 0;
        for (int64_t l = 0; l < m.N; l++)
            if (m.states[l + m.N * j] >= 2) tab[j * m.N + at++] = (int32_t)(l * (m.K - 1) + (m.states[l + m.N * j] - 2));
    }
}

}  // namespace

// the tables of the plan's current model(s) for the statistics calls, and their workspace, which grows with the
// length of the arrays a call is given
struct PathStatsDev {
    std::vector<int32_t> h_single, h_multi, h_slot, h_inptr, h_insrc;
    std::vector<double> h_mu;
    int nslot = 0, rstride = 1;
    DevBuf single, multi, states, slot, inptr, insrc, mu, part_sum, part_sm, part_cnt, part_y2, ints, nj;
};

namespace {

// the plan's PathStatsDev with the tables of its current model(s) on the device (uploaded on st and waited for when
// the model has changed since the last call)
int path_stats_tables(hmmsort_plan *p, hipStream_t st, PathStatsDev **out)
{
    const HostModel &m0 = p->model;
    const int64_t C = p->C, S = m0.S, N = m0.N, K = m0.K, nslot = p->eng->n_lp();
    int rc;
    HS_CHECK(N * (K - 1) <= (int64_t)1 << 24, HMMSORT_EUNSUP, "plan_path_stats: %lld x %lld template entries",
             (long long)N, (long long)(K - 1));
    if (!p->ps) {
        std::shared_ptr<PathStatsDev> d(new PathStatsDev());
        single_table(m0, d->h_single);
        multi_table(m0, d->h_multi);
        if ((rc = d->single.alloc(S * sizeof(int32_t))) || (rc = d->multi.alloc(d->h_multi.size() * sizeof(int32_t))) ||
            (rc = d->states.alloc(N * S * sizeof(int16_t))) || (rc = d->slot.alloc(C * S * sizeof(int32_t))) ||
            (rc = d->inptr.alloc(C * (S + 1) * sizeof(int32_t))) || (rc = d->mu.alloc(C * K * N * sizeof(double))) ||
            (rc = d->nj.alloc(C * S * sizeof(int64_t))))
            return rc;
        // once per plan, like plan creation: these wait for their copy
        HS_HIP(hipMemcpy(d->single.p, d->h_single.data(), S * sizeof(int32_t), hipMemcpyHostToDevice));
        HS_HIP(hipMemcpy(d->multi.p, d->h_multi.data(), d->h_multi.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HS_HIP(hipMemcpy(d->states.p, m0.states.data(), N * S * sizeof(int16_t), hipMemcpyHostToDevice));
        p->ps = d;
        p->ps_stale = true;
    }
    PathStatsDev &d = *p->ps;
    if (p->ps_stale) {
        int64_t rmax = 1;
        for (int64_t ch = 0; ch < C; ch++) rmax = std::max(rmax, (C > 1 ? p->models[ch] : m0).R);
        d.nslot = (int)nslot;
        d.rstride = (int)rmax;
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
        // waited for here: the host images are free for the next model, a call on another stream finds the tables
        // there, and nothing of the plan refers to `st` once it is gone (a cached plan outlives its channel's stream;
        // an event last recorded on a destroyed stream made hipEventSynchronize fail now and then)
        HS_HIP(hipStreamSynchronize(st));
        p->ps_stale = false;
    }
    *out = &d;
    return HMMSORT_OK;
}

PsGeom ps_geom(const hmmsort_plan *p, const PathStatsDev &d)
{
    const HostModel &m = p->model;
    PsGeom g{};
    g.S = (int)m.S, g.N = (int)m.N, g.K = (int)m.K;
    g.NE = (int)(m.N * (m.K - 1));
    g.W = (int)std::max<int64_t>(1, std::min<int64_t>(m.K - 1, 64));
    g.tile = std::max<int64_t>(kPuMinTile, 16 * (int64_t)g.NE);   // plan_path_update's
    g.nslot = d.nslot;
    g.rstride = d.rstride;
    g.len = plan_path_stats_len(p);
    return g;
}

}  // namespace

int64_t plan_path_stats_len(const hmmsort_plan *p)
{
    const HostModel &m = p->model;
    return 3 * m.N * (m.K - 1) + m.S + p->eng->n_lp() + kPsTail;
}

int plan_path_stats(hmmsort_plan *p, const double *d_y, const int16_t *d_x, int64_t T, int64_t own_lo, int64_t own_hi,
                    bool first, double *d_stats, hipStream_t st)
{
    const int64_t C = p->C;
    PathStatsDev *dp = nullptr;
    int rc;
    if ((rc = path_stats_tables(p, st, &dp))) return rc;
    PathStatsDev &d = *dp;
    PsGeom g = ps_geom(p, d);
    if (own_lo == own_hi) {   // an empty range owns nothing
        HS_HIP(hipMemsetAsync(d_stats, 0, C * g.len * sizeof(double), st));
        return HMMSORT_OK;
    }
    g.T = T, g.own_lo = own_lo, g.own_hi = own_hi, g.first = first;
    g.tile0 = own_lo / g.tile;
    const int64_t nt = (own_hi - 1) / g.tile - g.tile0 + 1;
    HS_CHECK(nt <= 2147483647LL / 64, HMMSORT_EUNSUP, "plan_path_stats: range too long");
    g.nt = (int)nt;
    const size_t npart = (size_t)C * g.nt * std::max(g.NE, 1);
    if ((rc = d.part_sum.ensure(npart * sizeof(double))) || (rc = d.part_sm.ensure(npart * sizeof(double))) ||
        (rc = d.part_cnt.ensure(npart * sizeof(uint32_t))) || (rc = d.part_y2.ensure((size_t)C * g.nt * sizeof(double))))
        return rc;
    unsigned long long *ints = d.ints.as<unsigned long long>(), *nj = d.nj.as<unsigned long long>();
    HS_HIP(hipMemsetAsync(ints, 0, C * (kPuInts + g.nslot) * sizeof(int64_t), st));
    HS_HIP(hipMemsetAsync(nj, 0, C * g.S * sizeof(int64_t), st));
    const int G = std::min(g.NE, kPsGroup), nsl = g.nslot <= kPuSlotLds ? g.nslot : 0;
    const size_t lds = (size_t)G * (2 * sizeof(double) + sizeof(uint32_t)) + (size_t)nsl * sizeof(uint32_t) + 8;
    hipLaunchKernelGGL(k_ps_counts, dim3(g.nt, C), dim3(64), lds, st, g, d_y, d_x, d.single.as<int32_t>(),
                       d.multi.as<int32_t>(), d.slot.as<int32_t>(), d.inptr.as<int32_t>(), d.insrc.as<int32_t>(),
                       d.part_sum.as<double>(), d.part_sm.as<double>(), d.part_cnt.as<uint32_t>(),
                       d.part_y2.as<double>(), ints, nj);
    const int extra = 1 + (int)((g.S + g.nslot + 63) / 64);
    hipLaunchKernelGGL(k_ps_final, dim3(g.NE + extra, C), dim3(64), 0, st, g, d_x, d.part_sum.as<double>(),
                       d.part_sm.as<double>(), d.part_cnt.as<uint32_t>(), d.part_y2.as<double>(), ints, nj, d_stats);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int plan_path_finish(hmmsort_plan *p, const double *d_stats, double *d_out, int64_t *d_counts, hipStream_t st)
{
    PathStatsDev *dp = nullptr;
    int rc;
    if ((rc = path_stats_tables(p, st, &dp))) return rc;
    const PsGeom g = ps_geom(p, *dp);
    const int64_t out_len = (int64_t)g.K * g.N + 1 + g.nslot + g.S;
    const unsigned extra = (unsigned)((g.nslot + (int64_t)g.S + kPsFinishThreads - 1) / kPsFinishThreads);
    hipLaunchKernelGGL(k_ps_finish, dim3(1 + extra, p->C), dim3(kPsFinishThreads), 0, st, g, d_stats, dp->states.as<int16_t>(),
                       dp->mu.as<double>(), d_out, out_len, reinterpret_cast<long long *>(d_counts));
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int dev_stats_sum(const double *d_parts, int64_t nparts, int64_t len, double *d_out, hipStream_t st)
{
    hipLaunchKernelGGL(k_stats_sum, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, d_parts, nparts, len, d_out);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int dev_stats_blend(double *d_acc, double w, const double *d_new, int64_t len, int64_t plain_tail, hipStream_t st)
{
    if (len <= 0) return HMMSORT_OK;
    hipLaunchKernelGGL(k_stats_blend, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, d_acc, w, d_new, len,
                       len - plain_tail);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

}  // namespace hmmsort
