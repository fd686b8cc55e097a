// Wave engine, part 4: smoothed state posteriors as an OUTPUT ("Posteriors").
//
// A ring runs deterministically once entered, so the onset posteriors rho_a(t') of the backward sweep
// (wave_estep.hip) are the whole posterior of a ring model:  gamma_t(a, phase k) = rho_a(t - k + 1).
// A posterior call runs the forward sweep and the UNFUSED backward sweep with the silent-posterior store
// (kw_bwd<N, UC, 0, true>: rho and gamma_t(silent) of every sample, no statistics), then
//   kw_post_head       virtual onsets t' = -j of the rings already running at t = 0 (the terms kw_stats_final
//                      forms for pp = gamma[:,1]: exp(V_a[j] + Yn_a(L-1-j) - z_0)) and the recording's logz
//   kw_post_marginals  occ[a,t] = sum of the L onsets rho_a(t-L+1 .. t), silent[t]   (one pass over rho)
//   kw_post_decode     xm[t] = arg max over silent and the N L ring candidates        (one pass over rho)
//   kw_spike_conf      per decoded event, the posterior mass of the trough state within +-J samples
// Window sums and maxima are formed inside an LDS tile of kPT samples + L-1 halo: a thread owns kPR
// consecutive samples, folds the L-kPR+1 onsets their windows share once and adds each window's few
// remaining onsets (no subtraction anywhere, so nothing cancels however long the recording is).
#include <cmath>

#include "fastmath.h"
#include "wave_common.h"

namespace hmmsort {

constexpr int kPT = 2048, kPR = 8;                       // samples per workgroup (256 threads), per thread
__host__ __device__ __forceinline__ int ppad(int i) { return i + (i >> 3); }   // lanes read at a stride of kPR doubles: one pad per 8

// Scale of chain c's forward values against chain c-1's, F_c - F_{c-1}: the difference between the warm-up copy of a
// boundary quantity in chain c and chain c-1's own value of it.  Every converged boundary entry gives the same
// number; it is read where the forward certificate (kw_fb_check, wave_estep.hip) reads its frame constant, at the
// entry of LARGEST POSTERIOR WEIGHT: the silent state at tc-1 or one of the N L onsets still inside their rings.
// (The silent entry alone is not enough: where a chain boundary falls inside a certain spike, "silent at tc-1" has a
// posterior of e^-500, the two sweeps agree on it to no digit -- which the certificate, weighting it by that
// posterior, rightly ignores -- and logz came out 2-3 % off: 9 and 13 rings of 64 states, tests/test_gpu_wave_dispatch.py.)
// One wavefront per chain; chain 0 of a channel has no boundary.
__global__ __launch_bounds__(64) void kw_post_shift(WaveGeom g, const double *__restrict__ FA0,
                                                    const double *__restrict__ FV, const double *__restrict__ FREF,
                                                    const double *__restrict__ fpre, const double *__restrict__ rho,
                                                    double *__restrict__ fshift)
{
    const int lane = threadIdx.x;
    const int cg = blockIdx.x, ch = cg / g.nch, c = cg % g.nch;
    if (c == 0) { if (lane == 0) fshift[cg] = 0.0; return; }
    const int N = g.N, L = g.L;
    const int64_t T = g.T, tc = (int64_t)c * g.B;            // tc >= B >= L + 16: every onset below is inside the data
    const int64_t FR = 1 + (int64_t)L * (N + 1);
    const double *FAc = FA0 + (int64_t)ch * T, *FRc = FREF + (int64_t)ch * T, *FVc = FV + (int64_t)ch * N * T;
    const double *rhoc = rho + (int64_t)ch * N * T;
    // entry (a, e): the onset t' = tc-1-e of ring a, e = 0..L-1
    auto diff = [&](int a, int e) {
        const int64_t tp = tc - 1 - e, jj = tp - (tc - L);
        const double hv = fpre[cg * FR + 1 + jj * (N + 1) + a], hs = fpre[cg * FR + 1 + jj * (N + 1) + N];
        const double mv = FVc[(int64_t)a * T + tp], ms = FRc[tp];
        if (hv == mv && hs == ms) return 0.0;
        return (hs - ms) + (flog(hv) - flog(mv));
    };
    double ringmass = 0.0;
    for (int idx = lane; idx < N * L; idx += 64) ringmass += rhoc[(int64_t)(idx / L) * T + (tc - 1 - idx % L)];
    ringmass = wave_sum(ringmass);
    double wb = lane == 0 ? fmax(1.0 - ringmass, 0.0) : -1.0;   // the silent entry: what the rings leave
    double db = fpre[cg * FR] - FAc[tc - 1];
    for (int idx = lane; idx < N * L; idx += 64) {
        const int a = idx / L, e = idx % L;
        const double w = rhoc[(int64_t)a * T + (tc - 1 - e)];
        if (w > wb) { wb = w; db = diff(a, e); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ow = __shfl_xor(wb, o), od = __shfl_xor(db, o);
        if (ow > wb) { wb = ow; db = od; }
    }
    if (lane == 0) fshift[cg] = db;
}

// one wavefront per channel
__global__ __launch_bounds__(64) void kw_post_head(WaveGeom g, const WaveConst *__restrict__ cst,
                                                   const double *__restrict__ virt,
                                                   const double *__restrict__ yhead, const double *__restrict__ Zc,
                                                   const double *__restrict__ fshift,
                                                   double *__restrict__ phead, double *__restrict__ plogz)
{
    const int N = g.N, L = g.L, ch = blockIdx.x, lane = threadIdx.x;
    const double *yh = yhead + (int64_t)ch * (N * L + 2);
    const double z0 = Zc[(int64_t)ch * g.nch];
    for (int i = lane; i < N * L; i += 64) {
        const int a = i / L, j = i % L;
        const double *V = virt + ((int64_t)ch * N + a) * (L + 1);
        phead[(int64_t)ch * N * L + i] = j >= 1 ? fexp((V[j] + yh[a * L + (L - 1 - j)]) - z0) : 0.0;
    }
    // Every chain's forward values carry the arbitrary scale F_c of its warm-up start (F_0 = 0); the last chain's
    // backward values are exact (beta = 0 at the end of the data), so its normaliser is z + F_last, and
    // F_c - F_{c-1} = (warm-up copy of la0(tc-1) in chain c) - (chain c-1's own la0(tc-1)): the pair the forward
    // certificate compares.  The sweeps leave the emission constant A = -log(sigma sqrt(2 pi)) of every sample out
    // (it cancels in every posterior): T A is added back here.  The differences: kw_post_shift.
    double s = 0.0;
    for (int c = 1 + lane; c < g.nch; c += 64) s += fshift[(int64_t)ch * g.nch + c];
    s = wave_sum(s);
    if (lane == 0) plogz[ch] = (Zc[(int64_t)ch * g.nch + g.nch - 1] - s) + (double)g.T * cst[ch].A;
}

// Staging of rho_a(t0-(L-1) .. t0+kPT-1) (virtual onsets in front of the recording, 0 behind it) in two steps, so
// that the loads of the next ring are in flight while the window sums of this one are formed: fetch() into
// registers, put() into the LDS tile.  kPF loads per thread cover kPT + L - 1 <= 256 kPF entries (L <= 256).
constexpr int kPF = 9;
struct PostStage {
    double v[kPF];
    __device__ __forceinline__ void fetch(const double *__restrict__ ra, const double *__restrict__ ha, int64_t t0,
                                          int64_t T, int L)
    {
        const int nst = kPT + L - 1;
#pragma unroll
        for (int j = 0; j < kPF; j++) {
            const int i = threadIdx.x + 256 * j;
            const int64_t tp = t0 - (L - 1) + i;
            v[j] = i < nst ? (tp < 0 ? ha[-tp] : (tp < T ? ra[tp] : 0.0)) : 0.0;
        }
    }
    __device__ __forceinline__ void put(double *st, int L) const
    {
        const int nst = kPT + L - 1;
#pragma unroll
        for (int j = 0; j < kPF; j++) {
            const int i = threadIdx.x + 256 * j;
            if (i < nst) st[ppad(i)] = v[j];
        }
    }
};

__global__ __launch_bounds__(256) void kw_post_marginals(WaveGeom g, const double *__restrict__ rho,
                                                         const double *__restrict__ gsil,
                                                         const double *__restrict__ phead, double *__restrict__ onset,
                                                         double *__restrict__ occ, double *__restrict__ silent)
{
    extern __shared__ double lds[];
    const int N = g.N, L = g.L, ch = blockIdx.y, tid = threadIdx.x;
    const int64_t T = g.T, t0 = (int64_t)blockIdx.x * kPT;
    double *st = lds, *ob = lds + ppad(kPT + L - 1) + 1;
    if (silent)
        for (int i = tid; i < kPT; i += 256)
            if (t0 + i < T) silent[(int64_t)ch * T + t0 + i] = gsil[(int64_t)ch * T + t0 + i];
    if (!occ && !onset) return;
    const int b = kPR * tid;                              // staged index of the first onset of this thread's first window
    PostStage ps;
    ps.fetch(rho + (int64_t)ch * N * T, phead + (int64_t)ch * N * L, t0, T, L);
    for (int a = 0; a < N; a++) {
        __syncthreads();
        ps.put(st, L);
        __syncthreads();
        if (a + 1 < N) ps.fetch(rho + ((int64_t)ch * N + a + 1) * T, phead + ((int64_t)ch * N + a + 1) * L, t0, T, L);
        if (onset) {                                      // the tile's own onsets: a copy of rho for the caller
            double *na = onset + ((int64_t)ch * N + a) * T;
            for (int i = tid; i < kPT; i += 256)
                if (t0 + i < T) na[t0 + i] = st[ppad(i + L - 1)];
        }
        if (!occ) continue;                               // wave-uniform
        if (L >= kPR) {
            double com = 0.0;                             // onsets b+kPR-1 .. b+L-1: in every window of this thread
            for (int i = b + kPR - 1; i <= b + L - 1; i++) com += st[ppad(i)];
#pragma unroll
            for (int r = 0; r < kPR; r++) {
                double s = com;
                for (int i = b + r; i <= b + kPR - 2; i++) s += st[ppad(i)];
                for (int i = b + L; i <= b + L - 1 + r; i++) s += st[ppad(i)];
                ob[ppad(b + r)] = s;
            }
        } else {
#pragma unroll
            for (int r = 0; r < kPR; r++) {
                double s = 0.0;
                for (int i = b + r; i <= b + r + L - 1; i++) s += st[ppad(i)];
                ob[ppad(b + r)] = s;
            }
        }
        __syncthreads();
        double *oa = occ + ((int64_t)ch * N + a) * T;
        for (int i = tid; i < kPT; i += 256)
            if (t0 + i < T) oa[t0 + i] = ob[ppad(i)];
    }
}

// candidate (a, k) of sample t has the value rho_a(t - k + 1); state number 2 + a L + (k - 1) (the single-active
// enumeration every ring plan has, statespace.cpp analyze_ring); ties go to the lower state number: silent, then
// the lower ring, then the lower phase = the LATER onset.
__global__ __launch_bounds__(256) void kw_post_decode(WaveGeom g, const double *__restrict__ rho,
                                                      const double *__restrict__ gsil,
                                                      const double *__restrict__ phead, int16_t *__restrict__ xm)
{
    extern __shared__ double lds[];
    const int N = g.N, L = g.L, ch = blockIdx.y, tid = threadIdx.x;
    const int64_t T = g.T, t0 = (int64_t)blockIdx.x * kPT;
    double *st = lds;
    const int b = kPR * tid;
    double bv[kPR];
    int bs[kPR];
#pragma unroll
    for (int r = 0; r < kPR; r++) {
        const int64_t t = t0 + b + r;
        bv[r] = t < T ? gsil[(int64_t)ch * T + t] : 0.0;
        bs[r] = 1;
    }
    PostStage ps;
    ps.fetch(rho + (int64_t)ch * N * T, phead + (int64_t)ch * N * L, t0, T, L);
    for (int a = 0; a < N; a++) {
        __syncthreads();
        ps.put(st, L);
        __syncthreads();
        if (a + 1 < N) ps.fetch(rho + ((int64_t)ch * N + a + 1) * T, phead + ((int64_t)ch * N + a + 1) * L, t0, T, L);
        // (value, staged index) of a window, the later index on equal values
        double cv = -1.0;
        int ci = -1;
        if (L >= kPR)
            for (int i = b + kPR - 1; i <= b + L - 1; i++) {
                const double v = st[ppad(i)];
                if (v >= cv) { cv = v; ci = i; }
            }
#pragma unroll
        for (int r = 0; r < kPR; r++) {
            double mv = -1.0;
            int mi = -1;
            if (L >= kPR) {
                for (int i = b + r; i <= b + kPR - 2; i++) {
                    const double v = st[ppad(i)];
                    if (v >= mv) { mv = v; mi = i; }
                }
                if (cv >= mv) { mv = cv; mi = ci; }
                for (int i = b + L; i <= b + L - 1 + r; i++) {
                    const double v = st[ppad(i)];
                    if (v >= mv) { mv = v; mi = i; }
                }
            } else {
                for (int i = b + r; i <= b + r + L - 1; i++) {
                    const double v = st[ppad(i)];
                    if (v >= mv) { mv = v; mi = i; }
                }
            }
            // the sample of window r is staged index b + r + L - 1; phase k - 1 = that - mi
            if (mv > bv[r]) { bv[r] = mv; bs[r] = 2 + a * L + (b + r + L - 1 - mi); }
        }
    }
#pragma unroll
    for (int r = 0; r < kPR; r++) {
        const int64_t t = t0 + b + r;
        if (t < T) xm[(int64_t)ch * T + t] = (int16_t)bs[r];
    }
}

// one thread per event
__global__ __launch_bounds__(256) void kw_spike_conf(const double *__restrict__ src, const double *__restrict__ head,
                                                     int64_t T, int64_t shift, int64_t J,
                                                     const int64_t *__restrict__ times, int64_t n,
                                                     double *__restrict__ conf)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t t = times[e] - 1;                       // times are 1-based (extract_spiketimes)
    double s = 0.0;
    for (int64_t d = -J; d <= J; d++) {
        const int64_t tau = t + d;
        if (tau < 0 || tau >= T) continue;
        const int64_t idx = tau - shift;
        if (idx >= 0) s += src[idx];
        else if (head) s += head[-idx];
    }
    conf[e] = fmin(s, 1.0);
}

__global__ __launch_bounds__(256) void kw_row_sums(const double *__restrict__ rows, int64_t T, double *__restrict__ part)
{
    __shared__ double red[4];
    const double *p = rows + (int64_t)blockIdx.y * T;
    const int64_t per = (T + gridDim.x - 1) / gridDim.x, lo = (int64_t)blockIdx.x * per;
    const int64_t hi = lo + per < T ? lo + per : T;
    double s = 0.0;
    for (int64_t t = lo + threadIdx.x; t < hi; t += 256) s += p[t];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

int dev_spike_conf(const double *d_src, const double *d_head, int64_t T, int64_t shift, int64_t jitter,
                   const int64_t *d_times, int64_t n, double *d_conf, hipStream_t st)
{
    if (n <= 0) return HMMSORT_OK;
    hipLaunchKernelGGL(kw_spike_conf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_src, d_head, T, shift,
                       jitter, d_times, n, d_conf);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

// out_host[row] = sum over time of row (two deterministic stages; synchronises the stream)
int dev_row_sums(const double *d_rows, int64_t nrows, int64_t T, double *d_part, double *out_host, hipStream_t st)
{
    hipLaunchKernelGGL(kw_row_sums, dim3(kPostParts, (unsigned)nrows), dim3(256), 0, st, d_rows, T, d_part);
    HS_HIP(hipGetLastError());
    std::vector<double> h((size_t)nrows * kPostParts);
    HS_HIP(hipMemcpyAsync(h.data(), d_part, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < nrows; i++) {
        double s = 0.0;
        for (int b = 0; b < kPostParts; b++) s += h[(size_t)i * kPostParts + b];
        out_host[i] = s;
    }
    return HMMSORT_OK;
}

static int post_alloc(WaveDev *r)
{
    if (r->gsil) return HMMSORT_OK;
    const WaveGeom &g = r->g;
    const size_t ct = (size_t)g.C * g.T, nl = (size_t)g.C * g.N * g.L;
    auto A = [&](double **p, size_t n) -> int {
        if (hipMalloc((void **)p, n * sizeof(double)) != hipSuccess) {
            (void)hipGetLastError();
            *p = nullptr;
            set_error("wave engine: hipMalloc of %.2f GB for the posterior buffers failed", n * 8 / 1e9);
            return HMMSORT_ENOMEM;
        }
        r->bytes += (int64_t)(n * sizeof(double));
        return HMMSORT_OK;
    };
    int rc;
    if ((rc = A(&r->phead, nl)) || (rc = A(&r->plogz, (size_t)g.C)) || (rc = A(&r->fshift, (size_t)g.C * g.nch)) ||
        (rc = A(&r->pcnt, (size_t)g.C * g.N * kPostParts)) || (rc = A(&r->gsil, ct)))
        return rc;
    if (getenv("HMMSORT_POISON")) (void)hipMemset(r->gsil, 0xFF, ct * sizeof(double));
    return HMMSORT_OK;
}

static size_t post_lds(const WaveGeom &g, bool with_out)
{
    return ((size_t)ppad(kPT + g.L - 1) + 1 + (with_out ? ppad(kPT) + 1 : 0)) * sizeof(double);
}

int wave_posteriors(WaveDev *r, const double *d_y, double *d_onset, double *d_occ, double *d_silent, double *d_logz,
                    hipStream_t st)
{
    const WaveGeom &g = r->g;
    HS_CHECK(g.own_lo == 0 && g.own_hi == g.T && g.first && g.last, HMMSORT_EINVAL,
             "plan_posteriors: the plan is a time shard (hmmsort_plan_set_shard); posteriors of shards are not supported");
    HS_CHECK(kPT + g.L - 1 <= 256 * kPF, HMMSORT_EUNSUP, "plan_posteriors: rings longer than %d states", 256 * kPF - kPT + 1);
    int rc;
    if ((rc = post_alloc(r))) return rc;
    r->post_valid = false;
    if ((rc = wave_post_sweeps(r, d_y, st))) return rc;
    { WPROF(r, "kw_post_head", st);
      hipLaunchKernelGGL(kw_post_shift, dim3(g.C * g.nch), dim3(64), 0, st, g, r->FA0, r->FV, r->FREF, r->fpre, r->rho,
                         r->fshift);
      hipLaunchKernelGGL(kw_post_head, dim3(g.C), dim3(64), 0, st, g, r->d_cst, r->virt, r->yhead, r->Zc, r->fshift,
                         r->phead, r->plogz); }
    HS_HIP(hipGetLastError());
    const size_t nct = (size_t)g.C * g.N * g.T * sizeof(double);
    const bool marg = d_occ || d_silent;                  // the marginals pass has rho staged: it writes the onsets too
    if (d_onset && !marg) HS_HIP(hipMemcpyAsync(d_onset, r->rho, nct, hipMemcpyDeviceToDevice, st));
    if (d_logz) HS_HIP(hipMemcpyAsync(d_logz, r->plogz, (size_t)g.C * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (marg) {
        WPROF(r, "kw_post_marginals", st);
        hipLaunchKernelGGL(kw_post_marginals, dim3((unsigned)((g.T + kPT - 1) / kPT), g.C), dim3(256), post_lds(g, true),
                           st, g, r->rho, r->gsil, r->phead, d_onset, d_occ, d_silent);
        HS_HIP(hipGetLastError());
    }
    r->post_valid = true;
    return HMMSORT_OK;
}

int wave_post_decode(WaveDev *r, int16_t *d_xm, hipStream_t st)
{
    const WaveGeom &g = r->g;
    HS_CHECK(r->post_valid, HMMSORT_EINVAL,
             "plan_posterior_decode: call hmmsort_plan_posteriors first (an E-step or a new model discards the posteriors)");
    WPROF(r, "kw_post_decode", st);
    hipLaunchKernelGGL(kw_post_decode, dim3((unsigned)((g.T + kPT - 1) / kPT), g.C), dim3(256), post_lds(g, false), st, g,
                       r->rho, r->gsil, r->phead, d_xm);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int wave_spike_conf(WaveDev *r, int ch, int a, int qv, int64_t jitter, const int64_t *d_times, int64_t n,
                    double *d_conf, hipStream_t st)
{
    const WaveGeom &g = r->g;
    HS_CHECK(r->post_valid, HMMSORT_EINVAL, "plan_spike_confidence: call hmmsort_plan_posteriors first");
    HS_CHECK(qv >= 2 && qv <= g.L + 1, HMMSORT_EUNSUP,
             "plan_spike_confidence: template %d has its minimum in the silent row; no trough state to score", a);
    WPROF(r, "kw_spike_conf", st);
    return dev_spike_conf(r->rho + ((int64_t)ch * g.N + a) * g.T, r->phead + ((int64_t)ch * g.N + a) * g.L, g.T, qv - 2,
                          jitter, d_times, n, d_conf, st);
}

int wave_expected_counts(WaveDev *r, double *counts_out, hipStream_t st)
{
    HS_CHECK(r->post_valid, HMMSORT_EINVAL, "plan_expected_counts: call hmmsort_plan_posteriors first");
    return dev_row_sums(r->rho, (int64_t)r->g.C * r->g.N, r->g.T, r->pcnt, counts_out, st);
}

}  // namespace hmmsort
