// Per-spike amplitude and residual, and the per-template summary (hmmsort_spike_fit / hmmsort_plan_spike_fit,
// include/hmmsort.h): how well the spike the path placed fits the samples under it, with the other
// templates the path says are active taken out first.
//
// Definitions (the numpy model tests/spike_fit_model.py states the same rules):
//   events   template a has an event at 0-based sample t when x[t] is in 1..S and states[a, x[t]] == qv_a, the trough
//            value of the BASE templates; the compacted 1-based times of hmmsort_extract_spiketimes, ascending.
//   model    M = mu, or under a track M = mu_track[c] for the last chunk c with first[c] <= t + 1 (the trough's chunk
//            serves the whole window).  An event before first[0]: amp = rss = energy = NaN, nused = 0, counted in n only.
//   window   phases k = 2..K ascending, u = t + (k - qv_a); phase k is used iff 0 <= u < T, x[u] in 1..S and
//            states[a, x[u]] == k.  nused = used phases; the event is full iff nused == K - 1.
//   phase    oth = 0.0; for b ascending, b != a: oth += M[states[b, x[u]] - 1, b];  r = y[u] - oth;  m = M[k - 1, a].
//   event    four serial folds from 0.0 in ascending k, product and sum rounded separately (-ffp-contract=off):
//            srm += r*m, smm += m*m, energy += r*r, rss += d*d with d = r - m;  amp = srm / smm (IEEE quotient).
//   summary  8 + 3 (K-1) doubles per template: [0] n, [1] n_full, [2] sum amp, [3] sum amp*amp, [4] sum rss,
//            [5] sum energy (2..5 over full events), [6] sum nused (all events), [7] smm of the base template (host),
//            then wsum, wsq, wcnt (K-1 each): sum of r, of r*r and the count per phase over every used phase of every
//            event.  Events in ascending order are cut into blocks of 256; each slot's block partial is a serial fold
//            from 0.0 in event order, the partials are folded serially from 0.0 in block order.  Counts are doubles.
//            No floating-point atomics: the same input gives the same bits.
//
// Three kernels: k_fit_events (one wavefront per event: lanes over phases, the four products staged in LDS and folded
// by lanes 0..3 in ascending phase order), k_fit_partials (grid over (block of 256 events, template): threads 0..6
// fold the scalar slots; the waveform slots recompute r for tiles of 2 048 (event, phase) pairs with all threads into
// LDS and the thread that owns a phase folds it over the tile's events in event order; no events x (K-1) array
// exists) and k_fit_final (one thread per slot folds the block partials).
#include <algorithm>

#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

struct FitArgs {
    const double *y;
    const int16_t *x;
    int64_t T;
    const int16_t *states;   // N x S
    int N, S, K;
    const double *M;         // [K*N], or the track [nchunks][K*N]
    int nchunks;             // 0: no track
    const int64_t *first;    // [nchunks] 1-based, ascending
    const int64_t *times;    // [N][dcap] 1-based, ascending
    int64_t dcap;
    double *amp, *rss, *energy;   // [N][dcap]
    int32_t *nused, *chunk;       // [N][dcap]; chunk: index into the track, -1 before first[0]
    int64_t n[32];
    int32_t qv[32];
};

// phase k of an event of template a at trough sample t under templates M: used?  *r = y[u] - the other templates
__device__ __forceinline__ bool fit_phase(const FitArgs &A, int a, int qv, const double *__restrict__ M, int64_t t,
                                          int k, double *r)
{
    const int64_t u = t + (k - qv);
    if (u < 0 || u >= A.T) return false;
    const int xs = A.x[u];
    if (xs < 1 || xs > A.S) return false;
    const int16_t *col = A.states + (int64_t)A.N * (xs - 1);
    if (col[a] != k) return false;
    double oth = 0.0;
    for (int b = 0; b < A.N; b++)
        if (b != a) oth += M[(col[b] - 1) + (int64_t)A.K * b];
    *r = A.y[u] - oth;
    return true;
}

__global__ __launch_bounds__(256) void k_fit_events(const FitArgs A)
{
    __shared__ double s_p[4][4][64];   // [wave][fold][lane]: r*m, m*m, r*r, d*d of one tile of 64 phases
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int a = blockIdx.y, qv = A.qv[a];
    const int64_t e = (int64_t)blockIdx.x * 4 + w;
    bool live = e < A.n[a];
    const int64_t t = live ? A.times[(int64_t)a * A.dcap + e] - 1 : 0;
    int c = 0;
    if (A.nchunks > 0) {   // chunks [0, lo) start at or before sample t + 1
        int lo = 0, hi = A.nchunks;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (A.first[mid] <= t + 1)
                lo = mid + 1;
            else
                hi = mid;
        }
        c = lo - 1;
    }
    const int64_t o = (int64_t)a * A.dcap + e;
    if (live && c < 0) {
        if (lane == 0) {
            A.amp[o] = NAN, A.rss[o] = NAN, A.energy[o] = NAN;
            A.nused[o] = 0, A.chunk[o] = -1;
        }
        live = false;
    }
    const double *M = A.M + (int64_t)(c < 0 ? 0 : c) * A.K * A.N;
    double acc = 0.0;   // lane q < 4 carries fold q
    int nu = 0;
    for (int k0 = 2; k0 <= A.K; k0 += 64) {   // the trip count is the same for every wave of the block
        const int k = k0 + lane;
        double r = 0.0, m = 0.0;
        bool used = false;
        if (live && k <= A.K) {
            used = fit_phase(A, a, qv, M, t, k, &r);
            if (used) m = M[(k - 1) + (int64_t)A.K * a];
        }
        const unsigned long long mask = __ballot(used);
        const double d = r - m;
        s_p[w][0][lane] = r * m;
        s_p[w][1][lane] = m * m;
        s_p[w][2][lane] = r * r;
        s_p[w][3][lane] = d * d;
        __syncthreads();
        if (lane < 4)
            for (unsigned long long mm = mask; mm; mm &= mm - 1) acc += s_p[w][lane][__ffsll((long long)mm) - 1];
        nu += __popcll(mask);
        __syncthreads();
    }
    const double srm = __shfl(acc, 0), smm = __shfl(acc, 1), en = __shfl(acc, 2), rs = __shfl(acc, 3);
    if (live && lane == 0) {
        A.amp[o] = srm / smm;
        A.rss[o] = rs;
        A.energy[o] = en;
        A.nused[o] = nu;
        A.chunk[o] = c;
    }
}

constexpr int kFitBlock = 256;     // events per summary block
constexpr int kFitThreads = 1024;  // threads of k_fit_partials: the tiles are bound by the latency of dependent loads
constexpr int kFitStage = 2048;  // (event, phase) pairs of one tile in LDS

// part: [N][nblk][L], L = 8 + 3 (K-1); slot 7 is the host's
__global__ __launch_bounds__(kFitThreads) void k_fit_partials(const FitArgs A, double *__restrict__ part, int nblk)
{
    __shared__ double s_amp[kFitBlock], s_rss[kFitBlock], s_en[kFitBlock];
    __shared__ int64_t s_t[kFitBlock];
    __shared__ int32_t s_nu[kFitBlock], s_c[kFitBlock];
    __shared__ double s_r[kFitStage];      // r of one tile of (event, phase) pairs
    __shared__ uint8_t s_u[kFitStage];     // ... and whether the phase is used
    const int a = blockIdx.y, qv = A.qv[a], tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * kFitBlock;
    const int64_t left = A.n[a] - e0;
    const int ne = left <= 0 ? 0 : (left < kFitBlock ? (int)left : kFitBlock);
    const int P = A.K - 1, L = 8 + 3 * P;
    if (tid < ne) {
        const int64_t o = (int64_t)a * A.dcap + e0 + tid;
        s_amp[tid] = A.amp[o], s_rss[tid] = A.rss[o], s_en[tid] = A.energy[o];
        s_t[tid] = A.times[o] - 1, s_nu[tid] = A.nused[o], s_c[tid] = A.chunk[o];
    }
    __syncthreads();
    double *out = part + ((int64_t)a * nblk + blockIdx.x) * L;
    if (tid < 8) {
        double v = 0.0;
        for (int e = 0; e < ne && tid < 7; e++) {
            const bool full = s_nu[e] == P;
            switch (tid) {
            case 0: v += 1.0; break;
            case 1: if (full) v += 1.0; break;
            case 2: if (full) v += s_amp[e]; break;
            case 3: if (full) { const double q = s_amp[e] * s_amp[e]; v += q; } break;
            case 4: if (full) v += s_rss[e]; break;
            case 5: if (full) v += s_en[e]; break;
            default: v += (double)s_nu[e]; break;
            }
        }
        out[tid] = v;
    }
    // Waveform slots.  Phase j belongs to thread j % 1024 throughout (PW below is a multiple of 1024 whenever it is not
    // P itself), which carries its three folds in the partial vector between rounds.  A round recomputes r for a tile
    // of et events x pw phases with all threads (lanes along phases: x and y coalesced) into LDS, then the owners fold
    // their phases over the tile's events in event order.
    for (int j = tid; j < P; j += kFitThreads) out[8 + j] = 0.0, out[8 + P + j] = 0.0, out[8 + 2 * P + j] = 0.0;
    const int PW = P < kFitStage ? P : kFitStage, ET = kFitStage / PW;
    for (int j0 = 0; j0 < P; j0 += PW) {
        const int pw = P - j0 < PW ? P - j0 : PW;
        for (int er = 0; er < ne; er += ET) {
            const int et = ne - er < ET ? ne - er : ET;
            __syncthreads();   // the previous tile has been folded
            for (int p = tid; p < et * pw; p += kFitThreads) {
                const int e = p / pw, c = s_c[er + e];
                double r = 0.0;
                const bool u = c >= 0 && fit_phase(A, a, qv, A.M + (int64_t)c * A.K * A.N, s_t[er + e],
                                                   j0 + (p - e * pw) + 2, &r);
                s_r[p] = r, s_u[p] = u;
            }
            __syncthreads();
            for (int jj = tid; jj < pw; jj += kFitThreads) {
                const int j = j0 + jj;
                double ws = out[8 + j], wq = out[8 + P + j], wc = out[8 + 2 * P + j];
                for (int e = 0; e < et; e++)
                    if (s_u[e * pw + jj]) {
                        const double r = s_r[e * pw + jj], q = r * r;
                        ws += r, wq += q, wc += 1.0;
                    }
                out[8 + j] = ws, out[8 + P + j] = wq, out[8 + 2 * P + j] = wc;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_fit_final(const FitArgs A, const double *__restrict__ part, int nblk,
                                                   double *__restrict__ summary)
{
    const int a = blockIdx.x, L = 8 + 3 * (A.K - 1);
    const int64_t nb = (A.n[a] + kFitBlock - 1) / kFitBlock;
    for (int s = threadIdx.x; s < L; s += blockDim.x) {
        double v = 0.0;
        for (int64_t b = 0; b < nb; b++) v += part[((int64_t)a * nblk + b) * L + s];
        summary[(int64_t)a * L + s] = v;
    }
}

}  // namespace

int dev_spike_fit(const double *d_y, const int16_t *d_x, int64_t T, const int16_t *d_states, int64_t N, int64_t S,
                  int64_t K, const double *d_M, int64_t nchunks, const int64_t *d_first, const int64_t *d_times,
                  int64_t dcap, const int64_t *counts, const int32_t *qv, double *d_amp, double *d_rss,
                  double *d_energy, int32_t *d_nused, int32_t *d_chunk, double *d_part, double *d_summary,
                  hipStream_t st)
{
    HS_CHECK(N >= 1 && N <= 32 && K >= 2 && nchunks >= 0 && nchunks <= kTrackChunks, HMMSORT_EINVAL,
             "spike_fit: bad sizes");
    FitArgs A;
    A.y = d_y, A.x = d_x, A.T = T, A.states = d_states, A.N = (int)N, A.S = (int)S, A.K = (int)K;
    A.M = d_M, A.nchunks = (int)nchunks, A.first = d_first, A.times = d_times, A.dcap = dcap;
    A.amp = d_amp, A.rss = d_rss, A.energy = d_energy, A.nused = d_nused, A.chunk = d_chunk;
    int64_t maxn = 0;
    for (int i = 0; i < 32; i++) {
        A.n[i] = i < N ? counts[i] : 0;
        A.qv[i] = i < N ? qv[i] : 2;
        maxn = std::max(maxn, A.n[i]);
    }
    HS_CHECK(maxn <= dcap, HMMSORT_EINVAL, "spike_fit: more events than the device arrays hold");
    if (maxn == 0) return HMMSORT_OK;
    const int nblk = (int)spike_fit_blocks(maxn);
    hipLaunchKernelGGL(k_fit_events, dim3((unsigned)((maxn + 3) / 4), (unsigned)N), dim3(256), 0, st, A);
    HS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_fit_partials, dim3((unsigned)nblk, (unsigned)N), dim3(kFitThreads), 0, st, A, d_part, nblk);
    HS_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_fit_final, dim3((unsigned)N), dim3(256), 0, st, A, (const double *)d_part, nblk, d_summary);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

}  // namespace hmmsort
