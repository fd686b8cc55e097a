// The blocked E-step and posterior sweep of generic_estep.hip for models whose two state columns do not fit the
// LDS of a CU (about 9 900 states): three- and four-template overlap models at K = 60 have 10 621 and 21 123.
// Opt-in through option "blocked_hbm_columns" (DESIGN 3.1c "Columns in device memory").
//
// Same recursion, same arithmetic (scaled linear domain, emission shift by the column maximum, gamma normalised
// per sample), same block / halo geometry, same boundary records and outputs as generic_estep_block.inc, so
// bes_check, bes_reduce, bes_mstep, bes_logz and the diagnostics are shared.  What differs is where things live:
//   - the two columns ping-pong in a per-workgroup scratch in device memory, cols[grid][2][S]; a column written in
//     one step is read in the next by other waves of the same workgroup, i.e. of the same CU, behind the
//     __syncthreads() the sweep already has.  LDS keeps the reduction slots and the silent state's xterm / xw / xd;
//   - a thread walks its states in a strided loop (j = tid; j < S; j += nt) and reads their constants -- mean, first
//     in-edge, first out-edge, the bounds of the rest of both lists, the posterior membership bits -- from one packed
//     record per state (BigRec, 56 B x S, shared by all workgroups); the emission exponent of the next column is
//     recomputed from the mean instead of being carried in a register (the same expression, the same bits);
//   - the unnormalised gamma of a sample waits for its normaliser in the window row its alpha came from (the alpha
//     has been consumed by then), and G0 / G1 are summed by plain read-modify-write in the block's partG row: a
//     state belongs to one thread of one workgroup, so neither needs an atomic.
#include <cmath>

#include "fastmath.h"
#include "generic_dev.h"
#include "hmmsort_internal.h"
#include "generic_estep_common.h"

namespace hmmsort {

namespace {

struct BigRec {
    double m, wi0, wo0;          // mean; weight of the first incoming / outgoing transition (0: none)
    int32_t si0, do0;            // their source / destination
    int32_t p0, p1, q0, q1;      // the rest of both lists in the CSR arrays
    int32_t memb, pad;           // 3 bits per template: onset, occupied, trough (posterior sweep)
};

struct BigQv { int v[kPostMaxN]; };

__global__ __launch_bounds__(256) void besb_pack(int S, const double *__restrict__ mean,
                                                 const int32_t *__restrict__ in_ptr, const int32_t *__restrict__ in_src,
                                                 const double *__restrict__ in_w, const int32_t *__restrict__ out_ptr,
                                                 const int32_t *__restrict__ out_dst, const double *__restrict__ out_w,
                                                 const int16_t *__restrict__ states, int N, BigQv qv,
                                                 BigRec *__restrict__ rec)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= S) return;
    BigRec r;
    r.m = mean[j];
    r.p0 = in_ptr[j];  r.p1 = in_ptr[j + 1];
    r.q0 = out_ptr[j]; r.q1 = out_ptr[j + 1];
    const bool hi = r.p1 > r.p0, ho = r.q1 > r.q0;
    r.si0 = hi ? in_src[r.p0] : 0;  r.wi0 = hi ? in_w[r.p0] : 0.0;
    r.do0 = ho ? out_dst[r.q0] : 0; r.wo0 = ho ? out_w[r.q0] : 0.0;
    r.p0 += hi; r.q0 += ho;               // the lists now start at their second edge
    int mk = 0;
    if (states)
        for (int l = 0; l < N && l < kPostMaxN; l++) {
            const int v = states[l + (size_t)N * j];
            mk |= ((v == 2 ? 1 : 0) | (v > 1 ? 2 : 0) | (v == qv.v[l] ? 4 : 0)) << (3 * l);
        }
    r.memb = mk; r.pad = 0;
    rec[j] = r;
}

// POST 0: the E-step (po unused); POST 1: the posterior sweep with partial sums for NP templates
template <int POST, int NP>
__global__ __launch_bounds__(1024) void besb_block(BesArgs a, BesPost po, const BigRec *__restrict__ srec, double *cols)
{
    extern __shared__ double sh[];
    const int S = a.S, B = a.B, H = a.H, tid = threadIdx.x, nt = blockDim.x;
    const int wv = tid >> 6, nw = nt >> 6;
    const int nred = POST ? po.nred : 3;
    double *col[2] = {cols + (size_t)blockIdx.x * 2 * S, cols + (size_t)blockIdx.x * 2 * S + S};
    double *red = sh;                              // [2][nred][kRedW]
    double *xterm = red + 2 * nred * kRedW;        // [2][nsrc1]
    double *xw = xterm + 2 * a.nsrc1, *xd = xw + a.nsrc1;
    for (int i = tid; i < a.nsrc1; i += nt) { xw[i] = a.out_w[i]; xd[i] = (double)a.out_dst[i]; }
    const int64_t T = a.T;
    const double rden = a.rden;
    double *win = a.win + (size_t)blockIdx.x * B * S;

    double pacc[3 * NP], bestv = -1.0;
    int bests = 0;
    auto post_clear = [&]() {
#pragma unroll
        for (int i = 0; i < 3 * NP; i++) pacc[i] = 0.0;
        bestv = -1.0; bests = 0;
    };
    auto post_add = [&](int memb, int j, double gk) {   // j rises within a thread: the lower state keeps a tie
        if (gk > bestv) { bestv = gk; bests = j; }
#pragma unroll
        for (int l = 0; l < NP; l++) {
            const int mk = memb >> (3 * l);
            pacc[3 * l + 0] += (mk & 1) ? gk : 0.0;
            pacc[3 * l + 1] += (mk & 2) ? gk : 0.0;
            pacc[3 * l + 2] += (mk & 4) ? gk : 0.0;
        }
    };
    auto post_reduce = [&](int par, double g0) {
        double *r = red + (size_t)(par * nred + 3) * kRedW;
#pragma unroll
        for (int l = 0; l < NP; l++)
            if (l < po.N) {
                const double v0 = wsum(pacc[3 * l]), v1 = wsum(pacc[3 * l + 1]), v2 = wsum(pacc[3 * l + 2]);
                if ((tid & 63) == 0) {
                    r[(3 * l + 0) * kRedW + wv] = v0;
                    r[(3 * l + 1) * kRedW + wv] = v1;
                    r[(3 * l + 2) * kRedW + wv] = v2;
                }
            }
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(bestv, o);
            const int os = __shfl_xor(bests, o);
            if (ov > bestv || (ov == bestv && os < bests)) { bestv = ov; bests = os; }
        }
        if ((tid & 63) == 0) {
            r[(3 * po.N + 1) * kRedW + wv] = bestv;
            r[(3 * po.N + 2) * kRedW + wv] = (double)bests;
        }
        if (tid == 0) r[(3 * po.N) * kRedW] = g0;
    };
    auto post_emit = [&](int par, double rz, int64_t t) {
        const double *r = red + (size_t)(par * nred + 3) * kRedW;
        const int n3 = 3 * po.N;
        if (tid < n3) {
            double v = 0.0;
            for (int w = 0; w < nw; w++) v += r[tid * kRedW + w];
            v *= rz;
            const int l = tid / 3, q = tid - 3 * l;
            double *dst = q == 0 ? po.onset : (q == 1 ? po.occ : po.tq);
            if (dst) dst[(size_t)l * a.T + t] = v;
        } else if (tid == n3) {
            if (po.silent) po.silent[t] = r[n3 * kRedW] * rz;
        } else if (tid == n3 + 1) {
            double bv = r[(n3 + 1) * kRedW];
            int bs = (int)r[(n3 + 2) * kRedW];
            for (int w = 1; w < nw; w++) {
                const double ov = r[(n3 + 1) * kRedW + w];
                const int os = (int)r[(n3 + 2) * kRedW + w];
                if (ov > bv || (ov == bv && os < bs)) { bv = ov; bs = os; }
            }
            po.xm[t] = (int16_t)(bs + 1);
        }
    };

    auto reduce3 = [&](int par, double s, double mx, double z) {
        s = wsum(s); mx = wmax(mx); z = wsum(z);
        if ((tid & 63) == 0) {
            red[(par * nred + 0) * kRedW + wv] = s;
            red[(par * nred + 1) * kRedW + wv] = mx;
            red[(par * nred + 2) * kRedW + wv] = z;
        }
    };
    auto read3 = [&](int par, double &s, double &mx, double &z) {
        s = 0.0; mx = -INFINITY; z = 0.0;
        for (int w = 0; w < nw; w++) {
            s += red[(par * nred + 0) * kRedW + w];
            mx = fmax(mx, red[(par * nred + 1) * kRedW + w]);
            z += red[(par * nred + 2) * kRedW + w];
        }
    };
    auto expo = [&](double yv, double m) { const double d = yv - m; return -(d * d) * rden; };

    for (int blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
        const int64_t lo = (int64_t)blk * B, hi = (lo + B) < T ? (lo + B) : T;
        double *rec = a.rec + (size_t)blk * 6 * S;
        double *pG = a.partG + (size_t)blk * 2 * S;
        // ------------------------------------------------------------------ forward
        {
            const int64_t t0 = lo > H ? lo - H : 0;   // a warm-up reaching the start of the data is the exact sweep
            const double y0 = a.y[t0];
            double pm = -INFINITY;
            for (int j = tid; j < S; j += nt) {
                pm = fmax(pm, expo(y0, srec[j].m));
                if (!POST) { pG[j] = 0.0; pG[S + j] = 0.0; }   // summed into by this thread only, in the backward sweep
            }
            __syncthreads();                       // previous block is done with red / col
            reduce3(0, 0.0, pm, 0.0);
            __syncthreads();
            double s, emax, z;
            read3(0, s, emax, z);
            __syncthreads();
            const double y1 = a.y[(t0 + 1) < T ? (t0 + 1) : t0];
            double ps = 0.0;
            pm = -INFINITY;
            for (int j = tid; j < S; j += nt) {
                const double m = srec[j].m;
                const double v = fexp(expo(y0, m) - emax);
                col[0][j] = v;
                ps += v;
                if (t0 >= lo) win[j] = v;
                pm = fmax(pm, expo(y1, m));
            }
            reduce3(0, ps, pm, 0.0);
            int par = 0;
            double *lls = POST ? po.lls + (size_t)blockIdx.x * B : nullptr;
            double esum = 0.0, eprev = emax;
            double yc = y1;                                         // y[t] of the step about to run
            double ynext = a.y[(t0 + 2) < T ? (t0 + 2) : T - 1];
            for (int64_t t = t0 + 1; t < hi; t++) {
                const double yn = ynext;                            // y[t + 1]
                ynext = a.y[(t + 2) < T ? (t + 2) : T - 1];
                __syncthreads();
                read3(par, s, emax, z);
                if (POST) {
                    if (t - 1 >= lo) {
                        esum += eprev;
                        if (tid == 0) lls[t - 1 - lo] = s;
                    }
                    eprev = emax;
                }
                const double inv = 1.0 / s;
                const double *prev = col[par];
                double *cur = col[par ^ 1];
                const bool own = t >= lo;
                double *wrow = win + (size_t)(own ? t - lo : 0) * S;
                ps = 0.0; pm = -INFINITY;
                for (int j = tid; j < S; j += nt) {
                    const BigRec r = srec[j];
                    double acc = prev[r.si0] * r.wi0;
                    for (int e = r.p0; e < r.p1; e++) acc += prev[a.in_src[e]] * a.in_w[e];   // :47
                    const double v = (acc * inv) * fexp(expo(yc, r.m) - emax);
                    cur[j] = v;
                    ps += v;
                    if (own) wrow[j] = v;
                    if (t == lo - 1) rec[j] = v;
                    if (t == hi - 1) rec[S + j] = v;
                    pm = fmax(pm, expo(yn, r.m));
                }
                par ^= 1;
                reduce3(par, ps, pm, 0.0);
                yc = yn;
            }
            if (POST) {
                __syncthreads();
                read3(par, s, emax, z);               // column hi - 1
                esum += eprev;
                if (tid == 0) lls[hi - 1 - lo] = s;
                __syncthreads();
                double pl = 0.0;
                for (int64_t i = tid; i < hi - lo; i += nt) pl += log(lls[i]);
                pl = wsum(pl);
                if ((tid & 63) == 0) red[wv] = pl;    // everyone has read red[par] before the barrier above
                __syncthreads();
                if (tid == 0) {
                    pl = 0.0;
                    for (int w = 0; w < nw; w++) pl += red[w];
                    po.partL[blk] = pl + esum;
                }
            }
        }
        // ------------------------------------------------------------------ backward + statistics
        {
            const int64_t te = (hi - 1 + H) < (T - 1) ? (hi - 1 + H) : (T - 1);
            double X = 0.0, Gam0 = 0.0;            // X: thread i < nsrc1 owns transition i; Gam0: thread 0
            double g0v = 0.0;                      // thread 0: the silent state's unnormalised gamma of time tprev
            const double ye = a.y[te];
            double pm = -INFINITY;
            for (int j = tid; j < S; j += nt) pm = fmax(pm, expo(ye, srec[j].m));
            __syncthreads();
            reduce3(0, 0.0, pm, 0.0);
            __syncthreads();
            double s, emax, z;
            read3(0, s, emax, z);
            __syncthreads();
            // column te: beta = 1 (:80 at the end of the data; a flat start elsewhere).  nxt = b(te) * beta(te)
            double ps = 0.0, pz = 0.0;
            pm = -INFINITY;
            if (POST) post_clear();
            {
                const double yp = a.y[te > 0 ? te - 1 : 0];
                for (int j = tid; j < S; j += nt) {
                    const BigRec r = srec[j];
                    const double cur = 1.0;
                    ps += cur;
                    if (te < hi) {                 // the last sample of the data is an owned sample
                        const double g = win[(size_t)(te - lo) * S + j] * cur;   // = alpha: the row already holds g
                        pz += g;
                        if (j == 0) g0v = g;
                        if (POST) post_add(r.memb, j, g);
                        if (te == lo) rec[4 * S + j] = cur;
                    }
                    if (te == hi) rec[3 * S + j] = cur;
                    col[0][j] = cur * fexp(expo(ye, r.m) - emax);
                    pm = fmax(pm, expo(yp, r.m));
                }
            }
            reduce3(0, ps, pm, pz);
            if (POST && te < hi) post_reduce(0, g0v);
            int par = 0;
            int64_t tprev = te;                    // time whose g (in its window row) / xterm wait for their normaliser
            double y_cur = a.y[te], y_m1 = a.y[te > 0 ? te - 1 : 0], y_m2 = a.y[te > 1 ? te - 2 : 0];
            for (int64_t t = te - 1; t >= lo; t--) {
                // y_cur = y[t+1], y_m1 = y[t], y_m2 = y[t-1]
                const double yv = y_cur, yt = y_m1, yp = y_m2;
                y_cur = y_m1; y_m1 = y_m2;
                y_m2 = a.y[t > 1 ? t - 2 : 0];
                __syncthreads();
                read3(par, s, emax, z);
                const double inv = 1.0 / s;
                // lagged statistics of time tprev = t + 1 (its normaliser z has just arrived)
                const bool lag = tprev < hi;
                const double rz = lag ? 1.0 / z : 0.0;
                const double *grow = win + (size_t)(lag ? tprev - lo : 0) * S;
                if (lag) {
                    if (POST) post_emit(par, rz, tprev);
                    else if (tprev <= T - 2) {
                        if (tid < a.nsrc1) X += xterm[par * a.nsrc1 + tid] * rz;
                        if (tid == 0) Gam0 += g0v * rz;
                    }
                }
                const double *nxt = col[par];
                double *out = col[par ^ 1];
                const bool own = t < hi;
                double *arow = win + (size_t)(own ? t - lo : 0) * S;
                ps = 0.0; pz = 0.0; pm = -INFINITY;
                if (POST) post_clear();
                for (int j = tid; j < S; j += nt) {
                    const BigRec r = srec[j];
                    if (lag) {
                        if (!POST) {
                            const double gm = grow[j] * rz;
                            pG[j] += gm;
                            pG[S + j] += gm * yv;
                            if (tprev == hi - 1) rec[2 * S + j] = gm;
                        } else if (tprev == hi - 1) rec[2 * S + j] = grow[j] * rz;
                    }
                    double cur = nxt[r.do0] * r.wo0;
                    for (int e = r.q0; e < r.q1; e++) cur += nxt[a.out_dst[e]] * a.out_w[e];   // :94
                    ps += cur;
                    if (own) {
                        const double al = arow[j];
                        const double g = al * cur;
                        arow[j] = g;               // alpha(t) is spent: its place keeps g until z arrives
                        pz += g;
                        if (j == 0) g0v = g;
                        if (t == lo) rec[4 * S + j] = cur;
                        if (POST) post_add(r.memb, j, g);
                        else if (j == 0 && t <= T - 2)
                            for (int i = 0; i < a.nsrc1; i++)   // :240  alpha_1(t) a_1j b_j(t+1) beta_j(t+1)
                                xterm[(par ^ 1) * a.nsrc1 + i] = al * (nxt[(int)xd[i]] * xw[i]);
                    }
                    if (t == hi) rec[3 * S + j] = cur;
                    out[j] = (cur * inv) * fexp(expo(yt, r.m) - emax);
                    pm = fmax(pm, expo(yp, r.m));
                }
                par ^= 1;
                reduce3(par, ps, pm, pz);
                if (POST && own) post_reduce(par, g0v);
                tprev = t;
            }
            // flush the statistics of the block's first sample
            __syncthreads();
            read3(par, s, emax, z);
            if (tprev < hi) {
                const double rz = 1.0 / z, yv = y_cur;              // y[tprev]
                if (POST) post_emit(par, rz, tprev);
                const double *grow = win + (size_t)(tprev - lo) * S;
                for (int j = tid; j < S; j += nt) {
                    const double gm = grow[j] * rz;
                    if (!POST) { pG[j] += gm; pG[S + j] += gm * yv; }
                    if (tprev == hi - 1) rec[2 * S + j] = gm;
                    if (tprev == lo) rec[5 * S + j] = gm;
                }
                if (!POST && tprev <= T - 2) {
                    if (tid < a.nsrc1) X += xterm[par * a.nsrc1 + tid] * rz;
                    if (tid == 0) Gam0 += g0v * rz;
                }
            }
            if (POST) continue;                    // no block statistics: bes_reduce and the M-step do not run
            double *pX = a.partX + (size_t)blk * (a.nsrc1 + 2);
            if (tid < a.nsrc1) pX[tid] = X;
            if (tid == 0) pX[a.nsrc1] = Gam0;
            double y2 = 0.0;
            for (int64_t t = lo + tid; t < hi; t += nt) { const double v = a.y[t]; y2 += v * v; }
            __syncthreads();
            reduce3(0, y2, 0.0, 0.0);
            __syncthreads();
            read3(0, s, emax, z);
            if (tid == 0) pX[a.nsrc1 + 1] = s;
        }
    }
}

}  // namespace

// Workspace of the device-memory-column path.  grid = min(blocks, CUs, what half of the free device memory holds),
// at least 1: every resident workgroup owns a window of B x S doubles (86 MB at 21 123 states, B = 512) and two
// columns.  Decided once per plan, on the first sweep.
int blocked_big_prepare(GenericDev *g)
{
    if (g->d_es_win && g->d_es_cols && g->d_es_srec) return HMMSORT_OK;
    const size_t S = (size_t)g->S, nb = (size_t)g->nblk;
    const size_t per_wg = ((size_t)g->B * S + 2 * S + (size_t)g->B) * sizeof(double);
    const size_t fixed = (nb * 8 * S + nb * (g->nsrc1 + 3) + 2 * (size_t)g->R + 2 * S + g->K * g->N) * sizeof(double) +
                         S * sizeof(BigRec);
    int dev = 0, ncu = 256;
    HS_HIP(hipGetDevice(&dev));
    HS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    size_t free_b = 0, total_b = 0;
    HS_HIP(hipMemGetInfo(&free_b, &total_b));
    HS_CHECK(per_wg + fixed <= free_b, HMMSORT_ENOMEM,
             "blocked E-step (device-memory columns): one workgroup needs %zu bytes of window and columns and the plan "
             "%zu bytes of boundary records and statistics; %zu bytes are free", per_wg, fixed, free_b);
    const size_t fit = std::max<size_t>((free_b / 2) / per_wg, 1);
    const int grid = (int)std::min<size_t>(std::min<size_t>(nb, (size_t)ncu), fit);
    int rc;
    if ((rc = balloc(&g->d_es_win, (size_t)grid * g->B * S, &g->bytes)) ||
        (rc = balloc(&g->d_es_cols, (size_t)grid * 2 * S, &g->bytes)) ||
        (rc = balloc(&g->d_es_srec, S * sizeof(BigRec), &g->bytes)))
        return rc;
    g->es_grid = grid;
    return HMMSORT_OK;
}

// the block kernel over buffers bes_run has allocated and cleared; post == nullptr: the E-step
int blocked_big_launch(GenericDev *g, const double *d_y, const BigPost *post, hipStream_t st)
{
    const size_t S = (size_t)g->S;
    BesArgs a;
    bes_fill_args(a, g, d_y);
    BesPost po = {};
    if (post) {
        po.states = g->d_states;
        for (int l = 0; l < kPostMaxN; l++) po.qv[l] = post->qv[l];
        po.N = (int)g->N; po.nred = 3 + 3 * (int)g->N + 3;
        po.onset = post->onset; po.occ = post->occ; po.tq = post->tq; po.silent = post->silent; po.xm = post->xm;
        po.lls = g->d_es_lls; po.partL = g->d_es_partL;
    }
    BigQv qv;
    for (int l = 0; l < kPostMaxN; l++) qv.v[l] = po.qv[l];
    BigRec *srec = (BigRec *)g->d_es_srec;
    hipLaunchKernelGGL(besb_pack, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, (int)S, a.mean, a.in_ptr, a.in_src,
                       a.in_w, a.out_ptr, a.out_dst, a.out_w, po.states, (int)g->N, qv, srec);
    const int nred = post ? po.nred : 3;
    const size_t lds = (2 * (size_t)nred * kRedW + 4 * (size_t)g->nsrc1) * sizeof(double);
    const int nt = S <= 256 ? 256 : (S <= 4096 ? 512 : 1024);
    const dim3 grid((unsigned)g->es_grid);
    if (!post) hipLaunchKernelGGL((besb_block<0, 1>), grid, dim3(nt), lds, st, a, po, (const BigRec *)srec, g->d_es_cols);
    else if (po.N <= 2) hipLaunchKernelGGL((besb_block<1, 2>), grid, dim3(nt), lds, st, a, po, (const BigRec *)srec, g->d_es_cols);
    else hipLaunchKernelGGL((besb_block<1, 4>), grid, dim3(nt), lds, st, a, po, (const BigRec *)srec, g->d_es_cols);
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

}  // namespace hmmsort
