// The block kernel of generic_estep.hip, included twice: BES_POST 0 gives bes_block, the E-step, whose text is
// what it was before the posterior path existed (the preprocessor, not the optimiser, removes the additions, so
// its instructions cannot move); BES_POST 1 gives bes_block_post, which keeps the gamma of every owned sample
// (DESIGN 3.5 "Blocked path").  There the partial sums of the UNNORMALISED g ride on the reduction that carries
// the normaliser z and are scaled by 1/z when z is read, one step late, behind the barrier the sweep already
// has.  occ is summed over its own set (phase > 1), not formed as 1 - complement: a sum of non-negative terms,
// absolute error <= S ulp.
#if BES_POST
#define BES_NRED po.nred
#else
#define BES_NRED 3
#endif

// NTH = threads per workgroup (the launch bound decides the register budget: 512 threads leave 256 VGPRs per
// lane, which the per-state constants of 8 states per thread need; under a 1024-thread bound they spill 776 B)
#if BES_POST
template <int SPT, int NTH, int NP>
__global__ __launch_bounds__(NTH) void bes_block_post(BesArgs a, BesPost po)
#else
template <int SPT, int NTH>
__global__ __launch_bounds__(NTH) void bes_block(BesArgs a)
#endif
{
    extern __shared__ double sh[];
    const int S = a.S, B = a.B, H = a.H, tid = threadIdx.x, nt = blockDim.x;
    const int wv = tid >> 6, nw = nt >> 6;
    double *col[2] = {sh, sh + S};
    double *red = sh + 2 * S;                      // [2][BES_NRED][kRedW]
    double *xterm = red + 2 * BES_NRED * kRedW;    // [2][nsrc1]
    double *xw = xterm + 2 * a.nsrc1, *xd = xw + a.nsrc1;   // the silent state's outgoing transitions: weight, destination
    for (int i = tid; i < a.nsrc1; i += nt) { xw[i] = a.out_w[i]; xd[i] = (double)a.out_dst[i]; }
    const int64_t T = a.T;
    // per-thread constants of its SPT states.  93 % of the states of an overlap model have ONE incoming and one
    // outgoing transition (the interior of the pair lattice): the first edge of each list lives in registers, the
    // rest of a list is read from the (L2-resident) CSR arrays -- one dependent global load per edge and step was
    // what bounded the first version (98 -> see DESIGN 3.1c)
    double m[SPT], en[SPT], wi0[SPT], wo0[SPT];
    int p0[SPT], p1[SPT], q0[SPT], q1[SPT], si0[SPT], do0[SPT];
#pragma unroll
    for (int k = 0; k < SPT; k++) {
        const int j = tid + k * nt;
        const bool ok = j < S;
        m[k] = ok ? a.mean[j] : 0.0;
        p0[k] = ok ? a.in_ptr[j] : 0;  p1[k] = ok ? a.in_ptr[j + 1] : 0;
        q0[k] = ok ? a.out_ptr[j] : 0; q1[k] = ok ? a.out_ptr[j + 1] : 0;
        const bool hi = p1[k] > p0[k], ho = q1[k] > q0[k];
        si0[k] = hi ? a.in_src[p0[k]] : 0;  wi0[k] = hi ? a.in_w[p0[k]] : 0.0;
        do0[k] = ho ? a.out_dst[q0[k]] : 0; wo0[k] = ho ? a.out_w[q0[k]] : 0.0;
        p0[k] += hi; q0[k] += ho;             // the lists now start at their second edge
    }
    double *win = a.win + (size_t)blockIdx.x * B * S;
#if BES_POST
    // membership of the thread's states, 3 bits per template (onset, occupied, trough), fixed for the whole sweep
    const int nred = po.nred;
    int memb[SPT];
    double pacc[3 * NP], bestv = -1.0;
    int bests = 0;
#pragma unroll
    for (int k = 0; k < SPT; k++) {
        const int j = tid + k * nt;
        int mk = 0;
        if (j < S)
            for (int l = 0; l < po.N; l++) {
                const int v = po.states[l + (size_t)po.N * j];
                mk |= ((v == 2 ? 1 : 0) | (v > 1 ? 2 : 0) | (v == po.qv[l] ? 4 : 0)) << (3 * l);
            }
        memb[k] = mk;
    }
    auto post_clear = [&]() {
#pragma unroll
        for (int i = 0; i < 3 * NP; i++) pacc[i] = 0.0;
        bestv = -1.0; bests = 0;
    };
    auto post_add = [&](int k, int j, double gk) {   // j rises with k: the lower state number keeps a tie
        if (gk > bestv) { bestv = gk; bests = j; }
#pragma unroll
        for (int l = 0; l < NP; l++) {
            const int mk = memb[k] >> (3 * l);
            pacc[3 * l + 0] += (mk & 1) ? gk : 0.0;
            pacc[3 * l + 1] += (mk & 2) ? gk : 0.0;
            pacc[3 * l + 2] += (mk & 4) ? gk : 0.0;
        }
    };
    // wave sums of the partial marginals into red[par][3 ..]; g0 = the silent state's g (thread 0 only)
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
    // marginals of sample t from red[par] once its normaliser is known: thread i < 3 N finishes slot i, the next
    // two the silent state and the arg max
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
#endif

    auto reduce3 = [&](int par, double s, double mx, double z) {
        s = wsum(s); mx = wmax(mx); z = wsum(z);
        if ((tid & 63) == 0) {
            red[(par * BES_NRED + 0) * kRedW + wv] = s;
            red[(par * BES_NRED + 1) * kRedW + wv] = mx;
            red[(par * BES_NRED + 2) * kRedW + wv] = z;
        }
    };
    auto read3 = [&](int par, double &s, double &mx, double &z) {
        s = 0.0; mx = -INFINITY; z = 0.0;
        for (int w = 0; w < nw; w++) {
            s += red[(par * BES_NRED + 0) * kRedW + w];
            mx = fmax(mx, red[(par * BES_NRED + 1) * kRedW + w]);
            z += red[(par * BES_NRED + 2) * kRedW + w];
        }
    };

    for (int blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
        const int64_t lo = (int64_t)blk * B, hi = (lo + B) < T ? (lo + B) : T;
        double *rec = a.rec + (size_t)blk * 6 * S;
        // ------------------------------------------------------------------ forward
        {
            const int64_t t0 = lo > H ? lo - H : 0;   // a warm-up reaching the start of the data is the exact sweep
            // column t0 = shifted emissions (baumwelch.jl:36 at the start of the data; a flat start elsewhere)
            const double y0 = a.y[t0];
            double pm = -INFINITY;
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                const double d = y0 - m[k];
                en[k] = -(d * d) * a.rden;
                if (tid + k * nt < S) pm = fmax(pm, en[k]);
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
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                const int j = tid + k * nt;
                if (j < S) {
                    const double v = fexp(en[k] - emax);
                    col[0][j] = v;
                    ps += v;
                    if (t0 >= lo) win[j] = v;
                    const double d = y1 - m[k];
                    en[k] = -(d * d) * a.rden;
                    pm = fmax(pm, en[k]);
                }
            }
            reduce3(0, ps, pm, 0.0);
            int par = 0;
#if BES_POST
            // log-likelihood terms of the owned samples: column t has the sum s_t over the shifted emissions
            // exp(e_j - emax_t), so log p(y_t | y_<t) = log s_t + emax_t - log(sigma sqrt(2 pi)).  s_t is read one
            // step late; thread 0 parks it in lls and the logs are taken in parallel after the sweep
            double *lls = po.lls + (size_t)blockIdx.x * B;
            double esum = 0.0, eprev = emax;
#endif
            double ynext = a.y[(t0 + 2) < T ? (t0 + 2) : T - 1];   // global loads run one step ahead of their use
            for (int64_t t = t0 + 1; t < hi; t++) {
                const double yn = ynext;                            // y[t + 1]
                ynext = a.y[(t + 2) < T ? (t + 2) : T - 1];
                __syncthreads();
                read3(par, s, emax, z);
#if BES_POST
                if (t - 1 >= lo) {
                    esum += eprev;
                    if (tid == 0) lls[t - 1 - lo] = s;
                }
                eprev = emax;
#endif
                const double inv = 1.0 / s;
                const double *prev = col[par];
                double *cur = col[par ^ 1];
                ps = 0.0; pm = -INFINITY;
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const int j = tid + k * nt;
                    if (j < S) {
                        double acc = prev[si0[k]] * wi0[k];
                        for (int e = p0[k]; e < p1[k]; e++) acc += prev[a.in_src[e]] * a.in_w[e];   // :47
                        const double v = (acc * inv) * fexp(en[k] - emax);
                        cur[j] = v;
                        ps += v;
                        if (t >= lo) win[(size_t)(t - lo) * S + j] = v;
                        if (t == lo - 1) rec[j] = v;
                        if (t == hi - 1) rec[S + j] = v;
                        const double d = yn - m[k];
                        en[k] = -(d * d) * a.rden;
                        pm = fmax(pm, en[k]);
                    }
                }
                par ^= 1;
                reduce3(par, ps, pm, 0.0);
            }
#if BES_POST
            {
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
#endif
        }
        // ------------------------------------------------------------------ backward + statistics
        {
            const int64_t te = (hi - 1 + H) < (T - 1) ? (hi - 1 + H) : (T - 1);
            double g[SPT], G0[SPT], G1[SPT];
#pragma unroll
            for (int k = 0; k < SPT; k++) { g[k] = 0.0; G0[k] = 0.0; G1[k] = 0.0; }
            double X = 0.0, Gam0 = 0.0;            // X: thread i < nsrc1 owns transition i; Gam0: thread 0
            // emission exponents of column te and their maximum
            const double ye = a.y[te];
            double pm = -INFINITY;
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                const double d = ye - m[k];
                en[k] = -(d * d) * a.rden;
                if (tid + k * nt < S) pm = fmax(pm, en[k]);
            }
            __syncthreads();
            reduce3(0, 0.0, pm, 0.0);
            __syncthreads();
            double s, emax, z;
            read3(0, s, emax, z);
            __syncthreads();
            // column te: beta = 1 (:80 at the end of the data; a flat start elsewhere).  nxt = b(te) * beta(te)
            double ps = 0.0, pz = 0.0;
            pm = -INFINITY;
#if BES_POST
            post_clear();
#endif
            {
                const double yp = a.y[te > 0 ? te - 1 : 0];
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const int j = tid + k * nt;
                    if (j < S) {
                        const double cur = 1.0;
                        ps += cur;
                        if (te < hi) {             // the last sample of the data is an owned sample
                            const double al = win[(size_t)(te - lo) * S + j];
                            g[k] = al * cur;
                            pz += g[k];
#if BES_POST
                            post_add(k, j, g[k]);
#endif
                            if (te == lo) rec[4 * S + j] = cur;
                        }
                        if (te == hi) rec[3 * S + j] = cur;
                        col[0][j] = cur * fexp(en[k] - emax);
                        const double d = yp - m[k];
                        en[k] = -(d * d) * a.rden;
                        pm = fmax(pm, en[k]);
                    }
                }
            }
            reduce3(0, ps, pm, pz);
#if BES_POST
            if (te < hi) post_reduce(0, g[0]);
#endif
            int par = 0;
            int64_t tprev = te;                    // time whose g[] / xterm wait for their normaliser
            // global loads one step ahead: y[t-1] for the next emissions, alpha(t) of the owned samples
            double y_cur = a.y[te], y_m1 = a.y[te > 0 ? te - 1 : 0], y_m2 = a.y[te > 1 ? te - 2 : 0];
            double alc[SPT];
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                const int j = tid + k * nt;
                alc[k] = (j < S && te - 1 < hi && te - 1 >= lo) ? win[(size_t)(te - 1 - lo) * S + j] : 0.0;
            }
            for (int64_t t = te - 1; t >= lo; t--) {
                // y_cur = y[t+1], y_m1 = y[t], y_m2 = y[t-1]; alc = alpha(t)
                const double yv = y_cur, yp = y_m2;
                y_cur = y_m1; y_m1 = y_m2;
                y_m2 = a.y[t > 1 ? t - 2 : 0];
                double aln[SPT];
                const bool own_next = t - 1 < hi && t - 1 >= lo;
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const int j = tid + k * nt;
                    aln[k] = (j < S && own_next) ? win[(size_t)(t - 1 - lo) * S + j] : 0.0;
                }
                __syncthreads();
                read3(par, s, emax, z);
                const double inv = 1.0 / s;
                // lagged statistics of time tprev = t + 1 (its normaliser z has just arrived)
                if (tprev < hi) {
                    const double rz = 1.0 / z;
#if BES_POST
                    post_emit(par, rz, tprev);
                    (void)yv;
                    if (tprev == hi - 1) {
#pragma unroll
                        for (int k = 0; k < SPT; k++) {
                            const int j = tid + k * nt;
                            if (j < S) rec[2 * S + j] = g[k] * rz;
                        }
                    }
#else
#pragma unroll
                    for (int k = 0; k < SPT; k++) {
                        const int j = tid + k * nt;
                        if (j < S) {
                            const double gm = g[k] * rz;
                            G0[k] += gm;
                            G1[k] += gm * yv;
                            if (tprev == hi - 1) rec[2 * S + j] = gm;
                        }
                    }
                    if (tprev <= T - 2) {
                        if (tid < a.nsrc1) X += xterm[par * a.nsrc1 + tid] * rz;
                        if (tid == 0) Gam0 += g[0] * rz;
                    }
#endif
                }
                const double *nxt = col[par];
                double *out = col[par ^ 1];
                const bool own = t < hi;
                ps = 0.0; pz = 0.0; pm = -INFINITY;
#if BES_POST
                post_clear();
#endif
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const int j = tid + k * nt;
                    if (j < S) {
                        double cur = nxt[do0[k]] * wo0[k];
                        for (int e = q0[k]; e < q1[k]; e++) cur += nxt[a.out_dst[e]] * a.out_w[e];   // :94
                        ps += cur;
                        if (own) {
                            const double al = alc[k];
                            g[k] = al * cur;
                            pz += g[k];
                            if (t == lo) rec[4 * S + j] = cur;
#if BES_POST
                            post_add(k, j, g[k]);
#else
                            if (j == 0 && t <= T - 2)
                                for (int i = 0; i < a.nsrc1; i++)   // :240  alpha_1(t) a_1j b_j(t+1) beta_j(t+1)
                                    xterm[(par ^ 1) * a.nsrc1 + i] = al * (nxt[(int)xd[i]] * xw[i]);
#endif
                        }
                        if (t == hi) rec[3 * S + j] = cur;
                        out[j] = (cur * inv) * fexp(en[k] - emax);
                        const double d = yp - m[k];
                        en[k] = -(d * d) * a.rden;
                        pm = fmax(pm, en[k]);
                    }
                }
                par ^= 1;
                reduce3(par, ps, pm, pz);
#if BES_POST
                if (own) post_reduce(par, g[0]);
#endif
                tprev = t;
#pragma unroll
                for (int k = 0; k < SPT; k++) alc[k] = aln[k];
            }
            // flush the statistics of the block's first sample
            __syncthreads();
            read3(par, s, emax, z);
            if (tprev < hi) {
                const double rz = 1.0 / z, yv = y_cur;              // y[tprev]
#if BES_POST
                post_emit(par, rz, tprev);
                (void)yv;
#endif
#pragma unroll
                for (int k = 0; k < SPT; k++) {
                    const int j = tid + k * nt;
                    if (j < S) {
                        const double gm = g[k] * rz;
                        G0[k] += gm;
                        G1[k] += gm * yv;
                        if (tprev == hi - 1) rec[2 * S + j] = gm;
                        if (tprev == lo) rec[5 * S + j] = gm;
                    }
                }
                if (tprev <= T - 2) {
                    if (tid < a.nsrc1) X += xterm[par * a.nsrc1 + tid] * rz;
                    if (tid == 0) Gam0 += g[0] * rz;
                }
            }
#if BES_POST
            continue;                              // no block statistics: bes_reduce and the M-step do not run
#endif
            double *pG = a.partG + (size_t)blk * 2 * S;
#pragma unroll
            for (int k = 0; k < SPT; k++) {
                const int j = tid + k * nt;
                if (j < S) { pG[j] = G0[k]; pG[S + j] = G1[k]; }
            }
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

#undef BES_NRED
