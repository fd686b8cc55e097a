// Wave engine, part 2: time-parallel Viterbi (reference src/viterbi.jl:44-98), one wavefront per
// chain.  Specification: tests/wave_model.py (vit_chain / vit_decode).
//
// Per sample t the recursion keeps, per chain:
//   D0(t)     = delta_t(silent)
//   P_a(t')   = delta of ring a's LAST state at t'+L-1 for the onset at t' = U_a(t') + Rfull_a(t'),
//               U_a(t') = best predecessor score of state (a,1) at t'
// and decides the back-pointer psi in {0 = silent, b = ring b's last state} of the N+1 junction
// states; candidates are scanned in source-state order (silent first, rings ascending) with a strict
// '>' -- the reference's tie rule (viterbi.jl:74-84).  Frame: delta'_t = delta_t - A*(t+1).
//
// A wavefront advances W = min(L, 64) samples per super-step: lane j owns sample t0 + j, the ring
// exits X_a(t) = P_a(t-L) it needs were produced in earlier super-steps (LDS delay line), so
// D0(t) = max(D0(t-1) + c00 + q0(t), max_a(X_a(t) + cend_a) + q0(t)) is a first-order max-plus
// recurrence across the lanes: one 6-level scan.  Every other quantity of the W samples is lane-local.
//
// Exactness.  (1) Chain starts: a chain starts Hw samples early from "silent, rings empty"; after the
// sweep its state at tc-1 is compared with the state the previous chain really ended on, ALL 1 + N*L
// entries up to one common constant (tolerance 1e-9); a chain that misses the certificate is swept
// again from the previous chain's exact end state (kw_vit with redo = 1), so the stored
// back-pointers are those of one sequential sweep.  (2) Rounding: inside a chain the arithmetic
// differs from the reference's by rounding at the 1e-13 level (pre-summed ring scores, scan order,
// per-chain offsets instead of the reference's O(t) cumulative sum, whose own rounding unit is
// larger).  Every decision records whether its winner beat the runner-up by less than
// thr = 16 (L+2) ulp(|T1|max) + 4e-9 (wave_thr, wave_common.h: the most the reference's own rounding can
// move the difference between two paths that have been apart for up to 8 (L+2) steps).  The flagged
// decisions ON THE DECODED PATH are then re-decided with the reference's own serial arithmetic
// (wave_ties.hip: exact prefix T1 along the path, candidates replayed op for op, strict '>' in list
// order); diag[7] counts the decisions that procedure could not settle (0 in every test).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "fastmath.h"
#include "wave_common.h"

namespace hmmsort {

constexpr double kVitTol = 1e-9;

// Round 11: the parts of the interior form of the sweep, each 1 = on, 0 = the parent's form (A/B builds)
#ifndef HS_VIT_INT
#define HS_VIT_INT 1    // the full owned super-steps run without the bookkeeping of partial steps
#endif
#ifndef HS_DL_REG
#define HS_DL_REG 1     // rings of at most 64 states: interior steps take the ring exits from registers, not from LDS
#endif
#ifndef HS_VIT_RCP
#define HS_VIT_RCP 1    // the division by the chain's invariant 2 sigma^2: reciprocal once, exact quotient per sample
#endif

template <int N>
struct WIn {
    double y;
    double R[N];
};

// Near-tie threshold (wave_thr, wave_common.h).  The reference compares candidates T1[k,t-1] + lp whose
// values have grown to |T1| ~ t |A - 1/2| (ulp 5e-10 after 1e7 samples, 4e-9 after 1e8).  Two candidate paths
// that separated d steps ago share the value at their common ancestor exactly and then collect 2d roundings of
// at most ulp/2 each, so the reference's computed margin differs from the exact one by at most (2d + 1) ulp.  A
// decision is flagged when its margin (in this engine's per-chain frame, rounding ~1e-13) is below
//     thr = 16 (L + 2) ulp(|T1|max) + 4e-9
// -- the worst case for paths apart for up to 8 (L + 2) steps, the 4e-9 covering the tolerance of the
// chain-boundary certificate.  Flagged decisions are not guessed: wave_ties.hip replays the reference's own
// serial arithmetic for every flagged decision on the decoded path and re-decides it exactly.
// UC ("uniform cx"): the log-probability of (b,L) -> (a,1) does not depend on b -- true for every
// list the reference builds (types.jl:94-113: lp[a] + (N-2) lpz, accumulated in an order in which the
// source ring only contributes an exact +0.0) and checked bitwise on the host (wave_set_model).  The
// best ring exit into ring a is then "largest X_b over b != a" + cxin_a: one top-3 pass over the N
// exits serves all N junctions (O(N) instead of O(N^2) per sample).  Adding the same constant is
// monotone, so the winner can differ from the reference's candidate-by-candidate scan only by a tie
// created in rounding; such a decision has a zero margin and is flagged like any other near-tie.
// One chain's sweep, the body of kw_vit (redo = false: every chain, from its warm-up) and of kw_vit_redo (redo = true:
// a chain whose certificate failed, from the previous chain's exact end state).
template <int N, bool UC, bool redo>
__device__ __forceinline__ void vit_chain(const WaveGeom &g, const WaveConst *__restrict__ cst,
                                          const double *__restrict__ y, const double *__restrict__ Rf,
                                          const double *__restrict__ virt, const double *__restrict__ ysum,
                                          uint32_t *__restrict__ psi, double *__restrict__ vpre,
                                          double *__restrict__ vend, uint32_t *__restrict__ trash, const int cg)
{
    constexpr int EB = wpsi_bits_c(N), EPW = wpsi_epw_c(N), PW = wpsi_words_c(N), D = wave_depth<N>();
    // Model constants live in LDS next to the delay line: they are wave-uniform and many; as
    // kernel-argument/global scalars the compiler hoists all their loads out of the sweep loop and spills
    // hundreds of SGPRs.  An LDS word that the loop's own stores may alias is re-read (broadcast) where
    // it is used.
    constexpr int KC0 = 3, KCEND = 3 + N, KCXT = 3 + 2 * N, KSIZE = 3 + 2 * N + N * N;
    extern __shared__ double lds_vit[];
    double *KC = lds_vit;           // c00 | mean0 | den | c0[N] | cend[N] | cxT[N*N] (UC: cxin[N] first)
    double *DL = lds_vit + KSIZE;   // [N][RB] delay line: P_a(t') at slot (t' - tinit + L) mod RB
    const int lane = threadIdx.x;
    const int ch = cg / g.nch, c = cg % g.nch;
    const int L = g.L, W = g.W, RB = g.RB, B = g.B;
    const int64_t T = g.T;
    const int64_t tc = (int64_t)c * B;
    const int nc = (int)((T - tc) < B ? (T - tc) : B);
    const int64_t tend = tc + nc;
    const double *yc = y + (int64_t)ch * T;
    const double *Rc = Rf + (int64_t)ch * N * T;
    uint32_t *psic = psi + (int64_t)ch * T;
    const int64_t SR = 1 + N * L;
    const int64_t planePsi = (int64_t)g.C * T;
    const double thr = wave_thr(g, cst[ch], ysum, ch);

    for (int i = lane; i < N * (RB + 1); i += 64) DL[i] = -INFINITY;
    {
        const WaveConst &Kg = cst[ch];
        if (lane == 0) { KC[0] = Kg.c00; KC[1] = Kg.mean0; KC[2] = Kg.den; }
        if (lane < N) { KC[KC0 + lane] = Kg.c0[lane]; KC[KCEND + lane] = Kg.cend[lane]; }
        if (UC) { if (lane < N) KC[KCXT + lane] = Kg.cxin[lane]; }
        else for (int i = lane; i < N * N; i += 64) KC[KCXT + i] = Kg.cxT[i];
    }
    __syncthreads();
    int64_t tinit;
    double D0;
    if (redo) {            // exact hand-off: the previous chain's end state
        tinit = tc - 1;
        D0 = vend[(cg - 1) * SR];
        for (int i = lane; i < N * L; i += 64) {
            const int a = i / L, j = i % L + 1;
            DL[a * (RB + 1) + (L + 1 - j)] = vend[(cg - 1) * SR + 1 + i];
        }
    } else if (c == 0) {   // the reference's first column (viterbi.jl:55-63): emission only, T1[1,1] = 0
        tinit = 0;
        D0 = -cst[ch].A;
        for (int i = lane; i < N * L; i += 64) {
            const int a = i / L, j = i % L + 1;  // virtual onset -j -> slot L - j
            DL[a * (RB + 1) + (L - j)] = virt[((int64_t)ch * N + a) * (L + 1) + j];
        }
        if (lane < N) DL[lane * (RB + 1) + L] = Rc[(int64_t)lane * T];
    } else {               // warm-up start: silent, rings empty
        tinit = tc - g.Hw;
        D0 = 0.0;
    }
    __syncthreads();

    const int n_total = (int)(tend - 1 - tinit);  // steps t = tinit+1 .. tend-1
    // Interior super-steps (STORE = 2 and 3 of run): the FULL owned steps, nact = W.  A full step's loads never
    // meet the clamp against T, every lane below W stores into the planes, and the carry leaves from lane W - 1.  The
    // scans and lane_prev move data from lower to higher lanes only, so what the lanes from W up hold is read by no
    // live lane: their inputs go unselected, and only what reaches memory (wsl, the psi stores) keeps its predicate.
    // The input pipeline looks D steps past the range; the loads clamp that offset to its last step (imax).
    const bool liveW = lane < W;
    const int liW = liveW ? lane : 0;
    int imax = 0;
    // inputs of the super-step that starts `off` steps into the sweep: uniform base + lane offset
    auto load = [&](WIn<N> &d, int off, auto store_tag) {
        if constexpr (decltype(store_tag)::value >= 2) {
            const int64_t tb = tinit + 1 + (off < imax ? off : imax);
            d.y = (yc + tb)[liW];
#pragma unroll
            for (int a = 0; a < N; a++) d.R[a] = (Rc + (int64_t)a * T + tb)[liW];
            return;
        }
        const int nact = n_total - off < W ? n_total - off : W;
        const int li = lane < nact ? lane : 0;
        int64_t tb = tinit + 1 + off;
        tb = tb < T ? tb : T - 1;
        d.y = (yc + tb)[li];
#pragma unroll
        for (int a = 0; a < N; a++) d.R[a] = (Rc + (int64_t)a * T + tb)[li];
    };
    int rs = (1 + lane) % RB, ws = (L + 1 + lane) % RB;
    // STORE = 0: warm-up super-step (no global stores at all); 1: owned super-step (psi stored by every
    // lane, idle lanes of the last partial step into a trash line).  Straight-line global accesses only:
    // with stores under divergent branches hipcc drains vmcnt to 0 every super-step, which serialises the
    // input pipeline on the HBM latency.
    // STORE = 2: interior super-step (above); 3: interior super-step of a ring with W == L, where rs and ws both
    // advance by W with ws - rs = L, so lane j reads the slot it wrote one step earlier: the exits X_a come from the
    // lane's own registers (Xr, primed from the delay line before the sweep).  Every LDS write stays, so the general
    // modes and dump find the delay line as they left it.
    [[maybe_unused]] double Xr[N];
    // The interior form, the register carry and the reciprocal are for the sweep of every chain with one entry value
    // per ring (UC), which is what every list the reference builds runs.  The re-sweep of a failed chain is held to
    // 80 registers beside an E-step and the per-source kernels have no registers to spare (DESIGN section 5 Round 11:
    // with these parts they spill); both are rare and keep the general form.
    constexpr bool FAST = UC && !redo;
    // the chain's one division (div_invariant, fastmath.h); wave-uniform, kept in scalar registers
    [[maybe_unused]] DivInv dv;
    if constexpr (FAST && HS_VIT_RCP) {
        dv = div_invariant_of(cst[ch].den);
        dv.den = wave_bcast(dv.den, 0); dv.r = wave_bcast(dv.r, 0); dv.nlo = wave_bcast(dv.nlo, 0);
    }
    auto run = [&](const WIn<N> &d, int off, auto store_tag) {
        constexpr int STORE = decltype(store_tag)::value;
        constexpr bool INT = STORE >= 2, CARRY = STORE == 3;
        const int nact = INT ? W : (n_total - off < W ? n_total - off : W);
        const bool live = INT ? liveW : lane < nact;
        const int64_t tb = tinit + 1 + off;
        double X[N];
#pragma unroll
        for (int a = 0; a < N; a++) {
            if constexpr (CARRY) X[a] = Xr[a];
            else {
                const double v = DL[a * (RB + 1) + rs];
                X[a] = (INT || live) ? v : -INFINITY;
            }
        }
        // ring exits into the silent state: best and runner-up among the rings (first maximum wins)
        double e1 = -INFINITY, e2 = -INFINITY;
        int earg = 0;
#pragma unroll
        for (int a = 0; a < N; a++) {
            const double v = X[a] + KC[KCEND + a];
            earg = v > e1 ? a + 1 : earg;
            e2 = fmax(e2, fmin(e1, v));
            e1 = fmax(e1, v);
        }
        const double c00 = KC[0];
        const double dd = d.y - KC[1];
        double q0;
        if constexpr (FAST && HS_VIT_RCP) q0 = -div_invariant(dd * dd, dv);
        else q0 = -((dd * dd) / KC[2]);
        double sa = (INT || live) ? c00 + q0 : 0.0;
        double sb = (INT || live) ? e1 + q0 : -INFINITY;
        scan_maxplus(sa, sb);
        const double Dn = fmax(D0 + sa, sb);
        const double Dprev = lane_prev(Dn, D0);
        uint32_t pw[PW];
#pragma unroll
        for (int w = 0; w < PW; w++) pw[w] = 0u;
        {
            const double v0 = Dprev + c00;
            const bool ring = e1 > v0;
            const double gap = ring ? e1 - fmax(e2, v0) : v0 - e1;
            const uint32_t fl = gap < thr ? 1u : 0u;
            pw[0] = (ring ? (uint32_t)earg : 0u) | (fl << (EB - 1));
        }
        // top three exits (first index wins ties) for the UC path
        double m1 = -INFINITY, m2 = -INFINITY, m3 = -INFINITY;
        int i1 = 0, i2 = 0;
        if (UC) {
#pragma unroll
            for (int b = 0; b < N; b++) {
                const double v = X[b];
                const bool g1 = v > m1, g2 = v > m2;
                m3 = g2 ? m2 : fmax(m3, v);
                i2 = g1 ? i1 : (g2 ? b + 1 : i2);
                m2 = g1 ? m1 : (g2 ? v : m2);
                i1 = g1 ? b + 1 : i1;
                m1 = g1 ? v : m1;
            }
        }
        const int wsl = live ? ws : RB;   // idle lanes write a spare slot behind the ring (branch-free stores)
#pragma unroll
        for (int a = 0; a < N; a++) {
            double r1 = -INFINITY, r2 = -INFINITY;
            int rarg = 0;
            if (UC) {
                const double cin = KC[KCXT + a];
                const bool first = (a + 1 == i1), second = (a + 1 == i2);
                r1 = (first ? m2 : m1) + cin;
                rarg = first ? i2 : i1;
                r2 = ((first || second) ? m3 : m2) + cin;
                if (N == 1) { r1 = -INFINITY; r2 = -INFINITY; rarg = 0; }
            } else {
#pragma unroll
                for (int b = 0; b < N; b++) {
                    if (b == a) continue;
                    const double v = X[b] + KC[KCXT + a * N + b];   // (b,L) -> (a,1)
                    rarg = v > r1 ? b + 1 : rarg;
                    r2 = fmax(r2, fmin(r1, v));
                    r1 = fmax(r1, v);
                }
            }
            const double v0 = Dprev + KC[KC0 + a];
            const bool ring = r1 > v0;
            const double u = ring ? r1 : v0;
            const double gap = ring ? r1 - fmax(r2, v0) : v0 - r1;
            const uint32_t fl = gap < thr ? 1u : 0u;
            const double P = u + d.R[a];
            DL[a * (RB + 1) + wsl] = P;
            if constexpr (CARRY) Xr[a] = P;
            const uint32_t ent = (ring ? (uint32_t)rarg : 0u) | (fl << (EB - 1));
            pw[(a + 1) / EPW] |= ent << (((a + 1) % EPW) * EB);
            if (!UC) __builtin_amdgcn_sched_barrier(0);   // keep the junctions sequential: N^2 live candidates otherwise
        }
        if constexpr (INT) {   // one uniform base per plane + the lane; the lanes from W up store nothing
            if (liveW) {
#pragma unroll
                for (int w = 0; w < PW; w++) (psic + w * planePsi + tb)[lane] = pw[w];
            }
        } else if (STORE) {
#pragma unroll
            for (int w = 0; w < PW; w++) {
                uint32_t *dst = live ? psic + w * planePsi + tb + lane : trash + lane;
                *dst = pw[w];
            }
        }
        D0 = wave_bcast(Dn, nact - 1);  // the last live lane
        rs += W; rs = rs >= RB ? rs - RB : rs;
        ws += W; ws = ws >= RB ? ws - RB : ws;
    };
    auto dump = [&](double *rec, int64_t tref) {   // state "just before tref": D0 and P_a(tref - j), j = 1..L
        __syncthreads();
        if (lane == 0) rec[0] = D0;
        for (int i = lane; i < N * L; i += 64) {
            const int a = i / L, j = i % L + 1;
            const int slot = (int)((tref - j - tinit + L) % RB);
            rec[1 + i] = DL[a * (RB + 1) + slot];
        }
        __syncthreads();
    };
    // D super-steps of input in flight; the ring of buffers is indexed statically
    // The main loop is branch-free (whole groups of D super-steps, loads clamped past the end), so that
    // hipcc can count vmcnt across the back edge; the last < D super-steps run from the buffers the main
    // loop has already filled.
    auto sweep = [&](int from, int to, auto store_tag) {
        WIn<N> buf[D];
#pragma unroll
        for (int i = 0; i < D; i++) load(buf[i], from + i * W, store_tag);
        if constexpr (decltype(store_tag)::value == 3) {
#pragma unroll
            for (int a = 0; a < N; a++) Xr[a] = DL[a * (RB + 1) + rs];
        }
        int off = from;
        for (; off + D * W <= to; off += D * W) {
#pragma unroll
            for (int i = 0; i < D; i++) {
                run(buf[i], off + i * W, store_tag);
                load(buf[i], off + (i + D) * W, store_tag);
            }
        }
#pragma unroll
        for (int i = 0; i < D; i++)
            if (off + i * W < to) run(buf[i], off + i * W, store_tag);
    };
    const int n_warm = (redo || c == 0) ? 0 : g.Hw - 1;
    if (n_warm > 0) {
        sweep(0, n_warm, std::integral_constant<int, 0>());
        dump(vpre + cg * SR, tc);
    }
    // the interior range [n_warm, n_int): the full owned steps (option "interior" = 0: none)
    int n_int = n_warm;
    if constexpr (FAST && HS_VIT_INT) {
        if (g.interior && n_total > n_warm) n_int = n_warm + ((n_total - n_warm) / W) * W;
    }
    if (n_int > n_warm) {
        imax = n_int - W;
        constexpr bool CARRY_OK = HS_DL_REG && FAST && N <= 8;
        if (CARRY_OK && W == L) sweep(n_warm, n_int, std::integral_constant<int, CARRY_OK ? 3 : 2>());
        else sweep(n_warm, n_int, std::integral_constant<int, 2>());
    }
    if (n_total > n_int) sweep(n_int, n_total, std::integral_constant<int, 1>());
    dump(vend + cg * SR, tend);
    if (redo) {  // the hand-off was exact by construction
        for (int i = lane; i < SR; i += 64) vpre[cg * SR + i] = vend[(cg - 1) * SR + i];
    }
}

template <int N, bool UC>
__global__ __launch_bounds__(64, wave_occ<N>()) void kw_vit(WaveGeom g, const WaveConst *__restrict__ cst,
                                                            const double *__restrict__ y,
                                                            const double *__restrict__ Rf,
                                                            const double *__restrict__ virt,
                                                            const double *__restrict__ ysum,
                                                            uint32_t *__restrict__ psi, double *__restrict__ vpre,
                                                            double *__restrict__ vend, uint32_t *__restrict__ trash)
{
    vit_chain<N, UC, false>(g, cst, y, Rf, virt, ysum, psi, vpre, vend, trash, (int)blockIdx.x);
}

// Re-sweep of the chains the previous kw_vit_check launch listed (its certificate failed, its predecessor's did
// not, so vend of the predecessor is final): a small fixed grid walks the list, and in the common case of an
// empty list its few waves exit at once.  TIGHT (the decode runs beside an E-step, up to four rings): the kernel is
// held to the 80 registers that are free on a SIMD beside two waves of the backward sweep (six waves per SIMD).  A
// launch that needs more waits, list empty or not, until a wave of that sweep retires on every XCD its workgroups
// were dealt to -- 0.2 ms measured.  The price is scratch traffic in the rare re-sweep of a chain (184 B per lane
// at N = 4), and a decode on its own, which has the registers to itself, does not pay it.  Not for more than four
// rings: there the backward sweep holds 330 registers in ONE wave per SIMD, which leaves 182, and the redo kernel
// of 5-8 rings (127-172 registers) fits beside it as it is; at 80 registers it would spill its whole delay-line
// state.
constexpr int kVitRedoGrid = 64;
template <int N, bool UC, bool TIGHT>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TIGHT ? 6 : 1))) void kw_vit_redo(WaveGeom g, const WaveConst *__restrict__ cst,
                                                                 const double *__restrict__ y,
                                                                 const double *__restrict__ Rf,
                                                                 const double *__restrict__ virt,
                                                                 const double *__restrict__ ysum,
                                                                 uint32_t *__restrict__ psi, double *__restrict__ vpre,
                                                                 double *__restrict__ vend, uint32_t *__restrict__ trash,
                                                                 const int32_t *__restrict__ head,
                                                                 const int32_t *__restrict__ list)
{
    const int n = head[0];
    for (int q = blockIdx.x; q < n; q += gridDim.x)   // wave-uniform; a chain's sweep ends on a barrier
        vit_chain<N, UC, true>(g, cst, y, Rf, virt, ysum, psi, vpre, vend, trash, list[q]);
}

// Boundary certificate: one wavefront per chain boundary; all 1 + N*L entries of the warm-up state
// must equal the previous chain's end state up to one constant.
struct VitCert {
    bool fail, anybad;
    double spread;
};

__device__ __forceinline__ VitCert vit_cert(const WaveGeom &g, const double *__restrict__ vpre,
                                            const double *__restrict__ vend, int cg, int lane, double *__restrict__ dbgrec)
{
    const int c = cg % g.nch;
    const int64_t SR = 1 + (int64_t)g.N * g.L;
    double lo = INFINITY, hi = -INFINITY;
    int64_t ilo = -1, ihi = -1, ibad = -1;
    bool bad = false;
    for (int64_t i = lane; i < SR; i += 64) {
        const double p = vpre[cg * SR + i], e = vend[(cg - 1) * SR + i];
        if (p == e) {   // -inf on both sides (an unreachable entry) says nothing about the frame constant
            if (fabs(p) < INFINITY) { lo = fmin(lo, 0.0); hi = fmax(hi, 0.0); }
            continue;
        }
        const double d = p - e;
        if (!(fabs(d) < INFINITY)) { bad = true; ibad = i; continue; }      // NaN or one-sided infinity
        if (d < lo) { lo = d; ilo = i; }
        if (d > hi) { hi = d; ihi = i; }
    }
    if (dbgrec) {   // debug record: the extreme entries of the first boundaries
        for (int o = 32; o > 0; o >>= 1) {
            const double l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
            const long long il2 = __shfl_xor((long long)ilo, o), ih2 = __shfl_xor((long long)ihi, o), ib2 = __shfl_xor((long long)ibad, o);
            if (l2 < lo) { lo = l2; ilo = il2; }
            if (h2 > hi) { hi = h2; ihi = ih2; }
            if (ib2 > ibad) ibad = ib2;
        }
        if (lane == 0 && c <= 3) {
            double *r = dbgrec + 16 + 8 * (c - 1);
            r[0] = (double)cg; r[1] = lo; r[2] = (double)ilo; r[3] = hi; r[4] = (double)ihi; r[5] = (double)ibad;
            r[6] = ilo >= 0 ? vpre[cg * SR + ilo] : 0.0; r[7] = ilo >= 0 ? vend[(cg - 1) * SR + ilo] : 0.0;
        }
    }
    lo = -wave_max(-lo); hi = wave_max(hi);
    VitCert v;
    v.anybad = __any(bad);
    v.spread = hi - lo;
    v.fail = v.anybad || !(v.spread <= kVitTol);
    return v;
}

// The rounds before the final one also list the chains the next kw_vit_redo launch sweeps again: chain cg failed,
// its predecessor did not (so the predecessor's end state is final) and it is not a channel's first chain.  The
// predecessor's verdict is another workgroup's result of this same launch, so a failing chain works it out itself.
//
// A round that would repeat the one before it returns at once.  prev_head is the list head of the previous round
// (nullptr: the first round, or option "cert_rounds" = 1).  When that list is empty no chain failed in the previous
// round -- the first failing chain of a channel has a passing predecessor (a channel's first chain never fails), so
// it is always listed -- hence nothing was swept again and every verdict of this round would be the previous
// round's.  A round before the final one then has nothing to do: vfail is all zeros already, its own list stays
// empty (the call zeroed the heads), diag[1] gains nothing.  The final round produces diag[2] from vcert, where every
// full round before it leaves what the final round filters and maximises: the spread's bits, or kVitNoSpread
// for a chain the filter drops.  Same values, same filter, same "read, then atomicMax only if larger" rule (per 64
// chains), and a maximum does not depend on the order; vfail and diag[0] (no failure: 0) are as the full round would leave them.
// The boundaries c <= 3 still run in full there: they write the dbg record.
constexpr unsigned long long kVitNoSpread = ~0ull;

__device__ __forceinline__ void vit_spread_max(int64_t *__restrict__ diag, unsigned long long sb)
{
    // a spread is >= 0, so its bits order like its value.  Most chains do not raise the maximum: they
    // read it and leave (a stale read only costs an atomic that changes nothing).
    if (sb > *reinterpret_cast<volatile unsigned long long *>(&diag[2]))
        atomicMax((unsigned long long *)&diag[2], sb);
}

__global__ __launch_bounds__(64) void kw_vit_check(WaveGeom g, const double *__restrict__ vpre,
                                                   const double *__restrict__ vend,
                                                   int32_t *__restrict__ vfail, int64_t *__restrict__ diag,
                                                   int final_round, double *__restrict__ dbg,
                                                   int32_t *__restrict__ head, int32_t *__restrict__ list,
                                                   const int32_t *__restrict__ prev_head,
                                                   unsigned long long *__restrict__ vcert)
{
    const int lane = threadIdx.x;
    const int cg = blockIdx.x, c = cg % g.nch;
    const bool same = prev_head && prev_head[0] == 0;   // uniform over the launch
    if (same && !final_round) return;
    if (c == 0 && !same) { if (lane == 0) vfail[cg] = 0; return; }
    if (same) {
        // one wave per 64 chains takes the maximum of their stored spreads first: two thousand waves that all leave
        // at once would all read diag[2] before any of them has raised it, and queue up on the same address
        if (cg % 64 == 0) {
            const int j = cg + lane;
            unsigned long long sb = 0;   // (a spread of 0 raises nothing)
            if (j < (int)gridDim.x && j % g.nch != 0) {
                const unsigned long long v = vcert[j];
                sb = v != kVitNoSpread ? v : 0;
            }
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long t = (unsigned long long)__shfl_xor((long long)sb, o);
                sb = t > sb ? t : sb;
            }
            if (lane == 0 && sb) vit_spread_max(diag, sb);
        }
        if (c >= 1 && c <= 3) (void)vit_cert(g, vpre, vend, cg, lane, dbg);   // the dbg record of the first boundaries
        return;
    }
    const VitCert v = vit_cert(g, vpre, vend, cg, lane, final_round ? dbg : nullptr);
    const bool counted = !v.anybad && v.spread == v.spread && v.spread < INFINITY;
    const unsigned long long sb = (unsigned long long)__double_as_longlong(v.spread);
    if (lane == 0) {
        vfail[cg] = v.fail ? 1 : 0;
        if (final_round) {
            if (v.fail) atomicAdd((unsigned long long *)&diag[0], 1ull);
            if (counted) vit_spread_max(diag, sb);
        } else {
            vcert[cg] = counted ? sb : kVitNoSpread;
            if (v.fail) atomicAdd((unsigned long long *)&diag[1], 1ull);  // chains swept again (all rounds)
        }
    }
    if (!final_round && v.fail) {   // wave-uniform
        const bool prev_fail = c > 1 && vit_cert(g, vpre, vend, cg - 1, lane, nullptr).fail;
        if (!prev_fail && lane == 0) list[atomicAdd(&head[0], 1)] = cg;
    }
}

// Final state = argmax over all S states at the last sample, first maximum in state order
// (viterbi.jl:90).  delta(a,k) at T-1 is P_a(T-k).  One wave per channel; every lane returns the same state.
// *flagged: the runner-up is within the near-tie threshold (wave_ties.hip re-decides the arg-max exactly).
__device__ __forceinline__ int vit_final_state(const WaveGeom &g, const WaveConst *__restrict__ cst,
                                               const double *__restrict__ ysum, const double *__restrict__ vend,
                                               int ch, int lane, bool *flagged)
{
    const int64_t SR = 1 + (int64_t)g.N * g.L;
    const double *rec = vend + ((int64_t)ch * g.nch + g.nch - 1) * SR;
    const int S = 1 + g.N * g.L;
    double best = -INFINITY, sec = -INFINITY;
    int bi = S;
    for (int j = lane; j < S; j += 64) {  // state j = 1 + a*L + (k-1) <-> record entry 1 + a*L + (k-1)
        const double v = rec[j];
        if (v > best) { sec = best; best = v; bi = j; }
        else sec = fmax(sec, v);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o), os = __shfl_xor(sec, o);
        const int oi = __shfl_xor(bi, o);
        const bool take = ov > best || (ov == best && oi < bi);
        const double lose = take ? best : ov;
        sec = fmax(fmax(sec, os), lose);
        if (take) { best = ov; bi = oi; }
    }
    *flagged = (best - sec) < wave_thr(g, cst[ch], ysum, ch);
    return (bi >= S) ? 0 : bi;
}

// Backtrace (viterbi.jl:93-94).  The path is cut into segments of Bb samples, one LANE per segment;
// a lane starts its walk Hb samples after its segment's end from the silent state (from the true
// final state where that is the end of the data) and has merged with the true path by the time it
// enters its segment (checked: kw_stitch_*).  psi is in natural time order, so a tile of 64 segments
// x 64 samples is read with coalesced rows into LDS and walked column-wise; x leaves the same way.
// Flagged (near-tie) junction decisions met inside the owned segment are counted per channel (the trigger of
// the exact resolver, wave_ties.hip).
// Two kernels.  kw_backtrace (register rows): a lane holds its whole tile row (one or two words per sample) in
// registers through the tile's unrolled walk -- 300 registers per lane, one wave per SIMD, the fastest when nothing
// else runs.  kw_backtrace_light: tiles of 64 / 32 / 16 samples in LDS, at most 80 registers and 32 KB of LDS, so
// that it fits on a SIMD beside two waves of the backward sweep (decode + E-step in one call), where a wave gets
// one issue slot in three and the length of the walk's dependent chain is what it costs.  Its walk therefore visits
// DECISIONS, not samples (HS_BT_EVENTS): the path only changes at junctions, so
//   * inside a ring (rem > 0) nothing is read: the next rem samples are id-1, id-2, ..., one jump;
//   * in the silent state every sample reads entry 0 and almost always finds "silent" again: the walk needs the
//     nearest earlier sample whose entry 0 names a ring, the highest set bit of a row mask (one ballot per row of
//     the tile, all lanes), and the flagged decisions it skips are a popcount of a second mask;
//   * only a ring's first state and the silent sample that leaves into a ring read their entry from the tile.
// A lane's walk through a tile is then a handful of passes (a 704-sample walk at the headline rates meets about
// five spikes) and leaves the ids as ramps, which all lanes expand while x is stored.  HS_BT_EVENTS = 0 is the
// per-sample walk: a lane reads its row from LDS in chunks of 8 / 4 samples and puts the decoded ids into an output
// tile.  Same integer decisions in all three: same x, bstate and tie counters (tests/backtrace_model.py states the
// two light walks; tests/test_gpu_backtrace_events.py compares them with the register rows).
// Start of the walks that begin at a channel's last sample.  The workgroups that hold such a walk find the final
// state themselves (vit_final_state: vend is final by now); the one that owns the last segment records it and its
// near-tie flag.  (wave-uniform branch)
template <int N>
__device__ __forceinline__ void bt_start(const WaveGeom &g, const WaveConst *__restrict__ cst,
                                         const double *__restrict__ ysum, const double *__restrict__ vend,
                                         int32_t *__restrict__ final_state, int64_t *__restrict__ tie_cnt, int ch, int lane,
                                         bool at_end, int &id, int &rem, int &wi, int &sh)
{
    constexpr int EB = wpsi_bits_c(N), EPW = wpsi_epw_c(N);
    if (!__any(at_end)) return;
    bool flagged;
    const int fs = vit_final_state(g, cst, ysum, vend, ch, lane, &flagged);
    if (blockIdx.x == gridDim.x - 1 && lane == 0) {   // the workgroup of the last segment
        final_state[ch] = fs;
        if (flagged) {   // wave_ties.hip re-decides it exactly
            tie_cnt[ch * 8 + kTieTail] = 1;
            atomicAdd((unsigned long long *)&tie_cnt[ch * 8 + kTieTrig], 1ull);
        }
    }
    if (at_end && fs > 0) {
        const int L = g.L, a0 = (fs - 1) / L, k0 = (fs - 1) % L + 1, e0 = a0 + 1;
        id = fs + 1; rem = k0 - 1; wi = e0 / EPW; sh = (e0 % EPW) * EB;
    }
}

// samples per tile of the light backtrace (the LDS of a workgroup stays below 32 KB)
template <int N> constexpr int bt_tile()
{
    constexpr int PW = wpsi_words_c(N);
    return PW == 1 ? 64 : (PW <= 3 ? 32 : 16);
}
// dynamic LDS of a light backtrace workgroup: the psi tile (rows padded by four words: a row starts on 16 bytes,
// and both the 128-bit staging writes and the 128-bit chunk reads of the walk are conflict-free per quarter wave)
// and the output tile (rows padded by one word)
#ifndef HS_BT_EVENTS
#define HS_BT_EVENTS 1    // the light backtrace walks junction decisions (0: one step per sample, the output tile in LDS)
#endif
// ramps a segment row can hold in one tile: a ring cut by the tile's newest sample, whole rings, a ring cut by its
// oldest sample; rings have at least 8 states (wave_supported)
template <int N> constexpr int bt_ramps() { return bt_tile<N>() / 8 + 2; }
template <int N, int SPW> constexpr size_t bt_lds_bytes()
{
    constexpr int PW = wpsi_words_c(N), TS = bt_tile<N>();
#if HS_BT_EVENTS
    // the output tile is not kept: the ramps of a row (a count and bt_ramps words) are expanded as x is stored
    return sizeof(uint32_t) * (size_t)(PW * SPW * (TS + 4) + SPW * (bt_ramps<N>() + 1));
#else
    return sizeof(uint32_t) * (size_t)(PW * SPW * (TS + 4) + SPW * (TS / 2 + 1));
#endif
}

// SPW: segments (tile rows) per workgroup, 64, 32 or 16.  With SPW < 64 the lanes < SPW walk, all 64 lanes stage
// the tile and move the output tile, a tile is fewer load and store instructions per lane, and 64 / SPW times as
// many waves are resident; a wave's walk is as many instructions as before, so the device issues 64 / SPW times the
// walk.  Which SPW a row width runs with is bt_spw (measured beside the backward sweep).
template <int N, int SPW>
__device__ __forceinline__ void backtrace_light_body(const WaveGeom &g, const WaveConst *__restrict__ cst,
                                               const double *__restrict__ ysum, const double *__restrict__ vend,
                                               const uint32_t *__restrict__ psi, int32_t *__restrict__ final_state,
                                               int16_t *__restrict__ x, int32_t *__restrict__ bstate,
                                               int64_t *__restrict__ tie_cnt)
{
    constexpr int EB = wpsi_bits_c(N), EPW = wpsi_epw_c(N), PW = wpsi_words_c(N);
    constexpr int TS = bt_tile<N>();
    constexpr int RPI = 64 / TS;            // segment rows per load instruction
    constexpr int XW = TS / 2;              // decoded ids leave as pairs (two int16 per word)
    constexpr int XRI = 64 / XW;            // rows per store instruction
    constexpr int CH = PW == 1 ? 8 : 4;     // samples per register chunk
    [[maybe_unused]] constexpr int NCH = TS / CH;
    constexpr int TSP = TS + 4;             // tile row stride in words
    constexpr int LPR = TS / 4;             // lanes per row of a 16-byte load instruction
    constexpr int RPW = 64 / LPR;           // segment rows per 16-byte load instruction (TS / 4 instructions per plane)
    constexpr int WU = SPW / RPW < 4 ? SPW / RPW : 4;   // 16-byte loads in flight while a tile is staged (up to 16 registers, dead in the walk)
    constexpr int SU = 2;                   // row loads in flight on the dword path (planes off 16 bytes)
    [[maybe_unused]] constexpr int XU = PW == 4 ? 2 : 4;     // row stores in flight while the output tile leaves (four spill at PW = 4)
    static_assert(CH % 4 == 0 && TS % CH == 0, "chunks are whole 16-byte groups");
    static_assert(SPW == 64 || SPW == 32 || SPW == 16, "segments per workgroup");
    static_assert(WU >= 1 && SPW % (RPW * WU) == 0, "whole batches of wide loads");
    static_assert(SPW % RPI == 0 && SPW % XRI == 0, "whole row instructions");
    static_assert(bt_lds_bytes<N, SPW>() <= 32 * 1024, "LDS budget");
    extern __shared__ __align__(16) uint32_t lds_bt[];    // tile[PW][SPW][TS + 4] | xt[SPW][XW + 1] (events: ramp[SPW][ND + 1])
    uint32_t (*tile)[SPW][TSP] = reinterpret_cast<uint32_t (*)[SPW][TSP]>(lds_bt);
#if HS_BT_EVENTS
    constexpr int ND = bt_ramps<N>();       // ramps per row and tile (odd row stride: conflict-free)
    static_assert(TS <= 64 && ND * 8 >= TS + 16 && (ND + 1) % 2 == 1, "ramp capacity");
    uint32_t (*ramp)[ND + 1] = reinterpret_cast<uint32_t (*)[ND + 1]>(lds_bt + PW * SPW * TSP);
    using Mask = std::conditional_t<TS == 64, uint64_t, uint32_t>;   // one bit per sample of a tile row
#else
    uint32_t (*xt)[XW + 1] = reinterpret_cast<uint32_t (*)[XW + 1]>(lds_bt + PW * SPW * TSP);
#endif
    const int lane = threadIdx.x, ch = blockIdx.y;
    const int L = g.L, Bb = g.Bb, Hb = g.Hb;
    const int64_t T = g.T;
    const int64_t sg0 = (int64_t)blockIdx.x * SPW, sg = sg0 + lane;
    const bool walker = SPW == 64 || lane < SPW;           // the lanes that hold a row
    const bool active = walker && sg < g.nseg;
    const int64_t s_lo = sg * Bb;
    const int64_t s_hi = active ? ((s_lo + Bb) < T ? (s_lo + Bb) : T) : s_lo;
    const int64_t te = (s_hi + Hb) < T ? (s_hi + Hb) : T;  // walk starts at te-1
    const int64_t planePsi = (int64_t)g.C * T;
    const uint32_t *pc = psi + (int64_t)ch * T;
    int16_t *xc = x + (int64_t)ch * T;
    const bool xal = ((reinterpret_cast<uintptr_t>(xc)) & 3) == 0;   // odd T puts later channels on odd samples
    // times relative to the segment start: u = t - s_lo
    const int te_rel = active ? (int)(te - s_lo) : 0, hi_rel = (int)(s_hi - s_lo);
    const int t1 = s_lo >= 1 ? 0 : 1;                      // the step at t = 0 has no predecessor
    const int t2 = 2 * t1;                                 // psi(1) only decides x[0]: kw_first_state (s_lo is 0 or at least Bb)
    // walk state: id = state id at the current sample, rem = steps left inside the ring (0 at a junction),
    // (wi, sh) = word and bit offset of the psi entry the next junction decision reads (entry e = ring + 1)
    int id = 1, rem = 0, wi = 0, sh = 0;
    bt_start<N>(g, cst, ysum, vend, final_state, tie_cnt, ch, lane, active && te == T, id, rem, wi, sh);
    int nflag = 0, bs = 0;
    const int lr = lane / TS, lc = lane % TS;
#if HS_BT_EVENTS
    // One tile of the walk, newest sample first, by EVENTS: u is the next sample the lane decides (relative to
    // its segment; te_rel - 1 before the walk has begun, so a lane enters the loop in the tile that holds its
    // start), and every pass of the loop takes it past one stretch of the path:
    //   silent state -- down to the nearest sample whose entry 0 names a ring (pm: one bit per sample of the
    //     tile row, set where entry 0 has a predecessor != 0), or out of the tile; the flagged decisions of the
    //     stretch are a popcount of fm (entry 0's flag bits) over it;
    //   inside a ring -- the rem samples that need no decision and, when it is still in the tile, the ring's
    //     first state, whose entry (wi, sh) is read from the tile and decides the junction.  Such a stretch is
    //     one RAMP of ids: (first sample, last sample, id at the last sample), 6 + 6 + 20 bits, left in LDS for
    //     the store phase when `emit` (the tile is inside the owned segments).  Silence leaves nothing.
    // A pass lowers u by at least 1.  FAST: every lane of the wave is inside its walk for the whole tile and
    // (OWN) inside / (not OWN) behind its own segment, so no per-lane time marks: the others apply the rules of
    // the per-sample walk (no step at u < t1, flags counted in [t2, hi_rel), bs = the id at hi_rel).
    constexpr uint32_t PJM = (1u << (EB - 1)) - 1u;
    int u = te_rel - 1;
    auto low = [](int p) -> Mask { return (Mask)(((Mask)2 << p) - 1); };   // bits 0..p (p < TS)
    auto msb = [](Mask m) -> int { return TS == 64 ? 63 - __clzll((long long)m) : 31 - __clz((int)m); };
    auto popc = [](Mask m) -> int { return TS == 64 ? __popcll((unsigned long long)m) : __popc((unsigned)m); };
    auto walk = [&](int u0, auto fast_tag, auto own_tag, bool emit, Mask pm, Mask fm) {
        constexpr bool FAST = decltype(fast_tag)::value, OWN = decltype(own_tag)::value;
        const uint32_t *row0 = &tile[0][lane][0];
        int nd = 0;
        while (u >= u0) {
            const int p = u - u0;
            if (id == 1) {   // silent (rem = 0, entry 0)
                const Mask below = pm & low(p);
                int j = below ? msb(below) : -1;
                if (!FAST && u0 + j < t1) j = -1;        // the step at t = 0 has no predecessor
                const int lo = j < 0 ? 0 : j;            // the stretch lo..p is silent; its decisions read entry 0
                if (FAST ? OWN : true) {
                    int a = lo, b = p;
                    if (!FAST) {
                        a = a > t2 - u0 ? a : t2 - u0;
                        b = b < hi_rel - 1 - u0 ? b : hi_rel - 1 - u0;
                    }
                    if (a <= b) nflag += popc(fm & low(b) & (Mask)(~(Mask)0 << a));
                }
                if (!FAST) {
                    const int h = hi_rel - u0;
                    bs = (h >= lo && h <= p) ? 1 : bs;
                }
                if (j < 0) { u = u0 - 1; break; }
                const int pj = (int)(row0[j] & PJM);     // != 0: the last state of ring pj - 1
                id = 1 + pj * L; rem = L - 1;
                wi = pj / EPW; sh = (pj % EPW) * EB;
                u = u0 + j - 1;
            } else {
                const int s = rem < p + 1 ? rem : p + 1;     // samples without a decision
                const bool junc = s <= p;                     // the ring's first state is in the tile
                const int n = s + (junc ? 1 : 0);
                if (emit) ramp[lane][1 + nd++] = (uint32_t)(p - n + 1) | ((uint32_t)p << 6) | ((uint32_t)id << 12);
                if (!FAST) {
                    const int d = u - hi_rel;
                    bs = (d >= 0 && d < n) ? id - d : bs;
                }
                if (junc) {
                    const int uj = u - s;
                    if (FAST || uj >= t1) {
                        const uint32_t ent = row0[wi * (SPW * TSP) + (uj - u0)] >> sh;
                        const int pj = (int)(ent & PJM);
                        if (FAST ? OWN : (uj < hi_rel && uj >= t2)) nflag += (int)((ent >> (EB - 1)) & 1u);
                        id = 1 + pj * L; rem = pj ? L - 1 : 0;
                        wi = pj / EPW; sh = (pj % EPW) * EB;
                    }
                } else {
                    id -= s; rem -= s;
                }
                u -= n;
            }
        }
        if (emit) ramp[lane][0] = (uint32_t)nd;
    };
#else
    // one tile of the walk, newest sample first.  FAST: every lane of the wave is inside its walk for the
    // whole tile and (OWN) inside / (not OWN) behind its own segment, so no per-lane time predicates.
    // The decoded ids of a chunk go to the output tile when `emit` (the tile is inside the owned segments).
    auto walk = [&](int q, auto fast_tag, auto own_tag, bool emit) {
        constexpr bool FAST = decltype(fast_tag)::value, OWN = decltype(own_tag)::value;
#pragma unroll 1
        for (int k = NCH - 1; k >= 0; k--) {
            uint32_t rowv[PW][CH], xr[CH / 2];
#pragma unroll
            for (int w = 0; w < PW; w++)
#pragma unroll
                for (int i = 0; i < CH; i += 4) {
                    const uint4 t4 = *reinterpret_cast<const uint4 *>(&tile[w][lane][k * CH + i]);
                    rowv[w][i] = t4.x; rowv[w][i + 1] = t4.y; rowv[w][i + 2] = t4.z; rowv[w][i + 3] = t4.w;
                }
            // the lane's time marks relative to the chunk: sample i of it is u = ub + i of the segment
            const int ub = TS * q + k * CH;
            const int te_c = te_rel - ub, hi_c = hi_rel - ub, t1_c = t1 - ub, t2_c = t1_c + t1;   // t2 = 2 t1: both mark the channel's first segment
#pragma unroll
            for (int i = CH - 1; i >= 0; i--) {
                const bool interior = rem > 0;
                if (FAST ? OWN : true) {
                    if (i & 1) xr[i / 2] = (uint32_t)id << 16;
                    else xr[i / 2] |= (uint32_t)id & 0xffffu;
                }
                uint32_t wsel = rowv[0][i];
#pragma unroll
                for (int w = 1; w < PW; w++) wsel = (wi == w) ? rowv[w][i] : wsel;
                const uint32_t ent = wsel >> sh;
                const int pj = (int)(ent & ((1u << (EB - 1)) - 1u));
                const int flag = (int)((ent >> (EB - 1)) & 1u);
                // junction: predecessor p = 0 silent (id 1), else the last state of ring p-1 (id 1 + p L)
                const int jid = 1 + pj * L, jrem = pj ? L - 1 : 0;
                const int jwi = pj / EPW, jsh = (pj % EPW) * EB;
                if (FAST) {
                    if (OWN) nflag += interior ? 0 : flag;
                    id = interior ? id - 1 : jid;
                    rem = interior ? rem - 1 : jrem;
                    wi = interior ? wi : jwi;
                    sh = interior ? sh : jsh;
                } else {
                    const bool live = i < te_c, step = live && i >= t1_c;
                    bs = (live && i == hi_c) ? id : bs;
                    if (step && !interior && i < hi_c && i >= t2_c) nflag += flag;
                    id = step ? (interior ? id - 1 : jid) : id;
                    rem = step ? (interior ? rem - 1 : jrem) : rem;
                    wi = step ? (interior ? wi : jwi) : wi;
                    sh = step ? (interior ? sh : jsh) : sh;
                }
            }
            if (FAST ? OWN : true) {
                if (emit) {
#pragma unroll
                    for (int j = 0; j < CH / 2; j++) xt[lane][k * (CH / 2) + j] = xr[j];
                }
            }
        }
    };
#endif
    const int nq = (Bb + Hb) / TS;
    for (int q = nq - 1; q >= 0; q--) {
        // stage psi rows: row r = segment sg0 + r, samples s_lo(r) + TS q + (0..TS-1).  Wave-uniform tile origin +
        // 32-bit lane offsets; rows that do not exist read the origin and are staged as zeros.  A plane that starts
        // on 16 bytes (rows start at multiples of 64 samples from it) comes in with 16-byte loads, four rows of 64
        // samples per instruction and WU of them in flight; the other planes (T decides where the planes w > 0 and
        // the channels ch > 0 start) and the one group of four samples that T cuts take the dword path.
        const int64_t tb = sg0 * Bb + (int64_t)TS * q, left = T - tb;
        const int nrow = g.nseg - sg0 < SPW ? (int)(g.nseg - sg0) : SPW;                // rows that exist
        const int lim = left < 0 ? 0 : (left < (int64_t)SPW * Bb ? (int)left : SPW * Bb);   // offsets below it are data
        {
#pragma unroll
            for (int w = 0; w < PW; w++) {
                const uint32_t *pw = pc + w * planePsi;
                if (T >= 4 && (reinterpret_cast<uintptr_t>(pw) & 15) == 0) {   // wave-uniform
                    const uint32_t *base = pw + (lim >= 4 ? tb : 0);          // no whole group in the tile: all read pw[0..3]
                    const int wr = lane / LPR, wc = 4 * (lane % LPR);
#pragma unroll 1
                    for (int r0 = 0; r0 < SPW; r0 += RPW * WU) {
                        uint4 v[WU];
#pragma unroll
                        for (int j = 0; j < WU; j++) {
                            const int r = r0 + j * RPW + wr, o = r * Bb + wc;
                            const bool ok = r < nrow && o + 4 <= lim;
                            v[j] = *reinterpret_cast<const uint4 *>(base + (ok ? (uint32_t)o : 0u));
                        }
#pragma unroll
                        for (int j = 0; j < WU; j++) {
                            const int r = r0 + j * RPW + wr, o = r * Bb + wc;
                            const bool ok = r < nrow && o + 4 <= lim;
                            *reinterpret_cast<uint4 *>(&tile[w][r][wc]) = ok ? v[j] : make_uint4(0u, 0u, 0u, 0u);
                        }
                    }
                    // the group T cuts (staged as zeros above) starts at offset lim & ~3; the lane whose row holds
                    // it in this tile, if there is one, brings in its one to three samples
                    if (left < (int64_t)SPW * Bb && (lim & 3)) {
                        const int c0 = (lim & ~3) - lane * Bb;
                        if (walker && c0 >= 0 && c0 < TS) {
#pragma unroll
                            for (int j = 0; j < 3; j++)
                                if (j < (lim & 3)) tile[w][lane][c0 + j] = pw[tb + (lim & ~3) + j];
                        }
                    }
                } else {
                    const uint32_t *base = pw + (lim > 0 ? tb : 0);
#pragma unroll SU
                    for (int rr = 0; rr < SPW; rr += RPI) {
                        const int r = rr + lr, o = r * Bb + lc;
                        const bool ok = r < nrow && o < lim;
                        const uint32_t v = base[ok ? (uint32_t)o : 0u];
                        tile[w][r][lc] = ok ? v : 0u;
                    }
                }
            }
        }
        __syncthreads();
        const int u0 = TS * q, u1 = u0 + TS;
        const bool own_tile = u0 < Bb;
        // wave-uniform choice of the tile body
        const bool lane_fast = u0 >= t1 && u1 <= te_rel &&
                               (own_tile ? (u1 <= hi_rel && u0 >= t2) : (u0 > hi_rel));
        const bool fast = __all(lane_fast || !walker);
#if HS_BT_EVENTS
        // the masks of the tile's rows, all lanes: lanes = samples of RPI rows, one LDS read and one compare per
        // ballot; the lane that walks a row keeps that row's bits (registers).  Rows that do not exist and samples
        // past T are staged as zeros: silent -> silent, not flagged.  Flags are counted in owned tiles only.
        Mask pm, fm;
        {
            unsigned long long mp = 0, mf = 0;
#pragma unroll 4
            for (int it = 0; it < SPW / RPI; it++) {
                const uint32_t w0 = tile[0][it * RPI + lr][lc];
                const bool mine = lane / RPI == it;
                const unsigned long long bp = __ballot((w0 & PJM) != 0u);
                mp = mine ? bp : mp;
                if (own_tile) {
                    const unsigned long long bf = __ballot(((w0 >> (EB - 1)) & 1u) != 0u);
                    mf = mine ? bf : mf;
                }
            }
            constexpr Mask row_bits = (Mask)(~(Mask)0 >> (8 * sizeof(Mask) - TS));
            const int shf = (lane % RPI) * TS;
            pm = (Mask)(mp >> shf) & row_bits;
            fm = (Mask)(mf >> shf) & row_bits;
        }
        if (walker) {   // (divergent: no barrier and no cross-lane move inside a walk)
            if (fast && own_tile) walk(u0, std::true_type(), std::true_type(), true, pm, fm);
            else if (fast) walk(u0, std::true_type(), std::false_type(), false, pm, fm);
            else walk(u0, std::false_type(), std::false_type(), own_tile, pm, fm);
        }
#else
        if (walker) {   // (no barrier and no cross-lane move inside a walk)
            if (fast && own_tile) walk(q, std::true_type(), std::true_type(), true);
            else if (fast) walk(q, std::true_type(), std::false_type(), false);
            else walk(q, std::false_type(), std::false_type(), own_tile);
        }
#endif
        if (own_tile) {  // owned rows: write x out, coalesced
            __syncthreads();
            const int xrw = lane / XW, xcw = lane % XW;
            int16_t *xb = xc + (lim > 0 ? tb : 0);   // wave-uniform tile origin + 32-bit lane offsets, as the loads
#if HS_BT_EVENTS
#pragma unroll 2
#else
#pragma unroll XU
#endif
            for (int rr = 0; rr < SPW; rr += XRI) {
                const int r = rr + xrw, o = r * Bb + 2 * xcw;
                if (r < nrow && o < lim) {
#if HS_BT_EVENTS
                    // the pair of samples 2 xcw, 2 xcw + 1 of row r: silent unless one of the row's ramps covers it
                    const uint32_t *rp = ramp[r];
                    const int nr = (int)rp[0], c0 = 2 * xcw;
                    uint32_t v = 0x00010001u;
                    for (int k = 1; k <= nr; k++) {
                        const uint32_t d = rp[k];
                        const int f = (int)(d & 63u), l = (int)((d >> 6) & 63u);
                        const uint32_t top = (d >> 12) - (uint32_t)l;      // id(c) = top + c for f <= c <= l
                        if (c0 >= f && c0 <= l) v = (v & 0xffff0000u) | (top + (uint32_t)c0);
                        if (c0 + 1 >= f && c0 + 1 <= l) v = (v & 0x0000ffffu) | ((top + (uint32_t)c0 + 1u) << 16);
                    }
#else
                    const uint32_t v = xt[r][xcw];
#endif
                    if (o + 1 < lim && xal) *reinterpret_cast<uint32_t *>(xb + o) = v;
                    else {
                        xb[o] = (int16_t)(v & 0xffffu);
                        if (o + 1 < lim) xb[o + 1] = (int16_t)(v >> 16);
                    }
                }
            }
        }
        __syncthreads();
    }
    // every segment but the channel's last has a successor whose first sample its walk crossed (hi_rel < te_rel);
    // wave-uniform base and bound: sg is not kept
    {
        const int64_t nb = g.nseg - 1 - sg0;
        const int nbs = nb < SPW ? (int)nb : SPW;
        if ((int)threadIdx.x < nbs) (bstate + ((int64_t)ch * g.nseg + sg0))[threadIdx.x] = bs;
    }
    for (int o = 32; o > 0; o >>= 1) nflag += __shfl_xor(nflag, o);
    if (threadIdx.x == 0 && nflag) atomicAdd((unsigned long long *)&tie_cnt[ch * 8 + kTieTrig], (unsigned long long)nflag);
}

template <int N>
__global__ __launch_bounds__(64) void kw_backtrace(WaveGeom g, const WaveConst *__restrict__ cst,
                                                   const double *__restrict__ ysum, const double *__restrict__ vend,
                                                   const uint32_t *__restrict__ psi, int32_t *__restrict__ final_state,
                                                   int16_t *__restrict__ x, int32_t *__restrict__ bstate,
                                                   int64_t *__restrict__ tie_cnt)
{
    constexpr int EB = wpsi_bits_c(N), EPW = wpsi_epw_c(N), PW = wpsi_words_c(N);
    constexpr int TS = PW <= 2 ? 64 : 32;   // samples per tile (static LDS stays below 64 KB)
    constexpr int RPI = 64 / TS;            // segment rows per load instruction
    constexpr int XW = TS / 2;              // decoded ids leave as pairs (two int16 per word)
    constexpr int XRI = 64 / XW;            // rows per store instruction
    __shared__ uint32_t tile[PW][64][TS + 1];
    __shared__ uint32_t xt[64][XW + 1];
    const int lane = threadIdx.x, ch = blockIdx.y;
    const int L = g.L, Bb = g.Bb, Hb = g.Hb;
    const int64_t T = g.T;
    const int64_t sg0 = (int64_t)blockIdx.x * 64, sg = sg0 + lane;
    const bool active = sg < g.nseg;
    const int64_t s_lo = sg * Bb;
    const int64_t s_hi = active ? ((s_lo + Bb) < T ? (s_lo + Bb) : T) : s_lo;
    const int64_t te = (s_hi + Hb) < T ? (s_hi + Hb) : T;  // walk starts at te-1
    const int64_t planePsi = (int64_t)g.C * T;
    const uint32_t *pc = psi + (int64_t)ch * T;
    int16_t *xc = x + (int64_t)ch * T;
    const bool xal = ((reinterpret_cast<uintptr_t>(xc)) & 3) == 0;   // odd T puts later channels on odd samples
    // times relative to the segment start: u = t - s_lo
    const int te_rel = active ? (int)(te - s_lo) : 0, hi_rel = (int)(s_hi - s_lo);
    const int t1 = s_lo >= 1 ? 0 : 1;                      // the step at t = 0 has no predecessor
    const int t2 = s_lo >= 2 ? 0 : (int)(2 - s_lo);        // psi(1) only decides x[0]: kw_first_state
    // walk state: id = state id at the current sample, rem = steps left inside the ring (0 at a junction),
    // (wi, sh) = word and bit offset of the psi entry the next junction decision reads (entry e = ring + 1)
    int id = 1, rem = 0, wi = 0, sh = 0;
    bt_start<N>(g, cst, ysum, vend, final_state, tie_cnt, ch, lane, active && te == T, id, rem, wi, sh);
    int nflag = 0, bs = 0;
    const int lr = lane / TS, lc = lane % TS;
    constexpr bool ROWREG = PW <= 2;        // the lane's tile row in registers (wider rows stay in LDS)
    uint32_t rowv[ROWREG ? PW : 1][ROWREG ? TS : 1], xr[XW];
    // one tile of the walk, newest sample first.  FAST: every lane of the wave is inside its walk for the
    // whole tile and (OWN) inside / (not OWN) behind its own segment, so no per-lane time predicates.
    auto walk = [&](int q, auto fast_tag, auto own_tag) {
        constexpr bool FAST = decltype(fast_tag)::value, OWN = decltype(own_tag)::value;
#pragma unroll
        for (int i = TS - 1; i >= 0; i--) {
            const int u = TS * q + i;
            const bool interior = rem > 0;
            if (FAST ? OWN : true) {
                if (i & 1) xr[i / 2] = (uint32_t)id << 16;
                else xr[i / 2] |= (uint32_t)id & 0xffffu;
            }
            uint32_t wsel;
            if constexpr (ROWREG) {
                wsel = rowv[0][i];
#pragma unroll
                for (int w = 1; w < PW; w++) wsel = (wi == w) ? rowv[w][i] : wsel;
            } else {
                wsel = tile[wi][lane][i];
            }
            const uint32_t ent = wsel >> sh;
            const int pj = (int)(ent & ((1u << (EB - 1)) - 1u));
            const int flag = (int)((ent >> (EB - 1)) & 1u);
            // junction: predecessor p = 0 silent (id 1), else the last state of ring p-1 (id 1 + p L)
            const int jid = 1 + pj * L, jrem = pj ? L - 1 : 0;
            const int jwi = pj / EPW, jsh = (pj % EPW) * EB;
            if (FAST) {
                if (OWN) nflag += interior ? 0 : flag;
                id = interior ? id - 1 : jid;
                rem = interior ? rem - 1 : jrem;
                wi = interior ? wi : jwi;
                sh = interior ? sh : jsh;
            } else {
                const bool live = u < te_rel, step = live && u >= t1;
                bs = (live && u == hi_rel) ? id : bs;
                if (step && !interior && u < hi_rel && u >= t2) nflag += flag;
                id = step ? (interior ? id - 1 : jid) : id;
                rem = step ? (interior ? rem - 1 : jrem) : rem;
                wi = step ? (interior ? wi : jwi) : wi;
                sh = step ? (interior ? sh : jsh) : sh;
            }
        }
    };
    const int nq = (Bb + Hb) / TS;
    for (int q = nq - 1; q >= 0; q--) {
        // stage psi rows: row r = segment sg0 + r, samples s_lo(r) + TS q + lc.  Wave-uniform tile origin +
        // 32-bit lane offsets; rows that do not exist read the origin and are staged as zeros.
        {
            const int64_t tb = sg0 * Bb + (int64_t)TS * q;
            const uint32_t *base = pc + (tb < T ? tb : 0);
#pragma unroll 16
            for (int rr = 0; rr < 64; rr += RPI) {
                const int r = rr + lr;
                const bool ok = (sg0 + r) < g.nseg && tb + (int64_t)r * Bb + lc < T;
                const uint32_t off = ok ? (uint32_t)(r * Bb + lc) : 0u;
                uint32_t v[PW];
#pragma unroll
                for (int w = 0; w < PW; w++) v[w] = (base + w * planePsi)[off];
#pragma unroll
                for (int w = 0; w < PW; w++) tile[w][r][lc] = ok ? v[w] : 0u;
            }
        }
        __syncthreads();
        if constexpr (ROWREG) {
#pragma unroll
            for (int w = 0; w < PW; w++)
#pragma unroll
                for (int i = 0; i < TS; i++) rowv[w][i] = tile[w][lane][i];
        }
        const int u0 = TS * q, u1 = u0 + TS;
        const bool own_tile = u0 < Bb;
        // wave-uniform choice of the tile body
        const bool lane_fast = u0 >= t1 && u1 <= te_rel &&
                               (own_tile ? (u1 <= hi_rel && u0 >= t2) : (u0 > hi_rel));
        const bool fast = __all(lane_fast);
        if (fast && own_tile) walk(q, std::true_type(), std::true_type());
        else if (fast) walk(q, std::true_type(), std::false_type());
        else walk(q, std::false_type(), std::false_type());
        if (own_tile) {  // owned rows: write x out, coalesced
#pragma unroll
            for (int j = 0; j < XW; j++) xt[lane][j] = xr[j];
            __syncthreads();
            const int xrw = lane / XW, xcw = lane % XW;
#pragma unroll 8
            for (int rr = 0; rr < 64; rr += XRI) {
                const int r = rr + xrw;
                const int64_t t = (sg0 + r) * Bb + (int64_t)TS * q + 2 * xcw;
                if ((sg0 + r) < g.nseg && t < T) {
                    const uint32_t v = xt[r][xcw];
                    if (t + 1 < T && xal) *reinterpret_cast<uint32_t *>(xc + t) = v;
                    else {
                        xc[t] = (int16_t)(v & 0xffffu);
                        if (t + 1 < T) xc[t + 1] = (int16_t)(v >> 16);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (active && hi_rel < te_rel) bstate[(int64_t)ch * g.nseg + sg] = bs;
    for (int o = 32; o > 0; o >>= 1) nflag += __shfl_xor(nflag, o);
    if (lane == 0 && nflag) atomicAdd((unsigned long long *)&tie_cnt[ch * 8 + kTieTrig], (unsigned long long)nflag);
}

// Six waves per SIMD is an 80-register budget.  The tiles are DYNAMIC shared memory: with a static size the
// compiler sees that LDS caps the waves per SIMD at two and takes twice the registers that are free beside the
// backward sweep.
template <int N, int SPW>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6)))
void kw_backtrace_light(WaveGeom g, const WaveConst *__restrict__ cst, const double *__restrict__ ysum,
                        const double *__restrict__ vend, const uint32_t *__restrict__ psi,
                        int32_t *__restrict__ final_state, int16_t *__restrict__ x, int32_t *__restrict__ bstate,
                        int64_t *__restrict__ tie_cnt)
{
    backtrace_light_body<N, SPW>(g, cst, ysum, vend, psi, final_state, x, bstate, tie_cnt);
}

__device__ __forceinline__ void wwalk_step(const WaveGeom &g, const uint32_t *__restrict__ pc, int64_t planePsi,
                                           int64_t t, int &a, int &k, int64_t &nflag)
{
    if (a >= 0 && k > 1) { k--; return; }
    const int e = a + 1;
    const uint32_t w = pc[(int64_t)(e / g.epw) * planePsi + t];
    const uint32_t ent = (w >> ((e % g.epw) * g.EB)) & ((1u << g.EB) - 1u);
    const int p = (int)(ent & ((1u << (g.EB - 1)) - 1u));
    if (t >= 2) nflag += ent >> (g.EB - 1);  // psi(1) only decides x[0], which kw_first_state re-decides exactly
    if (p == 0) { a = -1; k = 0; }
    else { a = p - 1; k = g.L; }
}

// Stitch check: the state segment s's walk had on the first sample of segment s+1 must equal what
// segment s+1 emitted there; otherwise segment s is queued for a re-walk.
__device__ __forceinline__ void stitch_check_one(const WaveGeom &g, const int16_t *x, const int32_t *bstate,
                                                 int32_t *head, int32_t *list, int64_t i)
{
    const int ch = (int)(i / g.nseg);
    const int64_t sg = i % g.nseg;
    if (sg >= g.nseg - 1) return;
    if (bstate[i] != (int)x[(int64_t)ch * g.T + (sg + 1) * g.Bb]) list[atomicAdd(&head[0], 1)] = (int32_t)i;
}

__global__ void kw_stitch_check(WaveGeom g, const int16_t *__restrict__ x, const int32_t *__restrict__ bstate,
                                int32_t *__restrict__ head, int32_t *__restrict__ list)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)g.C * g.nseg) return;
    stitch_check_one(g, x, bstate, head, list, i);
}

// Parallel repair of the queued segments whose successor is not queued itself (the common case: isolated
// disagreements on busy signals with long rings).  One workgroup per segment: its psi goes global -> LDS in
// full rows, lane 0 walks it from the successor's first state, all lanes write x.  A repaired segment whose
// own first sample changed is caught by the second check and the serial repair of kw_stitch_fix below, which
// also takes the chains of consecutive failures this kernel leaves alone.
__global__ __launch_bounds__(64) void kw_stitch_fix_par(WaveGeom g, const uint32_t *__restrict__ psi,
                                                        int16_t *__restrict__ x, int32_t *__restrict__ bstate,
                                                        const int32_t *__restrict__ head,
                                                        const int32_t *__restrict__ redo, int64_t *__restrict__ diag,
                                                        int64_t *__restrict__ tie_cnt)
{
    extern __shared__ uint32_t shp[];                 // [PW][Bb + 1] psi of the segment and the sample after it | Bb ids
    const int lane = threadIdx.x, n = head[0];
    const int L = g.L, Bb = g.Bb, PW = g.PW;
    int16_t *xs = reinterpret_cast<int16_t *>(shp + (size_t)PW * (Bb + 1));
    const int64_t planePsi = (int64_t)g.C * g.T;
    for (int q = blockIdx.x; q < n; q += gridDim.x) {
        const int32_t id = redo[q];
        const int ch = (int)(id / g.nseg);
        const int64_t sg = id % g.nseg;
        bool succ = false;
        for (int j = lane; j < n; j += 64) succ = succ || (redo[j] == id + 1 && sg + 1 < g.nseg);
        if (__any(succ)) continue;
        const uint32_t *pc = psi + (int64_t)ch * g.T;
        int16_t *xc = x + (int64_t)ch * g.T;
        const int64_t lo = sg * Bb, tn = lo + Bb;     // tn = first sample of segment sg + 1 (< T: sg is not the last)
        const int want = xc[tn];
        if (bstate[(int64_t)ch * g.nseg + sg] == want) continue;
        for (int w = 0; w < PW; w++)
            for (int i = lane; i <= Bb; i += 64) shp[w * (Bb + 1) + i] = pc[w * planePsi + lo + i];
        __syncthreads();
        if (lane == 0) {
            int a = -1, k = 0;
            int64_t nflag = 0;
            if (want > 1) { a = (want - 2) / L; k = (want - 2) % L + 1; }
            auto step = [&](int i) {                  // the move from sample lo + i to lo + i - 1
                if (a >= 0 && k > 1) { k--; return; }
                const int e = a + 1;
                const uint32_t wv = shp[(e / g.epw) * (Bb + 1) + i];
                const uint32_t ent = (wv >> ((e % g.epw) * g.EB)) & ((1u << g.EB) - 1u);
                const int p = (int)(ent & ((1u << (g.EB - 1)) - 1u));
                if (lo + i >= 2) nflag += ent >> (g.EB - 1);
                if (p == 0) { a = -1; k = 0; }
                else { a = p - 1; k = L; }
            };
            step(Bb);
            for (int i = Bb - 1; i >= 0; i--) {
                xs[i] = (int16_t)((a < 0) ? 1 : 2 + a * L + (k - 1));
                if (lo + i == 0) break;
                if (i > 0) step(i);
            }
            bstate[(int64_t)ch * g.nseg + sg] = want;
            atomicAdd((unsigned long long *)&diag[1], 1ull);
            if (nflag) atomicAdd((unsigned long long *)&tie_cnt[ch * 8 + kTieTrig], (unsigned long long)nflag);
        }
        __syncthreads();
        for (int i = lane; i < Bb; i += 64) xc[lo + i] = xs[i];
        __syncthreads();
    }
}

// The first decoded state, exactly as the reference finds it: x[0] = psi_1(x[1]) and psi_1 only sees
// the first trellis column, which is plain emission (viterbi.jl:55-63).  Template tails are ~1e-16, so
// the "ring in its last phase at sample 0" candidates differ by a few ulps only; re-deciding this one
// sample with the reference's own operations (strict '>', list order) makes it exact.
__device__ __forceinline__ void first_state(const WaveGeom &g, const WaveConst *__restrict__ cst,
                                            const double *__restrict__ y, const double *__restrict__ mean,
                                            const double *__restrict__ ctab_all, int16_t *x, int ch)
{
    const int N = g.N, L = g.L, S = 1 + N * L;
    const double *ctab = ctab_all + (int64_t)ch * (1 + 2 * N + N * N + N * L);
    const double *c0 = ctab + 1, *cend = ctab + 1 + N, *cx = ctab + 1 + 2 * N, *cint = ctab + 1 + 2 * N + N * N;
    const double *mc = mean + (int64_t)ch * S;
    const double A = cst[ch].A, den = cst[ch].den;
    int16_t *xc = x + (int64_t)ch * g.T;
    const double y0 = y[(int64_t)ch * g.T];
    auto T1 = [&](int a, int k) {  // funcl, utils.jl:4
        const double dd = y0 - mc[1 + a * L + (k - 1)];
        return A - (dd * dd) / den;
    };
    double best = -INFINITY;
    int arg = 1;
    auto cand = [&](int state, double t1, double lp) {
        const double tt = t1 + lp;
        if (tt > best) { best = tt; arg = state; }
    };
    const int x1 = *(const volatile int16_t *)&xc[1];   // the repair above may have rewritten it
    if (x1 == 1) {
        cand(1, 0.0, ctab[0]);
        for (int a = 0; a < N; a++) cand(1 + a * L + L, T1(a, L), cend[a]);
    } else {
        const int b = (x1 - 2) / L, k = (x1 - 2) % L + 1;
        if (k == 1) {
            cand(1, 0.0, c0[b]);
            for (int a = 0; a < N; a++)
                if (a != b) cand(1 + a * L + L, T1(a, L), cx[a * N + b]);
        } else {
            cand(1 + b * L + (k - 1), T1(b, k - 1), cint[b * L + (k - 1)]);
        }
    }
    xc[0] = (int16_t)arg;
}

// What is left after kw_stitch_fix_par, in ONE workgroup: when the first check listed anything (head1), the check
// is repeated (list 2), thread 0 repairs the listed segments serially -- chains of consecutive failures, first
// samples that changed -- and a workgroup barrier orders its stores before the last step, which every call needs:
// x[0] of every channel (first_state).  Nothing was listed: nothing can have changed, straight to that step.
__global__ __launch_bounds__(256) void kw_stitch_fix(WaveGeom g, const WaveConst *__restrict__ cst,
                                                     const double *__restrict__ y, const double *__restrict__ mean,
                                                     const double *__restrict__ ctab_all,
                                                     const uint32_t *__restrict__ psi, int16_t *x, int32_t *bstate,
                                                     const int32_t *__restrict__ head1, int32_t *head2, int32_t *redo,
                                                     int64_t *__restrict__ diag, int64_t *__restrict__ tie_cnt)
{
    const int tid = threadIdx.x;
    if (head1[0] != 0) {   // uniform over the workgroup
        const int64_t nsegT = (int64_t)g.C * g.nseg;
        for (int64_t i = tid; i < nsegT; i += blockDim.x) stitch_check_one(g, x, bstate, head2, redo, i);
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            const int n = atomicAdd(&head2[0], 0);
            const volatile int32_t *lst = redo;
            const int L = g.L, Bb = g.Bb;
            const int64_t planePsi = (int64_t)g.C * g.T;
            int64_t fixes = 0;
            for (int q = 0; q < n; q++) {
                const int32_t ent = lst[q];
                const int ch = (int)(ent / g.nseg);
                int64_t nflag = 0;
                int64_t sg = ent % g.nseg;
                const uint32_t *pc = psi + (int64_t)ch * g.T;
                int16_t *xc = x + (int64_t)ch * g.T;
                while (sg >= 0) {
                    const int64_t tn = (sg + 1) * Bb;  // first sample of segment sg+1
                    const int want = xc[tn];
                    if (bstate[(int64_t)ch * g.nseg + sg] == want) break;
                    bstate[(int64_t)ch * g.nseg + sg] = want;
                    fixes++;
                    int a = -1, k = 0;
                    if (want > 1) { a = (want - 2) / L; k = (want - 2) % L + 1; }
                    wwalk_step(g, pc, planePsi, tn, a, k, nflag);
                    for (int64_t t = tn - 1; t >= sg * Bb; t--) {
                        xc[t] = (int16_t)((a < 0) ? 1 : 2 + a * L + (k - 1));
                        if (t == 0) break;
                        if (t > sg * Bb) wwalk_step(g, pc, planePsi, t, a, k, nflag);
                    }
                    sg--;  // did the first sample of segment sg change?  then segment sg-1 must be re-checked
                }
                if (nflag) atomicAdd((unsigned long long *)&tie_cnt[ch * 8 + kTieTrig], (unsigned long long)nflag);
            }
            diag[1] += fixes;
        }
        __threadfence();
        __syncthreads();
    }
    if (g.T >= 2)
        for (int ch = tid; ch < g.C; ch += blockDim.x) first_state(g, cst, y, mean, ctab_all, x, ch);
}

// ll = sum_{t=1..T-1} T1[x_t, t]  (viterbi.jl:92-96) without the trellis:
//   T1[x_t,t] = T1[x_0,0] + sum_{u=1..t} inc_u  =>  ll = (T-1) T1[x_0,0] + sum_u (T-u) inc_u.
__global__ __launch_bounds__(256) void kw_ll_partial(WaveGeom g, const WaveConst *__restrict__ cst,
                                                     const double *__restrict__ y, const int16_t *__restrict__ x,
                                                     const double *__restrict__ mean,
                                                     const double *__restrict__ ctab_all, double *__restrict__ part)
{
    __shared__ double red[4];
    const int ch = blockIdx.y, N = g.N, L = g.L, S = 1 + N * L;
    const int64_t T = g.T;
    const double *yc = y + (int64_t)ch * T, *mc = mean + (int64_t)ch * S;
    const int16_t *xc = x + (int64_t)ch * T;
    const double *ctab = ctab_all + (int64_t)ch * (1 + 2 * N + N * N + N * L);
    const double A = cst[ch].A, den = cst[ch].den;
    double acc = 0.0;
    for (int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; u < T;
         u += (int64_t)gridDim.x * blockDim.x) {
        const int xp = xc[u - 1], xn = xc[u];
        const double d = yc[u] - mc[xn - 1];
        const double inc = wpath_lp(N, L, ctab, xp, xn) + (A - (d * d) / den);
        acc += (double)(T - u) * inc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int x0 = xc[0];
        if (x0 != 1) {  // T1[1,1] = 0 for the silent state (viterbi.jl:63)
            const double d = yc[0] - mc[x0 - 1];
            acc += (double)(T - 1) * (A - (d * d) / den);
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)ch * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void kw_sum_partials(const double *__restrict__ part, int n, double *__restrict__ out)
{
    __shared__ double red[4];
    const int ch = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) acc += part[(int64_t)ch * n + i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[ch] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename Kern>
static int wave_lds_attr(Kern kern, size_t lds)
{
    if (lds > 64 * 1024)
        HS_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return HMMSORT_OK;
}

// Segments per workgroup of the light backtrace (wave_common.h, with what was measured)
template <int N> constexpr int bt_spw() { return wave_bt_spw(N); }

constexpr int kVitRounds = 2;  // certificate + re-sweep rounds run unconditionally on device

// (which of the two calls with a decode does not matter to the sweep: wave_pick's uc is the same)
int wave_viterbi_sweep(WaveDev *r, const double *d_y, hipStream_t st)
{
    const WaveGeom &g = r->g;
    const int nchT = g.C * g.nch;
    const WavePick p = wave_pick(r, kWaveCallDecode);
    return dispatch_N(g.N, [&](auto n) {
        constexpr int N = decltype(n)::value;
        const size_t lds = ((size_t)N * (g.RB + 1) + 3 + 2 * N + N * N) * sizeof(double);
        auto kern = kw_vit<N, true>;
        if constexpr (N <= kWaveMaxPerSource) { if (!p.uc) kern = kw_vit<N, false>; }   // per-source values: up to 8 rings (wave_supported)
        int rc = wave_lds_attr(kern, lds);
        if (rc) return rc;
        { WPROF(r, "kw_vit", st);
          hipLaunchKernelGGL(kern, dim3(nchT), dim3(64), lds, st, g, r->d_cst, d_y, r->Rf, r->virt, r->ysum,
                             r->psi, r->vpre, r->vend, (uint32_t *)r->trash); }
        HS_HIP(hipGetLastError());
        return HMMSORT_OK;
    });
}

// boundary certificates with exact re-sweeps, final state + backtrace, stitch + x[0], near-ties, ll: all on st.  The call has
// zeroed diag, the tie counters and the list heads (wave_zero_bytes): every dependency below is a launch boundary.
int wave_viterbi_post(WaveDev *r, const double *d_y, int16_t *d_x, double *d_ll, hipStream_t st, bool beside)
{
    const WaveGeom &g = r->g;
    const int nchT = g.C * g.nch;
    const WavePick p = wave_pick(r, beside ? kWaveCallDecodeEstep : kWaveCallDecode);
    const bool light = p.light;
    int rc = dispatch_N(g.N, [&](auto n) {
        constexpr int N = decltype(n)::value;
        const size_t lds = ((size_t)N * (g.RB + 1) + 3 + 2 * N + N * N) * sizeof(double);
        auto kern = kw_vit_redo<N, true, false>;
        if constexpr (N <= kWaveMaxPerSource) { if (!p.uc) kern = kw_vit_redo<N, false, false>; }   // per-source values: up to 8 rings (wave_supported)
        if constexpr (N <= 4) { if (p.tight) kern = p.uc ? kw_vit_redo<N, true, true> : kw_vit_redo<N, false, true>; }
        HS_CHECK(p.spw == bt_spw<N>() && (N <= 4 || !p.tight), HMMSORT_EINVAL, "wave decode: no kernel for the picked row");
        int rc2 = wave_lds_attr(kern, lds);
        if (rc2) return rc2;
        // a round whose predecessor listed nothing returns at once (kw_vit_check); option "cert_rounds" = 1: all in full
        auto prev_head = [&](int round) -> const int32_t * {
            return (round > 0 && !g.cert_rounds && g.nch > 1) ? r->heads + round - 1 : nullptr;
        };
        for (int round = 0; round < kVitRounds && p.redo; round++) {
            int32_t *head = r->heads + round, *list = r->vlist + (size_t)round * nchT;
            { WPROF(r, "kw_vit_check", st);
              hipLaunchKernelGGL(kw_vit_check, dim3(nchT), dim3(64), 0, st, g, r->vpre, r->vend, r->vfail, r->diag, 0, nullptr,
                                 head, list, prev_head(round), (unsigned long long *)r->vcert); }
            { WPROF(r, "kw_vit_redo", st);
              hipLaunchKernelGGL(kern, dim3(std::min(nchT, kVitRedoGrid)), dim3(64), lds, st, g, r->d_cst, d_y, r->Rf,
                                 r->virt, r->ysum, r->psi, r->vpre, r->vend, (uint32_t *)r->trash, head, list); }
        }
        { WPROF(r, "kw_vit_check", st);
          hipLaunchKernelGGL(kw_vit_check, dim3(nchT), dim3(64), 0, st, g, r->vpre, r->vend, r->vfail, r->diag, 1, r->dbg,
                             nullptr, nullptr, prev_head(kVitRounds), (unsigned long long *)r->vcert); }
        { WPROF(r, "kw_backtrace", st);
          const dim3 grid_rows((unsigned)((g.nseg + 63) / 64), g.C);
          constexpr int SPW = bt_spw<N>();
          if (!light)   // the register-row form's tiles are static
              hipLaunchKernelGGL(kw_backtrace<N>, grid_rows, dim3(64), 0, st, g, r->d_cst, r->ysum, r->vend, r->psi,
                                 r->final_state, d_x, r->bstate, r->tie_cnt);
          else
              hipLaunchKernelGGL((kw_backtrace_light<N, SPW>), dim3((unsigned)((g.nseg + SPW - 1) / SPW), g.C), dim3(64),
                                 (bt_lds_bytes<N, SPW>()), st, g, r->d_cst, r->ysum, r->vend, r->psi, r->final_state, d_x,
                                 r->bstate, r->tie_cnt); }
        HS_HIP(hipGetLastError());
        return HMMSORT_OK;
    });
    if (rc) return rc;
    const int64_t nsegT = (int64_t)g.C * g.nseg;
    { WPROF(r, "kw_stitch_check", st);
      hipLaunchKernelGGL(kw_stitch_check, dim3((unsigned)((nsegT + 255) / 256)), dim3(256), 0, st, g, d_x, r->bstate,
                         r->heads + 2, r->redo); }
    { WPROF(r, "kw_stitch_fix", st);
      // isolated failures in parallel, then (one launch) a second check and the serial repair for what is left
      // (chains of consecutive failures, first samples that changed) and x[0] of every channel
      const size_t ldsp = ((size_t)g.PW * (g.Bb + 1)) * sizeof(uint32_t) + (size_t)g.Bb * sizeof(int16_t) + 8;
      hipLaunchKernelGGL(kw_stitch_fix_par, dim3(256), dim3(64), ldsp, st, g, r->psi, d_x, r->bstate, r->heads + 2, r->redo,
                         r->diag, r->tie_cnt);
      hipLaunchKernelGGL(kw_stitch_fix, dim3(1), dim3(256), 0, st, g, r->d_cst, d_y, r->d_mean, r->d_ctab, r->psi, d_x,
                         r->bstate, r->heads + 2, r->heads + 3, r->redo + nsegT, r->diag, r->tie_cnt); }
    // flagged near-ties on the decoded path: re-decided with the reference's own arithmetic (no-ops otherwise)
    if ((rc = wave_tie_resolve(r, d_y, d_x, st))) return rc;
    { WPROF(r, "kw_ll_partial", st);
      hipLaunchKernelGGL(kw_ll_partial, dim3(r->nparts, g.C), dim3(256), 0, st, g, r->d_cst, d_y, d_x, r->d_mean,
                         r->d_ctab, r->part); }
    { WPROF(r, "kw_sum_partials", st);
      hipLaunchKernelGGL(kw_sum_partials, dim3(g.C), dim3(256), 0, st, r->part, r->nparts, d_ll); }
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

int wave_viterbi(WaveDev *r, const double *d_y, int16_t *d_x, double *d_ll, hipStream_t st)
{
    return wave_graphed(r, 1, d_y, d_x, d_ll, nullptr, st, [&](hipStream_t s) -> int {
        int rc;
        HS_HIP(hipMemsetAsync(r->diag, 0, wave_zero_bytes(r, true), s));   // diag, the tie counters, the list heads
        if ((rc = wave_prepare(r, d_y, s))) return rc;
        if ((rc = wave_viterbi_sweep(r, d_y, s))) return rc;
        // (ll behind the resolver, on s: on a stream of its own beside it the decode alone was slower)
        return wave_viterbi_post(r, d_y, d_x, d_ll, s, false);
    });
}

}  // namespace hmmsort
