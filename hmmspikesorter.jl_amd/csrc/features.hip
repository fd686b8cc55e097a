// Waveform features and cluster isolation of sorted units (hmmsort_snippet_features / hmmsort_cluster_isolation and
// their device and plan forms, include/hmmsort.h).  Every figure is a gather plus small dense products in
// a fixed order -- no fused multiply-add (-ffp-contract=off), no floating-point atomics, no matrix cores -- so the same
// input gives the same bits and the numpy model tests/feature_model.py states the same rules.
//
// The U lists sit concatenated in device memory behind U + 1 host offsets, as for the footprints; entry e of unit u is
// row offs[u] - offs[0] + e.  The channel table is one row for all units, so the row kernels never ask for the unit.
//   k_ft_used     one block per unit: used[r] as bytes and the unit's count of used entries (integer sums).
//   k_ft_export   no basis.  A block takes kFtExportRows rows; its threads run over (slot, k), so a wave reads one
//                 contiguous run of a channel's row per spike and writes one contiguous run of the feature row.
//   k_ft_project  with a basis.  One lane per row: per slot and per group of kFtAcc components, a serial fold over k
//                 ascending of basis * (s - centre), the subtraction, product and sum rounded on their own.  basis and
//                 centre are indexed by loop counters only, the same for every lane (scalar loads).  The lane walks its
//                 window straight from the block: consecutive k of one lane share cache lines, lanes do not.
//   k_ft_moments  grid (tile, group, chunk of kFtPairs * 256 items of the group's G x G square; an item is one row a
//                 and four columns b).  A group is a slot (mode 1, G = P) or the whole row (mode 2, G = F).  The
//                 tile's features are staged in LDS kFtStage entries at a time (from the feature rows with a basis,
//                 from the block itself without one), and every lane folds its (a, b >= a) serially from +0.0 in
//                 entry order (an unused entry is staged as +0.0, which leaves a sum that started at +0.0 as it is to
//                 the bit): f_a is read once for four products.  The item that holds
//                 (a, a) also carries p1_a.  Partials go to [tile][group][G x G].
//   k_ft_mfold    one lane per (u, group, a, b >= a): the unit's tile partials folded from +0.0 in tile order; (a, b)
//                 is written with its mirror.
//   k_iso_d2      grid (rows / kIsoRows, unit).  One lane per row: d = f - mu[u] into LDS (component-major, so lanes
//                 sit side by side), then the quadratic form with Vinv[u] (loop counters only: scalar loads).  Writes
//                 the select's key of (u, r) -- the pattern of d2, all ones for a member or unused row -- and, for a
//                 member, own[r].
//   k_iso_pairs   grid (v, u).  Over the rows of v in tiles of 256 list entries: the strict count of key(u, r) <
//                 own[r] (patterns of non-negative doubles order as the doubles do), and Q_F(d2(u, r)) into LDS (+0.0
//                 for an unused entry: it leaves the sum as it is), which lane 0 folds serially from +0.0; tile
//                 partials added in tile order.
// The order statistic is dev_radix_select over the keys, all units side by side as slots.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

constexpr int kFtTile = 256;        // list entries of one tile (the constant of spike_fit and footprint)
constexpr int kFtExportRows = 16;   // rows of one export block
constexpr int kFtAcc = 4;           // components a projecting lane carries at once
constexpr int kFtStage = 32;        // tile entries staged at once: 32 x 128 doubles = 32 KB of LDS
constexpr int kFtMaxG = 128;        // largest group (mode 1: P <= 128; mode 2: F <= 64)
constexpr int kFtPairs = 4;         // items per lane; an item is one row and four columns of the G x G square
constexpr int kIsoRows = 64;        // rows of one distance block (one wave): 64 x F doubles of LDS, 32 KB at F = 64
constexpr unsigned long long kAllOnes = ~0ull;

struct FtArgs {
    const double *y;          // [C][T]
    const int64_t *t;         // the lists, from row 0
    const int64_t *offs;      // [U + 1] first row of a unit (offs[0] = 0)
    const int32_t *chan;      // [M] or null
    const double *basis;      // [M][Pp][W], Pp = P rounded up to kFtAcc, zero rows behind P; null: none
    const double *centre;     // [M][W] or null
    int64_t T, lo, hi, n;     // an entry t is used iff lo <= t <= hi (lo = 1 + pre, hi = T - W + 1 + pre); n rows
    int M, W, P, Pp, F;
    double *feat;             // [n][F] or null
    unsigned char *used;      // [n] or null
    int64_t *nused;           // [U]
    const double *src;        // mode != 0 with a basis: the feature rows the moments read
    int G, groups, U;
    const int64_t *tile_r;    // [ntiles] first row of a tile
    const int32_t *tile_n;    // [ntiles] its entries, 1..256
    const int64_t *first;     // [U + 1] first tile of a unit
    double *part1, *part2;    // [ntiles][groups][G], [ntiles][groups][G][G] (b >= a written)
    double *m1, *m2;          // [U][groups][G], [U][groups][G][G]
};

__global__ __launch_bounds__(kFtTile) void k_ft_used(const FtArgs A)
{
    __shared__ unsigned long long s_c;
    if (threadIdx.x == 0) s_c = 0;
    __syncthreads();
    const int64_t r0 = A.offs[blockIdx.x], r1 = A.offs[blockIdx.x + 1];
    unsigned long long c = 0;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += kFtTile) {
        const int64_t t = A.t[r];
        const bool u = t >= A.lo && t <= A.hi;
        if (A.used) A.used[r] = u ? 1 : 0;
        c += u ? 1 : 0;
    }
    if (c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0) A.nused[blockIdx.x] = (int64_t)s_c;
}

__global__ __launch_bounds__(kFtTile) void k_ft_export(const FtArgs A)
{
    const int64_t r0 = (int64_t)blockIdx.x * kFtExportRows;
    for (int i = 0; i < kFtExportRows; i++) {
        const int64_t r = r0 + i;
        if (r >= A.n) return;
        const int64_t t = A.t[r];
        const bool u = t >= A.lo && t <= A.hi;
        const int64_t b = u ? t - A.lo : 0;   // 0 <= b <= T - W
        for (int j = threadIdx.x; j < A.F; j += kFtTile) {
            const int m = j / A.W, k = j - m * A.W;
            const int ch = A.chan ? A.chan[m] : m;
            double v = A.y[(int64_t)ch * A.T + b + k];
            if (A.centre) v = v - A.centre[j];
            A.feat[r * A.F + j] = u ? v : 0.0;
        }
    }
}

__global__ __launch_bounds__(kFtTile) void k_ft_project(const FtArgs A)
{
    const int64_t r = (int64_t)blockIdx.x * kFtTile + threadIdx.x;
    if (r >= A.n) return;
    const int64_t t = A.t[r];
    const bool u = t >= A.lo && t <= A.hi;
    const int64_t b = u ? t - A.lo : 0;   // an unused entry reads the window at sample 0 and writes +0.0
    double *out = A.feat + r * A.F;
    for (int m = 0; m < A.M; m++) {
        const int ch = A.chan ? A.chan[m] : m;
        const double *yp = A.y + (int64_t)ch * A.T + b;
        const double *cm = A.centre + (int64_t)m * A.W;
        for (int p0 = 0; p0 < A.P; p0 += kFtAcc) {
            const double *bp = A.basis + ((int64_t)m * A.Pp + p0) * A.W;
            double acc[kFtAcc];
#pragma unroll
            for (int j = 0; j < kFtAcc; j++) acc[j] = 0.0;
            for (int k = 0; k < A.W; k++) {
                const double d = yp[k] - cm[k];
#pragma unroll
                for (int j = 0; j < kFtAcc; j++) {
                    const double q = bp[(int64_t)j * A.W + k] * d;   // rounded on its own (-ffp-contract=off)
                    acc[j] = acc[j] + q;
                }
            }
#pragma unroll
            for (int j = 0; j < kFtAcc; j++)
                if (p0 + j < A.P) out[m * A.P + p0 + j] = u ? acc[j] : 0.0;
        }
    }
}

__global__ __launch_bounds__(kFtTile) void k_ft_moments(const FtArgs A)
{
    __shared__ double s_f[kFtStage * kFtMaxG];   // [entry][Gp], Gp = G rounded up to 4, zeros behind G
    __shared__ int64_t s_b[kFtStage];
    const int grp = blockIdx.y, G = A.G, G4 = (G + 3) / 4, Gp = G4 * 4, gbase = grp * G;
    int a[kFtPairs], b0[kFtPairs];   // a lane's items: row a, columns b0 .. b0 + 3 of the square
    bool act[kFtPairs];
    double p1[kFtPairs], p2[kFtPairs][4];
#pragma unroll
    for (int j = 0; j < kFtPairs; j++) {
        const int it = ((int)blockIdx.z * kFtPairs + j) * kFtTile + (int)threadIdx.x;
        a[j] = it / G4, b0[j] = (it - a[j] * G4) * 4;
        act[j] = it < G * G4 && b0[j] + 3 >= a[j];   // some b >= a among the four
        if (!act[j]) a[j] = b0[j] = 0;
        p1[j] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) p2[j][i] = 0.0;
    }
    const int64_t tile = A.tile_r[blockIdx.x];
    const int nt = A.tile_n[blockIdx.x];
    for (int sub = 0; sub < nt; sub += kFtStage) {
        const int ns = nt - sub < kFtStage ? nt - sub : kFtStage;
        __syncthreads();   // the previous stage has been folded
        if ((int)threadIdx.x < ns) {
            const int64_t t = A.t[tile + sub + threadIdx.x];
            s_b[threadIdx.x] = t >= A.lo && t <= A.hi ? t - A.lo : -1;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ns * Gp; i += kFtTile) {
            const int e = i / Gp, g = i - e * Gp;
            const int64_t bb = s_b[e];
            double v = 0.0;
            if (bb >= 0 && g < G) {
                const int j = gbase + g;
                if (A.src) {
                    v = A.src[(tile + sub + e) * A.F + j];
                } else {
                    const int m = j / A.W, k = j - m * A.W;
                    const int ch = A.chan ? A.chan[m] : m;
                    v = A.y[(int64_t)ch * A.T + bb + k];
                    if (A.centre) v = v - A.centre[j];
                }
            }
            s_f[i] = v;
        }
        __syncthreads();
        for (int e = 0; e < ns; e++) {   // an unused entry was staged as +0.0: its products and adds change nothing
            const double *f = s_f + e * Gp;
#pragma unroll
            for (int j = 0; j < kFtPairs; j++) {
                const double fa = f[a[j]];
                p1[j] = p1[j] + fa;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const double q = fa * f[b0[j] + i];   // rounded on its own
                    p2[j][i] = p2[j][i] + q;
                }
            }
        }
    }
    const int64_t o = (int64_t)blockIdx.x * A.groups + grp;
#pragma unroll
    for (int j = 0; j < kFtPairs; j++) {
        if (!act[j]) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int b = b0[j] + i;
            if (b < a[j] || b >= G) continue;
            A.part2[(o * G + a[j]) * G + b] = p2[j][i];
            if (b == a[j]) A.part1[o * G + a[j]] = p1[j];
        }
    }
}

// one lane per (u, group, a, b >= a): the unit's tile partials folded from +0.0 in tile order, written with the mirror;
// the lane of (a, a) folds p1_a as well.  A unit without tiles gets zeros.
__global__ __launch_bounds__(kFtTile) void k_ft_mfold(const FtArgs A)
{
    const int64_t idx = (int64_t)blockIdx.x * kFtTile + threadIdx.x, GG = (int64_t)A.G * A.G;
    if (idx >= (int64_t)A.U * A.groups * GG) return;
    const int64_t ug = idx / GG;
    const int ab = (int)(idx - ug * GG), a = ab / A.G, b = ab - a * A.G;
    if (b < a) return;
    const int u = (int)(ug / A.groups), grp = (int)(ug - (int64_t)u * A.groups);
    double acc1 = 0.0, acc2 = 0.0;
    for (int64_t tile = A.first[u]; tile < A.first[u + 1]; tile++) {
        const int64_t o = tile * A.groups + grp;
        acc2 = acc2 + A.part2[(o * A.G + a) * A.G + b];
        if (a == b) acc1 = acc1 + A.part1[o * A.G + a];
    }
    A.m2[(ug * A.G + a) * A.G + b] = acc2;
    A.m2[(ug * A.G + b) * A.G + a] = acc2;
    if (a == b) A.m1[ug * A.G + a] = acc1;
}

struct IsoArgs {
    const double *feat;            // [n][F]
    const unsigned char *used;     // [n] or null: all used
    const int64_t *offs;           // [U + 1], offs[0] = 0
    const double *mu, *vinv;       // [U][F], [U][F][F]
    const unsigned char *scored;   // [U]
    int64_t n;
    int U, F;
    unsigned long long *keys;      // [U][n]
    unsigned long long *own;       // [n] pattern of d2[unit of r][r]
    int64_t *closer;               // [U][U]
    double *lpair;                 // [U][U]
};

__global__ __launch_bounds__(kIsoRows) void k_iso_d2(const IsoArgs A)
{
    extern __shared__ double s_d[];   // [F][kIsoRows]
    const int u = blockIdx.y, F = A.F;
    const int64_t r = (int64_t)blockIdx.x * kIsoRows + threadIdx.x;
    if (r >= A.n) return;   // no barrier below
    unsigned long long *key = A.keys + (int64_t)u * A.n + r;
    const bool use = !A.used || A.used[r];
    if (!A.scored[u] || !use) {
        *key = kAllOnes;
        return;
    }
    const double *f = A.feat + r * F, *mu = A.mu + (int64_t)u * F, *V = A.vinv + (int64_t)u * F * F;
    double *d = s_d + threadIdx.x;
    for (int b = 0; b < F; b++) d[b * kIsoRows] = f[b] - mu[b];
    double q = 0.0;
    for (int a = 0; a < F; a++) {
        double rr = 0.0;
        for (int b = 0; b < F; b++) {
            const double p = V[a * F + b] * d[b * kIsoRows];   // rounded on its own
            rr = rr + p;
        }
        const double p = d[a * kIsoRows] * rr;
        q = q + p;
    }
    const double d2 = q > 0.0 ? q : 0.0;   // a NaN is clamped as well
    const unsigned long long pat = (unsigned long long)__double_as_longlong(d2);
    const bool member = r >= A.offs[u] && r < A.offs[u + 1];
    *key = member ? kAllOnes : pat;
    if (member) A.own[r] = pat;
}

// the chi-square survival function of F degrees of freedom (include/hmmsort.h states the form)
__device__ double iso_chi2_sf(double x, int F)
{
    const double h = 0.5 * x;
    const double eh = exp(-h);
    if (eh == 0.0) return 0.0;   // past h = 745.2 the tail is below the smallest double; the series may overflow
    if ((F & 1) == 0) {
        double t = 1.0, s = 1.0;
        for (int j = 1; j < F / 2; j++) {
            t = t * h / (double)j;
            s = s + t;
        }
        return eh * s;
    }
    const double sh = sqrt(h);
    double res = erfc(sh);
    if (F >= 3) {
        double t = 1.0, s = 1.0;
        for (int j = 1; j <= (F - 3) / 2; j++) {
            t = t * h / ((double)j + 0.5);
            s = s + t;
        }
        res = res + eh * sh * 1.1283791670955126 * s;   // 2 / sqrt(pi)
    }
    return res;
}

__global__ __launch_bounds__(kFtTile) void k_iso_pairs(const IsoArgs A)
{
    __shared__ double s_q[kFtTile];
    __shared__ unsigned long long s_c;
    const int v = blockIdx.x, u = blockIdx.y;
    if (u == v || !A.scored[u]) return;   // the host fills these entries
    if (threadIdx.x == 0) s_c = 0;
    const int64_t r0 = A.offs[v], r1 = A.offs[v + 1];
    const bool count = A.scored[v] != 0;
    unsigned long long c = 0;
    double acc = 0.0;
    for (int64_t tile = r0; tile < r1; tile += kFtTile) {
        const int nt = (int)(r1 - tile < kFtTile ? r1 - tile : kFtTile);
        __syncthreads();   // lane 0 has folded the previous tile
        if ((int)threadIdx.x < nt) {
            const int64_t r = tile + threadIdx.x;
            const bool use = !A.used || A.used[r];
            double q = 0.0;   // an unused entry adds +0.0, which leaves a sum of non-negative terms from +0.0 as it is
            if (use) {
                const unsigned long long k = A.keys[(int64_t)u * A.n + r];
                if (count && k < A.own[r]) c++;
                q = iso_chi2_sf(__longlong_as_double((long long)k), A.F);
            }
            s_q[threadIdx.x] = q;
        } else {
            s_q[threadIdx.x] = 0.0;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double p = 0.0;
#pragma unroll 16
            for (int e = 0; e < kFtTile; e++) p = p + s_q[e];   // in entry order; the loads run ahead of the adds
            acc = acc + p;
        }
    }
    if (c) atomicAdd(&s_c, c);
    __syncthreads();
    if (threadIdx.x == 0) {
        A.closer[(int64_t)u * A.U + v] = (int64_t)s_c;
        A.lpair[(int64_t)u * A.U + v] = acc;
    }
}

bool all_finite(const double *p, int64_t n, int64_t *bad)
{
    for (int64_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) {
            *bad = i;
            return false;
        }
    return true;
}

}  // namespace

int feat_check(const char *who, int64_t C, int64_t T, int64_t U, const hmmsort_feat_opt *opt,
               const hmmsort_feat_out *out, FeatDims *d)
{
    HS_CHECK(opt && out && out->n, HMMSORT_EINVAL, "%s: null argument (the options, the output record and its n are "
             "required)", who);
    HS_CHECK(C >= 1 && C <= HMMSORT_PRE_MAX_CHANNELS, HMMSORT_EINVAL, "%s: C = %lld channels (1..%d)", who,
             (long long)C, HMMSORT_PRE_MAX_CHANNELS);
    HS_CHECK(T >= 1 && T <= (1ll << 36), HMMSORT_EINVAL, "%s: T = %lld samples (1..2^36)", who, (long long)T);
    HS_CHECK(U >= 1 && U <= HMMSORT_FP_MAX_UNITS, HMMSORT_EINVAL, "%s: U = %lld units (1..%d)", who, (long long)U,
             HMMSORT_FP_MAX_UNITS);
    HS_CHECK(opt->W >= 1 && opt->W <= HMMSORT_FP_MAX_W, HMMSORT_EINVAL, "%s: W = %lld window samples (1..%d)", who,
             (long long)opt->W, HMMSORT_FP_MAX_W);
    HS_CHECK(opt->pre >= 0 && opt->pre <= (1ll << 20), HMMSORT_EINVAL, "%s: pre = %lld (0..2^20)", who,
             (long long)opt->pre);
    const int64_t W = opt->W;
    int64_t M = C;
    if (opt->chan) {
        M = opt->M;
        HS_CHECK(M >= 1 && M <= HMMSORT_FP_MAX_SLOTS, HMMSORT_EINVAL, "%s: M = %lld slots (1..%d)", who, (long long)M,
                 HMMSORT_FP_MAX_SLOTS);
        for (int64_t m = 0; m < M; m++)
            HS_CHECK(opt->chan[m] >= 0 && opt->chan[m] < C, HMMSORT_EINVAL, "%s: chan: slot %lld: channel %d outside "
                     "0..%lld", who, (long long)m, (int)opt->chan[m], (long long)(C - 1));
    }
    HS_CHECK(opt->moments >= 0 && opt->moments <= 2, HMMSORT_EINVAL, "%s: moments = %lld (0, 1 or 2)", who,
             (long long)opt->moments);
    HS_CHECK(opt->P >= 1, HMMSORT_EINVAL, "%s: P = %lld components (at least 1)", who, (long long)opt->P);
    int64_t P = W, bad = 0;
    if (opt->basis) {
        P = opt->P;
        HS_CHECK(P <= W, HMMSORT_EINVAL, "%s: P = %lld components of a window of W = %lld samples", who, (long long)P,
                 (long long)W);
        HS_CHECK(all_finite(opt->basis, M * P * W, &bad), HMMSORT_EINVAL, "%s: basis: slot %lld, component %lld, "
                 "sample %lld is not finite", who, (long long)(bad / (P * W)), (long long)(bad / W % P),
                 (long long)(bad % W));
    }
    if (opt->centre)
        HS_CHECK(all_finite(opt->centre, M * W, &bad), HMMSORT_EINVAL, "%s: centre: slot %lld, sample %lld is not "
                 "finite", who, (long long)(bad / W), (long long)(bad % W));
    const int64_t F = M * P;
    if (opt->moments == 1) {
        HS_CHECK(out->b1 && out->b2, HMMSORT_EINVAL, "%s: moments = 1 needs the output arrays b1 and b2", who);
        HS_CHECK(P <= HMMSORT_FEAT_MAX_P1, HMMSORT_EUNSUP, "%s: moments = 1 with P = %lld components per slot (at "
                 "most %d)", who, (long long)P, HMMSORT_FEAT_MAX_P1);
        HS_CHECK(U * M * P * P <= (1ll << 26), HMMSORT_EUNSUP, "%s: %lld second moments (U * M * P * P = %lld * %lld * "
                 "%lld * %lld; at most 2^26)", who, (long long)(U * M * P * P), (long long)U, (long long)M,
                 (long long)P, (long long)P);
    }
    if (opt->moments == 2) {
        HS_CHECK(out->g1 && out->g2, HMMSORT_EINVAL, "%s: moments = 2 needs the output arrays g1 and g2", who);
        HS_CHECK(F <= HMMSORT_FEAT_MAX_F2, HMMSORT_EUNSUP, "%s: moments = 2 with F = %lld features (M * P = %lld * "
                 "%lld; at most %d)", who, (long long)F, (long long)M, (long long)P, HMMSORT_FEAT_MAX_F2);
        HS_CHECK(U * F * F <= (1ll << 26), HMMSORT_EUNSUP, "%s: %lld second moments (U * F * F = %lld * %lld * %lld; "
                 "at most 2^26)", who, (long long)(U * F * F), (long long)U, (long long)F, (long long)F);
    }
    d->M = M, d->P = P, d->F = F;
    return HMMSORT_OK;
}

int feat_check_rows(const char *who, int64_t n_total, int64_t F)
{
    HS_CHECK(n_total <= (1ll << 31) / F, HMMSORT_EUNSUP, "%s: %lld feature entries (n_total * F = %lld * %lld; at most "
             "2^31)", who, (long long)(n_total * F), (long long)n_total, (long long)F);
    return HMMSORT_OK;
}

int dev_snippet_features(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times,
                         const int64_t *offs, const hmmsort_feat_opt *opt, const hmmsort_feat_out *out,
                         const FeatDims &dm, double *d_feat, unsigned char *d_used, hipStream_t st)
{
    const int64_t W = opt->W, M = dm.M, P = dm.P, F = dm.F, n = offs[U] - offs[0];
    const int mode = (int)opt->moments;
    const int64_t G = mode == 1 ? P : F, groups = mode == 1 ? M : 1, n1 = mode ? U * groups * G : 0, n2 = n1 * G;
    double *h1 = mode == 1 ? out->b1 : out->g1, *h2 = mode == 1 ? out->b2 : out->g2;
    for (int64_t u = 0; u < U; u++) out->n[u] = offs[u + 1] - offs[u];
    if (n == 0 || W > T) {   // no spike, or no window fits: zeros, nothing is read
        if (d_feat && n > 0) HS_HIP(hipMemsetAsync(d_feat, 0, (size_t)(n * F) * sizeof(double), st));
        if (d_used && n > 0) HS_HIP(hipMemsetAsync(d_used, 0, (size_t)n, st));
        if (out->nused) std::fill(out->nused, out->nused + U, (int64_t)0);
        if (mode) std::fill(h1, h1 + n1, 0.0), std::fill(h2, h2 + n2, 0.0);
        HS_HIP(hipStreamSynchronize(st));
        return HMMSORT_OK;
    }
    // one table upload in 8-byte words: offsets from row 0, the channel row, the padded basis, the centre
    const int64_t Pp = (P + kFtAcc - 1) / kFtAcc * kFtAcc;
    const int64_t o_chan = U + 1, o_basis = o_chan + (opt->chan ? (M + 1) / 2 : 0);
    const int64_t o_centre = o_basis + (opt->basis ? M * Pp * W : 0);
    const bool centre = opt->centre || opt->basis;   // the projection always subtracts (zeros change nothing)
    int64_t ntiles = 0;   // the moments' tiles of 256 list entries: first row, entries; first tile per unit
    for (int64_t u = 0; mode && u < U; u++) ntiles += (out->n[u] + kFtTile - 1) / kFtTile;
    HS_CHECK(ntiles <= 0x7fffffffll, HMMSORT_EUNSUP, "snippet_features: %lld tiles of %d entries", (long long)ntiles,
             kFtTile);
    const int64_t o_tr = o_centre + (centre ? M * W : 0), o_tn = o_tr + ntiles, o_first = o_tn + (ntiles + 1) / 2;
    const int64_t o_nused = o_first + (mode ? U + 1 : 0), o_m1 = o_nused + U, o_m2 = o_m1 + n1, o_p1 = o_m2 + n2;
    const int64_t o_p2 = o_p1 + ntiles * groups * G, o_feat = o_p2 + ntiles * groups * G * G;
    const bool own_feat = opt->basis && mode && !d_feat;   // the moments of projected rows read the rows
    const int64_t words = o_feat + (own_feat ? n * F : 0);
    std::vector<int64_t> tab((size_t)o_nused, 0);
    for (int64_t u = 0; u <= U; u++) tab[(size_t)u] = offs[u] - offs[0];
    if (mode) {
        int32_t *tile_n = (int32_t *)(tab.data() + o_tn);
        for (int64_t u = 0, k = 0; u < U; u++) {
            tab[(size_t)(o_first + u)] = k;
            for (int64_t e = 0; e < out->n[u]; e += kFtTile, k++) {
                tab[(size_t)(o_tr + k)] = offs[u] - offs[0] + e;
                tile_n[k] = (int32_t)std::min<int64_t>(kFtTile, out->n[u] - e);
            }
            tab[(size_t)(o_first + u + 1)] = k;
        }
    }
    if (opt->chan) std::copy(opt->chan, opt->chan + M, (int32_t *)(tab.data() + o_chan));
    if (opt->basis) {
        double *bp = (double *)(tab.data() + o_basis);
        for (int64_t m = 0; m < M; m++)
            std::copy(opt->basis + m * P * W, opt->basis + (m + 1) * P * W, bp + m * Pp * W);
    }
    if (opt->centre) std::copy(opt->centre, opt->centre + M * W, (double *)(tab.data() + o_centre));
    DevBuf ws;
    int rc;
    if ((rc = ws.alloc((size_t)words * sizeof(int64_t)))) return rc;
    int64_t *w = ws.as<int64_t>();
    HS_HIP(hipMemcpyAsync(w, tab.data(), (size_t)o_nused * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if (own_feat) d_feat = (double *)(w + o_feat);
    FtArgs A;
    A.y = d_y, A.t = d_times + offs[0], A.offs = w;
    A.chan = opt->chan ? (const int32_t *)(w + o_chan) : nullptr;
    A.basis = opt->basis ? (const double *)(w + o_basis) : nullptr;
    A.centre = centre ? (const double *)(w + o_centre) : nullptr;
    A.T = T, A.lo = 1 + opt->pre, A.hi = T - W + 1 + opt->pre, A.n = n;
    A.M = (int)M, A.W = (int)W, A.P = (int)P, A.Pp = (int)Pp, A.F = (int)F;
    A.feat = d_feat, A.used = d_used, A.nused = w + o_nused;
    A.src = opt->basis ? d_feat : nullptr;
    A.G = (int)G, A.groups = (int)groups, A.U = (int)U;
    A.tile_r = w + o_tr, A.tile_n = (const int32_t *)(w + o_tn), A.first = w + o_first;
    A.part1 = (double *)(w + o_p1), A.part2 = (double *)(w + o_p2);
    A.m1 = (double *)(w + o_m1), A.m2 = (double *)(w + o_m2);
    if (d_used || out->nused) {
        hipLaunchKernelGGL(k_ft_used, dim3((unsigned)U), dim3(kFtTile), 0, st, A);
        HS_HIP(hipGetLastError());
    }
    if (d_feat) {
        if (opt->basis)
            hipLaunchKernelGGL(k_ft_project, dim3((unsigned)((n + kFtTile - 1) / kFtTile)), dim3(kFtTile), 0, st, A);
        else
            hipLaunchKernelGGL(k_ft_export, dim3((unsigned)((n + kFtExportRows - 1) / kFtExportRows)), dim3(kFtTile),
                               0, st, A);
        HS_HIP(hipGetLastError());
    }
    if (mode) {
        const int64_t chunks = (G * ((G + 3) / 4) + kFtPairs * kFtTile - 1) / (kFtPairs * kFtTile);
        hipLaunchKernelGGL(k_ft_moments, dim3((unsigned)ntiles, (unsigned)groups, (unsigned)chunks), dim3(kFtTile), 0,
                           st, A);
        HS_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_ft_mfold, dim3((unsigned)((n2 + kFtTile - 1) / kFtTile)), dim3(kFtTile), 0, st, A);
        HS_HIP(hipGetLastError());
        HS_HIP(hipMemcpyAsync(h1, A.m1, (size_t)n1 * sizeof(double), hipMemcpyDeviceToHost, st));
        HS_HIP(hipMemcpyAsync(h2, A.m2, (size_t)n2 * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    if (out->nused) HS_HIP(hipMemcpyAsync(out->nused, A.nused, U * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));   // the workspace and `tab` die with this frame
    return HMMSORT_OK;
}

int iso_check(const char *who, int64_t n, int64_t F, int64_t U, const int64_t *offs, const double *mu,
              const double *vinv, const hmmsort_iso_out *out, std::vector<unsigned char> *scored)
{
    HS_CHECK(offs && mu && vinv && out, HMMSORT_EINVAL, "%s: null argument (offs, mu, Vinv and the output record are "
             "required)", who);
    HS_CHECK(F >= 1 && F <= HMMSORT_FEAT_MAX_F2, HMMSORT_EINVAL, "%s: F = %lld features (1..%d)", who, (long long)F,
             HMMSORT_FEAT_MAX_F2);
    HS_CHECK(U >= 1 && U <= HMMSORT_FP_MAX_UNITS, HMMSORT_EINVAL, "%s: U = %lld units (1..%d)", who, (long long)U,
             HMMSORT_FP_MAX_UNITS);
    HS_CHECK(offs[0] >= 0, HMMSORT_EINVAL, "%s: offs[0] = %lld", who, (long long)offs[0]);
    for (int64_t u = 0; u < U; u++)
        HS_CHECK(offs[u + 1] >= offs[u], HMMSORT_EINVAL, "%s: offs: unit %lld has a count of %lld", who, (long long)u,
                 (long long)(offs[u + 1] - offs[u]));
    HS_CHECK(n == offs[U] - offs[0], HMMSORT_EINVAL, "%s: n = %lld rows, offs spans %lld", who, (long long)n,
             (long long)(offs[U] - offs[0]));
    scored->assign((size_t)U, 1);
    for (int64_t u = 0; u < U; u++) {
        if (std::isnan(vinv[u * F * F])) {
            (*scored)[(size_t)u] = 0;
            continue;
        }
        int64_t bad = 0;
        HS_CHECK(all_finite(mu + u * F, F, &bad), HMMSORT_EINVAL, "%s: mu: unit %lld, feature %lld is not finite", who,
                 (long long)u, (long long)bad);
        HS_CHECK(all_finite(vinv + u * F * F, F * F, &bad), HMMSORT_EINVAL, "%s: Vinv: unit %lld, entry (%lld, %lld) "
                 "is not finite", who, (long long)u, (long long)(bad / F), (long long)(bad % F));
    }
    HS_CHECK(n <= (1ll << 30) / U, HMMSORT_EUNSUP, "%s: %lld distances (U * n = %lld * %lld; at most 2^30)", who,
             (long long)(U * n), (long long)U, (long long)n);
    return HMMSORT_OK;
}

int dev_cluster_isolation(const double *d_feat, int64_t n, int64_t F, int64_t U, const int64_t *offs,
                          const unsigned char *d_used, const double *mu, const double *vinv,
                          const std::vector<unsigned char> &scored, const hmmsort_iso_out *out, hipStream_t st)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    auto fill_pairs = [&](const int64_t *closer, const double *lpair) {   // the entries no block writes
        for (int64_t u = 0; u < U; u++)
            for (int64_t v = 0; v < U; v++) {
                const bool both = scored[(size_t)u] && scored[(size_t)v];
                if (out->closer) out->closer[u * U + v] = u == v ? 0 : !both ? -1 : closer ? closer[u * U + v] : 0;
                if (out->lpair)
                    out->lpair[u * U + v] = u == v ? 0.0 : !scored[(size_t)u] ? nan : lpair ? lpair[u * U + v] : 0.0;
            }
    };
    if (n == 0) {
        if (out->iso_d2) std::fill(out->iso_d2, out->iso_d2 + U, nan);
        fill_pairs(nullptr, nullptr);
        HS_HIP(hipStreamSynchronize(st));
        return HMMSORT_OK;
    }
    // one table upload in 8-byte words: offsets from row 0, mu, Vinv (a not-scored unit's as zeros), the scored bytes
    const int64_t o_mu = U + 1, o_v = o_mu + U * F, o_sc = o_v + U * F * F, o_nu = o_sc + (U + 7) / 8;
    const int64_t o_own = o_nu + U, o_keys = o_own + n, o_sel = o_keys + U * n, o_hist = o_sel + 2 * U;
    const int64_t o_cl = o_hist + U * kSelBins, o_lp = o_cl + U * U, words = o_lp + U * U;
    std::vector<int64_t> tab((size_t)o_nu, 0);
    for (int64_t u = 0; u <= U; u++) tab[(size_t)u] = offs[u] - offs[0];
    double *hm = (double *)(tab.data() + o_mu), *hv = (double *)(tab.data() + o_v);
    for (int64_t u = 0; u < U; u++)
        if (scored[(size_t)u]) {
            std::copy(mu + u * F, mu + (u + 1) * F, hm + u * F);
            std::copy(vinv + u * F * F, vinv + (u + 1) * F * F, hv + u * F * F);
        }
    std::copy(scored.begin(), scored.end(), (unsigned char *)(tab.data() + o_sc));
    DevBuf ws;
    int rc;
    if ((rc = ws.alloc((size_t)words * sizeof(int64_t)))) return rc;
    int64_t *w = ws.as<int64_t>();
    HS_HIP(hipMemcpyAsync(w, tab.data(), (size_t)o_nu * sizeof(int64_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemsetAsync(w + o_hist, 0, (size_t)(words - o_hist) * sizeof(int64_t), st));   // histograms and pairs
    std::vector<int64_t> nu((size_t)U);
    IsoArgs A;
    A.feat = d_feat, A.used = d_used, A.offs = w;
    A.mu = (const double *)(w + o_mu), A.vinv = (const double *)(w + o_v);
    A.scored = (const unsigned char *)(w + o_sc);
    A.n = n, A.U = (int)U, A.F = (int)F;
    A.keys = (unsigned long long *)(w + o_keys), A.own = (unsigned long long *)(w + o_own);
    A.closer = w + o_cl, A.lpair = (double *)(w + o_lp);
    hipLaunchKernelGGL(k_iso_d2, dim3((unsigned)((n + kIsoRows - 1) / kIsoRows), (unsigned)U), dim3(kIsoRows),
                       (size_t)(kIsoRows * F) * sizeof(double), st, A);
    HS_HIP(hipGetLastError());
    if (out->closer || out->lpair) {
        hipLaunchKernelGGL(k_iso_pairs, dim3((unsigned)U, (unsigned)U), dim3(kFtTile), 0, st, A);
        HS_HIP(hipGetLastError());
    }
    // the used members of every unit, for the ranks: the bytes come to the host (n of them)
    if (d_used) {
        std::vector<unsigned char> hu((size_t)n);
        HS_HIP(hipMemcpyAsync(hu.data(), d_used, (size_t)n, hipMemcpyDeviceToHost, st));
        HS_HIP(hipStreamSynchronize(st));
        for (int64_t u = 0; u < U; u++) {
            int64_t c = 0;
            for (int64_t r = offs[u] - offs[0]; r < offs[u + 1] - offs[0]; r++) c += hu[(size_t)r] ? 1 : 0;
            nu[(size_t)u] = c;
        }
    } else {
        for (int64_t u = 0; u < U; u++) nu[(size_t)u] = offs[u + 1] - offs[u];
    }
    int64_t total = 0;
    for (int64_t u = 0; u < U; u++) total += nu[(size_t)u];
    std::vector<RadixSel> sel((size_t)U);
    std::vector<unsigned char> ranked((size_t)U);
    for (int64_t u = 0; u < U; u++) {
        const int64_t n_u = nu[(size_t)u], n_o = total - n_u;
        ranked[(size_t)u] = scored[(size_t)u] && n_u >= 1 && n_o >= n_u;
        sel[(size_t)u].prefix = 0;
        sel[(size_t)u].rank = ranked[(size_t)u] ? n_u - 1 : 0;
    }
    if (out->iso_d2) {
        RadixSel *d_sel = (RadixSel *)(w + o_sel);
        HS_HIP(hipMemcpyAsync(d_sel, sel.data(), (size_t)U * sizeof(RadixSel), hipMemcpyHostToDevice, st));
        const int blocks = (int)std::min<int64_t>(64, (n + 4095) / 4096);
        if ((rc = dev_radix_select(nullptr, A.keys, n, n, (int)U, blocks, d_sel, (unsigned long long *)(w + o_hist),
                                   st)))
            return rc;
        HS_HIP(hipMemcpyAsync(sel.data(), d_sel, (size_t)U * sizeof(RadixSel), hipMemcpyDeviceToHost, st));
    }
    std::vector<int64_t> hc;
    std::vector<double> hl;
    if (out->closer) {
        hc.resize((size_t)(U * U));
        HS_HIP(hipMemcpyAsync(hc.data(), A.closer, (size_t)(U * U) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    if (out->lpair) {
        hl.resize((size_t)(U * U));
        HS_HIP(hipMemcpyAsync(hl.data(), A.lpair, (size_t)(U * U) * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    HS_HIP(hipStreamSynchronize(st));   // the workspace and the tables die with this frame
    if (out->iso_d2)
        for (int64_t u = 0; u < U; u++) {
            double v = nan;
            if (ranked[(size_t)u]) std::memcpy(&v, &sel[(size_t)u].prefix, sizeof v);
            out->iso_d2[u] = v;
        }
    fill_pairs(out->closer ? hc.data() : nullptr, out->lpair ? hl.data() : nullptr);
    return HMMSORT_OK;
}

}  // namespace hmmsort
