// Argument blocks and wave reductions shared by the block kernels of the time-parallel E-step: the LDS-column
// kernels of generic_estep.hip and the device-memory-column kernels of generic_estep_big.hip.
#pragma once
#include <algorithm>

#include "generic_dev.h"
#include "hmmsort_internal.h"

namespace hmmsort {

namespace {

struct BesArgs {
    const double *y;
    int64_t T;
    int S, B, H, nblk, nsrc1;
    const double *mean;
    const int32_t *in_ptr, *in_src;
    const double *in_w;
    const int32_t *out_ptr, *out_dst;
    const double *out_w;
    double rden;
    double *win;    // [gridDim.x][B][S] scaled alpha of the owned samples
    double *rec;    // [nblk][6][S]  0 alpha warm (lo-1)  1 alpha exact (hi-1)  2 gamma (hi-1)
                    //               3 beta warm (hi)     4 beta exact (lo)     5 gamma (lo)
    double *partG;  // [nblk][2 S]
    double *partX;  // [nblk][nsrc1 + 2]: X_i | Gamma0 | sum y^2
};

// Outputs of the posterior instantiation (bes_block_post): the per-sample marginals of hmmsort_plan_posteriors
// instead of the block statistics.  Reduction slots of a step: [0..2] as below, then 3 per template (onset,
// occupancy, trough), the silent state's gamma, the arg-max value and its state.
constexpr int kPostMaxN = 4;   // templates the posterior instantiations hold partial sums for
struct BesPost {
    const int16_t *states;   // [S][N] phases, 1 = silent
    int qv[kPostMaxN];       // trough phase of each template
    int N, nred;             // nred = 3 + 3 N + 3
    double *onset, *occ, *tq, *silent;   // [N][T] x 3, [T]; occ and silent may be null
    int16_t *xm;             // [T]
    double *lls;             // [gridDim.x][B] column sums of the owned samples (forward sweep)
    double *partL;           // [nblk] sum over the owned samples of log(column sum) + emission shift
};

__device__ __forceinline__ double wsum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wmax(double v)
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// red[par][slot][wave]: slot 0 column sum, 1 emission exponent maximum of the NEXT column, 2 gamma normaliser
constexpr int kRedW = 16;

template <typename Tv>
int balloc(Tv **p, size_t n, int64_t *bytes)
{
    if (*p) return HMMSORT_OK;
    if (hipMalloc((void **)p, std::max<size_t>(n, 1) * sizeof(Tv)) != hipSuccess) {
        (void)hipGetLastError();
        set_error("blocked E-step: hipMalloc of %.2f GB failed", (double)n * sizeof(Tv) / 1e9);
        return HMMSORT_ENOMEM;
    }
    *bytes += (int64_t)(n * sizeof(Tv));
    return HMMSORT_OK;
}

// the kernel arguments that follow from the plan alone
inline void bes_fill_args(BesArgs &a, const GenericDev *g, const double *d_y)
{
    a.y = d_y; a.T = g->T; a.S = (int)g->S; a.B = (int)g->B; a.H = (int)g->H; a.nblk = (int)g->nblk;
    a.nsrc1 = g->nsrc1; a.mean = g->d_mean;
    a.in_ptr = g->d_in_ptr; a.in_src = g->d_in_src; a.in_w = g->d_es_inw;
    a.out_ptr = g->d_out_ptr; a.out_dst = g->d_out_dst; a.out_w = g->d_es_outw;
    a.rden = 1.0 / (2.0 * (g->sigma * g->sigma));
    a.win = g->d_es_win; a.rec = g->d_es_rec; a.partG = g->d_es_partG; a.partX = g->d_es_partX;
}

}  // namespace

}  // namespace hmmsort
