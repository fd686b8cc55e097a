// Exact order statistics by a most-significant-digit radix select over 64-bit keys (hmmsort_internal.h, "radix
// select"; DESIGN "Template seed" stage 1).  Non-negative doubles order as their integer patterns, so the key of a
// sample is the 63-bit pattern of its magnitude (sel_key).  Several selects run side by side, one slot each; the
// per-workgroup LDS histograms are merged with integer atomics, whose sums do not depend on arrival order.  The
// template seed (noise scale and the N amplitude quantiles of its events) and the whitening's per-channel noise scale
// are its callers; sel_sigmas is the one place the rule "sigma = lower median / upper normal quartile" is applied.
#include <algorithm>
#include <cstring>

#include "hmmsort_internal.h"

namespace hmmsort {
namespace {

constexpr int kSelThreads = 256;
constexpr int kSelPasses = 6;       // 5 x 11 bits + 9 bits = 64
constexpr double kMadToSigma = 0.6744897501960817;   // upper quartile of the normal distribution

// One pass: the histogram of digit (key >> shift) & (2^bits - 1) over the keys of slot blockIdx.y whose higher bits
// equal the slot's prefix.  kFromY: key i is the pattern of |y[i]|, else keys[i].  The slot's n keys start `stride`
// elements after the previous slot's (0: every slot reads the same array).  grid = (blocks, slots).
template <bool kFromY>
__global__ __launch_bounds__(kSelThreads) void k_sel_hist(const double *__restrict__ y,
                                                          const unsigned long long *__restrict__ keys, int64_t stride,
                                                          int64_t n, int shift, int bits, int first,
                                                          const RadixSel *__restrict__ st,
                                                          unsigned long long *__restrict__ hist)
{
    __shared__ unsigned int s_h[kSelBins];
    const int slot = blockIdx.y;
    for (int i = threadIdx.x; i < kSelBins; i += kSelThreads) s_h[i] = 0;
    __syncthreads();
    const unsigned long long prefix = st[slot].prefix;
    const unsigned int mask = (1u << bits) - 1u;
    const int hs = first ? 0 : shift + bits;   // first pass: no higher bits (and no shift by 64)
    const int64_t step = (int64_t)gridDim.x * kSelThreads;
    const double *yrow = kFromY ? y + (int64_t)slot * stride : nullptr;
    const unsigned long long *krow = kFromY ? nullptr : keys + (int64_t)slot * stride;
    for (int64_t i = (int64_t)blockIdx.x * kSelThreads + threadIdx.x; i < n; i += step) {
        const unsigned long long k = kFromY ? sel_key(yrow[i]) : krow[i];
        if (first || (k >> hs) == (prefix >> hs)) atomicAdd(&s_h[(unsigned int)(k >> shift) & mask], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kSelBins; i += kSelThreads)
        if (s_h[i]) atomicAdd(&hist[(size_t)slot * kSelBins + i], (unsigned long long)s_h[i]);
}

// the digit that holds the slot's rank: prefix gets it, rank becomes the rank within it; the histogram is zeroed for
// the next pass.  One workgroup per slot.
__global__ __launch_bounds__(kSelThreads) void k_sel_pick(unsigned long long *__restrict__ hist,
                                                          RadixSel *__restrict__ st, int shift)
{
    constexpr int kPer = kSelBins / kSelThreads;
    __shared__ unsigned long long s_part[kSelThreads];
    unsigned long long *h = hist + (size_t)blockIdx.x * kSelBins;
    unsigned long long sum = 0;
    for (int q = 0; q < kPer; q++) sum += h[threadIdx.x * kPer + q];
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long r = (unsigned long long)st[blockIdx.x].rank;
        int g = 0;
        while (g < kSelThreads - 1 && r >= s_part[g]) r -= s_part[g++];
        int b = g * kPer;
        while (b < g * kPer + kPer - 1 && r >= h[b]) r -= h[b++];
        st[blockIdx.x].prefix |= (unsigned long long)b << shift;
        st[blockIdx.x].rank = (long long)r;
    }
    __syncthreads();
    for (int q = 0; q < kPer; q++) h[threadIdx.x * kPer + q] = 0;
}

}  // namespace

int dev_radix_select(const double *d_y, const unsigned long long *d_keys, int64_t stride, int64_t n, int slots,
                     int blocks, RadixSel *d_st, unsigned long long *d_hist, hipStream_t st)
{
    const dim3 grid(blocks, slots);
    for (int p = 0; p < kSelPasses; p++) {
        const int shift = std::max(0, 64 - 11 * (p + 1));
        const int bits = p + 1 < kSelPasses ? 11 : 64 - 11 * (kSelPasses - 1);
        if (d_keys)
            hipLaunchKernelGGL(k_sel_hist<false>, grid, dim3(kSelThreads), 0, st, d_y, d_keys, stride, n, shift, bits,
                               (int)(p == 0), d_st, d_hist);
        else
            hipLaunchKernelGGL(k_sel_hist<true>, grid, dim3(kSelThreads), 0, st, d_y, d_keys, stride, n, shift, bits,
                               (int)(p == 0), d_st, d_hist);
        hipLaunchKernelGGL(k_sel_pick, dim3(slots), dim3(kSelThreads), 0, st, d_hist, d_st, shift);
    }
    HS_HIP(hipGetLastError());
    return HMMSORT_OK;
}

void sel_sigmas(const RadixSel *sel, int64_t n, double *sigma)
{
    for (int64_t i = 0; i < n; i++) {
        double m;
        std::memcpy(&m, &sel[i].prefix, sizeof m);
        sigma[i] = m / kMadToSigma;
    }
}

}  // namespace hmmsort
