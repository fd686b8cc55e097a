/* A C host of the per-spike fit: hmmsort_spike_fit with plain host pointers, and hmmsort_plan_spike_fit on device
 * buffers the host allocates itself through the HIP runtime's C entry points (no Python in the process).  Reads a
 * no-overlap model, a signal (float64, or int16 when the header says so), a path and a model track from a binary file
 * written by the test, and writes every output of both calls for the test to compare with the Python wrapper's.
 *   gcc -O2 -I include tests/c_host/quality_host.c -o quality_host -L hmmspikesorter.jl_amd -lhmmsort_hip \
 *       -L $ROCM/lib -lamdhip64 -Wl,-rpath,...
 *   ./quality_host in.bin out.bin */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hmmsort.h"

/* the three runtime calls the plan form needs, as hip_runtime_api.h declares them for C */
extern int hipMalloc(void **ptr, size_t size);
extern int hipMemcpy(void *dst, const void *src, size_t size, int kind /* 1 host to device */);
extern int hipFree(void *ptr);

#define CHECK(call)                                                                  \
    do {                                                                             \
        int rc_ = (call);                                                            \
        if (rc_ != 0) {                                                              \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, hmmsort_last_error());     \
            return 2;                                                                \
        }                                                                            \
    } while (0)

static int dump(FILE *f, const hmmsort_spike_fit_out *o, int64_t N, int64_t L)
{
    fwrite(o->counts, sizeof(int64_t), (size_t)N, f);
    fwrite(o->summary, sizeof(double), (size_t)(N * L), f);
    for (int64_t a = 0; a < N; a++) {
        const size_t n = (size_t)o->counts[a];
        fwrite(o->times + a * o->cap, sizeof(int64_t), n, f);
        fwrite(o->amp + a * o->cap, sizeof(double), n, f);
        fwrite(o->rss + a * o->cap, sizeof(double), n, f);
        fwrite(o->energy + a * o->cap, sizeof(double), n, f);
        fwrite(o->nused + a * o->cap, sizeof(int32_t), n, f);
    }
    return 0;
}

static int arrays(hmmsort_spike_fit_out *o, int64_t N, int64_t L, int64_t cap)
{
    const size_t n = (size_t)(N * (cap > 0 ? cap : 1));
    o->times = malloc(sizeof(int64_t) * n), o->amp = malloc(sizeof(double) * n), o->rss = malloc(sizeof(double) * n);
    o->energy = malloc(sizeof(double) * n), o->nused = malloc(sizeof(int32_t) * n), o->cap = cap;
    o->counts = malloc(sizeof(int64_t) * (size_t)N), o->summary = malloc(sizeof(double) * (size_t)(N * L));
    return o->times && o->amp && o->rss && o->energy && o->nused && o->counts && o->summary;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int64_t hdr[5]; /* N, K, T, 1 when the samples are int16, chunks of the track */
    double sigma;
    if (fread(hdr, sizeof(int64_t), 5, f) != 5 || fread(&sigma, sizeof(double), 1, f) != 1) return 1;
    const int64_t N = hdr[0], K = hdr[1], T = hdr[2], nch = hdr[4], L = 8 + 3 * (K - 1);
    const int raw = hdr[3] != 0;
    if (N < 1 || N > 32 || K < 2 || T < 1 || nch < 1) return 1;
    double *lp = malloc(sizeof(double) * (size_t)N), *mu = malloc(sizeof(double) * (size_t)(K * N));
    const size_t width = raw ? sizeof(int16_t) : sizeof(double);
    void *y = malloc(width * (size_t)T);
    int16_t *x = malloc(sizeof(int16_t) * (size_t)T);
    int64_t *first = malloc(sizeof(int64_t) * (size_t)nch);
    double *mut = malloc(sizeof(double) * (size_t)(nch * K * N));
    if (!lp || !mu || !y || !x || !first || !mut) return 1;
    if (fread(lp, sizeof(double), (size_t)N, f) != (size_t)N || fread(mu, sizeof(double), (size_t)(K * N), f) != (size_t)(K * N) ||
        fread(y, width, (size_t)T, f) != (size_t)T || fread(x, sizeof(int16_t), (size_t)T, f) != (size_t)T ||
        fread(first, sizeof(int64_t), (size_t)nch, f) != (size_t)nch ||
        fread(mut, sizeof(double), (size_t)(nch * K * N), f) != (size_t)(nch * K * N))
        return 1;
    fclose(f);

    /* the no-overlap model of these templates, from the library's own helpers */
    const int64_t S = hmmsort_generate_states(N, K, 0, NULL);
    if (S < 1) return 2;
    int16_t *states = malloc(sizeof(int16_t) * (size_t)(N * S));
    hmmsort_generate_states(N, K, 0, states);
    const int64_t R = hmmsort_build_transitions(N, K, lp, N, 0, NULL, 0);
    if (R < 1) return 2;
    hmm_trans *tr = malloc(sizeof(hmm_trans) * (size_t)R);
    hmmsort_build_transitions(N, K, lp, N, 0, tr, R);

    /* a missing counts array is refused before any GPU work */
    hmmsort_spike_fit_out none = {0};
    const int st = raw ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64;
    if (hmmsort_spike_fit(y, st, T, x, states, N, S, mu, K, 0, NULL, NULL, &none) != HMMSORT_EINVAL) return 3;

    /* host form under the track: counts first (cap = 0), then everything */
    hmmsort_spike_fit_out h0, h;
    if (!arrays(&h0, N, L, 0)) return 1;
    CHECK(hmmsort_spike_fit(y, st, T, x, states, N, S, mu, K, nch, first, mut, &h0));
    int64_t cap = 1;
    for (int64_t a = 0; a < N; a++)
        if (h0.counts[a] > cap) cap = h0.counts[a];
    if (!arrays(&h, N, L, cap)) return 1;
    CHECK(hmmsort_spike_fit(y, st, T, x, states, N, S, mu, K, nch, first, mut, &h));
    for (int64_t i = 0; i < N * L; i++) /* the summary does not depend on cap */
        if (h.summary[i] != h0.summary[i] && !(h.summary[i] != h.summary[i] && h0.summary[i] != h0.summary[i])) return 4;

    /* plan form without a track: the signal as float64 and the path go to the device by hand */
    double *yd = malloc(sizeof(double) * (size_t)T);
    for (int64_t i = 0; i < T; i++) yd[i] = raw ? (double)((const int16_t *)y)[i] : ((const double *)y)[i];
    void *d_y = NULL, *d_x = NULL;
    if (hipMalloc(&d_y, sizeof(double) * (size_t)T) != 0 || hipMalloc(&d_x, sizeof(int16_t) * (size_t)T) != 0) return 5;
    if (hipMemcpy(d_y, yd, sizeof(double) * (size_t)T, 1) != 0 || hipMemcpy(d_x, x, sizeof(int16_t) * (size_t)T, 1) != 0)
        return 5;
    hmmsort_plan *plan = NULL;
    CHECK(hmmsort_plan_create(&plan, T, states, N, K, S, tr, R, mu, sigma));
    hmmsort_spike_fit_out p;
    if (!arrays(&p, N, L, cap)) return 1;
    CHECK(hmmsort_plan_spike_fit(plan, d_y, d_x, 0, NULL, NULL, &p, NULL));
    CHECK(hmmsort_plan_destroy(plan));
    hipFree(d_y), hipFree(d_x);
    CHECK(hmmsort_shutdown());

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    dump(f, &h, N, L);
    dump(f, &p, N, L);
    fclose(f);
    printf("C host: %lld + %lld events under the track, %lld + %lld under the plan's model\n", (long long)h.counts[0],
           (long long)(N > 1 ? h.counts[1] : 0), (long long)p.counts[0], (long long)(N > 1 ? p.counts[1] : 0));
    return 0;
}
