/* A C host of the template seed: hmmsort_seed_templates with plain pointers only (no Python in the process).  Reads
 * a recording (float64, or int16 when the header says so) from a binary file written by the test, seeds N templates of
 * K states with the default options except the threshold, and writes every output for the test to compare with what
 * the Python binding gets for the same input.
 *   gcc -O2 -I include tests/c_host/seed_host.c -o seed_host -L hmmspikesorter.jl_amd -lhmmsort_hip -Wl,-rpath,...
 *   ./seed_host in.bin out.bin */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "hmmsort.h"

#define CHECK(call)                                                                  \
    do {                                                                             \
        int rc_ = (call);                                                            \
        if (rc_ != 0) {                                                              \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, hmmsort_last_error());     \
            return 2;                                                                \
        }                                                                            \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int64_t hdr[4]; /* N, K, T, 1 when the samples are int16 */
    double threshold;
    if (fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(&threshold, sizeof(double), 1, f) != 1) return 1;
    const int64_t N = hdr[0], K = hdr[1], T = hdr[2];
    const int raw = hdr[3] != 0;
    if (N < 1 || K < 2 || T < K) return 1;
    const size_t width = raw ? sizeof(int16_t) : sizeof(double);
    void *y = malloc(width * (size_t)T);
    if (!y || fread(y, width, (size_t)T, f) != (size_t)T) return 1;
    fclose(f);

    /* a bad argument is refused before any GPU work */
    hmmsort_seed_out none = {0};
    if (hmmsort_seed_templates(y, HMMSORT_SAMPLES_F64, T, N, K, NULL, &none) != HMMSORT_EINVAL) return 3;

    const int64_t cap = T / K + 1; /* refractory K - 1: events are at least K apart */
    double *mu = malloc(sizeof(double) * (size_t)(K * N)), *lp = malloc(sizeof(double) * (size_t)N), sigma = 0.0;
    int64_t *counts = malloc(sizeof(int64_t) * (size_t)N), *times = malloc(sizeof(int64_t) * (size_t)cap);
    int16_t *labels = malloc(sizeof(int16_t) * (size_t)cap);
    int64_t n_events = -1, iters = -1;
    const hmmsort_seed_opt opt = {threshold, 0.0, 0, -1, -1, 0}; /* everything else: the defaults */
    hmmsort_seed_out out = {mu, &sigma, lp, counts, &n_events, &iters, times, labels, cap};
    CHECK(hmmsort_seed_templates(y, raw ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, T, N, K, &opt, &out));
    /* the same with no options at all and none of the optional outputs, when the threshold is the default */
    if (threshold == 4.0) {
        double *mu2 = malloc(sizeof(double) * (size_t)(K * N)), sigma2 = 0.0;
        hmmsort_seed_out brief = {mu2, &sigma2, lp, counts, NULL, NULL, NULL, NULL, 0};
        CHECK(hmmsort_seed_templates(y, raw ? HMMSORT_SAMPLES_I16 : HMMSORT_SAMPLES_F64, T, N, K, NULL, &brief));
        for (int64_t i = 0; i < K * N; i++)
            if (mu2[i] != mu[i]) return 4;
        if (sigma2 != sigma) return 4;
    }
    CHECK(hmmsort_shutdown());
    if (n_events < 0 || n_events > cap) return 5;

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(&n_events, sizeof(int64_t), 1, f);
    fwrite(&iters, sizeof(int64_t), 1, f);
    fwrite(&sigma, sizeof(double), 1, f);
    fwrite(mu, sizeof(double), (size_t)(K * N), f);
    fwrite(lp, sizeof(double), (size_t)N, f);
    fwrite(counts, sizeof(int64_t), (size_t)N, f);
    fwrite(times, sizeof(int64_t), (size_t)n_events, f);
    fwrite(labels, sizeof(int16_t), (size_t)n_events, f);
    fclose(f);
    printf("C host: %lld events in %lld samples, %lld assignments, sigma %.6f\n", (long long)n_events, (long long)T,
           (long long)iters, sigma);
    return 0;
}
