/* A C host of the whitening stages: hmmsort_noise_cov and hmmsort_channel_mix with plain pointers only (no Python in
 * the process).  Reads a [C][T] float64 block, the noise options and a channel mix [R][M] from a binary file written
 * by the test, and writes sigma [C], n_quiet, s1 [C], s2 [C][C] and the mixed block [R][T], for the test to compare
 * with what the Python binding gets for the same input.
 *   gcc -O2 -I include tests/c_host/whiten_host.c -o whiten_host -L hmmspikesorter.jl_amd -lhmmsort_hip -Wl,-rpath,...
 *   ./whiten_host in.bin out.bin */
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
    int64_t hdr[5]; /* C, T, R, M, guard */
    double threshold;
    if (fread(hdr, sizeof(int64_t), 5, f) != 5 || fread(&threshold, sizeof(double), 1, f) != 1) return 1;
    const int64_t C = hdr[0], T = hdr[1], R = hdr[2], M = hdr[3], guard = hdr[4];
    if (C < 1 || T < 1 || R < 1 || M < 1) return 1;
    double *y = malloc(sizeof(double) * (size_t)(C * T)), *w = malloc(sizeof(double) * (size_t)(R * M));
    int32_t *nbr = malloc(sizeof(int32_t) * (size_t)(R * M));
    double *out = malloc(sizeof(double) * (size_t)(R * T));
    double *sigma = malloc(sizeof(double) * (size_t)C), *s1 = malloc(sizeof(double) * (size_t)C);
    double *s2 = malloc(sizeof(double) * (size_t)(C * C));
    if (!y || !w || !nbr || !out || !sigma || !s1 || !s2) return 1;
    if (fread(y, sizeof(double), (size_t)(C * T), f) != (size_t)(C * T)) return 1;
    if (fread(nbr, sizeof(int32_t), (size_t)(R * M), f) != (size_t)(R * M)) return 1;
    if (fread(w, sizeof(double), (size_t)(R * M), f) != (size_t)(R * M)) return 1;
    fclose(f);

    int64_t n_quiet = -1;
    hmmsort_noise_opt opt = {threshold, NULL, HMMSORT_WHITEN_MAX_GUARD + 1};
    hmmsort_noise_out res = {sigma, &n_quiet, s1, s2, NULL};
    /* a bad argument is refused before any GPU work, the outputs untouched */
    if (hmmsort_noise_cov(y, C, T, &opt, &res) != HMMSORT_EINVAL || n_quiet != -1) return 3;
    const int32_t saved = nbr[0];
    nbr[0] = (int32_t)C;
    if (hmmsort_channel_mix(y, C, T, R, M, nbr, w, out) != HMMSORT_EINVAL) return 3;
    nbr[0] = saved;

    opt.guard = guard;
    CHECK(hmmsort_noise_cov(y, C, T, &opt, &res));
    CHECK(hmmsort_channel_mix(y, C, T, R, M, nbr, w, out));
    CHECK(hmmsort_shutdown());

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(sigma, sizeof(double), (size_t)C, f);
    fwrite(&n_quiet, sizeof(int64_t), 1, f);
    fwrite(s1, sizeof(double), (size_t)C, f);
    fwrite(s2, sizeof(double), (size_t)(C * C), f);
    fwrite(out, sizeof(double), (size_t)(R * T), f);
    fclose(f);
    printf("C host: %lld channels x %lld samples, %lld quiet, mix %lld x %lld\n", (long long)C, (long long)T,
           (long long)n_quiet, (long long)R, (long long)M);
    return 0;
}
