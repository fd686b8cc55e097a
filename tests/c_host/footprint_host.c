/* A C host of the footprints: hmmsort_footprints with plain pointers only (no Python in the process).  Reads a fp64
 * channel-major block and U spike lists from a binary file written by the test, sums every unit on every channel and
 * writes sum, sumsq, nused and n one after the other, for the test to compare with the numpy model's bytes.
 *   gcc -O2 -I include tests/c_host/footprint_host.c -o footprint_host -L hmmspikesorter.jl_amd -lhmmsort_hip -Wl,-rpath,...
 *   ./footprint_host in.bin out.bin
 * in.bin: int64 C, T, U, pre, W; int64 counts[U]; the lists (int64, one after the other); double y[C][T]. */
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
    int64_t hdr[5]; /* C, T, U, pre, W */
    if (fread(hdr, sizeof(int64_t), 5, f) != 5) return 1;
    const int64_t C = hdr[0], T = hdr[1], U = hdr[2], pre = hdr[3], W = hdr[4];
    if (C < 1 || C > 64 || T < 1 || T > (1 << 24) || U < 1 || U > 64 || W < 1 || W > 1024) return 1;
    int64_t *counts = malloc(sizeof(int64_t) * (size_t)U);
    const int64_t **times = malloc(sizeof(int64_t *) * (size_t)U);
    if (!counts || !times) return 1;
    if (fread(counts, sizeof(int64_t), (size_t)U, f) != (size_t)U) return 1;
    int64_t total = 0;
    for (int64_t u = 0; u < U; u++) {
        if (counts[u] < 0 || counts[u] > (1 << 24)) return 1;
        total += counts[u];
    }
    int64_t *all = malloc(sizeof(int64_t) * (size_t)(total + 1));
    double *y = malloc(sizeof(double) * (size_t)(C * T));
    const size_t E = (size_t)(U * C * W);
    double *sum = malloc(sizeof(double) * E), *sumsq = malloc(sizeof(double) * E);
    int64_t *nused = malloc(sizeof(int64_t) * (size_t)U), *n = malloc(sizeof(int64_t) * (size_t)U);
    if (!all || !y || !sum || !sumsq || !nused || !n) return 1;
    if (fread(all, sizeof(int64_t), (size_t)total, f) != (size_t)total) return 1;
    if (fread(y, sizeof(double), (size_t)(C * T), f) != (size_t)(C * T)) return 1;
    fclose(f);
    for (int64_t u = 0, o = 0; u < U; o += counts[u], u++) times[u] = all + o;

    /* a bad argument is refused before any GPU work, and nothing is written */
    hmmsort_fp_opt opt = {pre, 0, 0, NULL};
    hmmsort_fp_out out = {sum, sumsq, nused, n};
    n[0] = -5;
    if (hmmsort_footprints(y, HMMSORT_SAMPLES_F64, C, T, U, times, counts, &opt, &out) != HMMSORT_EINVAL) return 3;
    if (n[0] != -5) return 3;

    opt.W = W;
    CHECK(hmmsort_footprints(y, HMMSORT_SAMPLES_F64, C, T, U, times, counts, &opt, &out));
    CHECK(hmmsort_shutdown());

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(sum, sizeof(double), E, f);
    fwrite(sumsq, sizeof(double), E, f);
    fwrite(nused, sizeof(int64_t), (size_t)U, f);
    fwrite(n, sizeof(int64_t), (size_t)U, f);
    fclose(f);
    printf("C host: %lld units on %lld channels x %lld samples, window %lld\n", (long long)U, (long long)C,
           (long long)T, (long long)W);
    return 0;
}
