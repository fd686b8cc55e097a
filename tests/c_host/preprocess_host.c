/* A C host of the front end: hmmsort_preprocess with plain pointers only (no Python in the process).  Reads a raw
 * int16 sample-major block and half a filter from a binary file written by the test, filters every channel, subtracts
 * the median reference of all channels and writes the [C][T] result, then channel 1 alone through `keep`, for the test
 * to compare with what the Python binding gets for the same input.
 *   gcc -O2 -I include tests/c_host/preprocess_host.c -o preprocess_host -L hmmspikesorter.jl_amd -lhmmsort_hip -Wl,-rpath,...
 *   ./preprocess_host in.bin out.bin */
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
    int64_t hdr[3]; /* C, T, P */
    if (fread(hdr, sizeof(int64_t), 3, f) != 3) return 1;
    const int64_t C = hdr[0], T = hdr[1], P = hdr[2];
    if (C < 2 || T < P + 1 || P < 0) return 1;
    double *taps = malloc(sizeof(double) * (size_t)(P + 1));
    int16_t *raw = malloc(sizeof(int16_t) * (size_t)(C * T));
    double *out = malloc(sizeof(double) * (size_t)(C * T)), *row = malloc(sizeof(double) * (size_t)T);
    if (!taps || !raw || !out || !row) return 1;
    if (fread(taps, sizeof(double), (size_t)(P + 1), f) != (size_t)(P + 1)) return 1;
    if (fread(raw, sizeof(int16_t), (size_t)(C * T), f) != (size_t)(C * T)) return 1;
    fclose(f);

    /* a bad argument is refused before any GPU work */
    hmmsort_pre_opt opt = {taps, P, 7, NULL, NULL, 0};
    if (hmmsort_preprocess(raw, HMMSORT_SAMPLES_I16, HMMSORT_LAYOUT_SAMPLE_MAJOR, C, T, &opt, out) != HMMSORT_EINVAL)
        return 3;

    opt.reference = HMMSORT_REF_MEDIAN;
    CHECK(hmmsort_preprocess(raw, HMMSORT_SAMPLES_I16, HMMSORT_LAYOUT_SAMPLE_MAJOR, C, T, &opt, out));
    const int32_t keep[1] = {1};
    opt.keep = keep;
    opt.nkeep = 1;
    CHECK(hmmsort_preprocess(raw, HMMSORT_SAMPLES_I16, HMMSORT_LAYOUT_SAMPLE_MAJOR, C, T, &opt, row));
    for (int64_t t = 0; t < T; t++)
        if (row[t] != out[T + t]) return 4;
    CHECK(hmmsort_shutdown());

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(out, sizeof(double), (size_t)(C * T), f);
    fclose(f);
    printf("C host: %lld channels x %lld samples, %lld taps\n", (long long)C, (long long)T, (long long)(2 * P + 1));
    return 0;
}
