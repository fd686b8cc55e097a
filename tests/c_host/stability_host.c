/* A C host of the unit stability: hmmsort_unit_stability with plain pointers only (no Python in the process).  Reads U
 * spike lists and their values from a binary file written by the test and writes every table one after the other, for
 * the test to compare with the numpy model's bytes.
 *   gcc -O2 -I include tests/c_host/stability_host.c -o stability_host -L hmmspikesorter.jl_amd -lhmmsort_hip -Wl,-rpath,...
 *   ./stability_host in.bin out.bin
 * in.bin: int64 U, T, bin, nq, q_den, HB; int64 q_num[8]; double hist_lo, hist_scale; int64 counts[U]; the lists
 * (int64, one after the other); the values (double, one list after the other). */
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
    int64_t hdr[6]; /* U, T, bin, nq, q_den, HB */
    hmmsort_stab_opt opt;
    if (fread(hdr, sizeof(int64_t), 6, f) != 6) return 1;
    const int64_t U = hdr[0], nq = hdr[3], HB = hdr[5];
    opt.T = hdr[1], opt.bin = hdr[2], opt.nq = nq, opt.q_den = hdr[4], opt.HB = HB;
    if (fread(opt.q_num, sizeof(int64_t), 8, f) != 8 || fread(&opt.hist_lo, sizeof(double), 1, f) != 1 ||
        fread(&opt.hist_scale, sizeof(double), 1, f) != 1)
        return 1;
    if (U < 1 || U > 64 || opt.T < 1 || opt.bin < 1 || nq < 0 || nq > 8 || HB < 0 || HB > 4096) return 1;
    const int64_t B = (opt.T + opt.bin - 1) / opt.bin;
    if (B > 4096) return 1;
    int64_t *counts = malloc(sizeof(int64_t) * (size_t)U);
    const int64_t **times = malloc(sizeof(int64_t *) * (size_t)U);
    const double **values = malloc(sizeof(double *) * (size_t)U);
    if (!counts || !times || !values || fread(counts, sizeof(int64_t), (size_t)U, f) != (size_t)U) return 1;
    int64_t total = 0;
    for (int64_t u = 0; u < U; u++) {
        if (counts[u] < 0 || counts[u] > (1 << 24)) return 1;
        total += counts[u];
    }
    int64_t *all = malloc(sizeof(int64_t) * (size_t)(total + 1));
    double *vals = malloc(sizeof(double) * (size_t)(total + 1));
    if (!all || !vals || fread(all, sizeof(int64_t), (size_t)total, f) != (size_t)total ||
        fread(vals, sizeof(double), (size_t)total, f) != (size_t)total)
        return 1;
    fclose(f);
    for (int64_t u = 0, o = 0; u < U; o += counts[u++]) times[u] = all + o, values[u] = vals + o;

    const size_t nu = (size_t)U, ns = (size_t)(U * B);
    int64_t *n = malloc(8 * nu), *count = malloc(8 * ns), *valid = malloc(8 * ns), *uvalid = malloc(8 * nu);
    int64_t *hist = malloc(8 * (nu * (size_t)HB + 1)), *under = malloc(8 * nu), *over = malloc(8 * nu);
    double *quant = malloc(8 * (ns * (size_t)nq + 1)), *sum = malloc(8 * ns), *sumsq = malloc(8 * ns);
    double *uquant = malloc(8 * (nu * (size_t)nq + 1)), *umin = malloc(8 * nu), *umax = malloc(8 * nu);
    double *usum = malloc(8 * nu), *usumsq = malloc(8 * nu);
    if (!n || !count || !valid || !uvalid || !hist || !under || !over || !quant || !sum || !sumsq || !uquant || !umin ||
        !umax || !usum || !usumsq)
        return 1;
    hmmsort_stab_out out = {n, count, valid, quant, sum, sumsq, uvalid, uquant, umin, umax, usum, usumsq, hist, under,
                            over};

    /* a bad argument is refused before any GPU work, and nothing is written */
    const int64_t bin = opt.bin;
    opt.bin = 0, n[0] = -5;
    if (hmmsort_unit_stability(U, times, values, counts, &opt, &out) != HMMSORT_EINVAL || n[0] != -5) return 3;
    opt.bin = bin;

    CHECK(hmmsort_unit_stability(U, times, values, counts, &opt, &out));
    CHECK(hmmsort_shutdown());

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(n, 8, nu, f), fwrite(count, 8, ns, f), fwrite(valid, 8, ns, f), fwrite(quant, 8, ns * (size_t)nq, f);
    fwrite(sum, 8, ns, f), fwrite(sumsq, 8, ns, f), fwrite(uvalid, 8, nu, f), fwrite(uquant, 8, nu * (size_t)nq, f);
    fwrite(umin, 8, nu, f), fwrite(umax, 8, nu, f), fwrite(usum, 8, nu, f), fwrite(usumsq, 8, nu, f);
    fwrite(hist, 8, nu * (size_t)HB, f), fwrite(under, 8, nu, f), fwrite(over, 8, nu, f);
    fclose(f);
    printf("C host: %lld units, %lld spikes, %lld time bins\n", (long long)U, (long long)total, (long long)B);
    return 0;
}
