/* A C host of the features and the isolation: hmmsort_snippet_features and hmmsort_cluster_isolation with plain
 * pointers only (no Python in the process).  Reads a fp64 channel-major block, U spike lists, a basis and a centre, and
 * the units' means and inverse covariances from a binary file written by the test; projects every spike, sums the
 * per-unit moments, scores the units and writes feat, used, nused, n, g1, g2, iso_d2 and closer one after the other,
 * for the test to compare with the numpy model's bytes.
 *   gcc -O2 -I include tests/c_host/isolation_host.c -o isolation_host -L hmmspikesorter.jl_amd -lhmmsort_hip -Wl,-rpath,...
 *   ./isolation_host in.bin out.bin
 * in.bin: int64 C, T, U, pre, W, P; int64 counts[U]; the lists (int64, one after the other); double y[C][T];
 * double basis[C][P][W]; double centre[C][W]; double mu[U][C P]; double Vinv[U][C P][C P]. */
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

static double *read_doubles(FILE *f, size_t n)
{
    double *p = malloc(sizeof(double) * (n + 1));
    if (!p || fread(p, sizeof(double), n, f) != n) return NULL;
    return p;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int64_t hdr[6]; /* C, T, U, pre, W, P */
    if (fread(hdr, sizeof(int64_t), 6, f) != 6) return 1;
    const int64_t C = hdr[0], T = hdr[1], U = hdr[2], pre = hdr[3], W = hdr[4], P = hdr[5];
    if (C < 1 || C > 64 || T < 1 || T > (1 << 24) || U < 1 || U > 64 || W < 1 || W > 1024 || P < 1 || P > W) return 1;
    const int64_t F = C * P;
    if (F > HMMSORT_FEAT_MAX_F2) return 1;
    int64_t *counts = malloc(sizeof(int64_t) * (size_t)U), *offs = malloc(sizeof(int64_t) * (size_t)(U + 1));
    const int64_t **times = malloc(sizeof(int64_t *) * (size_t)U);
    if (!counts || !times || !offs) return 1;
    if (fread(counts, sizeof(int64_t), (size_t)U, f) != (size_t)U) return 1;
    offs[0] = 0;
    for (int64_t u = 0; u < U; u++) {
        if (counts[u] < 0 || counts[u] > (1 << 24)) return 1;
        offs[u + 1] = offs[u] + counts[u];
    }
    const int64_t total = offs[U];
    int64_t *all = malloc(sizeof(int64_t) * (size_t)(total + 1));
    if (!all || fread(all, sizeof(int64_t), (size_t)total, f) != (size_t)total) return 1;
    double *y = read_doubles(f, (size_t)(C * T)), *basis = read_doubles(f, (size_t)(C * P * W));
    double *centre = read_doubles(f, (size_t)(C * W)), *mu = read_doubles(f, (size_t)(U * F));
    double *vinv = read_doubles(f, (size_t)(U * F * F));
    if (!y || !basis || !centre || !mu || !vinv) return 1;
    fclose(f);
    for (int64_t u = 0; u < U; u++) times[u] = all + offs[u];

    double *feat = malloc(sizeof(double) * (size_t)(total * F + 1));
    unsigned char *used = malloc((size_t)total + 1);
    int64_t *nused = malloc(sizeof(int64_t) * (size_t)U), *n = malloc(sizeof(int64_t) * (size_t)U);
    double *g1 = malloc(sizeof(double) * (size_t)(U * F)), *g2 = malloc(sizeof(double) * (size_t)(U * F * F));
    double *iso = malloc(sizeof(double) * (size_t)U);
    int64_t *closer = malloc(sizeof(int64_t) * (size_t)(U * U));
    if (!feat || !used || !nused || !n || !g1 || !g2 || !iso || !closer) return 1;

    /* a bad argument is refused before any GPU work, and nothing is written */
    hmmsort_feat_opt opt = {pre, W, 0, NULL, W + 1, basis, centre, 2};
    hmmsort_feat_out out = {feat, used, 0, n, nused, NULL, NULL, g1, g2};
    n[0] = -5;
    if (hmmsort_snippet_features(y, HMMSORT_SAMPLES_F64, C, T, U, times, counts, &opt, &out) != HMMSORT_EINVAL)
        return 3;
    if (n[0] != -5) return 3;

    opt.P = P;
    CHECK(hmmsort_snippet_features(y, HMMSORT_SAMPLES_F64, C, T, U, times, counts, &opt, &out));
    hmmsort_iso_out io = {iso, closer, NULL};
    CHECK(hmmsort_cluster_isolation(feat, total, F, U, offs, used, mu, vinv, &io));
    CHECK(hmmsort_shutdown());

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(feat, sizeof(double), (size_t)(total * F), f);
    fwrite(used, 1, (size_t)total, f);
    fwrite(nused, sizeof(int64_t), (size_t)U, f);
    fwrite(n, sizeof(int64_t), (size_t)U, f);
    fwrite(g1, sizeof(double), (size_t)(U * F), f);
    fwrite(g2, sizeof(double), (size_t)(U * F * F), f);
    fwrite(iso, sizeof(double), (size_t)U, f);
    fwrite(closer, sizeof(int64_t), (size_t)(U * U), f);
    fclose(f);
    printf("C host: %lld units, %lld rows of %lld features\n", (long long)U, (long long)total, (long long)F);
    return 0;
}
