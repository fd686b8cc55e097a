/* A C host of Viterbi training over channels: hmmsort_fit_step_channels with plain pointers only (no Python in the
 * process).  Reads a signal and a K x N template matrix from a binary file written by the test, builds the state
 * space with the library's host helpers, runs the recording as three channels on the device list {0, 0} -- once
 * with a re-estimated model per channel, once pooled -- and writes paths, log-likelihoods and the new models for
 * the test to compare with what the Python binding gets for the same inputs.
 *   gcc -O2 -I include tests/c_host/step_host.c -o step_host -L hmmspikesorter.jl_amd -lhmmsort_hip -Wl,-rpath,...
 *   ./step_host in.bin out.bin */
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

#define NCH 3

static void put_record(FILE *f, const hmmsort_step_out *o, int64_t KN)
{
    fwrite(o->mu, sizeof(double), (size_t)KN, f);
    fwrite(o->sigma, sizeof(double), 1, f);
    fwrite(o->n_lp, sizeof(int64_t), 1, f);
    fwrite(o->lp, sizeof(double), (size_t)*o->n_lp, f);
    fwrite(o->counts, sizeof(int64_t), 3, f);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 1;
    int64_t hdr[4]; /* N, K, T, chunksize */
    double sigma, lp_in[16];
    if (fread(hdr, sizeof(int64_t), 4, f) != 4 || fread(&sigma, sizeof(double), 1, f) != 1) return 1;
    const int64_t N = hdr[0], K = hdr[1], T = hdr[2], chunksize = hdr[3];
    if (N < 1 || N > 16 || fread(lp_in, sizeof(double), (size_t)N, f) != (size_t)N) return 1;
    double *mu = malloc(sizeof(double) * (size_t)(K * N)), *y = malloc(sizeof(double) * (size_t)T);
    if (fread(mu, sizeof(double), (size_t)(K * N), f) != (size_t)(K * N) || fread(y, sizeof(double), (size_t)T, f) != (size_t)T)
        return 1;
    fclose(f);

    const int64_t S = hmmsort_generate_states(N, K, 0, NULL);
    if (S < 0) { fprintf(stderr, "%s\n", hmmsort_last_error()); return 2; }
    int16_t *states = malloc(sizeof(int16_t) * (size_t)(N * S));
    hmmsort_generate_states(N, K, 0, states);
    const int64_t R = hmmsort_build_transitions(N, K, lp_in, N, 0, NULL, 0);
    if (R < 0) { fprintf(stderr, "%s\n", hmmsort_last_error()); return 2; }
    hmm_trans *tr = malloc(sizeof(hmm_trans) * (size_t)R);
    hmmsort_build_transitions(N, K, lp_in, N, 0, tr, R);

    const hmmsort_model model = {states, N, K, S, tr, R, mu, sigma};
    hmmsort_model models[NCH];
    const void *ys[NCH];
    int16_t *mls[NCH];
    double lls[NCH], sig[NCH + 1];
    int64_t nlp[NCH + 1], counts[NCH + 1][3];
    int status[NCH];
    hmmsort_step_out out[NCH + 1]; /* the last record takes the pooled step */
    const int devices[2] = {0, 0};
    for (int c = 0; c <= NCH; c++) {
        out[c].mu = malloc(sizeof(double) * (size_t)(K * N));
        out[c].sigma = &sig[c];
        out[c].lp = malloc(sizeof(double) * (size_t)R);
        out[c].lp_cap = R;
        out[c].n_lp = &nlp[c];
        out[c].pp = NULL;
        out[c].counts = counts[c];
    }
    for (int c = 0; c < NCH; c++) {
        models[c] = model;
        ys[c] = y;
        mls[c] = malloc(sizeof(int16_t) * (size_t)T);
    }
    CHECK(hmmsort_fit_step_channels(NCH, ys, HMMSORT_SAMPLES_F64, T, chunksize, models, devices, 2, 0, mls, lls, out, status));
    /* pooled, and no path asked for */
    double lls2[NCH];
    CHECK(hmmsort_fit_step_channels(NCH, ys, HMMSORT_SAMPLES_F64, T, chunksize, models, devices, 2, 1, NULL, lls2, &out[NCH], NULL));
    CHECK(hmmsort_shutdown());

    f = fopen(argv[2], "wb");
    if (!f) return 1;
    const int64_t nch = NCH;
    fwrite(&nch, sizeof(int64_t), 1, f);
    for (int c = 0; c < NCH; c++) {
        const int64_t st = status[c];
        fwrite(&st, sizeof(int64_t), 1, f);
        fwrite(&lls[c], sizeof(double), 1, f);
        fwrite(&lls2[c], sizeof(double), 1, f);
        fwrite(mls[c], sizeof(int16_t), (size_t)T, f);
        put_record(f, &out[c], K * N);
    }
    put_record(f, &out[NCH], K * N);
    fclose(f);
    printf("C host: hard step of %d channels of %lld samples in chunks of %lld, sigma' %.6f, pooled %.6f\n", NCH,
           (long long)T, (long long)chunksize, sig[0], sig[NCH]);
    return 0;
}
