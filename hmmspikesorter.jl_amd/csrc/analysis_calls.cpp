// Analysis entry points of libhmmsort_hip.so (include/hmmsort.h): what works on a recording, a decoded path or spike
// lists without the escalation ladder -- sample widening, the front end, whitening, reconstruct / unroll / extract,
// spike confidence, the per-spike fit, the template seed, correlograms, footprints, features, isolation and unit
// stability, each in its host, device and plan forms -- and the host staging they share.  Every call checks its
// arguments before it asks for a device, keeps no plan and no cached slot, and has no CPU compute path.
#include <algorithm>
#include <vector>

#include "hmmsort_internal.h"

using namespace hmmsort;

namespace {

// ---- shared host staging -------------------------------------------------------------------------------------------

int check_sample_type(const char *who, int sample_type)
{
    HS_CHECK(sample_type == HMMSORT_SAMPLES_F64 || sample_type == HMMSORT_SAMPLES_I16, HMMSORT_EINVAL,
             "%s: sample_type = %d: samples must be HMMSORT_SAMPLES_F64 or HMMSORT_SAMPLES_I16", who, sample_type);
    return HMMSORT_OK;
}

// n host samples (fp64 or int16, check_sample_type) into dy as fp64: int16 samples go up as they are and are widened
// on the device
int upload_samples_f64(const void *y, int sample_type, size_t n, DevBuf &dy)
{
    int rc;
    if ((rc = dy.alloc(n * sizeof(double)))) return rc;
    if (sample_type == HMMSORT_SAMPLES_I16) {
        DevBuf draw;
        if ((rc = draw.alloc(n * sizeof(int16_t)))) return rc;
        HS_HIP(hipMemcpy(draw.p, y, n * sizeof(int16_t), hipMemcpyHostToDevice));
        if ((rc = dev_widen(draw.p, sample_type, (int64_t)n, 1, dy.as<double>(), nullptr))) return rc;
        HS_HIP(hipDeviceSynchronize());   // draw dies with this frame
    } else {
        HS_HIP(hipMemcpy(dy.p, y, n * sizeof(double), hipMemcpyHostToDevice));
    }
    return HMMSORT_OK;
}

// U host spike lists: counts, null lists, every time in 1..2^40 and strictly ascending; offs[u] .. offs[u + 1] is where
// list u goes in the concatenation.  Needs no device and writes nothing but offs.
int check_unit_lists(const char *who, int64_t U, const int64_t *const *times, const int64_t *counts,
                     std::vector<int64_t> &offs)
{
    offs.assign((size_t)U + 1, 0);
    for (int64_t u = 0; u < U; u++) {
        HS_CHECK(counts[u] >= 0, HMMSORT_EINVAL, "%s: counts: unit %lld has a count of %lld", who, (long long)u,
                 (long long)counts[u]);
        HS_CHECK(counts[u] == 0 || times[u], HMMSORT_EINVAL, "%s: times: unit %lld has a null list of %lld times", who,
                 (long long)u, (long long)counts[u]);
        for (int64_t i = 0; i < counts[u]; i++) {
            const int64_t t = times[u][i];
            HS_CHECK(t >= 1 && t <= (1ll << 40), HMMSORT_EINVAL, "%s: times: unit %lld, position %lld: time %lld "
                     "outside 1..2^40", who, (long long)u, (long long)i, (long long)t);
            HS_CHECK(i == 0 || t > times[u][i - 1], HMMSORT_EINVAL, "%s: times: unit %lld, position %lld: time %lld "
                     "after %lld (a list must be strictly ascending)", who, (long long)u, (long long)i, (long long)t,
                     (long long)times[u][i - 1]);
        }
        offs[u + 1] = offs[u] + counts[u];
    }
    return HMMSORT_OK;
}

// the checked lists concatenated into dt
int upload_unit_lists(int64_t U, const int64_t *const *times, const int64_t *counts, const std::vector<int64_t> &offs,
                      DevBuf &dt)
{
    int rc;
    if ((rc = dt.alloc((size_t)offs[U] * sizeof(int64_t)))) return rc;
    for (int64_t u = 0; u < U; u++)
        if (counts[u] > 0)
            HS_HIP(hipMemcpy(dt.as<int64_t>() + offs[u], times[u], (size_t)counts[u] * sizeof(int64_t),
                             hipMemcpyHostToDevice));
    return HMMSORT_OK;
}

// a model track's chunk starts: 1-based, strictly ascending, at most kTrackChunks of them (nchunks >= 1)
int check_track(const char *who, int64_t nchunks, const int64_t *first)
{
    HS_CHECK(first[0] >= 1, HMMSORT_EINVAL, "%s: first[0] = %lld is no 1-based sample number", who,
             (long long)first[0]);
    for (int64_t c = 1; c < nchunks; c++)
        HS_CHECK(first[c] > first[c - 1], HMMSORT_EINVAL, "%s: chunk starts must ascend (first[%lld] = %lld after "
                 "%lld)", who, (long long)c, (long long)first[c], (long long)first[c - 1]);
    HS_CHECK(nchunks <= kTrackChunks, HMMSORT_EUNSUP, "%s: %lld chunks (at most %lld)", who, (long long)nchunks,
             (long long)kTrackChunks);
    return HMMSORT_OK;
}

// ---- events of a path in device memory -----------------------------------------------------------------------------

// extract_spiketimes on a path that already lives in device memory
int extract_from_device(const int16_t *d_x, int64_t T, const int16_t *states, int64_t N, int64_t S, const double *mu,
                        int64_t K, int64_t *times_out, int64_t cap, int64_t *counts_out, hipStream_t st,
                        DevBuf *dt_keep = nullptr, int64_t *dcap_all = nullptr)
{
    // dcap_all (with dt_keep): the device keeps EVERY event, rows of *dcap_all = max(1, largest count) entries,
    // whatever cap says; the host still receives the first min(count, cap) of each row (times_out may then be null)
    const bool all = dt_keep && dcap_all;
    // match table per state: the states in which a template is at its trough
    std::vector<uint32_t> match(S, 0u);
    for (int64_t i = 0; i < N; i++) {
        const int32_t qv = trough_value(mu, K, i);
        for (int64_t j = 0; j < S; j++)
            if (states[i + N * j] == qv) match[j] |= (1u << i);
    }
    const int64_t nb = (T + kSpikeChunkHost - 1) / kSpikeChunkHost;
    DevBuf dm, dcnt, doff, dt_own;
    DevBuf &dt = dt_keep ? *dt_keep : dt_own;   // compacted times [N][stride] stay on the device for the caller
    int rc;
    if ((rc = dm.alloc(S * sizeof(uint32_t))) || (rc = dcnt.alloc(nb * N * sizeof(int64_t))) ||
        (rc = doff.alloc(nb * N * sizeof(int64_t))))
        return rc;
    HS_HIP(hipMemcpyAsync(dm.p, match.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if ((rc = dev_spike_compact(d_x, T, dm.as<uint32_t>(), (int)N, (int)S, 0, dcnt.as<int64_t>(), nullptr,
                                nullptr, cap, st)))
        return rc;
    std::vector<int64_t> cnt(nb * N), off(nb * N);
    HS_HIP(hipMemcpyAsync(cnt.data(), dcnt.p, cnt.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; i < N; i++) {
        int64_t acc = 0;
        for (int64_t b = 0; b < nb; b++) { off[b * N + i] = acc; acc += cnt[b * N + i]; }
        counts_out[i] = acc;
    }
    int64_t stride = cap;   // of a device row
    if (all) {
        stride = 1;
        for (int64_t i = 0; i < N; i++) stride = std::max(stride, counts_out[i]);
        *dcap_all = stride;
    } else if (cap == 0) {
        return HMMSORT_OK;
    }
    if ((rc = dt.alloc((size_t)N * stride * sizeof(int64_t)))) return rc;
    HS_HIP(hipMemcpyAsync(doff.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if ((rc = dev_spike_compact(d_x, T, dm.as<uint32_t>(), (int)N, (int)S, 1, dcnt.as<int64_t>(),
                                doff.as<int64_t>(), dt.as<int64_t>(), stride, st)))
        return rc;
    for (int64_t i = 0; i < N && times_out; i++) {
        const int64_t n = std::min(counts_out[i], cap);
        if (n > 0)
            HS_HIP(hipMemcpyAsync(times_out + i * cap, dt.as<int64_t>() + i * stride, n * sizeof(int64_t),
                                  hipMemcpyDeviceToHost, st));
    }
    HS_HIP(hipStreamSynchronize(st));   // off and the compaction tables die with this frame
    return HMMSORT_OK;
}

// reconstruct_signal / unroll_mlseq on a path in device memory, results left in device memory
int plan_path_op(hmmsort_plan *p, const int16_t *d_x, double *d_y_out, int16_t *d_unrolled, hipStream_t st)
{
    const HostModel &m = p->model;
    DevBuf dst, dmu;
    int rc;
    if ((rc = dst.alloc(m.N * m.S * sizeof(int16_t))) || (rc = dmu.alloc(m.K * m.N * sizeof(double))))
        return rc;
    HS_HIP(hipMemcpyAsync(dst.p, m.states.data(), m.N * m.S * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemcpyAsync(dmu.p, m.mu.data(), m.K * m.N * sizeof(double), hipMemcpyHostToDevice, st));
    if (d_y_out)
        rc = dev_reconstruct(d_x, p->T, dst.as<int16_t>(), m.N, m.S, dmu.as<double>(), m.K, d_y_out, st);
    else
        rc = dev_unroll(d_x, p->T, dst.as<int16_t>(), m.N, m.S, d_unrolled, st);
    if (rc) return rc;
    HS_HIP(hipStreamSynchronize(st));  // the temporaries die with this frame
    return HMMSORT_OK;
}

// ---- per-spike fit (spike_fit.hip) ------------------------------------------------------------------

// what both entry points refuse before any GPU work; qv receives the N trough values of the base templates
int spike_fit_check(const char *who, int64_t N, int64_t S, const double *mu, int64_t K, int64_t nchunks,
                    const int64_t *first, const double *mu_track, const hmmsort_spike_fit_out *out, int32_t *qv)
{
    HS_CHECK(N >= 1 && N <= 32, HMMSORT_EINVAL, "%s: N = %lld templates (1..32)", who, (long long)N);
    HS_CHECK(K >= 2, HMMSORT_EINVAL, "%s: K = %lld (a template needs at least one phase besides the silent row)", who,
             (long long)K);
    HS_CHECK(S >= 1 && out->cap >= 0, HMMSORT_EINVAL, "%s: bad sizes (S = %lld, cap = %lld)", who, (long long)S,
             (long long)out->cap);
    HS_CHECK(nchunks >= 0, HMMSORT_EINVAL, "%s: nchunks = %lld", who, (long long)nchunks);
    // here a track that is too long is refused before its arrays are looked at
    HS_CHECK(nchunks <= kTrackChunks, HMMSORT_EUNSUP, "%s: %lld chunks (at most %lld)", who, (long long)nchunks,
             (long long)kTrackChunks);
    if (nchunks > 0) {
        HS_CHECK(first && mu_track, HMMSORT_EINVAL, "%s: a track needs first and mu_track", who);
        int rc = check_track(who, nchunks, first);
        if (rc) return rc;
    }
    for (int64_t a = 0; a < N; a++) {
        qv[a] = trough_value(mu, K, a);
        HS_CHECK(qv[a] != 1, HMMSORT_EINVAL, "%s: template %lld has its minimum in the silent row (trough value 1): "
                 "no state marks its spikes", who, (long long)a);
    }
    return HMMSORT_OK;
}

// the device side of one channel's fit: what dev_spike_fit reads and fills, rows of dcap entries per template
struct FitDev {
    DevBuf dst, dM, dfirst, damp, drss, den, dnu, dch, dpart, dsum;
};

// the fit of the compacted events d_t [N][dcap] (counts per template, at least one event in all), left in device memory
int spike_fit_rows(const double *d_y, const int16_t *d_x, int64_t T, const int16_t *states, int64_t N, int64_t S,
                   const double *mu, int64_t K, const int32_t *qv, int64_t nchunks, const int64_t *first,
                   const double *mu_track, const int64_t *d_t, int64_t dcap, const int64_t *counts, FitDev &f,
                   hipStream_t st)
{
    const int64_t L = spike_fit_len(K);
    int64_t maxn = 0;
    for (int64_t a = 0; a < N; a++) maxn = std::max(maxn, counts[a]);
    const int64_t nblk = spike_fit_blocks(maxn), nM = (nchunks > 0 ? nchunks : 1) * K * N;
    int rc;
    if ((rc = f.dst.alloc(N * S * sizeof(int16_t))) || (rc = f.dM.alloc(nM * sizeof(double))) ||
        (rc = f.dfirst.alloc(std::max<int64_t>(1, nchunks) * sizeof(int64_t))) ||
        (rc = f.damp.alloc(N * dcap * sizeof(double))) || (rc = f.drss.alloc(N * dcap * sizeof(double))) ||
        (rc = f.den.alloc(N * dcap * sizeof(double))) || (rc = f.dnu.alloc(N * dcap * sizeof(int32_t))) ||
        (rc = f.dch.alloc(N * dcap * sizeof(int32_t))) || (rc = f.dpart.alloc(N * nblk * L * sizeof(double))) ||
        (rc = f.dsum.alloc(N * L * sizeof(double))))
        return rc;
    HS_HIP(hipMemcpyAsync(f.dst.p, states, N * S * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemcpyAsync(f.dM.p, nchunks > 0 ? mu_track : mu, nM * sizeof(double), hipMemcpyHostToDevice, st));
    if (nchunks > 0)
        HS_HIP(hipMemcpyAsync(f.dfirst.p, first, nchunks * sizeof(int64_t), hipMemcpyHostToDevice, st));
    return dev_spike_fit(d_y, d_x, T, f.dst.as<int16_t>(), N, S, K, f.dM.as<double>(), nchunks, f.dfirst.as<int64_t>(),
                         d_t, dcap, counts, qv, f.damp.as<double>(), f.drss.as<double>(), f.den.as<double>(),
                         f.dnu.as<int32_t>(), f.dch.as<int32_t>(), f.dpart.as<double>(), f.dsum.as<double>(), st);
}

// one channel: resident signal and path in, host arrays out (rows of `cap` entries; any of them may be null)
int spike_fit_channel(const double *d_y, const int16_t *d_x, int64_t T, const int16_t *states, int64_t N, int64_t S,
                      const double *mu, int64_t K, const int32_t *qv, int64_t nchunks, const int64_t *first,
                      const double *mu_track, int64_t *times, double *amp, double *rss, double *energy, int32_t *nused,
                      int64_t cap, int64_t *counts, double *summary, hipStream_t st)
{
    const int64_t L = spike_fit_len(K);
    for (int64_t a = 0; a < N; a++) counts[a] = 0;
    if (summary) {
        std::fill(summary, summary + N * L, 0.0);
        for (int64_t a = 0; a < N; a++) {   // smm of the whole base template, k = 2..K ascending
            double s = 0.0;
            for (int64_t k = 1; k < K; k++) {
                const double q = mu[k + K * a] * mu[k + K * a];
                s += q;
            }
            summary[a * L + 7] = s;
        }
    }
    if (T == 0) return HMMSORT_OK;
    int rc = need_device();
    if (rc) return rc;
    DevBuf dt;
    int64_t dcap = 1;
    if ((rc = extract_from_device(d_x, T, states, N, S, mu, K, times, cap, counts, st, &dt, &dcap))) return rc;
    int64_t maxn = 0;
    for (int64_t a = 0; a < N; a++) maxn = std::max(maxn, counts[a]);
    if (maxn == 0) return HMMSORT_OK;
    FitDev f;
    if ((rc = spike_fit_rows(d_y, d_x, T, states, N, S, mu, K, qv, nchunks, first, mu_track, dt.as<int64_t>(), dcap,
                             counts, f, st)))
        return rc;
    for (int64_t a = 0; a < N; a++) {
        const size_t n = (size_t)std::min(counts[a], cap);
        if (n == 0) continue;
        if (amp) HS_HIP(hipMemcpyAsync(amp + a * cap, f.damp.as<double>() + a * dcap, n * 8, hipMemcpyDeviceToHost, st));
        if (rss) HS_HIP(hipMemcpyAsync(rss + a * cap, f.drss.as<double>() + a * dcap, n * 8, hipMemcpyDeviceToHost, st));
        if (energy)
            HS_HIP(hipMemcpyAsync(energy + a * cap, f.den.as<double>() + a * dcap, n * 8, hipMemcpyDeviceToHost, st));
        if (nused)
            HS_HIP(hipMemcpyAsync(nused + a * cap, f.dnu.as<int32_t>() + a * dcap, n * 4, hipMemcpyDeviceToHost, st));
    }
    std::vector<double> sum(summary ? N * L : 0);
    if (summary) HS_HIP(hipMemcpyAsync(sum.data(), f.dsum.p, N * L * sizeof(double), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; summary && i < N * L; i++)
        if (i % L != 7) summary[i] = sum[i];
    return HMMSORT_OK;
}

// ---- the units of a plan -------------------------------------------------------------------------------------------

// Every channel's events under the plan's current model, compacted on the device exactly as
// hmmsort_plan_extract_spiketimes finds them and concatenated into dt in unit order u = ch N + a behind the host
// offsets offs[0 .. U]; only the counts come to the host.  Shared by the calls that work on the units of a plan.  The
// copies into dt are enqueued on st and read `rows`, so the record must outlive the caller's next synchronisation.
// With the resident signal d_y, dv receives the amplitude of every event beside its time: hmmsort_plan_spike_fit's amp
// under the plan's current model (spike_fit_rows; the caller has run spike_fit_check on every channel).
struct PlanUnits {
    std::vector<DevBuf> rows;   // per channel: rows of dcap[ch] entries per template
    std::vector<FitDev> fits;   // per channel, with d_y
    DevBuf dt, dv;
    std::vector<int64_t> offs;
};

int plan_compact_units(hmmsort_plan *p, const int16_t *d_x, hipStream_t st, PlanUnits *pu, const double *d_y = nullptr)
{
    const int64_t N = p->model.N, nC = p->C, U = nC * N, T = p->T;
    int rc;
    std::vector<int64_t> dcap((size_t)nC, 1), &offs = pu->offs;
    pu->rows = std::vector<DevBuf>((size_t)nC);
    pu->fits = std::vector<FitDev>(d_y ? (size_t)nC : 0);
    offs.assign((size_t)U + 1, 0);
    for (int64_t ch = 0; ch < nC; ch++) {
        const HostModel &m = nC > 1 ? p->models[ch] : p->model;
        int64_t counts[32] = {0};
        if ((rc = extract_from_device(d_x + ch * T, T, m.states.data(), N, m.S, m.mu.data(), m.K, nullptr, 0, counts, st,
                                      &pu->rows[ch], &dcap[ch])))
            return rc;
        for (int64_t a = 0; a < N; a++) offs[ch * N + a + 1] = offs[ch * N + a] + counts[a];
        if (d_y && offs[ch * N + N] > offs[ch * N]) {
            int32_t qv[32];
            for (int64_t a = 0; a < N; a++) qv[a] = trough_value(m.mu.data(), m.K, a);
            if ((rc = spike_fit_rows(d_y + ch * T, d_x + ch * T, T, m.states.data(), N, m.S, m.mu.data(), m.K, qv, 0,
                                     nullptr, nullptr, pu->rows[ch].as<int64_t>(), dcap[ch], counts, pu->fits[ch], st)))
                return rc;
        }
    }
    if ((rc = pu->dt.alloc((size_t)offs[U] * sizeof(int64_t)))) return rc;
    if (d_y && (rc = pu->dv.alloc((size_t)offs[U] * sizeof(double)))) return rc;
    for (int64_t u = 0; u < U; u++) {
        const int64_t n = offs[u + 1] - offs[u], ch = u / N, a = u % N;
        if (n > 0)
            HS_HIP(hipMemcpyAsync(pu->dt.as<int64_t>() + offs[u], pu->rows[ch].as<int64_t>() + a * dcap[ch],
                                  (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
        if (n > 0 && d_y)
            HS_HIP(hipMemcpyAsync(pu->dv.as<double>() + offs[u], pu->fits[ch].damp.as<double>() + a * dcap[ch],
                                  (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    return HMMSORT_OK;
}

}  // namespace

extern "C" {

int hmmsort_samples_to_f64(const void *d_in, int sample_type, int64_t T, int64_t stride, double *d_out,
                           void *stream)
{
    HS_CHECK(T >= 0 && stride >= 1 && (T == 0 || (d_in && d_out)), HMMSORT_EINVAL,
             "samples_to_f64: bad argument (T = %lld, stride = %lld)", (long long)T, (long long)stride);
    int rc = need_device();
    if (rc) return rc;
    return dev_widen(d_in, sample_type, T, stride, d_out, (hipStream_t)stream);
}

// ---- front end (preprocess.hip) ------------------------------------------------------------------------------------

int hmmsort_preprocess_device(const void *d_in, int sample_type, int layout, int64_t C, int64_t T,
                              const hmmsort_pre_opt *opt, double *d_out, void *stream)
{
    PrePlan p;
    int rc = pre_resolve("preprocess_device", d_in, sample_type, layout, C, T, opt, d_out, false, &p);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return dev_preprocess(d_in, sample_type, layout, C, T, p, nullptr, d_out, (hipStream_t)stream);
}

int hmmsort_preprocess(const void *in, int sample_type, int layout, int64_t C, int64_t T, const hmmsort_pre_opt *opt,
                       double *out)
{
    PrePlan p;
    int rc = pre_resolve("preprocess", in, sample_type, layout, C, T, opt, out, true, &p);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    const size_t esize = sample_type == HMMSORT_SAMPLES_I16 ? 2 : (sample_type == HMMSORT_SAMPLES_F64 ? 8 : 4);
    // without a reference only the kept channels are filtered; with one every channel is, and the kept rows return
    const bool part = !p.keep.empty() && p.reference == HMMSORT_REF_NONE;
    const int64_t rows = part ? (int64_t)p.keep.size() : C;
    DevBuf din, dout;
    if ((rc = din.alloc((size_t)C * T * esize))) return rc;
    if ((rc = dout.alloc((size_t)rows * T * sizeof(double)))) return rc;
    HS_HIP(hipMemcpy(din.p, in, (size_t)C * T * esize, hipMemcpyHostToDevice));
    if ((rc = dev_preprocess(din.p, sample_type, layout, C, T, p, part ? &p.keep : nullptr, dout.as<double>(), nullptr)))
        return rc;
    if (p.keep.empty() || part) {
        HS_HIP(hipMemcpy(out, dout.p, (size_t)rows * T * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        for (size_t i = 0; i < p.keep.size(); i++)
            HS_HIP(hipMemcpy(out + i * T, dout.as<double>() + (int64_t)p.keep[i] * T, (size_t)T * sizeof(double),
                             hipMemcpyDeviceToHost));
    }
    return HMMSORT_OK;
}

// ---- spatial whitening (whiten.hip) --------------------------------------------------------------------------------

int hmmsort_noise_scale_device(const double *d_y, int64_t C, int64_t T, double *sigma, void *stream)
{
    int rc = wh_scale_check("noise_scale_device", d_y, C, T, sigma);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return dev_noise_scale(d_y, C, T, sigma, (hipStream_t)stream);
}

int hmmsort_noise_cov_device(const double *d_y, int64_t C, int64_t T, const hmmsort_noise_opt *opt,
                             hmmsort_noise_out *out, void *stream)
{
    NoiseParams p;
    int rc = wh_noise_check("noise_cov_device", d_y, C, T, opt, out, false, &p);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return dev_noise_cov(d_y, C, T, p, out, (hipStream_t)stream);
}

int hmmsort_noise_cov(const double *y, int64_t C, int64_t T, const hmmsort_noise_opt *opt, hmmsort_noise_out *out)
{
    NoiseParams p;
    int rc = wh_noise_check("noise_cov", y, C, T, opt, out, true, &p);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    DevBuf dy;
    if ((rc = dy.alloc((size_t)C * T * sizeof(double)))) return rc;
    HS_HIP(hipMemcpy(dy.p, y, (size_t)C * T * sizeof(double), hipMemcpyHostToDevice));
    return dev_noise_cov(dy.as<double>(), C, T, p, out, nullptr);
}

int hmmsort_channel_mix_device(const double *d_in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                               const double *w, double *d_out, void *stream)
{
    int rc = wh_mix_check("channel_mix_device", d_in, C, T, R, M, nbr, w, d_out);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return dev_channel_mix(d_in, C, T, R, M, nbr, w, d_out, (hipStream_t)stream);
}

int hmmsort_channel_mix(const double *in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                        const double *w, double *out)
{
    int rc = wh_mix_check("channel_mix", in, C, T, R, M, nbr, w, out);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    // one device buffer of max(C, R) rows, mixed in place when R == C
    DevBuf din, dout;
    if ((rc = din.alloc((size_t)C * T * sizeof(double)))) return rc;
    if (R != C && (rc = dout.alloc((size_t)R * T * sizeof(double)))) return rc;
    double *d_o = R != C ? dout.as<double>() : din.as<double>();
    HS_HIP(hipMemcpy(din.p, in, (size_t)C * T * sizeof(double), hipMemcpyHostToDevice));
    if ((rc = dev_channel_mix(din.as<double>(), C, T, R, M, nbr, w, d_o, nullptr))) return rc;
    HS_HIP(hipMemcpy(out, d_o, (size_t)R * T * sizeof(double), hipMemcpyDeviceToHost));
    return HMMSORT_OK;
}

// ---- reconstruct, unroll, extract ----------------------------------------------------------------------------------

int hmmsort_reconstruct(const int16_t *x, int64_t T, const int16_t *states, int64_t N, int64_t S,
                        const double *mu, int64_t K, double *y_out)
{
    HS_CHECK(states && mu && (T == 0 || (x && y_out)), HMMSORT_EINVAL, "reconstruct: null argument");
    HS_CHECK(T >= 0 && N >= 1 && S >= 1 && K >= 1, HMMSORT_EINVAL, "reconstruct: bad sizes");
    if (T == 0) return HMMSORT_OK;  // reference returns an empty vector
    int rc = need_device();
    if (rc) return rc;
    for (int64_t i = 0; i < T; i++)
        HS_CHECK(x[i] >= 1 && x[i] <= S, HMMSORT_EINVAL,
                 "reconstruct: x[%lld] = %d outside 1..S (reference would throw BoundsError)",
                 (long long)i, (int)x[i]);
    DevBuf dx, dst, dmu, dout;
    if ((rc = dx.alloc(T * sizeof(int16_t))) || (rc = dst.alloc(N * S * sizeof(int16_t))) ||
        (rc = dmu.alloc(K * N * sizeof(double))) || (rc = dout.alloc(T * sizeof(double))))
        return rc;
    HS_HIP(hipMemcpy(dx.p, x, T * sizeof(int16_t), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(dst.p, states, N * S * sizeof(int16_t), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(dmu.p, mu, K * N * sizeof(double), hipMemcpyHostToDevice));
    rc = dev_reconstruct(dx.as<int16_t>(), T, dst.as<int16_t>(), N, S, dmu.as<double>(), K,
                         dout.as<double>(), nullptr);
    if (rc) return rc;
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(y_out, dout.p, T * sizeof(double), hipMemcpyDeviceToHost));
    return HMMSORT_OK;
}

int hmmsort_reconstruct_tracked(const int16_t *x, int64_t T, const int16_t *states, int64_t N, int64_t S, int64_t K,
                                int64_t nchunks, const int64_t *first, const double *mu_track, double *y_out)
{
    HS_CHECK(states && first && mu_track && (T == 0 || (x && y_out)), HMMSORT_EINVAL,
             "reconstruct_tracked: null argument");
    HS_CHECK(T >= 0 && N >= 1 && S >= 1 && K >= 1 && nchunks >= 1, HMMSORT_EINVAL, "reconstruct_tracked: bad sizes");
    int rc = check_track("reconstruct_tracked", nchunks, first);
    if (rc) return rc;
    if (T == 0) return HMMSORT_OK;
    if ((rc = need_device())) return rc;
    // every phase the table names must be a row of the templates: the device code indexes with it
    for (int64_t i = 0; i < N * S; i++)
        HS_CHECK(states[i] >= 1 && states[i] <= K, HMMSORT_EINVAL, "reconstruct_tracked: states[%lld] = %d outside 1..K",
                 (long long)i, (int)states[i]);
    DevBuf dx, dst, dfirst, dmu, dout;
    if ((rc = dx.alloc(T * sizeof(int16_t))) || (rc = dst.alloc(N * S * sizeof(int16_t))) ||
        (rc = dfirst.alloc(nchunks * sizeof(int64_t))) || (rc = dmu.alloc(nchunks * K * N * sizeof(double))) ||
        (rc = dout.alloc(T * sizeof(double))))
        return rc;
    HS_HIP(hipMemcpy(dx.p, x, T * sizeof(int16_t), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(dst.p, states, N * S * sizeof(int16_t), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(dfirst.p, first, nchunks * sizeof(int64_t), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(dmu.p, mu_track, nchunks * K * N * sizeof(double), hipMemcpyHostToDevice));
    rc = dev_reconstruct_tracked(dx.as<int16_t>(), T, dst.as<int16_t>(), N, S, K, nchunks, dfirst.as<int64_t>(),
                                 dmu.as<double>(), dout.as<double>(), nullptr);
    if (rc) return rc;
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(y_out, dout.p, T * sizeof(double), hipMemcpyDeviceToHost));
    return HMMSORT_OK;
}

int hmmsort_unroll_mlseq(const int16_t *mlseq, int64_t T, const int16_t *states, int64_t N,
                         int64_t S, int16_t *out)
{
    HS_CHECK(states && (T == 0 || (mlseq && out)), HMMSORT_EINVAL, "unroll_mlseq: null argument");
    if (T == 0) return HMMSORT_OK;
    int rc = need_device();
    if (rc) return rc;
    for (int64_t i = 0; i < T; i++)
        HS_CHECK(mlseq[i] >= 1 && mlseq[i] <= S, HMMSORT_EINVAL,
                 "unroll_mlseq: mlseq[%lld] = %d outside 1..S", (long long)i, (int)mlseq[i]);
    DevBuf dx, dst, dout;
    if ((rc = dx.alloc(T * sizeof(int16_t))) || (rc = dst.alloc(N * S * sizeof(int16_t))) ||
        (rc = dout.alloc((size_t)N * T * sizeof(int16_t))))
        return rc;
    HS_HIP(hipMemcpy(dx.p, mlseq, T * sizeof(int16_t), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(dst.p, states, N * S * sizeof(int16_t), hipMemcpyHostToDevice));
    rc = dev_unroll(dx.as<int16_t>(), T, dst.as<int16_t>(), N, S, dout.as<int16_t>(), nullptr);
    if (rc) return rc;
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(out, dout.p, (size_t)N * T * sizeof(int16_t), hipMemcpyDeviceToHost));
    return HMMSORT_OK;
}

int hmmsort_extract_spiketimes(const int16_t *mlseq, int64_t T, const int16_t *states, int64_t N,
                               int64_t S, const double *mu, int64_t K, int64_t *times_out,
                               int64_t cap, int64_t *counts_out)
{
    HS_CHECK(states && mu && counts_out && (T == 0 || mlseq) && (cap == 0 || times_out), HMMSORT_EINVAL,
             "extract_spiketimes: null argument");
    HS_CHECK(N >= 1 && N <= 32 && S >= 1 && K >= 1 && T >= 0 && cap >= 0, HMMSORT_EINVAL,
             "extract_spiketimes: bad sizes");
    for (int64_t i = 0; i < N; i++) counts_out[i] = 0;
    if (T == 0) return HMMSORT_OK;
    int rc = need_device();
    if (rc) return rc;
    DevBuf dx;
    if ((rc = dx.alloc(T * sizeof(int16_t)))) return rc;
    HS_HIP(hipMemcpy(dx.p, mlseq, T * sizeof(int16_t), hipMemcpyHostToDevice));
    return extract_from_device(dx.as<int16_t>(), T, states, N, S, mu, K, times_out, cap, counts_out, nullptr);
}

int hmmsort_plan_reconstruct(hmmsort_plan *p, const int16_t *d_x, double *d_y_out, void *stream)
{
    HS_CHECK(p && d_x && d_y_out, HMMSORT_EINVAL, "plan_reconstruct: null argument");
    return plan_path_op(p, d_x, d_y_out, nullptr, (hipStream_t)stream);
}

int hmmsort_plan_unroll_mlseq(hmmsort_plan *p, const int16_t *d_x, int16_t *d_out, void *stream)
{
    HS_CHECK(p && d_x && d_out, HMMSORT_EINVAL, "plan_unroll_mlseq: null argument");
    return plan_path_op(p, d_x, nullptr, d_out, (hipStream_t)stream);
}

int hmmsort_plan_extract_spiketimes(hmmsort_plan *p, const int16_t *d_x, int64_t *times_out, int64_t cap,
                                    int64_t *counts_out, void *stream)
{
    HS_CHECK(p && d_x && counts_out && (cap == 0 || times_out) && cap >= 0, HMMSORT_EINVAL,
             "plan_extract_spiketimes: bad argument");
    const HostModel &m = p->model;
    HS_CHECK(m.N <= 32, HMMSORT_EINVAL, "plan_extract_spiketimes: more than 32 neurons");
    for (int64_t i = 0; i < m.N; i++) counts_out[i] = 0;
    return extract_from_device(d_x, p->T, m.states.data(), m.N, m.S, m.mu.data(), m.K, times_out, cap,
                               counts_out, (hipStream_t)stream);
}

// confidence of the decoded events from the plan's last posteriors (INTEGRATION.md "Posteriors")
int hmmsort_plan_spike_confidence(hmmsort_plan *p, const int16_t *d_x, int64_t jitter, int64_t *times_out,
                                  double *conf_out, int64_t cap, int64_t *counts_out, void *stream)
{
    HS_CHECK(p && d_x && counts_out && cap >= 0 && (cap == 0 || (times_out && conf_out)), HMMSORT_EINVAL,
             "plan_spike_confidence: bad argument");
    HS_CHECK(jitter >= 0, HMMSORT_EINVAL, "plan_spike_confidence: jitter must be >= 0 (got %lld)", (long long)jitter);
    HS_CHECK(p->eng->posteriors_valid(), HMMSORT_EINVAL, "plan_spike_confidence: call hmmsort_plan_posteriors first");
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = p->model.N, T = p->T;
    HS_CHECK(N <= 32, HMMSORT_EINVAL, "plan_spike_confidence: more than 32 neurons");
    for (int64_t ch = 0; ch < p->C; ch++) {
        const HostModel &m = p->C > 1 ? p->models[ch] : p->model;
        int64_t *cnt = counts_out + ch * N;
        for (int64_t i = 0; i < N; i++) cnt[i] = 0;
        DevBuf dt, dc;
        int rc = extract_from_device(d_x + ch * T, T, m.states.data(), N, m.S, m.mu.data(), m.K,
                                     times_out ? times_out + ch * N * cap : nullptr, cap, cnt, st, &dt);
        if (rc) return rc;
        if (cap == 0) continue;
        if ((rc = dc.alloc((size_t)N * cap * sizeof(double)))) return rc;
        for (int64_t i = 0; i < N; i++) {
            const int64_t n = std::min(cnt[i], cap);
            if (n == 0) continue;
            rc = p->eng->spike_conf((int)ch, (int)i, trough_value(m.mu.data(), m.K, i), jitter, dt.as<int64_t>() + i * cap,
                                    n, dc.as<double>() + i * cap, st);
            if (rc) return rc;
            HS_HIP(hipMemcpyAsync(conf_out + (ch * N + i) * cap, dc.as<double>() + i * cap, n * sizeof(double),
                                  hipMemcpyDeviceToHost, st));
        }
        HS_HIP(hipStreamSynchronize(st));
    }
    return HMMSORT_OK;
}

// ---- per-spike fit -------------------------------------------------------------------------------------------------

int hmmsort_spike_fit(const void *y, int sample_type, int64_t T, const int16_t *x, const int16_t *states, int64_t N,
                      int64_t S, const double *mu, int64_t K, int64_t nchunks, const int64_t *first,
                      const double *mu_track, hmmsort_spike_fit_out *out)
{
    HS_CHECK(states && mu && out && out->counts && (T == 0 || (y && x)), HMMSORT_EINVAL, "spike_fit: null argument");
    int32_t qv[32];
    int rc = check_sample_type("spike_fit", sample_type);
    if (rc) return rc;
    HS_CHECK(T >= 0, HMMSORT_EINVAL, "spike_fit: T = %lld", (long long)T);
    if ((rc = spike_fit_check("spike_fit", N, S, mu, K, nchunks, first, mu_track, out, qv))) return rc;
    // every phase the table names must be a row of the templates: the device code indexes with it
    for (int64_t i = 0; i < N * S; i++)
        HS_CHECK(states[i] >= 1 && states[i] <= K, HMMSORT_EINVAL, "spike_fit: states[%lld] = %d outside 1..K",
                 (long long)i, (int)states[i]);
    DevBuf dy, dx;
    if (T > 0) {
        if ((rc = need_device())) return rc;
        if ((rc = upload_samples_f64(y, sample_type, (size_t)T, dy)) || (rc = dx.alloc((size_t)T * sizeof(int16_t))))
            return rc;
        HS_HIP(hipMemcpy(dx.p, x, (size_t)T * sizeof(int16_t), hipMemcpyHostToDevice));
    }
    return spike_fit_channel(dy.as<double>(), dx.as<int16_t>(), T, states, N, S, mu, K, qv, nchunks, first, mu_track,
                             out->times, out->amp, out->rss, out->energy, out->nused, out->cap, out->counts,
                             out->summary, nullptr);
}

int hmmsort_plan_spike_fit(hmmsort_plan *p, const double *d_y, const int16_t *d_x, int64_t nchunks,
                           const int64_t *first, const double *mu_track, hmmsort_spike_fit_out *out, void *stream)
{
    HS_CHECK(p && d_y && d_x && out && out->counts, HMMSORT_EINVAL, "plan_spike_fit: null argument");
    HS_CHECK(p->C == 1 || nchunks == 0, HMMSORT_EINVAL, "plan_spike_fit: a batched plan takes no model track");
    const int64_t N = p->model.N, K = p->model.K, S = p->model.S, T = p->T, cap = out->cap, L = spike_fit_len(K);
    std::vector<int32_t> qv((size_t)p->C * 32);
    for (int64_t ch = 0; ch < p->C; ch++) {
        const HostModel &m = p->C > 1 ? p->models[ch] : p->model;
        int rc = spike_fit_check("plan_spike_fit", N, S, m.mu.data(), K, nchunks, first, mu_track, out, &qv[ch * 32]);
        if (rc) return rc;
    }
    for (int64_t ch = 0; ch < p->C; ch++) {
        const HostModel &m = p->C > 1 ? p->models[ch] : p->model;
        const int64_t o = ch * N * cap;
        int rc = spike_fit_channel(d_y + ch * T, d_x + ch * T, T, m.states.data(), N, S, m.mu.data(), K, &qv[ch * 32],
                                   nchunks, first, mu_track, out->times ? out->times + o : nullptr,
                                   out->amp ? out->amp + o : nullptr, out->rss ? out->rss + o : nullptr,
                                   out->energy ? out->energy + o : nullptr, out->nused ? out->nused + o : nullptr, cap,
                                   out->counts + ch * N, out->summary ? out->summary + ch * N * L : nullptr,
                                   (hipStream_t)stream);
        if (rc) return rc;
    }
    return HMMSORT_OK;
}

// ---- template seed (seed_templates.hip) ----------------------------------------------------------------------------

int hmmsort_seed_templates_device(const double *d_y, int64_t T, int64_t N, int64_t K, const hmmsort_seed_opt *opt,
                                  hmmsort_seed_out *out, void *stream)
{
    HS_CHECK(d_y, HMMSORT_EINVAL, "seed_templates_device: null signal");
    SeedParams p;
    int rc = seed_resolve(T, N, K, opt, out, &p);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    return dev_seed_templates(d_y, T, N, K, p, out, (hipStream_t)stream);
}

int hmmsort_seed_templates(const void *y, int sample_type, int64_t T, int64_t N, int64_t K,
                           const hmmsort_seed_opt *opt, hmmsort_seed_out *out)
{
    HS_CHECK(y, HMMSORT_EINVAL, "seed_templates: null signal");
    SeedParams p;
    int rc = check_sample_type("seed_templates", sample_type);
    if (rc) return rc;
    if ((rc = seed_resolve(T, N, K, opt, out, &p))) return rc;
    if ((rc = need_device())) return rc;
    DevBuf dy;
    if ((rc = upload_samples_f64(y, sample_type, (size_t)T, dy))) return rc;
    return dev_seed_templates(dy.as<double>(), T, N, K, p, out, nullptr);
}

// ---- correlograms (correlogram.hip) -----------------------------------------------------------------

int hmmsort_correlograms(int64_t U, const int64_t *const *times, const int64_t *counts, const hmmsort_ccg_opt *opt,
                         hmmsort_ccg_out *out)
{
    HS_CHECK(times && counts, HMMSORT_EINVAL, "correlograms: null argument (times and counts are required)");
    int rc = ccg_check("correlograms", U, opt, out);
    if (rc) return rc;
    std::vector<int64_t> offs;
    DevBuf dt;
    if ((rc = check_unit_lists("correlograms", U, times, counts, offs))) return rc;
    if ((rc = need_device())) return rc;
    if ((rc = upload_unit_lists(U, times, counts, offs, dt))) return rc;
    return dev_correlograms(U, dt.as<int64_t>(), offs.data(), opt, out, nullptr);
}

int hmmsort_plan_correlograms(hmmsort_plan *p, const int16_t *d_x, const hmmsort_ccg_opt *opt, hmmsort_ccg_out *out,
                              void *stream)
{
    HS_CHECK(p && d_x, HMMSORT_EINVAL, "plan_correlograms: null argument");
    const int64_t N = p->model.N, U = p->C * N;
    HS_CHECK(N <= 32, HMMSORT_EINVAL, "plan_correlograms: more than 32 templates");
    int rc = ccg_check("plan_correlograms", U, opt, out);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    PlanUnits pu;
    if ((rc = plan_compact_units(p, d_x, (hipStream_t)stream, &pu))) return rc;
    return dev_correlograms(U, pu.dt.as<int64_t>(), pu.offs.data(), opt, out, (hipStream_t)stream);
}

// ---- footprints (footprint.hip) ---------------------------------------------------------------------
// The device form takes the resident block and lists; the host form uploads the block once and the lists concatenated.

int hmmsort_footprints_device(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times,
                              const int64_t *offs, const hmmsort_fp_opt *opt, hmmsort_fp_out *out, void *stream)
{
    HS_CHECK(d_y && offs, HMMSORT_EINVAL, "footprints_device: null argument (d_y and offs are required)");
    int64_t M;
    int rc = fp_check("footprints_device", C, T, U, opt, out, &M);
    if (rc) return rc;
    HS_CHECK(offs[0] >= 0, HMMSORT_EINVAL, "footprints_device: offs[0] = %lld", (long long)offs[0]);
    for (int64_t u = 0; u < U; u++)
        HS_CHECK(offs[u + 1] >= offs[u], HMMSORT_EINVAL, "footprints_device: offs: unit %lld has a count of %lld",
                 (long long)u, (long long)(offs[u + 1] - offs[u]));
    HS_CHECK(d_times || offs[U] == offs[0], HMMSORT_EINVAL, "footprints_device: null d_times");
    if ((rc = need_device())) return rc;
    return dev_footprints(d_y, C, T, U, d_times, offs, opt, out, (hipStream_t)stream);
}

int hmmsort_footprints(const void *y, int sample_type, int64_t C, int64_t T, int64_t U, const int64_t *const *times,
                       const int64_t *counts, const hmmsort_fp_opt *opt, hmmsort_fp_out *out)
{
    HS_CHECK(y && times && counts, HMMSORT_EINVAL, "footprints: null argument (y, times and counts are required)");
    int64_t M;
    int rc = check_sample_type("footprints", sample_type);
    if (rc) return rc;
    if ((rc = fp_check("footprints", C, T, U, opt, out, &M))) return rc;
    std::vector<int64_t> offs;
    DevBuf dy, dt;
    if ((rc = check_unit_lists("footprints", U, times, counts, offs))) return rc;
    if ((rc = need_device())) return rc;
    if ((rc = upload_samples_f64(y, sample_type, (size_t)C * (size_t)T, dy))) return rc;
    if ((rc = upload_unit_lists(U, times, counts, offs, dt))) return rc;
    return dev_footprints(dy.as<double>(), C, T, U, dt.as<int64_t>(), offs.data(), opt, out, nullptr);
}

int hmmsort_plan_footprints(hmmsort_plan *p, const int16_t *d_x, const double *d_block, int64_t Cb,
                            const hmmsort_fp_opt *opt, hmmsort_fp_out *out, void *stream)
{
    HS_CHECK(p && d_x && d_block, HMMSORT_EINVAL, "plan_footprints: null argument (the plan, d_x and d_block are "
             "required)");
    const int64_t N = p->model.N, U = p->C * N;
    HS_CHECK(N <= 32, HMMSORT_EINVAL, "plan_footprints: more than 32 templates");
    int64_t M;
    int rc = fp_check("plan_footprints", Cb, p->T, U, opt, out, &M);
    if (rc) return rc;
    if ((rc = need_device())) return rc;
    PlanUnits pu;
    if ((rc = plan_compact_units(p, d_x, (hipStream_t)stream, &pu))) return rc;
    return dev_footprints(d_block, Cb, p->T, U, pu.dt.as<int64_t>(), pu.offs.data(), opt, out, (hipStream_t)stream);
}

// ---- features and isolation (features.hip) ----------------------------------------------------------
// The forms differ in where the block, the lists and the rows live; the rules are one (feat_check, iso_check).

int hmmsort_snippet_features_device(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times,
                                    const int64_t *offs, const hmmsort_feat_opt *opt, hmmsort_feat_out *out,
                                    void *stream)
{
    HS_CHECK(d_y && offs, HMMSORT_EINVAL, "snippet_features_device: null argument (d_y and offs are required)");
    FeatDims dm;
    int rc = feat_check("snippet_features_device", C, T, U, opt, out, &dm);
    if (rc) return rc;
    HS_CHECK(offs[0] >= 0, HMMSORT_EINVAL, "snippet_features_device: offs[0] = %lld", (long long)offs[0]);
    for (int64_t u = 0; u < U; u++)
        HS_CHECK(offs[u + 1] >= offs[u], HMMSORT_EINVAL, "snippet_features_device: offs: unit %lld has a count of "
                 "%lld", (long long)u, (long long)(offs[u + 1] - offs[u]));
    HS_CHECK(d_times || offs[U] == offs[0], HMMSORT_EINVAL, "snippet_features_device: null d_times");
    if ((rc = feat_check_rows("snippet_features_device", offs[U] - offs[0], dm.F))) return rc;
    if ((rc = need_device())) return rc;
    return dev_snippet_features(d_y, C, T, U, d_times, offs, opt, out, dm, out->feat, out->used, (hipStream_t)stream);
}

int hmmsort_snippet_features(const void *y, int sample_type, int64_t C, int64_t T, int64_t U,
                             const int64_t *const *times, const int64_t *counts, const hmmsort_feat_opt *opt,
                             hmmsort_feat_out *out)
{
    HS_CHECK(y && times && counts, HMMSORT_EINVAL, "snippet_features: null argument (y, times and counts are "
             "required)");
    FeatDims dm;
    int rc = check_sample_type("snippet_features", sample_type);
    if (rc) return rc;
    if ((rc = feat_check("snippet_features", C, T, U, opt, out, &dm))) return rc;
    std::vector<int64_t> offs;
    DevBuf dy, dt, df, du;
    if ((rc = check_unit_lists("snippet_features", U, times, counts, offs))) return rc;
    const int64_t n = offs[(size_t)U];
    if ((rc = feat_check_rows("snippet_features", n, dm.F))) return rc;
    if ((rc = need_device())) return rc;
    if ((rc = upload_samples_f64(y, sample_type, (size_t)C * (size_t)T, dy))) return rc;
    if ((rc = upload_unit_lists(U, times, counts, offs, dt))) return rc;
    if (out->feat && (rc = df.alloc((size_t)(n * dm.F) * sizeof(double)))) return rc;
    if (out->used && (rc = du.alloc((size_t)n))) return rc;
    if ((rc = dev_snippet_features(dy.as<double>(), C, T, U, dt.as<int64_t>(), offs.data(), opt, out, dm,
                                   df.as<double>(), du.as<unsigned char>(), nullptr)))
        return rc;
    if (out->feat && n > 0) HS_HIP(hipMemcpy(out->feat, df.p, (size_t)(n * dm.F) * sizeof(double), hipMemcpyDeviceToHost));
    if (out->used && n > 0) HS_HIP(hipMemcpy(out->used, du.p, (size_t)n, hipMemcpyDeviceToHost));
    return HMMSORT_OK;
}

int hmmsort_plan_snippet_features(hmmsort_plan *p, const int16_t *d_x, const double *d_block, int64_t Cb,
                                  const hmmsort_feat_opt *opt, hmmsort_feat_out *out, void *stream)
{
    HS_CHECK(p && d_x && d_block, HMMSORT_EINVAL, "plan_snippet_features: null argument (the plan, d_x and d_block "
             "are required)");
    const int64_t N = p->model.N, U = p->C * N;
    HS_CHECK(N <= 32, HMMSORT_EINVAL, "plan_snippet_features: more than 32 templates");
    FeatDims dm;
    int rc = feat_check("plan_snippet_features", Cb, p->T, U, opt, out, &dm);
    if (rc) return rc;
    HS_CHECK(!(out->feat || out->used) || out->cap_rows >= 0, HMMSORT_EINVAL, "plan_snippet_features: cap_rows = %lld",
             (long long)out->cap_rows);
    if ((rc = need_device())) return rc;
    PlanUnits pu;
    if ((rc = plan_compact_units(p, d_x, (hipStream_t)stream, &pu))) return rc;
    const int64_t n = pu.offs[(size_t)U];
    if ((rc = feat_check_rows("plan_snippet_features", n, dm.F))) {
        (void)hipStreamSynchronize((hipStream_t)stream);   // the compaction's copies read `pu`
        return rc;
    }
    const bool fits = out->cap_rows >= n;
    return dev_snippet_features(d_block, Cb, p->T, U, pu.dt.as<int64_t>(), pu.offs.data(), opt, out, dm,
                                fits ? out->feat : nullptr, fits ? out->used : nullptr, (hipStream_t)stream);
}

int hmmsort_cluster_isolation_device(const double *d_feat, int64_t n, int64_t F, int64_t U, const int64_t *offs,
                                     const unsigned char *d_used, const double *mu, const double *Vinv,
                                     hmmsort_iso_out *out, void *stream)
{
    std::vector<unsigned char> scored;
    int rc = iso_check("cluster_isolation_device", n, F, U, offs, mu, Vinv, out, &scored);
    if (rc) return rc;
    HS_CHECK(d_feat || n == 0, HMMSORT_EINVAL, "cluster_isolation_device: null d_feat");
    if ((rc = need_device())) return rc;
    return dev_cluster_isolation(d_feat, n, F, U, offs, d_used, mu, Vinv, scored, out, (hipStream_t)stream);
}

int hmmsort_cluster_isolation(const double *feat, int64_t n, int64_t F, int64_t U, const int64_t *offs,
                              const unsigned char *used, const double *mu, const double *Vinv, hmmsort_iso_out *out)
{
    std::vector<unsigned char> scored;
    int rc = iso_check("cluster_isolation", n, F, U, offs, mu, Vinv, out, &scored);
    if (rc) return rc;
    HS_CHECK(feat || n == 0, HMMSORT_EINVAL, "cluster_isolation: null feat");
    if ((rc = need_device())) return rc;
    DevBuf df, du;
    if ((rc = df.alloc((size_t)(n * F) * sizeof(double)))) return rc;
    if (n > 0) HS_HIP(hipMemcpy(df.p, feat, (size_t)(n * F) * sizeof(double), hipMemcpyHostToDevice));
    if (used) {
        if ((rc = du.alloc((size_t)n))) return rc;
        if (n > 0) HS_HIP(hipMemcpy(du.p, used, (size_t)n, hipMemcpyHostToDevice));
    }
    return dev_cluster_isolation(df.as<double>(), n, F, U, offs, used ? du.as<unsigned char>() : nullptr, mu, Vinv,
                                 scored, out, nullptr);
}

// ---- unit stability (stability.hip) -----------------------------------------------------------------

int hmmsort_unit_stability_device(int64_t U, const int64_t *d_times, const double *d_values, const int64_t *offs,
                                  const hmmsort_stab_opt *opt, hmmsort_stab_out *out, void *stream)
{
    HS_CHECK(offs, HMMSORT_EINVAL, "unit_stability_device: null argument (offs is required)");
    int64_t B;
    int rc = stab_check("unit_stability_device", U, opt, out, &B);
    if (rc) return rc;
    HS_CHECK(offs[0] >= 0, HMMSORT_EINVAL, "unit_stability_device: offs[0] = %lld", (long long)offs[0]);
    for (int64_t u = 0; u < U; u++)
        HS_CHECK(offs[u + 1] >= offs[u], HMMSORT_EINVAL, "unit_stability_device: offs: unit %lld has a count of %lld",
                 (long long)u, (long long)(offs[u + 1] - offs[u]));
    HS_CHECK(d_times || offs[U] == offs[0], HMMSORT_EINVAL, "unit_stability_device: null d_times");
    HS_CHECK(offs[U] - offs[0] < (1ll << 31), HMMSORT_EUNSUP, "unit_stability_device: %lld spikes in all (below 2^31)",
             (long long)(offs[U] - offs[0]));
    if ((rc = need_device())) return rc;
    return dev_unit_stability(U, d_times, d_values, offs, opt, out, B, (hipStream_t)stream);
}

int hmmsort_unit_stability(int64_t U, const int64_t *const *times, const double *const *values, const int64_t *counts,
                           const hmmsort_stab_opt *opt, hmmsort_stab_out *out)
{
    HS_CHECK(times && counts, HMMSORT_EINVAL, "unit_stability: null argument (times and counts are required)");
    int64_t B;
    int rc = stab_check("unit_stability", U, opt, out, &B);
    if (rc) return rc;
    std::vector<int64_t> offs;
    if ((rc = check_unit_lists("unit_stability", U, times, counts, offs))) return rc;
    for (int64_t u = 0; u < U; u++) {
        HS_CHECK(counts[u] == 0 || times[u][counts[u] - 1] <= opt->T, HMMSORT_EINVAL, "unit_stability: times: unit %lld: "
                 "time %lld outside 1..T = %lld", (long long)u, (long long)times[u][counts[u] - 1], (long long)opt->T);
        HS_CHECK(!values || counts[u] == 0 || values[u], HMMSORT_EINVAL, "unit_stability: values: unit %lld has a null "
                 "list of %lld values", (long long)u, (long long)counts[u]);
    }
    HS_CHECK(offs[(size_t)U] < (1ll << 31), HMMSORT_EUNSUP, "unit_stability: %lld spikes in all (below 2^31)",
             (long long)offs[(size_t)U]);
    if ((rc = need_device())) return rc;
    DevBuf dt, dv;
    if ((rc = upload_unit_lists(U, times, counts, offs, dt))) return rc;
    if (values) {
        if ((rc = dv.alloc((size_t)offs[(size_t)U] * sizeof(double)))) return rc;
        for (int64_t u = 0; u < U; u++)
            if (counts[u] > 0)
                HS_HIP(hipMemcpy(dv.as<double>() + offs[u], values[u], (size_t)counts[u] * sizeof(double),
                                 hipMemcpyHostToDevice));
    }
    return dev_unit_stability(U, dt.as<int64_t>(), values ? dv.as<double>() : nullptr, offs.data(), opt, out, B, nullptr);
}

int hmmsort_plan_unit_stability(hmmsort_plan *p, const double *d_y, const int16_t *d_x, const hmmsort_stab_opt *opt,
                                hmmsort_stab_out *out, void *stream)
{
    HS_CHECK(p && d_y && d_x, HMMSORT_EINVAL, "plan_unit_stability: null argument (the plan, d_y and d_x are required)");
    const int64_t N = p->model.N, U = p->C * N;
    HS_CHECK(N <= 32, HMMSORT_EINVAL, "plan_unit_stability: more than 32 templates");
    int64_t B;
    int rc = stab_check("plan_unit_stability", U, opt, out, &B);
    if (rc) return rc;
    HS_CHECK(opt->T == p->T, HMMSORT_EINVAL, "plan_unit_stability: T = %lld, the plan has %lld samples",
             (long long)opt->T, (long long)p->T);
    hmmsort_spike_fit_out none = {};
    int32_t qv[32];
    for (int64_t ch = 0; ch < p->C; ch++) {
        const HostModel &m = p->C > 1 ? p->models[ch] : p->model;
        if ((rc = spike_fit_check("plan_unit_stability", N, m.S, m.mu.data(), m.K, 0, nullptr, nullptr, &none, qv)))
            return rc;
    }
    if ((rc = need_device())) return rc;
    PlanUnits pu;
    if ((rc = plan_compact_units(p, d_x, (hipStream_t)stream, &pu, d_y))) {
        (void)hipStreamSynchronize((hipStream_t)stream);   // the compaction's copies read `pu`
        return rc;
    }
    return dev_unit_stability(U, pu.dt.as<int64_t>(), pu.dv.as<double>(), pu.offs.data(), opt, out, B,
                              (hipStream_t)stream);
}

}  // extern "C"
