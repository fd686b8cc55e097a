// C ABI of libhmmsort_hip.so (see include/hmmsort.h): options, plan creation (the one place that chooses an
// engine) and the plan API, which is argument checks plus one call forwarded to the plan's Engine
// (hmmsort_internal.h).  The host-buffer entry points of the decode / fit ladder are in host_calls.cpp, the analysis
// entry points (front end, whitening, events of a path, seed, correlograms, footprints) in analysis_calls.cpp.  No CPU
// compute path exists here.
#include <algorithm>
#include <cstring>
#include <memory>

#include "hmmsort_internal.h"

using namespace hmmsort;

int hmmsort::need_device()
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1) {
        (void)hipGetLastError();
        set_error("no HIP device available (%s); libhmmsort_hip has no CPU fallback",
                  e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
        return HMMSORT_EHIP;
    }
    return HMMSORT_OK;
}

int hmmsort::plan_create_engine(hmmsort_plan **out, int64_t T, const int16_t *states, int64_t N, int64_t K,
                                int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                                int64_t engine_req, int64_t halo_req)
{
    HS_CHECK(out, HMMSORT_EINVAL, "plan_create: null output pointer");
    *out = nullptr;
    HS_CHECK(T >= 1, HMMSORT_EINVAL, "plan_create: T must be >= 1 (got %lld)", (long long)T);
    int rc = need_device();
    if (rc) return rc;
    const Options opt = options_get();
    std::unique_ptr<hmmsort_plan> p(new hmmsort_plan());
    p->T = T;
    rc = build_host_model(p->model, states, N, K, S, tr, R, mu, sigma);
    if (rc) return rc;
    std::string why;
    const bool wave_ok = wave_supported(p->model, T, &why);
    if (engine_req == HMMSORT_ENGINE_WAVE && !wave_ok) {
        set_error("wave engine unavailable for this model/signal: %s", why.c_str());
        return HMMSORT_EUNSUP;
    }
    const bool ring_ok = ring_supported(p->model, T, &why);
    if (engine_req == HMMSORT_ENGINE_RING && !ring_ok) {
        set_error("ring engine unavailable for this model/signal: %s", why.c_str());
        return HMMSORT_EUNSUP;
    }
    // the round-1 lane-per-chain engine is kept as a second implementation for cross-checks only: AUTO never
    // picks it (what the wave engine does not take goes to the blocked / strict engines, which take any list)
    const bool want_ring = engine_req == HMMSORT_ENGINE_RING;
    const int64_t halo = halo_req >= 0 ? halo_req : opt.halo;
    if ((engine_req == HMMSORT_ENGINE_AUTO || engine_req == HMMSORT_ENGINE_WAVE) && wave_ok) {
        p->models.assign(1, p->model);
        rc = wave_engine_create(&p->eng, p->models, T, opt.block, halo);
    } else if (want_ring && ring_ok) {
        rc = ring_engine_create(&p->eng, p->model, T, opt.block, halo);
    } else if (engine_req == HMMSORT_ENGINE_BLOCKED ||
               (engine_req == HMMSORT_ENGINE_AUTO && T >= blocked_min_samples())) {
        // overlap models and other lists the ring engine does not take: blocked sweep
        rc = generic_engine_create(&p->eng, p->model, T, true, opt.block, halo, opt.blocked_hbm_columns);
        // a list the blocked sweep does not take (in-degree > 256): op-for-op single sweep
        if (rc == HMMSORT_EUNSUP && engine_req == HMMSORT_ENGINE_AUTO) rc = generic_engine_create(&p->eng, p->model, T);
    } else {
        rc = generic_engine_create(&p->eng, p->model, T);
    }
    if (rc) return rc;
    *out = p.release();
    return HMMSORT_OK;
}

extern "C" {

const char *hmmsort_last_error(void) { return last_error(); }
int hmmsort_version(void) { return 110; /* 0.1.1: posteriors */ }

int hmmsort_device_count(int *count)
{
    HS_CHECK(count, HMMSORT_EINVAL, "device_count: null pointer");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *count = n;
    return HMMSORT_OK;
}

int hmmsort_set_device(int device)
{
    HS_HIP(hipSetDevice(device));
    return HMMSORT_OK;
}

int hmmsort_set_option(const char *key, int64_t value)
{
    HS_CHECK(key, HMMSORT_EINVAL, "set_option: null key");
    if (!strcmp(key, "engine")) {
        HS_CHECK(value >= 0 && value <= 4, HMMSORT_EINVAL, "set_option: engine must be 0..4");
        options_modify([&](Options &o) { o.engine = value; });
    } else if (!strcmp(key, "block")) {
        HS_CHECK(value >= 0, HMMSORT_EINVAL, "set_option: block must be >= 0");
        options_modify([&](Options &o) { o.block = value; });
    } else if (!strcmp(key, "halo")) {
        HS_CHECK(value >= 0, HMMSORT_EINVAL, "set_option: halo must be >= 0");
        options_modify([&](Options &o) { o.halo = value; });
    } else if (!strcmp(key, "escalate")) {
        options_modify([&](Options &o) { o.escalate = value != 0; });
    } else if (!strcmp(key, "strict_limit_mb")) {
        HS_CHECK(value >= 0, HMMSORT_EINVAL, "set_option: strict_limit_mb must be >= 0");
        options_modify([&](Options &o) { o.strict_limit_mb = value; });
    } else if (!strcmp(key, "blocked_hbm_columns")) {
        HS_CHECK(value >= 0 && value <= 2, HMMSORT_EINVAL, "set_option: blocked_hbm_columns must be 0..2");
        options_modify([&](Options &o) { o.blocked_hbm_columns = value; });
    } else if (!strcmp(key, "tie_scale")) {
        HS_CHECK(value >= 1, HMMSORT_EINVAL, "set_option: tie_scale must be >= 1");
        options_modify([&](Options &o) { o.tie_scale = value; });
    } else if (!strcmp(key, "tie_debug")) {
        HS_CHECK(value >= 0 && value <= 3, HMMSORT_EINVAL, "set_option: tie_debug must be 0..3");
        options_modify([&](Options &o) { o.tie_debug = value; });
    } else if (!strcmp(key, "cert_rounds")) {
        HS_CHECK(value >= 0 && value <= 1, HMMSORT_EINVAL, "set_option: cert_rounds must be 0 or 1");
        options_modify([&](Options &o) { o.cert_rounds = value; });
    } else if (!strcmp(key, "interior")) {
        HS_CHECK(value >= 0 && value <= 1, HMMSORT_EINVAL, "set_option: interior must be 0 or 1");
        options_modify([&](Options &o) { o.interior = value; });
    } else if (!strcmp(key, "backtrace")) {
        HS_CHECK(value >= 0 && value <= 2, HMMSORT_EINVAL, "set_option: backtrace must be 0..2");
        options_modify([&](Options &o) { o.backtrace = value; });
    } else if (!strcmp(key, "fit_streams")) {
        HS_CHECK(value >= 1 && value <= 16, HMMSORT_EINVAL, "set_option: fit_streams must be 1..16");
        options_modify([&](Options &o) { o.fit_streams = value; });
    } else if (!strcmp(key, "plan_cache")) {
        HS_CHECK(value >= 0 && value <= 64, HMMSORT_EINVAL, "set_option: plan_cache must be 0..64");
        options_modify([&](Options &o) { o.plan_cache = value; });
        host_slots_trim((size_t)value);
    } else {
        set_error("set_option: unknown key '%s'", key);
        return HMMSORT_EINVAL;
    }
    return HMMSORT_OK;
}

int hmmsort_get_option(const char *key, int64_t *value)
{
    HS_CHECK(key && value, HMMSORT_EINVAL, "get_option: null argument");
    const Options o = options_get();
    if (!strcmp(key, "engine")) *value = o.engine;
    else if (!strcmp(key, "block")) *value = o.block;
    else if (!strcmp(key, "halo")) *value = o.halo;
    else if (!strcmp(key, "escalate")) *value = o.escalate;
    else if (!strcmp(key, "plan_cache")) *value = o.plan_cache;
    else if (!strcmp(key, "strict_limit_mb")) *value = o.strict_limit_mb;
    else if (!strcmp(key, "blocked_hbm_columns")) *value = o.blocked_hbm_columns;
    else if (!strcmp(key, "tie_scale")) *value = o.tie_scale;
    else if (!strcmp(key, "tie_debug")) *value = o.tie_debug;
    else if (!strcmp(key, "cert_rounds")) *value = o.cert_rounds;
    else if (!strcmp(key, "interior")) *value = o.interior;
    else if (!strcmp(key, "backtrace")) *value = o.backtrace;
    else if (!strcmp(key, "fit_streams")) *value = o.fit_streams;
    else if (!strcmp(key, "last_escalations")) *value = last_escalations();
    else {
        set_error("get_option: unknown key '%s'", key);
        return HMMSORT_EINVAL;
    }
    return HMMSORT_OK;
}

// frees what the library keeps between calls: the idle plans and device buffers of the host-buffer
// entry points (plans the caller created stay the caller's to destroy)
int hmmsort_shutdown(void)
{
    host_slots_trim(0);
    return HMMSORT_OK;
}

// ---- plan API ------------------------------------------------------------------------------

int hmmsort_plan_create(hmmsort_plan **plan_out, int64_t T, const int16_t *states, int64_t N,
                        int64_t K, int64_t S, const hmm_trans *tr, int64_t R, const double *mu,
                        double sigma)
{
    return plan_create_engine(plan_out, T, states, N, K, S, tr, R, mu, sigma, options_get().engine);
}

// Batched plan: C recording channels of the same length and model SHAPE, each with its own transition
// values / templates / sigma (the reference sorts one channel per call with its own model,
// src/hmmsort.jl:79-83); one set of launches sweeps all channels (chains = channels x chains per channel).
int hmmsort_plan_create_batched(hmmsort_plan **plan_out, int64_t C, int64_t T, const int16_t *states,
                                int64_t N, int64_t K, int64_t S, const hmm_trans *tr, int64_t R,
                                const double *mu, const double *sigma)
{
    HS_CHECK(plan_out, HMMSORT_EINVAL, "plan_create_batched: null output pointer");
    *plan_out = nullptr;
    HS_CHECK(C >= 1 && C <= 4096 && T >= 1 && tr && mu && sigma, HMMSORT_EINVAL,
             "plan_create_batched: bad argument (C = %lld, T = %lld)", (long long)C, (long long)T);
    int rc = need_device();
    if (rc) return rc;
    std::unique_ptr<hmmsort_plan> p(new hmmsort_plan());
    p->T = T;
    p->C = C;
    p->models.resize(C);
    for (int64_t ch = 0; ch < C; ch++) {
        rc = build_host_model(p->models[ch], states, N, K, S, tr + ch * R, R, mu + ch * K * N, sigma[ch]);
        if (rc) return rc;
    }
    p->model = p->models[0];
    std::string why;
    if (!wave_supported(p->model, T, &why)) {
        set_error("plan_create_batched needs the wave engine: %s", why.c_str());
        return HMMSORT_EUNSUP;
    }
    const Options opt = options_get();
    rc = wave_engine_create(&p->eng, p->models, T, opt.block, opt.halo);
    if (rc) return rc;
    *plan_out = p.release();
    return HMMSORT_OK;
}

int64_t hmmsort_plan_channels(const hmmsort_plan *p) { return p ? p->C : 0; }

// new numbers for channel `channel` of a plan: the model is rebuilt on the plan's own state table
static int plan_set_model(const char *who, hmmsort_plan *p, int64_t channel, const hmm_trans *tr, int64_t R,
                          const double *mu, double sigma)
{
    HostModel m;
    std::vector<int16_t> st = p->model.states;
    int rc = build_host_model(m, st.data(), p->model.N, p->model.K, p->model.S, tr, R, mu, sigma);
    if (rc) return rc;
    HS_CHECK(!p->eng->ring_models_only() || m.ring.valid, HMMSORT_EUNSUP, "%s: new model is not a ring model", who);
    if ((rc = p->eng->set_model(channel, m))) return rc;
    if (!p->models.empty()) p->models[channel] = m;
    if (channel == 0) p->model = std::move(m);
    p->pu_stale = true;
    p->ps_stale = true;
    return HMMSORT_OK;
}

int hmmsort_plan_set_model_channel(hmmsort_plan *p, int64_t channel, const hmm_trans *tr, int64_t R,
                                   const double *mu, double sigma)
{
    HS_CHECK(p && tr && mu, HMMSORT_EINVAL, "plan_set_model_channel: null argument");
    HS_CHECK(p->eng->id == HMMSORT_ENGINE_WAVE, HMMSORT_EUNSUP, "plan_set_model_channel: needs a wave-engine plan");
    HS_CHECK(channel >= 0 && channel < p->C, HMMSORT_EINVAL, "plan_set_model_channel: channel %lld outside 0..%lld",
             (long long)channel, (long long)p->C - 1);
    return plan_set_model("plan_set_model_channel", p, channel, tr, R, mu, sigma);
}

int hmmsort_plan_set_model(hmmsort_plan *p, const hmm_trans *tr, int64_t R, const double *mu,
                           double sigma)
{
    HS_CHECK(p && tr && mu, HMMSORT_EINVAL, "plan_set_model: null argument");
    HS_CHECK(R == p->model.R || p->eng->ring_models_only(), HMMSORT_EINVAL,
             "plan_set_model: R changed (%lld -> %lld)", (long long)p->model.R, (long long)R);
    return plan_set_model("plan_set_model", p, 0, tr, R, mu, sigma);
}

int hmmsort_plan_destroy(hmmsort_plan *p)
{
    delete p;
    return HMMSORT_OK;
}

int hmmsort_plan_info(const hmmsort_plan *p, int64_t *engine, int64_t *block, int64_t *halo,
                      int64_t *nchains, int64_t *workspace_bytes)
{
    HS_CHECK(p, HMMSORT_EINVAL, "plan_info: null plan");
    int64_t b = 0, h = 0, n = 0;
    p->eng->geometry(&b, &h, &n);
    if (engine) *engine = p->eng->id;
    if (block) *block = b;
    if (halo) *halo = h;
    if (nchains) *nchains = n;
    if (workspace_bytes) *workspace_bytes = p->eng->workspace_bytes();
    return HMMSORT_OK;
}

int64_t hmmsort_plan_overlap_sweep(const hmmsort_plan *p) { return p ? p->eng->overlap_sweep() : 0; }

int hmmsort_plan_bind(hmmsort_plan *p, const double *d_y, void *stream)
{
    HS_CHECK(p && d_y, HMMSORT_EINVAL, "plan_bind: null argument");
    return p->eng->bind(d_y, (hipStream_t)stream);
}

int hmmsort_plan_unbind(hmmsort_plan *p)
{
    HS_CHECK(p, HMMSORT_EINVAL, "plan_unbind: null plan");
    p->eng->unbind();
    return HMMSORT_OK;
}

int hmmsort_plan_viterbi(hmmsort_plan *p, const double *d_y, int16_t *d_x, double *d_ll,
                         void *stream)
{
    HS_CHECK(p && d_y && d_x && d_ll, HMMSORT_EINVAL, "plan_viterbi: null argument");
    return p->eng->viterbi(d_y, d_x, d_ll, (hipStream_t)stream);
}

int hmmsort_plan_decode_estep(hmmsort_plan *p, const double *d_y, int16_t *d_x, double *d_ll,
                              double *d_stats, void *stream)
{
    HS_CHECK(p && d_y && d_x && d_ll && d_stats, HMMSORT_EINVAL, "plan_decode_estep: null argument");
    return p->eng->decode_estep(d_y, d_x, d_ll, d_stats, (hipStream_t)stream);
}

int hmmsort_plan_set_shard(hmmsort_plan *p, int64_t own_lo, int64_t own_hi, int first, int last)
{
    HS_CHECK(p, HMMSORT_EINVAL, "plan_set_shard: null plan");
    int rc = p->eng->set_shard(own_lo, own_hi, first != 0, last != 0);
    if (rc == HMMSORT_OK) p->sharded = !(own_lo == 0 && own_hi == p->T && first && last);
    return rc;
}

int64_t hmmsort_plan_stats_len(const hmmsort_plan *p) { return p ? p->eng->stats_len() : 0; }

// [mu K*N | sigma | lp_new | pp S] per channel: the wave and ring M-step kernels always write N entry
// log-probabilities (a template whose entry transitions were dropped from the list keeps its slot);
// the generic/blocked engines one per transition leaving state 1 except the first (baumwelch.jl:226,264)
int64_t hmmsort_plan_mstep_len(const hmmsort_plan *p)
{
    if (!p) return 0;
    const HostModel &m = p->model;
    return m.K * m.N + 1 + p->eng->n_lp() + m.S;
}

int hmmsort_plan_estep(hmmsort_plan *p, const double *d_y, double *d_stats, void *stream)
{
    HS_CHECK(p && d_y && d_stats, HMMSORT_EINVAL, "plan_estep: null argument");
    return p->eng->estep(d_y, d_stats, (hipStream_t)stream);
}

int hmmsort_plan_mstep(hmmsort_plan *p, const double *d_stats, double *d_out, void *stream)
{
    HS_CHECK(p && d_stats && d_out, HMMSORT_EINVAL, "plan_mstep: null argument");
    return p->eng->mstep(d_stats, d_out, (hipStream_t)stream);
}

int hmmsort_plan_path_update(hmmsort_plan *p, const double *d_y, const int16_t *d_x, double *d_out,
                             int64_t *d_counts, void *stream)
{
    HS_CHECK(p && d_y && d_x && d_out, HMMSORT_EINVAL, "plan_path_update: null argument");
    // sigma' needs the means of the whole recording: there is no additive statistics vector to all-reduce
    HS_CHECK(!p->sharded, HMMSORT_EINVAL, "plan_path_update: the plan is a time shard (hmmsort_plan_set_shard); the "
                                          "update needs the whole recording");
    return plan_path_update(p, d_y, d_x, d_out, d_counts, (hipStream_t)stream);
}

int64_t hmmsort_plan_path_stats_len(const hmmsort_plan *p) { return p ? plan_path_stats_len(p) : 0; }

int hmmsort_plan_path_stats(hmmsort_plan *p, const double *d_y, const int16_t *d_x, int64_t T, int64_t own_lo,
                            int64_t own_hi, int first, double *d_stats, void *stream)
{
    HS_CHECK(p && d_y && d_x && d_stats, HMMSORT_EINVAL, "plan_path_stats: null argument");
    HS_CHECK(p->C == 1 || T == p->T, HMMSORT_EINVAL, "plan_path_stats: a batched plan takes [C][T] arrays of its own "
             "T = %lld, not %lld", (long long)p->T, (long long)T);
    HS_CHECK(own_lo >= 0 && own_lo <= own_hi && own_hi <= T, HMMSORT_EINVAL,
             "plan_path_stats: range [%lld, %lld) outside [0, %lld]", (long long)own_lo, (long long)own_hi, (long long)T);
    return plan_path_stats(p, d_y, d_x, T, own_lo, own_hi, first != 0, d_stats, (hipStream_t)stream);
}

int hmmsort_plan_path_finish(hmmsort_plan *p, const double *d_stats, double *d_out, int64_t *d_counts, void *stream)
{
    HS_CHECK(p && d_stats && d_out, HMMSORT_EINVAL, "plan_path_finish: null argument");
    return plan_path_finish(p, d_stats, d_out, d_counts, (hipStream_t)stream);
}

int hmmsort_stats_sum(const double *d_parts, int64_t nparts, int64_t len, double *d_out, void *stream)
{
    HS_CHECK(d_parts && d_out && nparts >= 1 && len >= 1, HMMSORT_EINVAL, "stats_sum: null argument or nothing to add");
    HS_CHECK(len <= (int64_t)2147483647 * 256, HMMSORT_EUNSUP, "stats_sum: vector too long");
    int rc;
    if ((rc = need_device())) return rc;
    return dev_stats_sum(d_parts, nparts, len, d_out, (hipStream_t)stream);
}

int hmmsort_stats_blend(double *d_acc, double w, const double *d_new, int64_t len, int64_t plain_tail, void *stream)
{
    HS_CHECK(w >= 0.0 && w <= 1.0, HMMSORT_EINVAL, "stats_blend: weight %g outside [0, 1]", w);
    HS_CHECK(plain_tail >= 0 && len >= plain_tail, HMMSORT_EINVAL, "stats_blend: %lld entries, %lld of them unweighted",
             (long long)len, (long long)plain_tail);
    HS_CHECK(len == 0 || (d_acc && d_new), HMMSORT_EINVAL, "stats_blend: null argument");
    HS_CHECK(len <= (int64_t)2147483647 * 256, HMMSORT_EUNSUP, "stats_blend: vector too long");
    int rc;
    if ((rc = need_device())) return rc;
    return dev_stats_blend(d_acc, w, d_new, len, plain_tail, (hipStream_t)stream);
}

int hmmsort_plan_diagnostics(hmmsort_plan *p, void *stream, int64_t diag[8])
{
    HS_CHECK(p && diag, HMMSORT_EINVAL, "plan_diagnostics: null argument");
    for (int i = 0; i < 8; i++) diag[i] = 0;
    return p->eng->diagnostics((hipStream_t)stream, diag);
}

int hmmsort_plan_tie_stats(hmmsort_plan *p, void *stream, int64_t out[8])
{
    HS_CHECK(p && out, HMMSORT_EINVAL, "plan_tie_stats: null argument");
    for (int i = 0; i < 8; i++) out[i] = 0;
    return p->eng->tie_stats((hipStream_t)stream, out);
}

// debugging aids (not part of the documented ABI): raw debug record / an internal per-sample array of the wave engine
int hmmsort_plan_debug_record(hmmsort_plan *p, double *out64)
{
    HS_CHECK(p && out64, HMMSORT_EINVAL, "plan_debug_record: needs a wave plan");
    return p->eng->debug_record(out64);
}

int hmmsort_plan_debug_array(hmmsort_plan *p, int which, double *out, int64_t n)
{
    HS_CHECK(p && out, HMMSORT_EINVAL, "plan_debug_array: needs a wave plan");
    return p->eng->debug_array(which, out, n);
}

int hmmsort_plan_profile(hmmsort_plan *p, int enable)
{
    HS_CHECK(p, HMMSORT_EINVAL, "plan_profile: null plan");
    return p->eng->profile(enable);
}

int hmmsort_plan_profile_read(hmmsort_plan *p, void *stream, char *names, int64_t names_cap,
                              double *ms, int64_t *calls, int64_t cap, int64_t *n_out)
{
    HS_CHECK(p && names && ms && calls && n_out, HMMSORT_EINVAL, "plan_profile_read: null argument");
    *n_out = 0;
    if (names_cap > 0) names[0] = 0;
    std::vector<std::string> nm;
    std::vector<double> m;
    std::vector<int64_t> c;
    int rc = p->eng->profile_read((hipStream_t)stream, nm, m, c);
    if (rc) return rc;
    std::string joined;
    int64_t n = std::min<int64_t>((int64_t)nm.size(), cap);
    for (int64_t i = 0; i < n; i++) {
        if (i) joined += "\n";
        joined += nm[i];
        ms[i] = m[i];
        calls[i] = c[i];
    }
    HS_CHECK((int64_t)joined.size() + 1 <= names_cap, HMMSORT_EINVAL, "plan_profile_read: names buffer too small");
    memcpy(names, joined.c_str(), joined.size() + 1);
    *n_out = n;
    return HMMSORT_OK;
}

// ---- posteriors (INTEGRATION.md "Posteriors") -------------------------------------------------

int hmmsort_plan_posteriors(hmmsort_plan *p, const double *d_y, double *d_onset, double *d_occ, double *d_silent,
                            double *d_logz, void *stream)
{
    HS_CHECK(p && d_y, HMMSORT_EINVAL, "plan_posteriors: null argument");
    return p->eng->posteriors(p->model, d_y, d_onset, d_occ, d_silent, d_logz, (hipStream_t)stream);
}

int hmmsort_plan_posterior_decode(hmmsort_plan *p, int16_t *d_xm, void *stream)
{
    HS_CHECK(p && d_xm, HMMSORT_EINVAL, "plan_posterior_decode: null argument");
    return p->eng->posterior_decode(d_xm, (hipStream_t)stream);
}

int hmmsort_plan_expected_counts(hmmsort_plan *p, double *counts_out, void *stream)
{
    HS_CHECK(p && counts_out, HMMSORT_EINVAL, "plan_expected_counts: null argument");
    return p->eng->expected_counts(counts_out, (hipStream_t)stream);
}

}  // extern "C"
