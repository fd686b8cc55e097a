// C ABI of libhmmsort_hip.so (see include/hmmsort.h): options, plan creation (the one place that chooses an
// engine) and the plan API, which is argument checks plus one call forwarded to the plan's Engine
// (hmmsort_internal.h).  The host-buffer entry points are in host_calls.cpp.  No CPU compute path exists here.
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

int hmmsort_samples_to_f64(const void *d_in, int sample_type, int64_t T, int64_t stride, double *d_out,
                           void *stream)
{
    HS_CHECK(T >= 0 && stride >= 1 && (T == 0 || (d_in && d_out)), HMMSORT_EINVAL,
             "samples_to_f64: bad argument (T = %lld, stride = %lld)", (long long)T, (long long)stride);
    int rc = need_device();
    if (rc) return rc;
    return dev_widen(d_in, sample_type, T, stride, d_out, (hipStream_t)stream);
}

// Front end (preprocess.hip).  No plan and no cached slot.
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

// Spatial whitening (whiten.hip).  No plan and no cached slot.
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
    HS_CHECK(first[0] >= 1, HMMSORT_EINVAL, "reconstruct_tracked: first[0] = %lld is no 1-based sample number",
             (long long)first[0]);
    for (int64_t c = 1; c < nchunks; c++)
        HS_CHECK(first[c] > first[c - 1], HMMSORT_EINVAL, "reconstruct_tracked: chunk starts must ascend (first[%lld] = "
                 "%lld after %lld)", (long long)c, (long long)first[c], (long long)first[c - 1]);
    HS_CHECK(nchunks <= kTrackChunks, HMMSORT_EUNSUP, "reconstruct_tracked: %lld chunks (at most %lld)",
             (long long)nchunks, (long long)kTrackChunks);
    if (T == 0) return HMMSORT_OK;
    int rc = need_device();
    if (rc) return rc;
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

// extract_spiketimes on a path that already lives in device memory
static int extract_from_device(const int16_t *d_x, int64_t T, const int16_t *states, int64_t N,
                               int64_t S, const double *mu, int64_t K, int64_t *times_out,
                               int64_t cap, int64_t *counts_out, hipStream_t st, DevBuf *dt_keep = nullptr,
                               int64_t *dcap_all = nullptr)
{
    // dcap_all (with dt_keep): the device keeps EVERY event, rows of *dcap_all = max(1, largest count) entries,
    // whatever cap says; the host still receives the first min(count, cap) of each row
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
    DevBuf &dt = dt_keep ? *dt_keep : dt_own;   // compacted times [N][cap] stay on the device for the caller
    int rc;
    if ((rc = dm.alloc(S * sizeof(uint32_t))) || (rc = dcnt.alloc(nb * N * sizeof(int64_t))) ||
        (rc = doff.alloc(nb * N * sizeof(int64_t))) ||
        (!all && (rc = dt.alloc(std::max<int64_t>(1, N * cap) * sizeof(int64_t)))))
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
    if (all) {
        int64_t dcap = 1;
        for (int64_t i = 0; i < N; i++) dcap = std::max(dcap, counts_out[i]);
        *dcap_all = dcap;
        if ((rc = dt.alloc((size_t)N * dcap * sizeof(int64_t)))) return rc;
        HS_HIP(hipMemcpyAsync(doff.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
        if ((rc = dev_spike_compact(d_x, T, dm.as<uint32_t>(), (int)N, (int)S, 1, dcnt.as<int64_t>(),
                                    doff.as<int64_t>(), dt.as<int64_t>(), dcap, st)))
            return rc;
        for (int64_t i = 0; i < N && times_out; i++) {
            const int64_t n = std::min(counts_out[i], cap);
            if (n > 0)
                HS_HIP(hipMemcpyAsync(times_out + i * cap, dt.as<int64_t>() + i * dcap, n * sizeof(int64_t),
                                      hipMemcpyDeviceToHost, st));
        }
        HS_HIP(hipStreamSynchronize(st));   // off and the compaction tables die with this frame
        return HMMSORT_OK;
    }
    if (cap == 0) return HMMSORT_OK;
    HS_HIP(hipMemcpyAsync(doff.p, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if ((rc = dev_spike_compact(d_x, T, dm.as<uint32_t>(), (int)N, (int)S, 1, dcnt.as<int64_t>(),
                                doff.as<int64_t>(), dt.as<int64_t>(), cap, st)))
        return rc;
    for (int64_t i = 0; i < N; i++) {
        const int64_t n = std::min(counts_out[i], cap);
        HS_HIP(hipMemcpyAsync(times_out + i * cap, dt.as<int64_t>() + i * cap, n * sizeof(int64_t),
                              hipMemcpyDeviceToHost, st));
    }
    HS_HIP(hipStreamSynchronize(st));
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

// reconstruct_signal / unroll_mlseq on a path in device memory, results left in device memory
static int plan_path_op(hmmsort_plan *p, const int16_t *d_x, double *d_y_out, int16_t *d_unrolled,
                        hipStream_t st)
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

int hmmsort_plan_expected_counts(hmmsort_plan *p, double *counts_out, void *stream)
{
    HS_CHECK(p && counts_out, HMMSORT_EINVAL, "plan_expected_counts: null argument");
    return p->eng->expected_counts(counts_out, (hipStream_t)stream);
}

// ---- per-spike fit (spike_fit.hip) -------------------------------------------------

// what both entry points refuse before any GPU work; qv receives the N trough values of the base templates
static int spike_fit_check(const char *who, int64_t N, int64_t S, const double *mu, int64_t K, int64_t nchunks,
                           const int64_t *first, const double *mu_track, const hmmsort_spike_fit_out *out, int32_t *qv)
{
    HS_CHECK(N >= 1 && N <= 32, HMMSORT_EINVAL, "%s: N = %lld templates (1..32)", who, (long long)N);
    HS_CHECK(K >= 2, HMMSORT_EINVAL, "%s: K = %lld (a template needs at least one phase besides the silent row)", who,
             (long long)K);
    HS_CHECK(S >= 1 && out->cap >= 0, HMMSORT_EINVAL, "%s: bad sizes (S = %lld, cap = %lld)", who, (long long)S,
             (long long)out->cap);
    HS_CHECK(nchunks >= 0, HMMSORT_EINVAL, "%s: nchunks = %lld", who, (long long)nchunks);
    HS_CHECK(nchunks <= kTrackChunks, HMMSORT_EUNSUP, "%s: %lld chunks (at most %lld)", who, (long long)nchunks,
             (long long)kTrackChunks);
    if (nchunks > 0) {
        HS_CHECK(first && mu_track, HMMSORT_EINVAL, "%s: a track needs first and mu_track", who);
        HS_CHECK(first[0] >= 1, HMMSORT_EINVAL, "%s: first[0] = %lld is no 1-based sample number", who,
                 (long long)first[0]);
        for (int64_t c = 1; c < nchunks; c++)
            HS_CHECK(first[c] > first[c - 1], HMMSORT_EINVAL, "%s: chunk starts must ascend (first[%lld] = %lld after "
                     "%lld)", who, (long long)c, (long long)first[c], (long long)first[c - 1]);
    }
    for (int64_t a = 0; a < N; a++) {
        qv[a] = trough_value(mu, K, a);
        HS_CHECK(qv[a] != 1, HMMSORT_EINVAL, "%s: template %lld has its minimum in the silent row (trough value 1): "
                 "no state marks its spikes", who, (long long)a);
    }
    return HMMSORT_OK;
}

// one channel: resident signal and path in, host arrays out (rows of `cap` entries; any of them may be null)
static int spike_fit_channel(const double *d_y, const int16_t *d_x, int64_t T, const int16_t *states, int64_t N,
                             int64_t S, const double *mu, int64_t K, const int32_t *qv, int64_t nchunks,
                             const int64_t *first, const double *mu_track, int64_t *times, double *amp, double *rss,
                             double *energy, int32_t *nused, int64_t cap, int64_t *counts, double *summary,
                             hipStream_t st)
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
    const int64_t nblk = spike_fit_blocks(maxn), nM = (nchunks > 0 ? nchunks : 1) * K * N;
    DevBuf dst, dM, dfirst, damp, drss, den, dnu, dch, dpart, dsum;
    if ((rc = dst.alloc(N * S * sizeof(int16_t))) || (rc = dM.alloc(nM * sizeof(double))) ||
        (rc = dfirst.alloc(std::max<int64_t>(1, nchunks) * sizeof(int64_t))) ||
        (rc = damp.alloc(N * dcap * sizeof(double))) || (rc = drss.alloc(N * dcap * sizeof(double))) ||
        (rc = den.alloc(N * dcap * sizeof(double))) || (rc = dnu.alloc(N * dcap * sizeof(int32_t))) ||
        (rc = dch.alloc(N * dcap * sizeof(int32_t))) || (rc = dpart.alloc(N * nblk * L * sizeof(double))) ||
        (rc = dsum.alloc(N * L * sizeof(double))))
        return rc;
    HS_HIP(hipMemcpyAsync(dst.p, states, N * S * sizeof(int16_t), hipMemcpyHostToDevice, st));
    HS_HIP(hipMemcpyAsync(dM.p, nchunks > 0 ? mu_track : mu, nM * sizeof(double), hipMemcpyHostToDevice, st));
    if (nchunks > 0)
        HS_HIP(hipMemcpyAsync(dfirst.p, first, nchunks * sizeof(int64_t), hipMemcpyHostToDevice, st));
    if ((rc = dev_spike_fit(d_y, d_x, T, dst.as<int16_t>(), N, S, K, dM.as<double>(), nchunks, dfirst.as<int64_t>(),
                            dt.as<int64_t>(), dcap, counts, qv, damp.as<double>(), drss.as<double>(),
                            den.as<double>(), dnu.as<int32_t>(), dch.as<int32_t>(), dpart.as<double>(),
                            dsum.as<double>(), st)))
        return rc;
    for (int64_t a = 0; a < N; a++) {
        const size_t n = (size_t)std::min(counts[a], cap);
        if (n == 0) continue;
        if (amp) HS_HIP(hipMemcpyAsync(amp + a * cap, damp.as<double>() + a * dcap, n * 8, hipMemcpyDeviceToHost, st));
        if (rss) HS_HIP(hipMemcpyAsync(rss + a * cap, drss.as<double>() + a * dcap, n * 8, hipMemcpyDeviceToHost, st));
        if (energy)
            HS_HIP(hipMemcpyAsync(energy + a * cap, den.as<double>() + a * dcap, n * 8, hipMemcpyDeviceToHost, st));
        if (nused)
            HS_HIP(hipMemcpyAsync(nused + a * cap, dnu.as<int32_t>() + a * dcap, n * 4, hipMemcpyDeviceToHost, st));
    }
    std::vector<double> sum(summary ? N * L : 0);
    if (summary) HS_HIP(hipMemcpyAsync(sum.data(), dsum.p, N * L * sizeof(double), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    for (int64_t i = 0; summary && i < N * L; i++)
        if (i % L != 7) summary[i] = sum[i];
    return HMMSORT_OK;
}

int hmmsort_spike_fit(const void *y, int sample_type, int64_t T, const int16_t *x, const int16_t *states, int64_t N,
                      int64_t S, const double *mu, int64_t K, int64_t nchunks, const int64_t *first,
                      const double *mu_track, hmmsort_spike_fit_out *out)
{
    HS_CHECK(states && mu && out && out->counts && (T == 0 || (y && x)), HMMSORT_EINVAL, "spike_fit: null argument");
    HS_CHECK(sample_type == HMMSORT_SAMPLES_F64 || sample_type == HMMSORT_SAMPLES_I16, HMMSORT_EINVAL,
             "spike_fit: samples must be HMMSORT_SAMPLES_F64 or HMMSORT_SAMPLES_I16");
    HS_CHECK(T >= 0, HMMSORT_EINVAL, "spike_fit: T = %lld", (long long)T);
    int32_t qv[32];
    int rc = spike_fit_check("spike_fit", N, S, mu, K, nchunks, first, mu_track, out, qv);
    if (rc) return rc;
    // every phase the table names must be a row of the templates: the device code indexes with it
    for (int64_t i = 0; i < N * S; i++)
        HS_CHECK(states[i] >= 1 && states[i] <= K, HMMSORT_EINVAL, "spike_fit: states[%lld] = %d outside 1..K",
                 (long long)i, (int)states[i]);
    DevBuf draw, dy, dx;
    if (T > 0) {
        if ((rc = need_device())) return rc;
        if ((rc = dy.alloc((size_t)T * sizeof(double))) || (rc = dx.alloc((size_t)T * sizeof(int16_t)))) return rc;
        HS_HIP(hipMemcpy(dx.p, x, (size_t)T * sizeof(int16_t), hipMemcpyHostToDevice));
        if (sample_type == HMMSORT_SAMPLES_I16) {
            if ((rc = draw.alloc((size_t)T * sizeof(int16_t)))) return rc;
            HS_HIP(hipMemcpy(draw.p, y, (size_t)T * sizeof(int16_t), hipMemcpyHostToDevice));
            if ((rc = dev_widen(draw.p, sample_type, T, 1, dy.as<double>(), nullptr))) return rc;
        } else {
            HS_HIP(hipMemcpy(dy.p, y, (size_t)T * sizeof(double), hipMemcpyHostToDevice));
        }
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

// ---- correlograms (correlogram.hip) ---------------------------------------------------

// Every channel's events under the plan's current model, compacted on the device exactly as
// hmmsort_plan_extract_spiketimes finds them and concatenated into dt in unit order u = ch N + a behind the host
// offsets offs[0 .. U]; only the counts come to the host.  Shared by the calls that work on the units of a plan.  The
// copies into dt are enqueued on st and read `rows`, so the record must outlive the caller's next synchronisation.
struct PlanUnits {
    std::vector<DevBuf> rows;   // per channel: rows of dcap[ch] entries per template
    DevBuf dt;
    std::vector<int64_t> offs;
};

static int plan_compact_units(hmmsort_plan *p, const int16_t *d_x, hipStream_t st, PlanUnits *pu)
{
    const int64_t N = p->model.N, nC = p->C, U = nC * N, T = p->T;
    int rc;
    std::vector<int64_t> dcap((size_t)nC, 1), &offs = pu->offs;
    pu->rows = std::vector<DevBuf>((size_t)nC);
    offs.assign((size_t)U + 1, 0);
    for (int64_t ch = 0; ch < nC; ch++) {
        const HostModel &m = nC > 1 ? p->models[ch] : p->model;
        int64_t counts[32] = {0};
        if ((rc = extract_from_device(d_x + ch * T, T, m.states.data(), N, m.S, m.mu.data(), m.K, nullptr, 0, counts, st,
                                      &pu->rows[ch], &dcap[ch])))
            return rc;
        for (int64_t a = 0; a < N; a++) offs[ch * N + a + 1] = offs[ch * N + a] + counts[a];
    }
    if ((rc = pu->dt.alloc((size_t)offs[U] * sizeof(int64_t)))) return rc;
    for (int64_t u = 0; u < U; u++) {
        const int64_t n = offs[u + 1] - offs[u], ch = u / N, a = u % N;
        if (n > 0)
            HS_HIP(hipMemcpyAsync(pu->dt.as<int64_t>() + offs[u], pu->rows[ch].as<int64_t>() + a * dcap[ch],
                                  (size_t)n * sizeof(int64_t), hipMemcpyDeviceToDevice, st));
    }
    return HMMSORT_OK;
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

// ---- footprints (footprint.hip) -------------------------------------------------------

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

}  // extern "C"
