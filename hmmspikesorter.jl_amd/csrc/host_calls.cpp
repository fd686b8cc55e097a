// Host-buffer entry points of libhmmsort_hip.so (include/hmmsort.h): what a reference-side binding calls with
// arrays in host memory.  They keep their plans and device buffers between calls (slots) and share one driver
// that uploads the signal, runs the call on a plan and climbs the escalation ladder when the plan's own
// certificates fail.  No CPU compute path exists here.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>

#include "hmmsort_internal.h"

using namespace hmmsort;

namespace {

// ---- idle plans of the host-buffer entry points ---------------------------------------------
// hmmsort_viterbi / hmmsort_em_step are what a reference-side binding calls once per EM iteration or per
// channel: same T, same model shape, new numbers.  Creating the plan (workspace hipMalloc,
// geometry) and the signal/output buffers costs more than the sweeps, so an entry point leaves its plan and
// buffers here when it returns and the next call with the same key takes them and re-arms the plan with
// hmmsort_plan_set_model.  A slot is owned by exactly one call while in use (taken OUT of the list), so
// host threads never share a plan; the list itself is behind a mutex.  hmmsort_shutdown() empties it.
struct HostSlot {
    hmmsort_plan *plan = nullptr;
    DevBuf dy, dx, dll, dstats, dout;
    int64_t T = 0, engine_opt = 0, block = 0, halo = 0, hbm_cols = 0;
    int device = 0;
    // every slot works on a stream of its own and waits for that stream only: host threads that decode or
    // train at the same time overlap on the device instead of meeting in hipDeviceSynchronize
    hipStream_t st = nullptr;
    bool keep = true;  // the plan is the one a first attempt with these options builds: worth caching
    ~HostSlot()
    {
        drop_plan();
        if (st) (void)hipStreamDestroy(st);
    }
    void drop_plan()
    {
        if (plan) hmmsort_plan_destroy(plan);
        plan = nullptr;
    }
};
std::mutex g_slots_mu;
std::vector<std::unique_ptr<HostSlot>> g_slots;  // idle, least recently used first

struct ModelArgs {  // the model arguments every host-buffer entry point takes
    const int16_t *states;
    int64_t N, K, S;
    const hmm_trans *tr;
    int64_t R;
    const double *mu;
    double sigma;
};

std::unique_ptr<HostSlot> take_slot(int64_t T, const ModelArgs &a, const Options &opt)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(g_slots_mu);
    for (size_t i = g_slots.size(); i-- > 0;) {
        HostSlot &h = *g_slots[i];
        const HostModel &m = h.plan->model;
        if (h.T != T || h.device != dev || h.engine_opt != opt.engine || h.block != opt.block ||
            h.halo != opt.halo || h.hbm_cols != opt.blocked_hbm_columns || m.N != a.N || m.K != a.K || m.S != a.S)
            continue;
        if (memcmp(m.states.data(), a.states, m.states.size() * sizeof(int16_t))) continue;
        std::unique_ptr<HostSlot> out = std::move(g_slots[i]);
        g_slots.erase(g_slots.begin() + i);
        return out;
    }
    return nullptr;
}

void give_slot(std::unique_ptr<HostSlot> slot, const Options &opt)
{
    if (!slot || !slot->plan || opt.plan_cache <= 0) return;
    {
        std::lock_guard<std::mutex> lk(g_slots_mu);
        g_slots.push_back(std::move(slot));
    }
    host_slots_trim((size_t)options_get().plan_cache);
}

std::unique_ptr<HostSlot> new_slot(int64_t T, const Options &opt)
{
    std::unique_ptr<HostSlot> h(new HostSlot());
    h->T = T;
    h->engine_opt = opt.engine;
    h->block = opt.block;
    h->halo = opt.halo;
    h->hbm_cols = opt.blocked_hbm_columns;
    if (hipGetDevice(&h->device) != hipSuccess) (void)hipGetLastError();
    if (hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        h->st = nullptr;   // the null stream still works, it only serialises
    }
    return h;
}

// ---- the escalation ladder --------------------------------------------------------------------
// The time-parallel engines certify their own chain / block boundaries on the device.  When a check fails, a
// host-buffer entry point retries with a doubled warm-up (up to the length of the signal) and finally with the
// strict engine.  What differs between the entries is in this table; everything else is host_call() below.
constexpr unsigned under(int64_t engine) { return 1u << engine; }
struct Entry {
    const char *name;
    // true: a decode, failed = diag[0] (block boundaries) or diag[7] (near-ties left open on the path of a blocked
    // or wave plan); false: a forward-backward call, failed = diag[3] + diag[5] (chain boundaries)
    bool decode;
    // a plan this entry can run on; any other is replaced by a strict plan (which every entry can use)
    bool (*usable)(const Engine &, const Options &);
    // requested engines (option "engine") under which the ladder may end on the strict engine; under any other the
    // call fails with HMMSORT_ENOCONV.  The three sets differ for no recorded reason and are kept as they were.
    unsigned strict_after;
};
const Entry kViterbi = {"viterbi", true, [](const Engine &, const Options &) { return true; },
                        under(HMMSORT_ENGINE_AUTO)};
// a strict plan has no sufficient-statistics E-step: em_step runs forward -> backward -> update on it instead
const Entry kEmStep = {"em_step", false,
                       [](const Engine &e, const Options &) { return e.has_estep() || e.id == HMMSORT_ENGINE_STRICT; },
                       under(HMMSORT_ENGINE_AUTO) | under(HMMSORT_ENGINE_STRICT)};
// what the wave engine does not take goes to the strict engine (materialised alpha/beta) unless the caller asked
// for the blocked engine by name and the model fits it.  A named BLOCKED (or RING) engine quietly ends on the
// strict engine when its boundaries keep failing.
const Entry kPosteriors = {"posteriors", false,
                           [](const Engine &e, const Options &opt) {
                               return e.id == HMMSORT_ENGINE_WAVE || e.id == HMMSORT_ENGINE_STRICT ||
                                      (e.id == HMMSORT_ENGINE_BLOCKED && opt.engine == HMMSORT_ENGINE_BLOCKED &&
                                       e.has_posteriors());
                           },
                           under(HMMSORT_ENGINE_AUTO) | under(HMMSORT_ENGINE_STRICT) | under(HMMSORT_ENGINE_RING) |
                               under(HMMSORT_ENGINE_BLOCKED)};

int64_t next_halo(const hmmsort_plan *p)
{
    int64_t b = 0, h = 0, n = 0;
    p->eng->geometry(&b, &h, &n);
    return h * 2;
}

// Near-ties the exact resolver could not settle (none on any signal seen), every boundary certified, engine AUTO:
// the op-for-op sweep decides.  It keeps back-pointers for the states with more than one incoming transition only
// (N + 1 of a ring model: 3.4 GB at 4081 states x 10^8 samples instead of the reference's S x T table, 0.8 TB).
// Should even that not fit, the time-parallel path stands: it differs from the reference's at most at the open
// decisions, whose margins are inside the reference's own rounding noise.  last_escalations < 0 = minus the
// number of such decisions.
bool strict_table_does_not_fit(const hmmsort_plan *p, const Options &opt, int64_t open_ties)
{
    const HostModel &m = p->model;
    int64_t nmulti = 0;
    for (int64_t j = 0; j < m.S; j++) nmulti += (m.in_ptr[j + 1] - m.in_ptr[j]) > 1;
    const double need = (double)std::max<int64_t>(nmulti, 1) * (double)p->T * 2.0 + 16.0 * (double)p->T;
    const double limit = strict_limit_bytes(opt);
    if (need <= limit) return false;
    last_escalations() = -open_ties;
    set_error("viterbi: %lld near-tie decisions on the decoded path; the strict sweep needs %.1f GB of "
              "back-pointers (limit %.1f GB): time-parallel path returned", (long long)open_ties, need / 1e9,
              limit / 1e9);
    return true;
}

// One host-buffer call: the signal goes up into a slot (its own from an earlier call with the same key, or a new
// one), run(slot) enqueues the work on the slot's plan and stream, the plan's diagnostics decide whether the
// result stands, and out(slot) brings it to the caller.  The slot goes back to the cache only with the plan a
// first attempt builds.
template <class Run, class Out>
int host_call(const Entry &e, const void *y, int sample_type, int64_t T, const ModelArgs &a, Run run, Out out)
{
    int rc;
    if ((rc = need_device())) return rc;
    const Options opt = options_get();
    last_escalations() = 0;
    std::unique_ptr<HostSlot> slot = take_slot(T, a, opt);
    if (!slot) slot = new_slot(T, opt);
    HostSlot &h = *slot;
    if ((rc = h.dy.ensure(T * sizeof(double)))) return rc;
    if (sample_type == HMMSORT_SAMPLES_F64) {
        HS_HIP(hipMemcpyAsync(h.dy.p, y, T * sizeof(double), hipMemcpyHostToDevice, h.st));
    } else {
        // raw samples: the decoded path's buffer has the size of an int16 signal and is free until the sweep
        HS_CHECK(sample_type == HMMSORT_SAMPLES_I16, HMMSORT_EINVAL, "%s: unsupported sample type", e.name);
        if ((rc = h.dx.ensure(T * sizeof(int16_t)))) return rc;
        HS_HIP(hipMemcpyAsync(h.dx.p, y, T * sizeof(int16_t), hipMemcpyHostToDevice, h.st));
        if ((rc = dev_widen(h.dx.p, sample_type, T, 1, h.dy.as<double>(), h.st))) return rc;
    }
    // an idle plan of the same shape: new numbers in, workspace kept.  A list it cannot take (a ring
    // model that stopped being one) falls through to a fresh plan.
    if (h.plan && hmmsort_plan_set_model(h.plan, a.tr, a.R, a.mu, a.sigma)) h.drop_plan();
    int64_t halo = -1, engine = opt.engine;
    for (int attempt = 0;; attempt++) {
        if (!h.plan) {
            rc = plan_create_engine(&h.plan, T, a.states, a.N, a.K, a.S, a.tr, a.R, a.mu, a.sigma, engine, halo);
            if (rc) return rc;
        }
        Engine &eng = *h.plan->eng;
        if (!e.usable(eng, opt)) {
            engine = HMMSORT_ENGINE_STRICT;
            h.drop_plan();
            h.keep = false;
            continue;
        }
        if ((rc = run(h))) return rc;
        HS_HIP(hipStreamSynchronize(h.st));
        if (eng.id == HMMSORT_ENGINE_STRICT) break;   // the reference's own sweep: nothing to certify
        int64_t diag[8] = {0};
        if ((rc = eng.diagnostics(h.st, diag))) return rc;
        const int64_t bad = e.decode ? diag[0] : diag[3] + diag[5];   // boundaries that fail their certificate
        const bool ties = e.decode && (eng.id == HMMSORT_ENGINE_BLOCKED || eng.id == HMMSORT_ENGINE_WAVE) && diag[7] != 0;
        if ((bad == 0 && !ties) || !opt.escalate) break;
        if (ties && bad == 0 && opt.engine == HMMSORT_ENGINE_AUTO && strict_table_does_not_fit(h.plan, opt, diag[7]))
            break;
        last_escalations() = attempt + 1;
        if (ties && bad == 0 && eng.drop_structured_sweep()) {
            // overlap model: a decision on the path is inside the noise of the structured sweep's own arithmetic --
            // decode again with the generic blocked sweep (the reference's operation order per block)
            h.keep = false;
            continue;
        }
        halo = next_halo(h.plan);
        if (attempt >= 3 || halo > T || ties) {
            // near-ties depend on the frame, not on the warm-up: straight to the op-for-op sweep
            if (!(e.strict_after & under(opt.engine))) {
                if (e.decode)
                    set_error("viterbi: %lld block boundaries fail the warm-up check, %lld blocks hold near-ties",
                              (long long)diag[0], (long long)diag[7]);
                else
                    set_error("%s: %lld chain boundaries still fail the warm-up check", e.name, (long long)bad);
                return HMMSORT_ENOCONV;
            }
            engine = HMMSORT_ENGINE_STRICT;
        }
        // a wider warm-up changes the geometry: the plan and what was sized for it are rebuilt
        h.drop_plan();
        h.dstats.release();
        h.dout.release();
        h.keep = false;
    }
    if ((rc = out(h))) return rc;
    if (h.keep) give_slot(std::move(slot), opt);
    return HMMSORT_OK;
}

int viterbi_host(const void *y, int sample_type, int64_t T, const ModelArgs &a, int16_t *x_out, double *ll_out)
{
    HS_CHECK(y && x_out && ll_out, HMMSORT_EINVAL, "viterbi: null argument");
    HS_CHECK(T >= 1, HMMSORT_EINVAL, "viterbi: empty signal (T = %lld)", (long long)T);
    return host_call(
        kViterbi, y, sample_type, T, a,
        [&](HostSlot &h) {
            int rc;
            if ((rc = h.dx.ensure(T * sizeof(int16_t))) || (rc = h.dll.ensure(sizeof(double)))) return rc;
            return h.plan->eng->viterbi(h.dy.as<double>(), h.dx.as<int16_t>(), h.dll.as<double>(), h.st);
        },
        [&](HostSlot &h) {
            HS_HIP(hipMemcpyAsync(x_out, h.dx.p, T * sizeof(int16_t), hipMemcpyDeviceToHost, h.st));
            HS_HIP(hipMemcpyAsync(ll_out, h.dll.p, sizeof(double), hipMemcpyDeviceToHost, h.st));
            HS_HIP(hipStreamSynchronize(h.st));
            return HMMSORT_OK;
        });
}

int fwd_bwd_host(bool fwd, const double *y, int64_t T, const ModelArgs &a, double *out)
{
    HS_CHECK(y && out, HMMSORT_EINVAL, "forward/backward: null argument");
    HS_CHECK(T >= 1, HMMSORT_EINVAL, "forward/backward: empty signal");
    PlanGuard pg;
    // materialising S x T output is the strict engine's job whatever the model
    int rc = plan_create_engine(&pg.p, T, a.states, a.N, a.K, a.S, a.tr, a.R, a.mu, a.sigma, HMMSORT_ENGINE_STRICT);
    if (rc) return rc;
    DevBuf dy, da;
    if ((rc = dy.alloc(T * sizeof(double))) || (rc = da.alloc((size_t)a.S * T * sizeof(double))))
        return rc;
    HS_HIP(hipMemcpy(dy.p, y, T * sizeof(double), hipMemcpyHostToDevice));
    rc = fwd ? pg.p->eng->forward(dy.as<double>(), da.as<double>(), nullptr)
             : pg.p->eng->backward(dy.as<double>(), da.as<double>(), nullptr);
    if (rc) return rc;
    HS_HIP(hipDeviceSynchronize());
    HS_HIP(hipMemcpy(out, da.p, (size_t)a.S * T * sizeof(double), hipMemcpyDeviceToHost));
    return HMMSORT_OK;
}

// unpack [mu K*N | sigma | lp nlp | pp S] from the device into the caller's buffers
int unpack_mstep(const double *d_out, int64_t K, int64_t N, int64_t S, int64_t nlp, double *mu_inout,
                 double *sigma_out, double *lp_out, int64_t lp_cap, int64_t *n_lp_out, double *pp_out)
{
    std::vector<double> h(K * N + 1 + nlp + S);
    HS_HIP(hipMemcpy(h.data(), d_out, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    memcpy(mu_inout, h.data(), K * N * sizeof(double));
    *sigma_out = h[K * N];
    if (n_lp_out) *n_lp_out = nlp;
    HS_CHECK(lp_cap >= nlp, HMMSORT_EINVAL, "lp_out too small: need %lld entries, got %lld",
             (long long)nlp, (long long)lp_cap);
    memcpy(lp_out, h.data() + K * N + 1, nlp * sizeof(double));
    if (pp_out) memcpy(pp_out, h.data() + K * N + 1 + nlp, S * sizeof(double));
    return HMMSORT_OK;
}

}  // namespace

void hmmsort::host_slots_trim(size_t keep)
{
    std::vector<std::unique_ptr<HostSlot>> dead;
    {
        std::lock_guard<std::mutex> lk(g_slots_mu);
        while (g_slots.size() > keep) {
            dead.push_back(std::move(g_slots.front()));
            g_slots.erase(g_slots.begin());
        }
    }
    // hipFree outside the lock
}

extern "C" {

int hmmsort_viterbi(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                    int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                    int16_t *x_out, double *ll_out)
{
    return viterbi_host(y, HMMSORT_SAMPLES_F64, T, {states, N, K, S, tr, R, mu, sigma}, x_out, ll_out);
}

int hmmsort_viterbi_i16(const int16_t *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                        int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                        int16_t *x_out, double *ll_out)
{
    return viterbi_host(y, HMMSORT_SAMPLES_I16, T, {states, N, K, S, tr, R, mu, sigma}, x_out, ll_out);
}

int hmmsort_forward(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                    int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                    double *alpha_out)
{
    return fwd_bwd_host(true, y, T, {states, N, K, S, tr, R, mu, sigma}, alpha_out);
}

int hmmsort_backward(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                     int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                     double *beta_out)
{
    return fwd_bwd_host(false, y, T, {states, N, K, S, tr, R, mu, sigma}, beta_out);
}

int hmmsort_update(const double *alpha, const double *beta, const double *x, int64_t T,
                   const int16_t *states, int64_t N, int64_t K, int64_t S, const hmm_trans *tr,
                   int64_t R, double *mu_inout, double sigma, double *sigma_out, double *lp_out,
                   int64_t lp_cap, int64_t *n_lp_out, double *pp_out)
{
    HS_CHECK(alpha && beta && x && mu_inout && sigma_out && lp_out, HMMSORT_EINVAL,
             "update: null argument");
    HS_CHECK(T >= 2, HMMSORT_EINVAL, "update: need T >= 2");
    PlanGuard pg;
    int rc = plan_create_engine(&pg.p, T, states, N, K, S, tr, R, mu_inout, sigma,
                                HMMSORT_ENGINE_STRICT);
    if (rc) return rc;
    const int64_t nlp = pg.p->eng->n_lp();
    DevBuf dy, da, db, dout;
    const size_t st = (size_t)S * T * sizeof(double);
    if ((rc = dy.alloc(T * sizeof(double))) || (rc = da.alloc(st)) || (rc = db.alloc(st)) ||
        (rc = dout.alloc((K * N + 1 + nlp + S) * sizeof(double))))
        return rc;
    HS_HIP(hipMemcpy(dy.p, x, T * sizeof(double), hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(da.p, alpha, st, hipMemcpyHostToDevice));
    HS_HIP(hipMemcpy(db.p, beta, st, hipMemcpyHostToDevice));
    rc = pg.p->eng->update(da.as<double>(), db.as<double>(), dy.as<double>(), dout.as<double>(), nullptr);
    if (rc) return rc;
    HS_HIP(hipDeviceSynchronize());
    return unpack_mstep(dout.as<double>(), K, N, S, nlp, mu_inout, sigma_out, lp_out, lp_cap,
                        n_lp_out, pp_out);
}

int hmmsort_em_step(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K,
                    int64_t S, const hmm_trans *tr, int64_t R, double *mu_inout, double sigma,
                    double *sigma_out, double *lp_out, int64_t lp_cap, int64_t *n_lp_out,
                    double *pp_out)
{
    HS_CHECK(y && mu_inout && sigma_out && lp_out, HMMSORT_EINVAL, "em_step: null argument");
    HS_CHECK(T >= 2, HMMSORT_EINVAL, "em_step: need T >= 2");
    return host_call(
        kEmStep, y, HMMSORT_SAMPLES_F64, T, {states, N, K, S, tr, R, mu_inout, sigma},
        [&](HostSlot &h) {
            Engine &eng = *h.plan->eng;
            double *dy = h.dy.as<double>();
            int rc;
            // sized for THIS plan: a cached slot's buffers may come from a plan of another engine or list
            // (the slot key holds neither R nor the engine)
            if ((rc = h.dout.ensure(hmmsort_plan_mstep_len(h.plan) * sizeof(double)))) return rc;
            if (eng.has_estep()) {
                if ((rc = h.dstats.ensure(eng.stats_len() * sizeof(double)))) return rc;
                if ((rc = eng.estep(dy, h.dstats.as<double>(), h.st))) return rc;
                return eng.mstep(h.dstats.as<double>(), h.dout.as<double>(), h.st);
            }
            // strict plan: forward -> backward -> update with materialised alpha/beta, all on device
            h.keep = false;
            DevBuf da, db;
            const size_t st = (size_t)S * T * sizeof(double);
            if ((rc = da.alloc(st)) || (rc = db.alloc(st))) return rc;
            if ((rc = eng.forward(dy, da.as<double>(), h.st))) return rc;
            if ((rc = eng.backward(dy, db.as<double>(), h.st))) return rc;
            if ((rc = eng.update(da.as<double>(), db.as<double>(), dy, h.dout.as<double>(), h.st))) return rc;
            HS_HIP(hipStreamSynchronize(h.st));   // alpha and beta die with this frame
            return HMMSORT_OK;
        },
        [&](HostSlot &h) {
            return unpack_mstep(h.dout.as<double>(), K, N, S, h.plan->eng->n_lp(), mu_inout, sigma_out, lp_out,
                                lp_cap, n_lp_out, pp_out);
        });
}

int hmmsort_posteriors(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K, int64_t S,
                       const hmm_trans *tr, int64_t R, const double *mu, double sigma, double *onset, double *occ,
                       double *silent, int16_t *xm, double *logz)
{
    HS_CHECK(y && states && tr && mu, HMMSORT_EINVAL, "posteriors: null argument");
    HS_CHECK(T >= 2, HMMSORT_EINVAL, "posteriors: need T >= 2");
    DevBuf don, docc, dsil, dxm, dz;
    return host_call(
        kPosteriors, y, HMMSORT_SAMPLES_F64, T, {states, N, K, S, tr, R, mu, sigma},
        [&](HostSlot &h) {
            int rc;
            if ((onset && (rc = don.ensure((size_t)N * T * 8))) || (occ && (rc = docc.ensure((size_t)N * T * 8))) ||
                (silent && (rc = dsil.ensure((size_t)T * 8))) || (xm && (rc = dxm.ensure((size_t)T * 2))) ||
                (rc = dz.ensure(8)))
                return rc;
            if ((rc = hmmsort_plan_posteriors(h.plan, h.dy.as<double>(), don.as<double>(), docc.as<double>(),
                                              dsil.as<double>(), dz.as<double>(), h.st)))
                return rc;
            return xm ? hmmsort_plan_posterior_decode(h.plan, dxm.as<int16_t>(), h.st) : HMMSORT_OK;
        },
        [&](HostSlot &) {
            if (onset) HS_HIP(hipMemcpy(onset, don.p, (size_t)N * T * 8, hipMemcpyDeviceToHost));
            if (occ) HS_HIP(hipMemcpy(occ, docc.p, (size_t)N * T * 8, hipMemcpyDeviceToHost));
            if (silent) HS_HIP(hipMemcpy(silent, dsil.p, (size_t)T * 8, hipMemcpyDeviceToHost));
            if (xm) HS_HIP(hipMemcpy(xm, dxm.p, (size_t)T * 2, hipMemcpyDeviceToHost));
            if (logz) HS_HIP(hipMemcpy(logz, dz.p, 8, hipMemcpyDeviceToHost));
            return HMMSORT_OK;
        });
}

}  // extern "C"
