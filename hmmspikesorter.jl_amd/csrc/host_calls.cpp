// Host-buffer entry points of libhmmsort_hip.so (include/hmmsort.h): what a reference-side binding calls with
// arrays in host memory.  They keep their plans and device buffers between calls (slots) and share one driver
// that uploads the signal, runs the call on a plan and climbs the escalation ladder when the plan's own
// certificates fail.  No CPU compute path exists here.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

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
int host_call(const Entry &e, const void *y, int sample_type, int64_t T, const ModelArgs &a, Run run, Out out,
              const Options *snapshot = nullptr)
{
    int rc;
    if ((rc = need_device())) return rc;
    const Options opt = snapshot ? *snapshot : options_get();   // a chunked decode passes the one it took on entry
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

// what a caller may run on the plan, signal and path of a decode before its slot goes back to the cache
using AfterDecode = std::function<int(hmmsort_plan *, const double *, const int16_t *, hipStream_t)>;

int viterbi_host(const void *y, int sample_type, int64_t T, const ModelArgs &a, int16_t *x_out, double *ll_out,
                 const Options *snapshot = nullptr, const AfterDecode *after = nullptr)
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
            return after ? (*after)(h.plan, h.dy.as<double>(), h.dx.as<int16_t>(), h.st) : HMMSORT_OK;
        },
        snapshot);
}

// ---- chunked decode (fit.jl:11-42) ---------------------------------------------------------------
// One recording channel's walk through its chunks.  The signal and the stitched path stay in device memory; a
// chunk is decode (the chunk length's plan) + stitch (chunk_stitch.hip) + a 24-byte copy into pinned memory, all
// enqueued on the channel's stream by enqueue(); finish() waits for the stream once, reads the plan's
// diagnostics, the trim points and the chunk's log-likelihood, and advances.  Several channels are driven in step
// by fit_worker() below: all enqueue, then all finish.
// The chunk's log-likelihood is the reference's to the last bit (fit.jl:37 adds the chunks' values and the sum is
// compared with ==): the strict engine's own value, or, where a time-parallel engine or the ladder decoded the
// chunk -- they sum ll in parts, 1e-9 relative -- k_chunk_ll's serial fold along the decoded path.
bool fit_stops_call(int rc) { return rc == HMMSORT_EHIP || rc == HMMSORT_ENOMEM; }

// ---- Viterbi training on top of the loop (hmmsort_fit_step_channels) -----------------------------------------------
// A channel that ends well takes the path statistics of its whole recording while signal and stitched path are
// still in device memory, on a plan of its model (a chunk plan needs no more than the model), and either finishes
// them into its own record or hands the vector to the caller, who adds the channels' vectors and finishes once.
enum StepMode { kNoStep = 0, kStepFinish = 1, kStepStats = 2 };

// [mu K*N | sigma | lp nlp | pp S] and the three counts, in host memory, into a caller's record
int unpack_step(const double *h, const int64_t *counts, int64_t K, int64_t N, int64_t S, int64_t nlp,
                const hmmsort_step_out &o)
{
    if (o.n_lp) *o.n_lp = nlp;
    HS_CHECK(o.lp_cap >= nlp, HMMSORT_EINVAL, "fit_step_channels: lp too small: need %lld entries, got %lld",
             (long long)nlp, (long long)o.lp_cap);
    memcpy(o.mu, h, K * N * sizeof(double));
    *o.sigma = h[K * N];
    memcpy(o.lp, h + K * N + 1, nlp * sizeof(double));
    if (o.pp) memcpy(o.pp, h + K * N + 1 + nlp, S * sizeof(double));
    if (o.counts) memcpy(o.counts, counts, 3 * sizeof(int64_t));
    return HMMSORT_OK;
}

// d_stats (one channel) finished with the plan's model on st, waited for, into the caller's record
int finish_step(hmmsort_plan *p, const double *d_stats, hipStream_t st, const hmmsort_step_out &o)
{
    const HostModel &m = p->model;
    const int64_t len = hmmsort_plan_mstep_len(p);
    DevBuf dout, dcnt;
    int rc;
    if ((rc = dout.alloc(len * sizeof(double))) || (rc = dcnt.alloc(3 * sizeof(int64_t)))) return rc;
    if ((rc = plan_path_finish(p, d_stats, dout.as<double>(), dcnt.as<int64_t>(), st))) return rc;
    std::vector<double> h(len);
    int64_t counts[3] = {0, 0, 0};
    HS_HIP(hipMemcpyAsync(h.data(), dout.p, len * sizeof(double), hipMemcpyDeviceToHost, st));
    HS_HIP(hipMemcpyAsync(counts, dcnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
    HS_HIP(hipStreamSynchronize(st));
    return unpack_step(h.data(), counts, m.K, m.N, m.S, p->eng->n_lp(), o);
}

struct FitChannel {
    const void *y;
    const int sample_type;
    const int64_t T, chunksize;
    ModelArgs a;                  // the caller's model; a channel that re-estimates it points this at its own copy
    const Options &opt;
    int16_t *const ml_out;
    double *const ll_out;

    DevBuf dy, dml, dx, dsmall;   // signal (fp64), stitched path, one chunk's decode, [l, kk, chunk ll]
    // what k_chunk_ll folds along, from the first chunk plan's HostModel (every plan of the channel holds the same
    // model): per-state means and incoming transitions; and one chunk's path values
    DevBuf dmean, dinptr, dinsrc, dinlp, dpv;
    bool tables = false;
    bool path_ready = false;      // dml holds the initial ones: only then is there a path to bring back
    void *pin = nullptr;          // pinned copy of dsmall
    hipStream_t st = nullptr;
    std::map<int64_t, std::unique_ptr<HostSlot>> slots;   // chunk length -> plan
    bool twins = false;           // duplicate templates: a ring-engine plan cannot see their near-ties
    int64_t i = 1, j = 1, k = 0;  // fit.jl's i and j, the chunk in flight is [i, j] of k samples
    bool lead = false, trail = false, ladder = false;
    hmmsort_plan *plan = nullptr; // the plan of the chunk in flight
    double ll = 0.0;
    int64_t escalations = 0;
    bool done = false;
    int status = HMMSORT_OK;      // the channel's code once done
    std::string message;

    // the training step after the decode: what to do with the statistics, where they go, whether they were taken
    int step_mode = kNoStep;
    const hmmsort_step_out *step_out = nullptr;
    std::vector<double> *step_stats = nullptr;
    DevBuf dstats;
    bool stepped = false;

    FitChannel(const void *y_, int type, int64_t T_, int64_t chunk, const ModelArgs &a_, const Options &o, int16_t *ml,
               double *ll_)
        : y(y_), sample_type(type), T(T_), chunksize(chunk), a(a_), opt(o), ml_out(ml), ll_out(ll_)
    {
    }
    ~FitChannel()
    {
        for (auto &kv : slots) give_slot(std::move(kv.second), opt);
        if (pin) (void)hipHostFree(pin);
        if (st) (void)hipStreamDestroy(st);
    }
    int64_t *pin_lk() { return static_cast<int64_t *>(pin); }
    int64_t *d_lk() { return dsmall.as<int64_t>(); }
    double *d_ll() { return dsmall.as<double>() + 2; }

    // the channel ends here with `code`; the thread's message is kept because a worker's is lost with its thread
    int end(int code)
    {
        done = true;
        status = code;
        if (code) message = last_error();
        return code;
    }

    // ends the channel with its own errors (returns 0); passes on what stops the call
    int guard(int rc)
    {
        if (rc && !fit_stops_call(rc)) {
            end(rc);
            return HMMSORT_OK;
        }
        return rc;
    }

    int escalated(const void *yc, int64_t n, int16_t *x, double *ll_chunk, const AfterDecode *after = nullptr)
    {
        int rc = viterbi_host(yc, sample_type, n, a, x, ll_chunk, &opt, after);
        escalations += std::max<int64_t>(last_escalations(), 0);
        return rc;
    }

    // the statistics of the whole recording (dyp, dxp) on plan p, then this channel's share of the step
    int step(hmmsort_plan *p, const double *dyp, const int16_t *dxp, hipStream_t s)
    {
        const int64_t len = plan_path_stats_len(p);
        int rc;
        if ((rc = dstats.ensure(len * sizeof(double)))) return rc;
        if ((rc = plan_path_stats(p, dyp, dxp, T, 0, T, true, dstats.as<double>(), s))) return rc;
        stepped = true;
        if (step_mode == kStepFinish) return finish_step(p, dstats.as<double>(), s, *step_out);
        step_stats->resize(len);
        HS_HIP(hipMemcpyAsync(step_stats->data(), dstats.p, len * sizeof(double), hipMemcpyDeviceToHost, s));
        HS_HIP(hipStreamSynchronize(s));
        return HMMSORT_OK;
    }

    // the step of a channel the chunk loop has finished: signal and stitched path are resident, any chunk plan holds
    // the model.  A one-sample recording never went to the device: it goes now, with a plan made for the purpose.
    int step_resident()
    {
        int rc;
        if (!path_ready) {
            if (!st) HS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            if ((rc = dy.alloc(T * sizeof(double))) || (rc = dml.alloc(T * sizeof(int16_t)))) return rc;
            if (sample_type == HMMSORT_SAMPLES_F64) {
                HS_HIP(hipMemcpyAsync(dy.p, y, T * sizeof(double), hipMemcpyHostToDevice, st));
            } else {
                HS_HIP(hipMemcpyAsync(dml.p, y, T * sizeof(int16_t), hipMemcpyHostToDevice, st));
                if ((rc = dev_widen(dml.p, sample_type, T, 1, dy.as<double>(), st))) return rc;
            }
            HS_HIP(hipMemcpyAsync(dml.p, ml_out, T * sizeof(int16_t), hipMemcpyHostToDevice, st));
        }
        hmmsort_plan *p = nullptr;
        for (auto &kv : slots)
            if (!p && kv.second && kv.second->plan) p = kv.second->plan;
        if (!p && (rc = plan_for(std::min(chunksize > 0 ? chunksize : T, T), &p))) return rc;
        return step(p, dy.as<double>(), dml.as<int16_t>(), st);
    }

    bool has_twins() const
    {
        for (int64_t p = 0; p < a.N; p++)
            for (int64_t q = p + 1; q < a.N; q++)
                if (std::equal(a.mu + a.K * p, a.mu + a.K * (p + 1), a.mu + a.K * q)) return true;
        return false;
    }

    // uploads the signal, sets the path to ones; a whole-recording decode (chunksize <= 0) is finished here
    int open()
    {
        // fit.jl:6-9; one chunk that holds the recording (more than one sample of it) is the same decode
        if (chunksize <= 0 || (chunksize >= T && T > 1)) {
            // the step runs on the decode's own slot, before it goes back to the cache
            const AfterDecode after = [this](hmmsort_plan *p, const double *dyp, const int16_t *dxp, hipStream_t s) {
                return step(p, dyp, dxp, s);
            };
            int rc = escalated(y, T, ml_out, ll_out, step_mode ? &after : nullptr);
            return rc ? guard(rc) : end(HMMSORT_OK);
        }
        if (T == 1) {           // `while j < n` is never entered
            ml_out[0] = 1;
            *ll_out = 0.0;
            return end(HMMSORT_OK);
        }
        twins = has_twins();
        int rc;
        HS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HS_HIP(hipHostMalloc(&pin, 3 * sizeof(int64_t), hipHostMallocDefault));
        if ((rc = dy.alloc(T * sizeof(double))) || (rc = dml.alloc(T * sizeof(int16_t))) ||
            (rc = dx.alloc(std::min(chunksize, T) * sizeof(int16_t))) || (rc = dsmall.alloc(3 * sizeof(int64_t))))
            return rc;
        if ((rc = dpv.alloc(std::min(chunksize, T) * sizeof(double)))) return rc;
        if (sample_type == HMMSORT_SAMPLES_F64) {
            HS_HIP(hipMemcpyAsync(dy.p, y, T * sizeof(double), hipMemcpyHostToDevice, st));
        } else {
            // raw samples cross as they are; the path's buffer holds them until they are widened
            HS_HIP(hipMemcpyAsync(dml.p, y, T * sizeof(int16_t), hipMemcpyHostToDevice, st));
            if ((rc = dev_widen(dml.p, sample_type, T, 1, dy.as<double>(), st))) return rc;
        }
        if ((rc = dev_fill_i16(dml.as<int16_t>(), T, 1, st))) return rc;   // fit.jl:15
        path_ready = true;
        return HMMSORT_OK;
    }

    // the plan's model tables to the device, once per channel and again after the channel's model was replaced (the
    // plan and its model outlive the copies: the slot stays with the channel)
    int upload_tables(const HostModel &m)
    {
        int rc;
        if ((rc = dmean.ensure(m.mean.size() * sizeof(double))) || (rc = dinptr.ensure(m.in_ptr.size() * sizeof(int32_t))) ||
            (rc = dinsrc.ensure(m.in_src.size() * sizeof(int32_t))) || (rc = dinlp.ensure(m.in_lp.size() * sizeof(double))))
            return rc;
        HS_HIP(hipMemcpyAsync(dmean.p, m.mean.data(), m.mean.size() * sizeof(double), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(dinptr.p, m.in_ptr.data(), m.in_ptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(dinsrc.p, m.in_src.data(), m.in_src.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        HS_HIP(hipMemcpyAsync(dinlp.p, m.in_lp.data(), m.in_lp.size() * sizeof(double), hipMemcpyHostToDevice, st));
        tables = true;
        return HMMSORT_OK;
    }

    int plan_for(int64_t n, hmmsort_plan **out)
    {
        std::unique_ptr<HostSlot> &slot = slots[n];
        if (!slot) {
            slot = take_slot(n, a, opt);
            if (!slot) slot = new_slot(n, opt);
            if (slot->plan && hmmsort_plan_set_model(slot->plan, a.tr, a.R, a.mu, a.sigma)) slot->drop_plan();
        }
        if (!slot->plan) {
            int rc = plan_create_engine(&slot->plan, n, a.states, a.N, a.K, a.S, a.tr, a.R, a.mu, a.sigma, opt.engine);
            if (rc) return rc;
        }
        *out = slot->plan;
        return HMMSORT_OK;
    }

    // d_ll = the ll of the chunk in dx, rounded as the reference rounds it
    int exact_ll()
    {
        return dev_chunk_ll(dy.as<double>() + (i - 1), dx.as<int16_t>(), k, a.S, dmean.as<double>(), dinptr.as<int32_t>(),
                            dinsrc.as<int32_t>(), dinlp.as<double>(), a.sigma, dpv.as<double>(), d_ll(), st);
    }

    int stitch() { return dev_chunk_stitch(dx.as<int16_t>(), k, lead, trail, dml.as<int16_t>() + (i - 1), d_lk(), st); }

    int enqueue_chunk()
    {
        j = std::min(i + chunksize - 1, T);
        k = j - i + 1;
        lead = i > 1;
        trail = j < T;
        int rc;
        if ((rc = plan_for(k, &plan))) return rc;
        if (!tables && (rc = upload_tables(plan->model))) return rc;
        // the lane-per-chain ring engine has no near-tie detector: with twin templates the ladder decodes
        ladder = twins && plan->eng->id == HMMSORT_ENGINE_RING;
        if (ladder) return HMMSORT_OK;
        if ((rc = plan->eng->viterbi(dy.as<double>() + (i - 1), dx.as<int16_t>(), d_ll(), st))) return rc;
        if (plan->eng->id != HMMSORT_ENGINE_STRICT && (rc = exact_ll())) return rc;
        if ((rc = stitch())) return rc;
        HS_HIP(hipMemcpyAsync(pin, dsmall.p, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        return HMMSORT_OK;
    }

    // the chunk again through hmmsort_viterbi's ladder, from the caller's host buffer, stitched like any other
    int ladder_chunk(bool stitched_before, double *ll_chunk)
    {
        std::vector<int16_t> x(k);
        double ll_ladder = 0.0;   // of whichever engine the ladder ended on: replaced by the fold along its path
        const char *yc = static_cast<const char *>(y) +
                         (i - 1) * (sample_type == HMMSORT_SAMPLES_F64 ? sizeof(double) : sizeof(int16_t));
        int rc;
        if ((rc = escalated(yc, k, x.data(), &ll_ladder))) return rc;
        // what the first stitch wrote lies inside the chunk, where the path still held its initial ones
        if (stitched_before && (rc = dev_fill_i16(dml.as<int16_t>() + (i - 1), k, 1, st))) return rc;
        HS_HIP(hipMemcpyAsync(dx.p, x.data(), k * sizeof(int16_t), hipMemcpyHostToDevice, st));
        if ((rc = exact_ll()) || (rc = stitch())) return rc;
        HS_HIP(hipMemcpyAsync(pin, dsmall.p, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
        HS_HIP(hipStreamSynchronize(st));
        memcpy(ll_chunk, pin_lk() + 2, sizeof(double));
        return HMMSORT_OK;
    }

    int finish_chunk()
    {
        int rc;
        double ll_chunk = 0.0;
        bool again = ladder;
        if (!ladder) {
            HS_HIP(hipStreamSynchronize(st));   // the one wait of this chunk
            Engine &eng = *plan->eng;
            if (eng.id != HMMSORT_ENGINE_STRICT && opt.escalate) {
                int64_t diag[8] = {0};
                if ((rc = eng.diagnostics(st, diag))) return rc;
                again = diag[0] != 0 ||
                        ((eng.id == HMMSORT_ENGINE_BLOCKED || eng.id == HMMSORT_ENGINE_WAVE) && diag[7] != 0);
            }
            memcpy(&ll_chunk, pin_lk() + 2, sizeof(double));
        }
        if (again && (rc = ladder_chunk(!ladder, &ll_chunk))) return rc;
        const int64_t l = pin_lk()[0], kk = pin_lk()[1];
        if (l > k) {
            set_error("fit_chunked: the chunk at sample %lld (%lld samples) holds no silent sample: its leading trim "
                      "runs off the chunk (fit.jl:26, BoundsError in the reference)", (long long)i, (long long)k);
            return end(HMMSORT_ENOSILENT);
        }
        ll += ll_chunk;
        j = i + kk - 1;
        if (j <= i) {
            set_error("fit_chunked: the chunk at sample %lld (%lld samples) has no silent sample after its first: "
                      "the next chunk would not advance (fit.jl:41, the reference loops forever)", (long long)i,
                      (long long)k);
            return end(HMMSORT_ENOSILENT);
        }
        i = j;
        if (!(j < T)) end(HMMSORT_OK);
        return HMMSORT_OK;
    }

    // the path and the sum as they stand, complete or not
    int collect()
    {
        if (!st || !path_ready) return HMMSORT_OK;   // finished in open(), or ended there before there was a path
        HS_HIP(hipMemcpyAsync(ml_out, dml.p, T * sizeof(int16_t), hipMemcpyDeviceToHost, st));
        HS_HIP(hipStreamSynchronize(st));
        *ll_out = ll;
        return HMMSORT_OK;
    }
};

struct FitJob {
    int64_t C, T, chunksize;
    const void *const *y;
    int sample_type;
    const hmmsort_model *models;
    int16_t *const *ml_out;
    double *ll_out;
    Options opt;
    std::vector<int> status;
    std::vector<std::string> message;
    std::atomic<bool> stop{false};
    std::atomic<int64_t> escalations{0};
    // hmmsort_fit_step_channels: per-channel records (kStepFinish) or per-channel vectors for the caller (kStepStats)
    int step_mode = kNoStep;
    const hmmsort_step_out *step_out = nullptr;
    std::vector<std::vector<double>> step_stats;
};

// channels first, first + stride, ... of the job on the current device of the calling thread
int fit_worker(FitJob &job, int64_t first, int64_t stride)
{
    std::vector<std::unique_ptr<FitChannel>> live;   // their position in `live` is their turn
    std::vector<int64_t> which;
    int64_t next = first;
    int fatal = HMMSORT_OK;
    auto retire = [&](size_t at) {
        FitChannel &ch = *live[at];
        int rc = HMMSORT_OK;
        if (ch.step_mode && ch.status == HMMSORT_OK && !ch.stepped) rc = ch.guard(ch.step_resident());
        if (!rc) rc = ch.collect();
        job.status[which[at]] = rc ? rc : ch.status;
        job.message[which[at]] = rc ? std::string(last_error()) : ch.message;
        job.escalations += ch.escalations;
        live.erase(live.begin() + at);   // signal and path buffers go before the next channel is taken
        which.erase(which.begin() + at);
        return rc;
    };
    while (!fatal && !job.stop && (next < job.C || !live.empty())) {
        while (!fatal && next < job.C && (int64_t)live.size() < job.opt.fit_streams) {
            const hmmsort_model &m = job.models[next];
            live.emplace_back(new FitChannel(job.y[next], job.sample_type, job.T, job.chunksize,
                                             {m.states, m.N, m.K, m.S, m.tr, m.R, m.mu, m.sigma}, job.opt,
                                             job.ml_out[next], &job.ll_out[next]));
            live.back()->step_mode = job.step_mode;
            if (job.step_mode == kStepFinish) live.back()->step_out = &job.step_out[next];
            if (job.step_mode == kStepStats) live.back()->step_stats = &job.step_stats[next];
            which.push_back(next);
            next += stride;
            fatal = live.back()->guard(live.back()->open());
            if (!fatal && live.back()->done) fatal = retire(live.size() - 1);
        }
        for (size_t n = 0; n < live.size() && !fatal; n++) fatal = live[n]->guard(live[n]->enqueue_chunk());
        for (size_t n = 0; n < live.size() && !fatal; n++)
            if (!live[n]->done) fatal = live[n]->guard(live[n]->finish_chunk());
        for (size_t n = live.size(); n-- > 0 && !fatal;)
            if (live[n]->done) fatal = retire(n);
    }
    if (fatal) {
        job.stop = true;
        // work of the other channels may still be in flight on their streams: wait before their buffers go
        for (auto &ch : live)
            if (ch->st) (void)hipStreamSynchronize(ch->st);
        (void)hipGetLastError();
    }
    return fatal;
}

int fit_channels_host(int64_t C, const void *const *y, int sample_type, int64_t T, int64_t chunksize,
                      const hmmsort_model *models, const int *devices, int64_t ndev, int16_t *const *ml_out,
                      double *ll_out, int *status_out, bool prefix, int step_mode = kNoStep,
                      const hmmsort_step_out *step_out = nullptr, std::vector<std::vector<double>> *step_stats = nullptr)
{
    HS_CHECK(C >= 1 && y && models && ml_out && ll_out, HMMSORT_EINVAL, "fit_channels: null argument or no channel");
    HS_CHECK(T >= 1, HMMSORT_EINVAL, "fit_channels: empty signal (T = %lld)", (long long)T);
    HS_CHECK(sample_type == HMMSORT_SAMPLES_F64 || sample_type == HMMSORT_SAMPLES_I16, HMMSORT_EINVAL,
             "fit_channels: samples must be HMMSORT_SAMPLES_F64 or HMMSORT_SAMPLES_I16");
    for (int64_t c = 0; c < C; c++)
        HS_CHECK(y[c] && ml_out[c] && models[c].states && models[c].tr && models[c].mu, HMMSORT_EINVAL,
                 "fit_channels: null pointer in channel %lld", (long long)c);
    int rc;
    if ((rc = need_device())) return rc;
    if (!devices) ndev = 0;
    HS_CHECK(ndev >= 0 && ndev <= 64, HMMSORT_EINVAL, "fit_channels: device list of %lld entries", (long long)ndev);
    int count = 0;
    HS_HIP(hipGetDeviceCount(&count));
    for (int64_t d = 0; d < ndev; d++)
        HS_CHECK(devices[d] >= 0 && devices[d] < count, HMMSORT_EINVAL, "fit_channels: no device %d", devices[d]);
    FitJob job;
    job.C = C, job.T = T, job.chunksize = chunksize, job.y = y, job.sample_type = sample_type, job.models = models;
    job.ml_out = ml_out, job.ll_out = ll_out;
    job.opt = options_get();
    job.step_mode = step_mode, job.step_out = step_out;
    if (step_mode == kStepStats) job.step_stats.resize(C);
    job.status.assign(C, HMMSORT_EHIP);
    job.message.assign(C, "fit_channels: the call stopped before this channel was decoded");
    last_escalations() = 0;
    int fatal = HMMSORT_OK;
    std::string fatal_message;
    if (ndev == 0) {
        fatal = fit_worker(job, 0, 1);
        if (fatal) fatal_message = last_error();
    } else {
        // hipSetDevice is per host thread: the workers leave the caller's current device alone
        std::vector<int> rcs(ndev, HMMSORT_OK);
        std::vector<std::string> msgs(ndev);
        std::vector<std::thread> workers;
        for (int64_t p = 0; p < ndev; p++)
            workers.emplace_back([&, p] {
                if (hipSetDevice(devices[p]) != hipSuccess) {
                    (void)hipGetLastError();
                    set_error("fit_channels: hipSetDevice(%d) failed", devices[p]);
                    rcs[p] = HMMSORT_EHIP;
                    job.stop = true;
                } else {
                    rcs[p] = fit_worker(job, p, ndev);
                }
                if (rcs[p]) msgs[p] = last_error();
            });
        for (auto &w : workers) w.join();
        for (int64_t p = ndev; p-- > 0;)
            if (rcs[p]) fatal = rcs[p], fatal_message = msgs[p];
    }
    last_escalations() = job.escalations;
    if (status_out)
        for (int64_t c = 0; c < C; c++) status_out[c] = job.status[c];
    if (fatal) {
        set_error("%s", fatal_message.c_str());
        return fatal;
    }
    for (int64_t c = 0; c < C; c++)
        if (job.status[c]) {
            if (prefix)
                set_error("channel %lld: %s", (long long)c, job.message[c].c_str());
            else
                set_error("%s", job.message[c].c_str());
            return job.status[c];
        }
    if (step_stats) *step_stats = std::move(job.step_stats);
    return HMMSORT_OK;
}

// hmmsort_fit_channels with a Viterbi-training step per channel, or one pooled step for all
int fit_step_channels_host(int64_t C, const void *const *y, int sample_type, int64_t T, int64_t chunksize,
                           const hmmsort_model *models, const int *devices, int64_t ndev, bool pooled,
                           int16_t *const *ml_out, double *ll_out, const hmmsort_step_out *out, int *status_out)
{
    HS_CHECK(C >= 1 && y && models && ll_out && out, HMMSORT_EINVAL, "fit_step_channels: null argument or no channel");
    for (int64_t c = 0; c < (pooled ? 1 : C); c++)
        HS_CHECK(out[c].mu && out[c].sigma && out[c].lp, HMMSORT_EINVAL,
                 "fit_step_channels: null pointer in record %lld", (long long)c);
    for (int64_t c = 0; c < C; c++)
        HS_CHECK(models[c].states, HMMSORT_EINVAL, "fit_step_channels: null pointer in channel %lld", (long long)c);
    const hmmsort_model &m0 = models[0];
    for (int64_t c = 1; pooled && c < C; c++)
        HS_CHECK(models[c].N == m0.N && models[c].K == m0.K && models[c].S == m0.S &&
                     !memcmp(models[c].states, m0.states, (size_t)(m0.N * m0.S) * sizeof(int16_t)),
                 HMMSORT_EINVAL, "fit_step_channels: pooled channels must share N, K, S and the state table (channel %lld "
                 "differs)", (long long)c);
    HS_CHECK(T >= 1, HMMSORT_EINVAL, "fit_channels: empty signal (T = %lld)", (long long)T);
    // a path nobody asked for still has to exist for the statistics
    std::vector<std::vector<int16_t>> own(C);
    std::vector<int16_t *> ml(C);
    for (int64_t c = 0; c < C; c++) {
        ml[c] = ml_out ? ml_out[c] : nullptr;
        if (!ml[c]) own[c].resize(T), ml[c] = own[c].data();
    }
    std::vector<std::vector<double>> stats;
    int rc = fit_channels_host(C, y, sample_type, T, chunksize, models, devices, ndev, ml.data(), ll_out, status_out, true,
                               pooled ? kStepStats : kStepFinish, out, pooled ? &stats : nullptr);
    if (rc || !pooled) return rc;
    // the vectors added in channel order; the sum is finished on the device of channel 0 with its model
    for (int64_t c = 1; c < C; c++) {
        HS_CHECK(stats[c].size() == stats[0].size(), HMMSORT_EINVAL, "fit_step_channels: channel %lld ended on a plan "
                 "whose lp' has another layout than channel 0's: its statistics do not pool", (long long)c);
        for (size_t i = 0; i < stats[0].size(); i++) stats[0][i] += stats[c][i];
    }
    int before = 0;
    HS_HIP(hipGetDevice(&before));
    if (devices && ndev > 0) HS_HIP(hipSetDevice(devices[0]));
    const Options opt = options_get();
    const ModelArgs a = {m0.states, m0.N, m0.K, m0.S, m0.tr, m0.R, m0.mu, m0.sigma};
    const int64_t n = std::min(chunksize > 0 ? chunksize : T, T);
    {
        std::unique_ptr<HostSlot> slot = take_slot(n, a, opt);
        if (!slot) slot = new_slot(n, opt);
        if (slot->plan && hmmsort_plan_set_model(slot->plan, a.tr, a.R, a.mu, a.sigma)) slot->drop_plan();
        if (!slot->plan) rc = plan_create_engine(&slot->plan, n, a.states, a.N, a.K, a.S, a.tr, a.R, a.mu, a.sigma, opt.engine);
        if (!rc && plan_path_stats_len(slot->plan) != (int64_t)stats[0].size()) {
            set_error("fit_step_channels: the finishing plan's lp' has another layout than the channels' statistics");
            rc = HMMSORT_EINVAL;
        }
        if (!rc) rc = slot->dstats.ensure(stats[0].size() * sizeof(double));
        if (!rc && hipMemcpyAsync(slot->dstats.p, stats[0].data(), stats[0].size() * sizeof(double), hipMemcpyHostToDevice,
                                  slot->st) != hipSuccess) {
            set_error("fit_step_channels: upload of the pooled statistics failed");
            (void)hipGetLastError();
            rc = HMMSORT_EHIP;
        }
        if (!rc) rc = finish_step(slot->plan, slot->dstats.as<double>(), slot->st, out[0]);
        if (slot->st) (void)hipStreamSynchronize(slot->st);   // the host vector leaves scope below
        if (!rc) give_slot(std::move(slot), opt);
    }
    if (devices && ndev > 0) (void)hipSetDevice(before);
    return rc;
}

int fit_chunked_host(const void *y, int sample_type, int64_t T, int64_t chunksize, const ModelArgs &a,
                     int16_t *ml_out, double *ll_out)
{
    HS_CHECK(y && ml_out && ll_out, HMMSORT_EINVAL, "fit_chunked: null argument");
    const hmmsort_model m = {a.states, a.N, a.K, a.S, a.tr, a.R, a.mu, a.sigma};
    return fit_channels_host(1, &y, sample_type, T, chunksize, &m, nullptr, 0, &ml_out, ll_out, nullptr, false);
}

// ---- drift tracking on top of the loop (hmmsort_fit_adaptive) -------------------------------------------------------
// The channel owns its model.  After every finished chunk it takes the path statistics of the range that chunk
// contributed (from the trim points, hence a second wait), blends them into an exponentially weighted accumulator,
// finishes the accumulator under the current model and decodes the next chunk with the result: every chunk plan is
// re-armed, the tables k_chunk_ll folds along go up again, and the ladder sees the new ModelArgs.  Nothing here runs
// for the other chunked calls.
struct AdaptiveChannel : FitChannel {
    const hmmsort_adapt ad;
    hmmsort_track *const track;
    const hmmsort_step_out *const final_model;
    std::vector<hmm_trans> tr_own;   // what the next chunk is decoded with
    std::vector<double> mu_own;
    DevBuf dacc, dnew, dfin, dcnt;
    std::vector<double> hfin;
    int64_t len = 0;                 // doubles of the statistics vector, the same for every chunk plan
    int64_t nchunks = 0, owned = 0;  // finished chunks; samples that entered the statistics, undecayed

    AdaptiveChannel(const void *y_, int type, int64_t T_, int64_t chunk, const ModelArgs &a_, const Options &o, int16_t *ml,
                    double *ll_, const hmmsort_adapt &ad_, hmmsort_track *track_, const hmmsort_step_out *fin)
        : FitChannel(y_, type, T_, chunk, a_, o, ml, ll_), ad(ad_), track(track_), final_model(fin),
          tr_own(a_.tr, a_.tr + a_.R), mu_own(a_.mu, a_.mu + a_.K * a_.N)
    {
        a.tr = tr_own.data();
        a.mu = mu_own.data();
        if (track && track->n) *track->n = 0;
    }

    // record c of the track: the chunk that started at fit.jl's i0, decoded with the current model
    void record(int64_t i0, int64_t lo, int64_t hi, double w)
    {
        const int64_t c = nchunks++;
        if (!track) return;
        if (track->n) *track->n = nchunks;
        if (c >= track->cap) return;
        if (track->first) track->first[c] = i0;
        if (track->own) track->own[2 * c] = lo, track->own[2 * c + 1] = hi;
        if (track->w) track->w[c] = w;
        if (track->mu) memcpy(track->mu + c * a.K * a.N, a.mu, a.K * a.N * sizeof(double));
        if (track->sigma) track->sigma[c] = a.sigma;
    }

    double weight(int64_t n) const { return std::exp2(-(double)n / ad.halflife); }

    // the chunk that started at i0 is finished (stitched, its ll added): its share of the statistics, and the model
    // the next chunk is decoded with.  pin still holds the chunk's trim points.
    int after_chunk(int64_t i0, bool last)
    {
        const int64_t l = pin_lk()[0], kk = pin_lk()[1];
        const int64_t lo = i0 + l - 2, hi = last ? T : i0 + kk - 2;
        HS_CHECK(0 <= lo && lo <= hi && hi <= T, HMMSORT_EINVAL, "fit_adaptive: the chunk at sample %lld owns [%lld, %lld) "
                 "of %lld samples", (long long)i0, (long long)lo, (long long)hi, (long long)T);
        const double w = weight(hi - lo);
        record(i0, lo, hi, w);
        int rc;
        const int64_t n = plan_path_stats_len(plan);
        if (!len) {
            len = n;
            if ((rc = dacc.alloc(len * sizeof(double))) || (rc = dnew.alloc(len * sizeof(double)))) return rc;
            HS_HIP(hipMemsetAsync(dacc.p, 0, len * sizeof(double), st));
        }
        HS_CHECK(n == len, HMMSORT_EUNSUP, "fit_adaptive: the plan of the chunk at sample %lld has %lld statistics, the "
                 "channel's accumulator %lld (another lp' layout): they do not blend", (long long)i0, (long long)n,
                 (long long)len);
        if ((rc = plan_path_stats(plan, dy.as<double>(), dml.as<int16_t>(), T, lo, hi, i0 == 1, dnew.as<double>(), st)) ||
            (rc = dev_stats_blend(dacc.as<double>(), w, dnew.as<double>(), len, 3, st)))
            return rc;
        owned += hi - lo;
        const bool replace = !done && owned >= ad.warmup, report = done && final_model;
        if (!replace && !report) return HMMSORT_OK;
        const int64_t KN = a.K * a.N, nlp = plan->eng->n_lp(), mlen = hmmsort_plan_mstep_len(plan);
        if ((rc = dfin.ensure(mlen * sizeof(double))) || (rc = dcnt.ensure(3 * sizeof(int64_t)))) return rc;
        if ((rc = plan_path_finish(plan, dacc.as<double>(), dfin.as<double>(), dcnt.as<int64_t>(), st))) return rc;
        hfin.resize(mlen);
        int64_t counts[3] = {0, 0, 0};
        // a replacement needs mu', sigma' and lp' only, not the S entries of pp'
        HS_HIP(hipMemcpyAsync(hfin.data(), dfin.p, (report ? mlen : KN + 1 + nlp) * sizeof(double), hipMemcpyDeviceToHost, st));
        if (report) HS_HIP(hipMemcpyAsync(counts, dcnt.p, sizeof(counts), hipMemcpyDeviceToHost, st));
        HS_HIP(hipStreamSynchronize(st));   // the second wait of this chunk
        if (report) return unpack_step(hfin.data(), counts, a.K, a.N, a.S, nlp, *final_model);
        return replace_model(hfin.data(), hfin[KN], hfin.data() + KN + 1, nlp);
    }

    int replace_model(const double *mu_new, double sigma_new, const double *lp_new, int64_t nlp)
    {
        std::copy(mu_new, mu_new + a.K * a.N, mu_own.begin());
        if (ad.update_sigma && std::isfinite(sigma_new) && sigma_new > 0.0) a.sigma = sigma_new;
        if (ad.update_lp) {
            // the rebuild after a hard step (baumwelch.jl:265 feeds xb[2:end] back as lp); entries that are not finite
            // leave the list (types.jl:121)
            const int overlaps = a.S > 1 + a.N * (a.K - 1);
            const int64_t R = hmmsort_build_transitions(a.N, a.K, lp_new, nlp, overlaps, nullptr, 0);
            if (R < 0) return (int)R;
            HS_CHECK(R >= 1, HMMSORT_EINVAL, "fit_adaptive: the re-estimated transition list is empty");
            tr_own.resize(R);
            hmmsort_build_transitions(a.N, a.K, lp_new, nlp, overlaps, tr_own.data(), R);
            a.tr = tr_own.data();
            a.R = R;
        }
        // every chunk plan of the channel; one that refuses (a list of another length on a generic plan) is made anew
        // when its chunk length comes up again
        hmmsort_plan *live = nullptr;
        for (auto &kv : slots) {
            if (!kv.second || !kv.second->plan) continue;
            if (hmmsort_plan_set_model(kv.second->plan, a.tr, a.R, a.mu, a.sigma))
                kv.second->drop_plan();
            else
                live = kv.second->plan;
        }
        plan = nullptr;
        tables = false;
        if (live) {
            int rc = upload_tables(live->model);
            if (rc) return rc;
        }
        twins = has_twins();
        return HMMSORT_OK;
    }
};

int fit_adaptive_host(const void *y, int sample_type, int64_t T, int64_t chunksize, const hmmsort_model *model,
                      const hmmsort_adapt *ad, int16_t *ml_out, double *ll_out, hmmsort_track *track,
                      const hmmsort_step_out *final_model)
{
    HS_CHECK(y && model && ad && ml_out && ll_out, HMMSORT_EINVAL, "fit_adaptive: null argument");
    HS_CHECK(model->states && model->tr && model->mu, HMMSORT_EINVAL, "fit_adaptive: null pointer in the model");
    HS_CHECK(ad->halflife > 0.0, HMMSORT_EINVAL, "fit_adaptive: halflife must be > 0 (+Inf: never forget), got %g",
             ad->halflife);
    HS_CHECK(ad->warmup >= 0, HMMSORT_EINVAL, "fit_adaptive: warmup must be >= 0, got %lld", (long long)ad->warmup);
    HS_CHECK(T >= 1, HMMSORT_EINVAL, "fit_adaptive: empty signal (T = %lld)", (long long)T);
    HS_CHECK(sample_type == HMMSORT_SAMPLES_F64 || sample_type == HMMSORT_SAMPLES_I16, HMMSORT_EINVAL,
             "fit_adaptive: samples must be HMMSORT_SAMPLES_F64 or HMMSORT_SAMPLES_I16");
    HS_CHECK(!track || track->cap >= 0, HMMSORT_EINVAL, "fit_adaptive: track of %lld records",
             (long long)(track ? track->cap : 0));
    HS_CHECK(!final_model || (final_model->mu && final_model->sigma && final_model->lp), HMMSORT_EINVAL,
             "fit_adaptive: null pointer in final_model");
    HS_CHECK(model->N >= 1 && model->K >= 1 && model->S >= 1 && model->R >= 1, HMMSORT_EINVAL,
             "fit_adaptive: need N, K, S, R >= 1");
    int rc;
    if ((rc = need_device())) return rc;
    const Options opt = options_get();
    last_escalations() = 0;
    const hmmsort_model &m = *model;
    AdaptiveChannel ch(y, sample_type, T, chunksize, {m.states, m.N, m.K, m.S, m.tr, m.R, m.mu, m.sigma}, opt, ml_out,
                       ll_out, *ad, track, final_model);
    // a recording that open() finishes (one decode, or one sample) takes its step as hmmsort_fit_step_channels does
    if (final_model) ch.step_mode = kStepFinish, ch.step_out = final_model;
    rc = ch.guard(ch.open());
    if (!rc && ch.done && ch.status == HMMSORT_OK) {
        if (T > 1) ch.record(1, 0, T, ch.weight(T));
        if (final_model && !ch.stepped) rc = ch.guard(ch.step_resident());
    }
    while (!rc && !ch.done) {
        if ((rc = ch.guard(ch.enqueue_chunk())) || ch.done) break;
        const int64_t i0 = ch.i;
        const bool last = !ch.trail;
        rc = ch.guard(ch.finish_chunk());
        if (!rc && ch.status == HMMSORT_OK) rc = ch.guard(ch.after_chunk(i0, last));
    }
    if (rc) {
        if (ch.st) (void)hipStreamSynchronize(ch.st);
        (void)hipGetLastError();
        return rc;
    }
    const std::string message = ch.message;
    rc = ch.collect();
    last_escalations() = ch.escalations;
    if (rc) return rc;
    if (ch.status) set_error("%s", message.c_str());
    return ch.status;
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

int hmmsort_fit_chunked(const double *y, int64_t T, int64_t chunksize, const int16_t *states, int64_t N,
                        int64_t K, int64_t S, const hmm_trans *tr, int64_t R, const double *mu, double sigma,
                        int16_t *ml_seq_out, double *ll_out)
{
    return fit_chunked_host(y, HMMSORT_SAMPLES_F64, T, chunksize, {states, N, K, S, tr, R, mu, sigma}, ml_seq_out,
                            ll_out);
}

int hmmsort_fit_chunked_i16(const int16_t *y, int64_t T, int64_t chunksize, const int16_t *states, int64_t N,
                            int64_t K, int64_t S, const hmm_trans *tr, int64_t R, const double *mu,
                            double sigma, int16_t *ml_seq_out, double *ll_out)
{
    return fit_chunked_host(y, HMMSORT_SAMPLES_I16, T, chunksize, {states, N, K, S, tr, R, mu, sigma}, ml_seq_out,
                            ll_out);
}

int hmmsort_fit_channels(int64_t C, const void *const *y, int sample_type, int64_t T, int64_t chunksize,
                         const hmmsort_model *models, const int *devices, int64_t ndev,
                         int16_t *const *ml_seq_out, double *ll_out, int *status_out)
{
    return fit_channels_host(C, y, sample_type, T, chunksize, models, devices, ndev, ml_seq_out, ll_out, status_out,
                             true);
}

int hmmsort_fit_step_channels(int64_t C, const void *const *y, int sample_type, int64_t T, int64_t chunksize,
                              const hmmsort_model *models, const int *devices, int64_t ndev, int pooled,
                              int16_t *const *ml_seq_out, double *ll_out, hmmsort_step_out *out, int *status_out)
{
    return fit_step_channels_host(C, y, sample_type, T, chunksize, models, devices, ndev, pooled != 0, ml_seq_out,
                                  ll_out, out, status_out);
}

int hmmsort_fit_adaptive(const void *y, int sample_type, int64_t T, int64_t chunksize, const hmmsort_model *model,
                         const hmmsort_adapt *opt, int16_t *ml_seq_out, double *ll_out, hmmsort_track *track,
                         hmmsort_step_out *final_model)
{
    return fit_adaptive_host(y, sample_type, T, chunksize, model, opt, ml_seq_out, ll_out, track, final_model);
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

// hmmsort_viterbi, then the model re-estimated from the path while signal and path are still in device memory.  The
// update runs once, in the `out` stage, on whatever path the ladder finally returned.
int hmmsort_viterbi_step(const double *y, int64_t T, const int16_t *states, int64_t N, int64_t K, int64_t S,
                         const hmm_trans *tr, int64_t R, double *mu_inout, double sigma, double *sigma_out,
                         double *lp_out, int64_t lp_cap, int64_t *n_lp_out, double *pp_out, int16_t *x_out,
                         double *ll_out)
{
    HS_CHECK(y && mu_inout && sigma_out && lp_out, HMMSORT_EINVAL, "viterbi_step: null argument");
    HS_CHECK(T >= 1, HMMSORT_EINVAL, "viterbi_step: empty signal (T = %lld)", (long long)T);
    return host_call(
        kViterbi, y, HMMSORT_SAMPLES_F64, T, {states, N, K, S, tr, R, mu_inout, sigma},
        [&](HostSlot &h) {
            int rc;
            if ((rc = h.dx.ensure(T * sizeof(int16_t))) || (rc = h.dll.ensure(sizeof(double)))) return rc;
            return h.plan->eng->viterbi(h.dy.as<double>(), h.dx.as<int16_t>(), h.dll.as<double>(), h.st);
        },
        [&](HostSlot &h) {
            int rc;
            // sized for THIS plan, as in em_step
            if ((rc = h.dout.ensure(hmmsort_plan_mstep_len(h.plan) * sizeof(double)))) return rc;
            if ((rc = hmmsort_plan_path_update(h.plan, h.dy.as<double>(), h.dx.as<int16_t>(), h.dout.as<double>(),
                                               nullptr, h.st)))
                return rc;
            if (x_out) HS_HIP(hipMemcpyAsync(x_out, h.dx.p, T * sizeof(int16_t), hipMemcpyDeviceToHost, h.st));
            if (ll_out) HS_HIP(hipMemcpyAsync(ll_out, h.dll.p, sizeof(double), hipMemcpyDeviceToHost, h.st));
            HS_HIP(hipStreamSynchronize(h.st));
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
