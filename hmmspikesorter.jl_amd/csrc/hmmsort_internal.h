// Internal declarations shared by the C ABI (capi.cpp, host_calls.cpp, analysis_calls.cpp), the host-side
// state-space code (statespace.cpp) and the device engines (generic_engine.hip, ring_engine.hip, wave_engine.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <memory>
#include <string>
#include <vector>
#include "../../include/hmmsort.h"

namespace hmmsort {

void set_error(const char *fmt, ...);
const char *last_error();

#define HS_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            hmmsort::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_),         \
                               __FILE__, __LINE__);                                           \
            return HMMSORT_EHIP;                                                              \
        }                                                                                     \
    } while (0)

#define HS_CHECK(cond, code, ...)                                                             \
    do {                                                                                      \
        if (!(cond)) {                                                                        \
            hmmsort::set_error(__VA_ARGS__);                                                  \
            return (code);                                                                    \
        }                                                                                     \
    } while (0)

// 0.5*log(2*pi)  (reference utils.jl:1); the double nearest to 0.918938533204672741780...
constexpr double kLog2Pi = 0.9189385332046727;

struct Options {
    int64_t engine = HMMSORT_ENGINE_AUTO;
    int64_t block = 0;
    int64_t halo = 0;
    int64_t escalate = 1;          // host-buffer entry points retry with a doubled warm-up
    int64_t plan_cache = 4;        // idle plans (+ device buffers) the host-buffer entry points keep
    int64_t strict_limit_mb = 0;   // largest back-pointer table the strict fallback may allocate (0 = what is free)
    int64_t tie_scale = 1;         // test aid: multiplies the wave engine's near-tie threshold (more decisions flagged)
    int64_t blocked_hbm_columns = 0;   // blocked E-step / posteriors with the state columns in device memory: 0, 1, 2
    int64_t tie_debug = 0;         // test aids: 1 the resolver folds the exact prefix to the end, 2 resolver off
    int64_t fit_streams = 4;       // hmmsort_fit_channels: channels one worker keeps in flight, each on its own stream
    int64_t cert_rounds = 0;       // test aid: 1 the wave decode runs every certificate round in full (0: a round that repeats nothing returns at once)
    int64_t interior = 1;          // test aid: 0 the wave engine's sweeps run every super-step in the general form (no interior range)
    int64_t backtrace = 0;         // wave engine's backtrace kernel: 0 auto (light beside an E-step, register rows alone), 1 register rows, 2 light
};
// process-wide options behind a mutex: entry points work on a snapshot taken when they start
Options options_get();
void options_modify(const std::function<void(Options &)> &f);
int64_t &last_escalations();       // per host thread: retries of its last host-buffer call

// ---- host-side model -----------------------------------------------------------------------
// Ring structure of a no-overlap model (reference types.jl:94-113 with allow_overlaps=false):
// N rings of L = K-1 states through one silent state.  All log-probabilities are taken from the
// caller's transition list, not recomputed.
struct RingModel {
    bool valid = false;
    int N = 0, L = 0;
    double c00 = 0;                 // silent -> silent
    std::vector<double> c0;         // [a]      silent -> (a,1)
    std::vector<double> cint;       // [a*L+k]  (a,k) -> (a,k+1), k = 1..L-1 (index k; [a*L+0] unused)
    std::vector<double> cend;       // [a]      (a,L) -> silent
    std::vector<double> cx;         // [a*N+b]  (a,L) -> (b,1), b != a
};

struct HostModel {
    int64_t N = 0, K = 0, S = 0, R = 0;
    std::vector<int16_t> states;    // N x S, 1-based
    std::vector<hmm_trans> tr;      // reference order
    std::vector<double> mu;         // K x N
    double sigma = 0;
    std::vector<double> mean;       // per-state mean, accumulated from 0.0 in neuron order
    // CSR by destination (incoming, list order kept) and by source (outgoing, list order)
    std::vector<int32_t> in_ptr, in_src;
    std::vector<double> in_lp;
    std::vector<int32_t> out_ptr, out_dst;
    std::vector<double> out_lp;
    RingModel ring;
};

int build_host_model(HostModel &m, const int16_t *states, int64_t N, int64_t K, int64_t S,
                     const hmm_trans *tr, int64_t R, const double *mu, double sigma);
int analyze_ring(const HostModel &m, RingModel &ring);
// trough state value of template i: indmin(mu[:,i]) + 1, first minimum (extraction.jl:18)
inline int32_t trough_value(const double *mu, int64_t K, int64_t i)
{
    int64_t q = 0;
    for (int64_t k = 1; k < K; k++)
        if (mu[k + K * i] < mu[q + K * i]) q = k;
    return (int32_t)(q + 1);
}
// largest table the strict engine may allocate: option "strict_limit_mb", 0 = 0.9 x the free device memory
inline double strict_limit_bytes(const Options &opt)
{
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
    return opt.strict_limit_mb > 0 ? (double)opt.strict_limit_mb * 1048576.0 : 0.9 * (double)free_b;
}

struct DevBuf {  // RAII device buffer of the host side
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    int alloc(size_t bytes)
    {
        release();
        bytes = bytes < 8 ? 8 : bytes;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("hipMalloc of %zu bytes failed", bytes);
            p = nullptr;
            return HMMSORT_ENOMEM;
        }
        cap = bytes;
        return HMMSORT_OK;
    }
    // cached buffers of a host slot: keep when large enough, else replace (a re-armed or rebuilt plan may
    // need more: blocked statistics grow with the finite entry transitions, a wave plan needs 3NL+N+4)
    int ensure(size_t bytes) { return (p && cap >= (bytes < 8 ? 8 : bytes)) ? HMMSORT_OK : alloc(bytes); }
    template <typename Tv> Tv *as() { return static_cast<Tv *>(p); }
};

// ---- what a plan runs on ---------------------------------------------------------------------
// One virtual per operation the C ABI forwards (capi.cpp) or a host-buffer entry point runs (host_calls.cpp).
// The default of an operation an engine does not serve is the refusal the ABI documents, so each such sentence
// exists here and nowhere else.  Implementations: wave_engine.hip, ring_engine.hip, generic_engine.hip (strict and
// blocked); the only code that names one is plan creation (capi.cpp).
class Engine {
public:
    const int64_t id;  // HMMSORT_ENGINE_*
    explicit Engine(int64_t id_) : id(id_) {}
    virtual ~Engine() = default;
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;

    // new numbers for a plan of the same shape (channel 0 unless the plan is batched)
    virtual int set_model(int64_t channel, const HostModel &m) = 0;
    // Ring models only.  Such an engine takes the list apart into junction constants, so a list that has lost the
    // entry transitions of a vanished template (types.jl:121 keeps finite entries only) fits the same plan.
    virtual bool ring_models_only() const { return false; }
    virtual void geometry(int64_t *block, int64_t *halo, int64_t *nchains) const = 0;
    virtual int64_t workspace_bytes() const = 0;
    virtual int bind(const double *, hipStream_t) { return HMMSORT_OK; }
    virtual void unbind() {}
    virtual int viterbi(const double *d_y, int16_t *d_x, double *d_ll, hipStream_t st) = 0;
    virtual int decode_estep(const double *, int16_t *, double *, double *, hipStream_t)
    {
        return refuse(HMMSORT_EUNSUP, "plan_decode_estep: needs the wave or ring engine");
    }
    virtual int64_t stats_len() const { return 0; }   // 0: no sufficient-statistics E-step for this plan
    bool has_estep() const { return stats_len() > 0; }
    virtual int estep(const double *, double *, hipStream_t)
    {
        return refuse(HMMSORT_EUNSUP, "plan_estep: sufficient-statistics E-step needs the wave, ring or blocked "
                                      "engine (use hmmsort_em_step)");
    }
    virtual int mstep(const double *, double *, hipStream_t)
    {
        return refuse(HMMSORT_EUNSUP, "plan_mstep: needs the wave, ring or blocked engine");
    }
    virtual int64_t n_lp() const = 0;   // entry log-probabilities in the M-step's output
    virtual int set_shard(int64_t, int64_t, bool, bool)
    {
        return refuse(HMMSORT_EUNSUP, "plan_set_shard: needs the wave or ring engine");
    }
    virtual int diagnostics(hipStream_t, int64_t[8]) { return HMMSORT_OK; }
    virtual int tie_stats(hipStream_t, int64_t[8]) { return HMMSORT_OK; }
    virtual int profile(int) { return HMMSORT_OK; }
    virtual int profile_read(hipStream_t, std::vector<std::string> &, std::vector<double> &, std::vector<int64_t> &)
    {
        return HMMSORT_OK;
    }
    // posteriors of the plan's model m; the results of the last call serve the four operations after it
    virtual bool has_posteriors() const { return false; }
    virtual int posteriors(const HostModel &, const double *, double *, double *, double *, double *, hipStream_t)
    {
        set_error("plan_posteriors: needs a wave plan (ring models), a blocked plan (overlap models within the LDS "
                  "limit) or a strict plan (any model); this plan runs engine %lld", (long long)id);
        return HMMSORT_EUNSUP;
    }
    virtual bool posteriors_valid() const { return false; }
    virtual int posterior_decode(int16_t *, hipStream_t)
    {
        return refuse(HMMSORT_EINVAL, "plan_posterior_decode: call hmmsort_plan_posteriors first");
    }
    // confidences of n events of template a on channel ch (1-based times in device memory, trough value qv)
    virtual int spike_conf(int, int, int, int64_t, const int64_t *, int64_t, double *, hipStream_t)
    {
        return refuse(HMMSORT_EINVAL, "plan_spike_confidence: call hmmsort_plan_posteriors first");
    }
    virtual int expected_counts(double *, hipStream_t)
    {
        return refuse(HMMSORT_EINVAL, "plan_expected_counts: call hmmsort_plan_posteriors first");
    }
    virtual int64_t overlap_sweep() const { return 0; }   // 0 generic sweeps, 2 pair sweep, 3..5 multi sweep
    // switch the structure-exploiting overlap sweep off for this plan; false: none was in use
    virtual bool drop_structured_sweep() { return false; }
    // materialised S x T sweeps and the reference's update() on them: the strict engine's job
    virtual int forward(const double *, double *, hipStream_t) { return refuse(HMMSORT_EUNSUP, "forward: needs the strict engine"); }
    virtual int backward(const double *, double *, hipStream_t) { return refuse(HMMSORT_EUNSUP, "backward: needs the strict engine"); }
    virtual int update(const double *, const double *, const double *, double *, hipStream_t)
    {
        return refuse(HMMSORT_EUNSUP, "update: needs the strict engine");
    }
    // debugging aids outside the documented ABI
    virtual int debug_record(double *) { return refuse(HMMSORT_EINVAL, "plan_debug_record: needs a wave plan"); }
    virtual int debug_array(int, double *, int64_t) { return refuse(HMMSORT_EINVAL, "plan_debug_array: needs a wave plan"); }

protected:
    static int refuse(int code, const char *msg)
    {
        set_error("%s", msg);
        return code;
    }
    // what every engine that takes a time shard asks of it first
    static int check_shard(int64_t T, int64_t own_lo, int64_t own_hi, bool first, bool last)
    {
        HS_CHECK(own_lo >= 0 && own_lo <= own_hi && own_hi <= T, HMMSORT_EINVAL,
                 "plan_set_shard: owned range [%lld, %lld) outside [0, %lld]", (long long)own_lo,
                 (long long)own_hi, (long long)T);
        HS_CHECK((!first || own_lo == 0) && (!last || own_hi == T), HMMSORT_EINVAL,
                 "plan_set_shard: a first/last shard must own its first/last sample");
        return HMMSORT_OK;
    }
};

// engines behind the interface, for plan creation.  generic: strict, or blocked with option "blocked_hbm_columns"
// as it stands now (fixed for the life of the plan)
bool wave_supported(const HostModel &m, int64_t T, std::string *why);
int wave_engine_create(std::unique_ptr<Engine> *out, const std::vector<HostModel> &models, int64_t T,
                       int64_t block_req, int64_t halo_req);
int ring_engine_create(std::unique_ptr<Engine> *out, const HostModel &m, int64_t T, int64_t block_req,
                       int64_t halo_req);
int generic_engine_create(std::unique_ptr<Engine> *out, const HostModel &m, int64_t T, bool blocked = false,
                          int64_t block_req = 0, int64_t halo_req = 0, int64_t hbm_columns = 0);

// ---- device engines ------------------------------------------------------------------------
struct GenericDev;  // generic_engine.hip
struct RingDev;     // ring_engine.hip
struct PathUpdateDev;  // path_update.hip
struct PathStatsDev;   // path_update.hip

// generic (strict) engine: single sequential sweep in the reference's operation order
// blocked = time-parallel Viterbi over blocks with a certified warm-up (generic_blocked.hip)
int generic_create(GenericDev **g, const HostModel &m, int64_t T, bool blocked = false,
                   int64_t block_req = 0, int64_t halo_req = 0);
// two-template overlap models: the blocked engine's structure-exploiting sweep (pair_sweep.hip) is in use /
// switch it off for this plan (host fallback to the generic blocked sweep when a near-tie is flagged on the path)
bool generic_pair_active(const GenericDev *g);
void generic_pair_disable(GenericDev *g);
int64_t generic_overlap_sweep(const GenericDev *g);   // 0 generic sweeps, 2 pair sweep, 3..5 multi sweep
int64_t blocked_min_samples();
int generic_set_model(GenericDev *g, const HostModel &m);
void generic_destroy(GenericDev *g);
int generic_viterbi(GenericDev *g, const double *d_y, int16_t *d_x, double *d_ll,
                    hipStream_t st);
int generic_forward(GenericDev *g, const double *d_y, double *d_alpha, hipStream_t st);
int generic_backward(GenericDev *g, const double *d_y, double *d_beta, hipStream_t st);
// update() on device from materialised alpha/beta; d_out = [mu K*N | sigma | lp (nsrc1-1) | pp S]
int generic_update(GenericDev *g, const double *d_alpha, const double *d_beta, const double *d_y,
                   double *d_out, hipStream_t st);
// smoothed posteriors from materialised alpha/beta (generic_post.hip): per sample, gamma reduced over the state
// table into onset / occ / trough-state mass (N x T each), silent (T), arg-max state (1-based) and logz
int generic_posteriors(const double *d_alpha, const double *d_beta, int64_t T, int64_t S, int64_t N,
                       const int16_t *d_states, const int32_t *d_qv, double *d_logz, double *d_onset,
                       double *d_occ, double *d_silent, double *d_tq, int16_t *d_xm, hipStream_t st);
// time-parallel E-step of the blocked generic engine (generic_estep.hip; its calls are in generic_dev.h): sufficient
// statistics without S x T arrays.  stats = [G0 (S) | G1 (S) | X (n_lp + 1) | Gamma0 | sum y^2]
bool blocked_estep_supported(const GenericDev *g);
// option "blocked_hbm_columns" (0 off, 1 models the LDS test refuses, 2 every model), fixed when the plan is created
void blocked_set_hbm_columns(GenericDev *g, int64_t v);
// the E-step's sweep with the per-sample marginals kept (generic_estep.hip, bes_block_post): onset, occ, tq [N][T],
// silent [T], arg-max state xm [T], logz; d_occ, d_silent and d_logz may be null.  trough: N phases (host)
bool blocked_post_supported(const GenericDev *g);
int blocked_posteriors(GenericDev *g, const double *d_y, const int32_t *trough, double *d_onset, double *d_occ,
                       double *d_silent, double *d_tq, int16_t *d_xm, double *d_logz, hipStream_t st);

// ring (time-parallel) engine
int ring_create(RingDev **r, const HostModel &m, int64_t T, int64_t block_req, int64_t halo_req);
int ring_set_model(RingDev *r, const HostModel &m);
void ring_destroy(RingDev *r);
int ring_diagnostics(RingDev *r, hipStream_t st, int64_t diag[8]);
bool ring_supported(const HostModel &m, int64_t T, std::string *why);

// misc device helpers (generic_engine.hip)
int dev_reconstruct(const int16_t *d_x, int64_t T, const int16_t *d_states, int64_t N, int64_t S,
                    const double *d_mu, int64_t K, double *d_out, hipStream_t st);
// the same under a model track: sample t takes the templates of the last chunk whose 1-based first sample is <= t + 1
// (d_first: nchunks <= kTrackChunks ascending values, d_mu_track: [nchunks][K*N])
constexpr int64_t kTrackChunks = 8192;
int dev_reconstruct_tracked(const int16_t *d_x, int64_t T, const int16_t *d_states, int64_t N, int64_t S, int64_t K,
                            int64_t nchunks, const int64_t *d_first, const double *d_mu_track, double *d_out,
                            hipStream_t st);
int dev_widen(const void *d_in, int dtype, int64_t T, int64_t stride, double *d_out, hipStream_t st);
constexpr int kSpikeChunkHost = 4096;
int dev_spike_compact(const int16_t *d_x, int64_t T, const uint32_t *d_match, int N, int S, int pass,
                      int64_t *d_cnt, const int64_t *d_offs, int64_t *d_times, int64_t cap,
                      hipStream_t st);
int dev_unroll(const int16_t *d_x, int64_t T, const int16_t *d_states, int64_t N, int64_t S,
               int16_t *d_out, hipStream_t st);
// chunked decode (chunk_stitch.hip): the stitch rule of fit.jl:24-36 on a decoded chunk (hmmsort_chunk_stitch), and
// p[0..n) = v for the path's initial ones
int dev_chunk_stitch(const int16_t *d_x, int64_t k, bool lead, bool trail, int16_t *d_dst, int64_t *d_lk,
                     hipStream_t st);
int dev_fill_i16(int16_t *d_p, int64_t n, int16_t v, hipStream_t st);
// d_ll[0] = viterbi.jl:92-96 along the decoded chunk d_x[0..k) in the reference's operation order, bit for bit;
// mean / in_* as in HostModel, d_pv: k doubles of scratch
int dev_chunk_ll(const double *d_y, const int16_t *d_x, int64_t k, int64_t S, const double *d_mean,
                 const int32_t *d_in_ptr, const int32_t *d_in_src, const double *d_in_lp, double sigma, double *d_pv,
                 double *d_ll, hipStream_t st);
// posterior helpers (wave_post.hip): sum_{|d| <= J} src[t + d - shift] (head[-index] for a negative index when
// head is given, 0 otherwise and outside [0, T)), capped at 1; sums over time of n rows of length T
constexpr int kPostParts = 256;
int dev_spike_conf(const double *d_src, const double *d_head, int64_t T, int64_t shift, int64_t jitter,
                   const int64_t *d_times, int64_t n, double *d_conf, hipStream_t st);
int dev_row_sums(const double *d_rows, int64_t nrows, int64_t T, double *d_part, double *out_host, hipStream_t st);
// per-spike fit (spike_fit.hip; rules in its header and include/hmmsort.h): the events d_times [N][dcap] (1-based,
// ascending, counts[a] <= dcap of them per template, trough values qv) of the path d_x of d_y under the templates d_M
// ([K*N], or with nchunks > 0 the track [nchunks][K*N] with chunk starts d_first) into the per-event arrays
// [N][dcap] and d_summary [N][spike_fit_len(K)] (slot 7 left 0.0 for the caller).  d_part: N x spike_fit_blocks(max
// count) x spike_fit_len(K) doubles of scratch.  Nothing is launched when no template has an event.
inline int64_t spike_fit_len(int64_t K) { return 8 + 3 * (K - 1); }
inline int64_t spike_fit_blocks(int64_t n) { return (n + 255) / 256; }
int dev_spike_fit(const double *d_y, const int16_t *d_x, int64_t T, const int16_t *d_states, int64_t N, int64_t S,
                  int64_t K, const double *d_M, int64_t nchunks, const int64_t *d_first, const int64_t *d_times,
                  int64_t dcap, const int64_t *counts, const int32_t *qv, double *d_amp, double *d_rss,
                  double *d_energy, int32_t *d_nused, int32_t *d_chunk, double *d_part, double *d_summary,
                  hipStream_t st);
// correlograms (correlogram.hip; rules in include/hmmsort.h): ccg_check is what both entry points refuse about U, the
// options and the output record before any GPU work.  dev_correlograms takes the U lists concatenated in device memory
// (d_times, offs[u] .. offs[u + 1] with offs a host array of U + 1 ascending entries; every list strictly ascending),
// fills the caller's host arrays and synchronises st.  Nothing beyond offs[U] entries of d_times is read.
int ccg_check(const char *who, int64_t U, const hmmsort_ccg_opt *opt, const hmmsort_ccg_out *out);
int dev_correlograms(int64_t U, const int64_t *d_times, const int64_t *offs, const hmmsort_ccg_opt *opt,
                     const hmmsort_ccg_out *out, hipStream_t st);
// footprints (footprint.hip; rules in include/hmmsort.h): fp_check is what the three entry points refuse about the
// sizes, the options and the output record before any GPU work (*M_out: the slots per unit, C without a table).
// dev_footprints takes the resident fp64 block and the U lists as dev_correlograms does (offs already checked), fills
// the caller's host arrays and synchronises st.  Every read is guarded by the window rule, so the times need not be
// checked: nothing outside d_y[0 .. C T) and d_times[offs[0] .. offs[U]) is read.
int fp_check(const char *who, int64_t C, int64_t T, int64_t U, const hmmsort_fp_opt *opt, const hmmsort_fp_out *out,
             int64_t *M_out);
int dev_footprints(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times, const int64_t *offs,
                   const hmmsort_fp_opt *opt, const hmmsort_fp_out *out, hipStream_t st);
// features and isolation (features.hip; rules in include/hmmsort.h).  feat_check is what the three feature entry points
// refuse before any GPU work and the sizes that follow (M slots, P components per slot, F = M P); feat_check_rows the
// one refusal that needs the number of rows.  dev_snippet_features takes the block and lists as dev_footprints does,
// d_feat / d_used device memory or null, fills the host arrays of `out` (its feat / used are not read) and
// synchronises st.  iso_check / dev_cluster_isolation: the same split for the isolation; `scored` is per unit.
struct FeatDims {
    int64_t M, P, F;
};
int feat_check(const char *who, int64_t C, int64_t T, int64_t U, const hmmsort_feat_opt *opt,
               const hmmsort_feat_out *out, FeatDims *d);
int feat_check_rows(const char *who, int64_t n_total, int64_t F);
int dev_snippet_features(const double *d_y, int64_t C, int64_t T, int64_t U, const int64_t *d_times,
                         const int64_t *offs, const hmmsort_feat_opt *opt, const hmmsort_feat_out *out,
                         const FeatDims &dm, double *d_feat, unsigned char *d_used, hipStream_t st);
int iso_check(const char *who, int64_t n, int64_t F, int64_t U, const int64_t *offs, const double *mu,
              const double *vinv, const hmmsort_iso_out *out, std::vector<unsigned char> *scored);
int dev_cluster_isolation(const double *d_feat, int64_t n, int64_t F, int64_t U, const int64_t *offs,
                          const unsigned char *d_used, const double *mu, const double *vinv,
                          const std::vector<unsigned char> &scored, const hmmsort_iso_out *out, hipStream_t st);
// unit stability (stability.hip; rules in include/hmmsort.h).  stab_check is what the three entry points refuse about U,
// the options and the output record before any GPU work (*B: the time bins).  dev_unit_stability takes the U lists of
// times and values (d_vals null: counts only) concatenated in device memory behind the host offsets, as
// dev_correlograms does, fills the caller's host arrays and synchronises st.
int stab_check(const char *who, int64_t U, const hmmsort_stab_opt *opt, const hmmsort_stab_out *out, int64_t *B);
int dev_unit_stability(int64_t U, const int64_t *d_times, const double *d_vals, const int64_t *offs,
                       const hmmsort_stab_opt *opt, const hmmsort_stab_out *out, int64_t B, hipStream_t st);

}  // namespace hmmsort

// ---- plans (capi.cpp) and the host-buffer entry points on top of them (host_calls.cpp) ---------
struct hmmsort_plan {
    hmmsort::HostModel model;
    std::vector<hmmsort::HostModel> models;   // per-channel models of a wave plan (models[0] == model)
    int64_t T = 0;
    int64_t C = 1;                            // channels (batched wave plans)
    std::unique_ptr<hmmsort::Engine> eng;     // its id is the engine the plan runs on
    bool sharded = false;                     // hmmsort_plan_set_shard left the plan with part of a recording
    // path update (path_update.hip): lookup tables of the current model(s) and workspace, made when first needed;
    // stale after hmmsort_plan_set_model
    std::shared_ptr<hmmsort::PathUpdateDev> pu;
    bool pu_stale = true;
    // the same for the statistics form (hmmsort_plan_path_stats / _finish); its workspace grows with the arrays
    std::shared_ptr<hmmsort::PathStatsDev> ps;
    bool ps_stale = true;
};

namespace hmmsort {
int need_device();
// the plan engine_req asks for under the current options; halo_req >= 0 overrides option "halo"
int plan_create_engine(hmmsort_plan **out, int64_t T, const int16_t *states, int64_t N, int64_t K, int64_t S,
                       const hmm_trans *tr, int64_t R, const double *mu, double sigma, int64_t engine_req,
                       int64_t halo_req = -1);
struct PlanGuard {
    hmmsort_plan *p = nullptr;
    ~PlanGuard() { if (p) hmmsort_plan_destroy(p); }
};
// the model re-estimated from the path d_x of d_y (path_update.hip): d_out as hmmsort_plan_mstep writes it, d_counts
// three device int64 per channel or null; enqueued on st
int plan_path_update(hmmsort_plan *p, const double *d_y, const int16_t *d_x, double *d_out, int64_t *d_counts,
                     hipStream_t st);
// the additive form (path_update.hip): the statistics of samples [own_lo, own_hi) of arrays of length T (per channel
// plan_path_stats_len doubles), the finish of such a vector with the plan's current model into d_out / d_counts as
// above, and out = parts[0] + parts[1] + ... in that order for nparts vectors of len doubles
int64_t plan_path_stats_len(const hmmsort_plan *p);
int plan_path_stats(hmmsort_plan *p, const double *d_y, const int16_t *d_x, int64_t T, int64_t own_lo, int64_t own_hi,
                    bool first, double *d_stats, hipStream_t st);
int plan_path_finish(hmmsort_plan *p, const double *d_stats, double *d_out, int64_t *d_counts, hipStream_t st);
int dev_stats_sum(const double *d_parts, int64_t nparts, int64_t len, double *d_out, hipStream_t st);
// acc[i] = w * acc[i] + new[i] in two rounded steps for i < len - plain_tail, acc[i] += new[i] for the rest
int dev_stats_blend(double *d_acc, double w, const double *d_new, int64_t len, int64_t plain_tail, hipStream_t st);
// radix select (radix_select.hip): `slots` exact order statistics side by side.  Slot s selects among n keys -- the
// patterns of |d_y[s * stride + i]|, or d_keys[s * stride + i] when d_keys is given; stride 0: every slot reads the
// same array -- with `blocks` histogram workgroups per slot.  d_st holds the ranks and zero prefixes on entry, the
// selected keys and the ranks among equal keys on return; d_hist: slots * kSelBins zeros, zeros again on return.
// Everything is enqueued on st.  sel_sigmas: the noise scale of n selected lower medians, pattern as a double over the
// upper quartile of the normal distribution -- the one rule of hmmsort_seed_templates and hmmsort_noise_scale_device.
struct RadixSel {   // one select in flight: the key's leading digits found so far, and the rank among what matches them
    unsigned long long prefix;
    long long rank;
};
constexpr int kSelBins = 2048;      // 11-bit digits: 8 KB of LDS counters per workgroup
__device__ __forceinline__ unsigned long long sel_key(double v)   // the 63-bit pattern of |v|
{
    return (unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffULL;
}
int dev_radix_select(const double *d_y, const unsigned long long *d_keys, int64_t stride, int64_t n, int slots,
                     int blocks, RadixSel *d_st, unsigned long long *d_hist, hipStream_t st);
void sel_sigmas(const RadixSel *sel, int64_t n, double *sigma);
// template seed (seed_templates.hip): the options with the defaults filled in, checked against the limits of
// include/hmmsort.h before any GPU work; then the seed of the resident signal d_y into the caller's host arrays
// (synchronises st)
struct SeedParams {
    double threshold, sigma;
    int polarity;
    int64_t align, refractory, max_iters;
};
int seed_resolve(int64_t T, int64_t N, int64_t K, const hmmsort_seed_opt *opt, const hmmsort_seed_out *out,
                 SeedParams *p);
int dev_seed_templates(const double *d_y, int64_t T, int64_t N, int64_t K, const SeedParams &p, hmmsort_seed_out *out,
                       hipStream_t st);
// front end (preprocess.hip): what both entry points refuse, before any GPU work, and the call resolved: the filter's
// half (taps null: none), the reference mode, the groups' member channels (ascending; groups in ascending id) and, in
// the host form, the rows to return.  dev_preprocess filters source channel (*rows)[r] (null: r, all C) into row r of
// d_out, applies the reference to the groups (members are row numbers) in place and synchronises st.
struct PrePlan {
    int64_t half = 0;
    const double *taps = nullptr;
    int reference = 0;
    std::vector<std::vector<int32_t>> groups;
    std::vector<int32_t> keep;
};
int pre_resolve(const char *who, const void *in, int sample_type, int layout, int64_t C, int64_t T,
                const hmmsort_pre_opt *opt, const double *out, bool host_form, PrePlan *p);
int dev_preprocess(const void *d_in, int sample_type, int layout, int64_t C, int64_t T, const PrePlan &p,
                   const std::vector<int32_t> *rows, double *d_out, hipStream_t st);
// spatial whitening (whiten.hip; rules in include/hmmsort.h).  wh_noise_check / wh_mix_check are what the entry
// points refuse before any GPU work; the check of a noise call fills in the defaults (guard, threshold).  The dev_
// functions take the resident fp64 block, fill the caller's host arrays and synchronise st.
struct NoiseParams {
    double threshold = 4.0;
    const double *thr = nullptr;
    int64_t guard = 30;
};
int wh_scale_check(const char *who, const double *y, int64_t C, int64_t T, const double *sigma);
int wh_noise_check(const char *who, const double *y, int64_t C, int64_t T, const hmmsort_noise_opt *opt,
                   const hmmsort_noise_out *out, bool host_form, NoiseParams *p);
int wh_mix_check(const char *who, const double *in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                 const double *w, const double *out);
int dev_noise_scale(const double *d_y, int64_t C, int64_t T, double *sigma, hipStream_t st);
int dev_noise_cov(const double *d_y, int64_t C, int64_t T, const NoiseParams &p, const hmmsort_noise_out *out,
                  hipStream_t st);
int dev_channel_mix(const double *d_in, int64_t C, int64_t T, int64_t R, int64_t M, const int32_t *nbr,
                    const double *w, double *d_out, hipStream_t st);
void host_slots_trim(size_t keep);   // idle plans of the host-buffer entry points: keep the newest `keep`
}  // namespace hmmsort
