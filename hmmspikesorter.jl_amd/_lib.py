"""ctypes binding of libhmmsort_hip.so (the C ABI declared in include/hmmsort.h).

There is no fallback of any kind: if the shared library is missing this module raises, and if no
HIP device is present every compute entry point returns HMMSORT_EHIP, surfaced as HmmsortError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HMMSORT_LIB", os.path.join(_HERE, "libhmmsort_hip.so"))  # override: A/B builds

# Julia Tuple{Int64,Int64,Float64} == struct hmm_trans (include/hmmsort.h)
TRANS_DTYPE = np.dtype([("src", np.int64), ("dst", np.int64), ("lp", np.float64)], align=True)
assert TRANS_DTYPE.itemsize == 24

OK, EINVAL, ENOMEM, EHIP, ENOCONV, EUNSUP, ENOSILENT = 0, -1, -2, -3, -4, -5, -6
SAMPLES_I16, SAMPLES_I32, SAMPLES_F32, SAMPLES_F64 = 0, 1, 2, 3
ENGINE_AUTO, ENGINE_STRICT, ENGINE_RING, ENGINE_BLOCKED, ENGINE_WAVE = 0, 1, 2, 3, 4
# option "blocked_hbm_columns": the blocked E-step / posteriors with their state columns in device memory.  OFF
# (default): models past the LDS limit (~9 900 states) are refused as before; AUTO: they take the device-memory
# kernels; FORCE: every blocked plan does (cross-checks).  A plan keeps the value it was created under.
OPT_BLOCKED_HBM_COLUMNS = "blocked_hbm_columns"
HBM_COLUMNS_OFF, HBM_COLUMNS_AUTO, HBM_COLUMNS_FORCE = 0, 1, 2
# option "fit_streams": channels one worker of hmmsort_fit_channels keeps in flight, each on its own stream (1..16)
OPT_FIT_STREAMS = "fit_streams"


class HmmsortError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hmmsort error %d: %s" % (code, msg))
        self.code = code


_i64, _f64, _int = C.c_int64, C.c_double, C.c_int
_vp = C.c_void_p
_pi64 = C.POINTER(C.c_int64)


class Model(C.Structure):
    """struct hmmsort_model: the model arguments of hmmsort_viterbi, one record per channel"""
    _fields_ = [("states", _vp), ("N", _i64), ("K", _i64), ("S", _i64), ("tr", _vp), ("R", _i64), ("mu", _vp),
                ("sigma", _f64)]


class StepOut(C.Structure):
    """struct hmmsort_step_out: what hmmsort_fit_step_channels returns per channel (pooled: record 0 only)"""
    _fields_ = [("mu", _vp), ("sigma", _vp), ("lp", _vp), ("lp_cap", _i64), ("n_lp", _vp), ("pp", _vp),
                ("counts", _vp)]


class Adapt(C.Structure):
    """struct hmmsort_adapt: how hmmsort_fit_adaptive forgets and when it starts to re-estimate"""
    _fields_ = [("halflife", _f64), ("warmup", _i64), ("update_sigma", _int), ("update_lp", _int)]


class Track(C.Structure):
    """struct hmmsort_track: the caller's arrays of `cap` records hmmsort_fit_adaptive fills, one per chunk"""
    _fields_ = [("cap", _i64), ("n", _vp), ("first", _vp), ("own", _vp), ("w", _vp), ("mu", _vp), ("sigma", _vp)]


class SeedOpt(C.Structure):
    """struct hmmsort_seed_opt: negative align / refractory, max_iters <= 0 and a NaN threshold ask for the defaults"""
    _fields_ = [("threshold", _f64), ("sigma", _f64), ("polarity", _int), ("align", _i64), ("refractory", _i64),
                ("max_iters", _i64)]


class SeedOut(C.Structure):
    """struct hmmsort_seed_out: host arrays hmmsort_seed_templates fills"""
    _fields_ = [("mu", _vp), ("sigma", _vp), ("lp", _vp), ("counts", _vp), ("n_events", _vp), ("iters", _vp),
                ("times", _vp), ("labels", _vp), ("cap", _i64)]


class SpikeFitOut(C.Structure):
    """struct hmmsort_spike_fit_out: host arrays hmmsort_spike_fit fills (rows of `cap` entries; counts is required)"""
    _fields_ = [("times", _vp), ("amp", _vp), ("rss", _vp), ("energy", _vp), ("nused", _vp), ("cap", _i64),
                ("counts", _vp), ("summary", _vp)]


class CcgOpt(C.Structure):
    """struct hmmsort_ccg_opt: bin width, bins on each side of lag 0, refractory period, coincidence window (samples)"""
    _fields_ = [("bin", _i64), ("half_bins", _i64), ("refractory", _i64), ("coincidence", _i64)]


class CcgOut(C.Structure):
    """struct hmmsort_ccg_out: host int64 arrays hmmsort_correlograms fills ([U][U][2H], [U], [U][U], [U]; n is
    required)"""
    _fields_ = [("ccg", _vp), ("viol", _vp), ("coinc", _vp), ("n", _vp)]


class FpOpt(C.Structure):
    """struct hmmsort_fp_opt: samples before the spike time, window length, slots per unit and the host table [U][M] of
    block channels (NULL: all C channels in order)"""
    _fields_ = [("pre", _i64), ("W", _i64), ("M", _i64), ("chan", _vp)]


class FpOut(C.Structure):
    """struct hmmsort_fp_out: host arrays hmmsort_footprints fills ([U][M][W] doubles twice, [U] int64 twice; n is
    required)"""
    _fields_ = [("sum", _vp), ("sumsq", _vp), ("nused", _vp), ("n", _vp)]


class FeatOpt(C.Structure):
    """struct hmmsort_feat_opt: the footprints' window and ONE channel row [M] for all units, the components per slot,
    the host basis [M][P][W] and centre [M][W] (each may be NULL) and the moments mode (0, 1, 2)"""
    _fields_ = [("pre", _i64), ("W", _i64), ("M", _i64), ("chan", _vp), ("P", _i64), ("basis", _vp), ("centre", _vp),
                ("moments", _i64)]


class FeatOut(C.Structure):
    """struct hmmsort_feat_out: feat / used (host arrays in the host form, device memory otherwise; cap_rows: what
    they hold, plan form), host n (required) and nused, and the host moments of mode 1 (b1, b2) or 2 (g1, g2)"""
    _fields_ = [("feat", _vp), ("used", _vp), ("cap_rows", _i64), ("n", _vp), ("nused", _vp), ("b1", _vp), ("b2", _vp),
                ("g1", _vp), ("g2", _vp)]


class IsoOut(C.Structure):
    """struct hmmsort_iso_out: host arrays hmmsort_cluster_isolation fills ([U] doubles, [U][U] int64, [U][U] doubles;
    each may be NULL)"""
    _fields_ = [("iso_d2", _vp), ("closer", _vp), ("lpair", _vp)]


class StabOpt(C.Structure):
    """struct hmmsort_stab_opt: recording length, samples per time bin, the quantiles q_num[k] / q_den, and the
    histogram (bins, left edge, 1 / bin width)"""
    _fields_ = [("T", _i64), ("bin", _i64), ("nq", _i64), ("q_num", _i64 * 8), ("q_den", _i64), ("HB", _i64),
                ("hist_lo", _f64), ("hist_scale", _f64)]


class StabOut(C.Structure):
    """struct hmmsort_stab_out: host arrays hmmsort_unit_stability fills (n is required, the others may be NULL)"""
    _fields_ = [(k, _vp) for k in ("n", "count", "valid", "quant", "sum", "sumsq", "uvalid", "uquant", "umin", "umax",
                                   "usum", "usumsq", "hist", "under", "over")]


class PreOpt(C.Structure):
    """struct hmmsort_pre_opt: half filter (taps NULL: none), reference mode, group id per channel (NULL: one group)
    and, in the host form, the rows to return (NULL: all)"""
    _fields_ = [("taps", _vp), ("half", _i64), ("reference", _int), ("group", _vp), ("keep", _vp), ("nkeep", _i64)]


class NoiseOpt(C.Structure):
    """struct hmmsort_noise_opt: threshold in noise scales (NaN: 4.0), absolute thresholds per channel (NULL: from the
    noise scale) and the guard either side of a loud sample (negative: 30)"""
    _fields_ = [("threshold", _f64), ("thr", _vp), ("guard", _i64)]


class NoiseOut(C.Structure):
    """struct hmmsort_noise_out: host arrays hmmsort_noise_cov fills (sigma may be NULL) and the optional device mask"""
    _fields_ = [("sigma", _vp), ("n_quiet", _vp), ("s1", _vp), ("s2", _vp), ("d_quiet", _vp)]


SEED_MAX_K, SEED_MAX_N, SEED_MAX_R = 1025, 16, 1024
LAYOUT_CHANNEL_MAJOR, LAYOUT_SAMPLE_MAJOR = 0, 1
REF_NONE, REF_MEDIAN, REF_MEAN = 0, 1, 2
PRE_MAX_HALF, PRE_MAX_CHANNELS, PRE_MAX_GROUP = 4096, 1024, 64
CCG_MAX_UNITS, CCG_MAX_HALF_BINS = 4096, 2048
FP_MAX_UNITS, FP_MAX_W, FP_MAX_SLOTS = 4096, 1024, 1024
WHITEN_MAX_CHANNELS, WHITEN_MAX_GUARD = 1024, 65536
FEAT_MAX_P1, FEAT_MAX_F2 = 128, 64
STAB_MAX_UNITS, STAB_MAX_Q, STAB_MAX_QDEN, STAB_MAX_HIST, STAB_MAX_BINS = 4096, 8, 1 << 20, 4096, 1 << 24

# name -> (restype, argtypes); every symbol include/hmmsort.h declares
SIGNATURES = {
    "hmmsort_last_error": (C.c_char_p, []),
    "hmmsort_version": (_int, []),
    "hmmsort_device_count": (_int, [C.POINTER(_int)]),
    "hmmsort_set_device": (_int, [_int]),
    "hmmsort_set_option": (_int, [C.c_char_p, _i64]),
    "hmmsort_get_option": (_int, [C.c_char_p, _pi64]),
    "hmmsort_shutdown": (_int, []),
    "hmmsort_generate_states": (_i64, [_i64, _i64, _int, _vp]),
    "hmmsort_build_transitions": (_i64, [_i64, _i64, _vp, _i64, _int, _vp, _i64]),
    "hmmsort_viterbi": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp]),
    "hmmsort_viterbi_i16": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp]),
    "hmmsort_fit_chunked": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp]),
    "hmmsort_fit_chunked_i16": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp]),
    "hmmsort_fit_channels": (_int, [_i64, C.POINTER(_vp), _int, _i64, _i64, C.POINTER(Model), C.POINTER(_int), _i64,
                                    C.POINTER(_vp), _vp, C.POINTER(_int)]),
    "hmmsort_fit_step_channels": (_int, [_i64, C.POINTER(_vp), _int, _i64, _i64, C.POINTER(Model), C.POINTER(_int),
                                         _i64, _int, C.POINTER(_vp), _vp, C.POINTER(StepOut), C.POINTER(_int)]),
    "hmmsort_fit_adaptive": (_int, [_vp, _int, _i64, _i64, C.POINTER(Model), C.POINTER(Adapt), _vp, _vp,
                                    C.POINTER(Track), C.POINTER(StepOut)]),
    "hmmsort_stats_blend": (_int, [_vp, _f64, _vp, _i64, _i64, _vp]),
    "hmmsort_reconstruct_tracked": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "hmmsort_chunk_stitch": (_int, [_vp, _i64, _int, _int, _vp, _vp, _vp]),
    "hmmsort_samples_to_f64": (_int, [_vp, C.c_int, _i64, _i64, _vp, _vp]),
    "hmmsort_preprocess": (_int, [_vp, _int, _int, _i64, _i64, C.POINTER(PreOpt), _vp]),
    "hmmsort_preprocess_device": (_int, [_vp, _int, _int, _i64, _i64, C.POINTER(PreOpt), _vp, _vp]),
    "hmmsort_noise_scale_device": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "hmmsort_noise_cov_device": (_int, [_vp, _i64, _i64, C.POINTER(NoiseOpt), C.POINTER(NoiseOut), _vp]),
    "hmmsort_noise_cov": (_int, [_vp, _i64, _i64, C.POINTER(NoiseOpt), C.POINTER(NoiseOut)]),
    "hmmsort_channel_mix_device": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp]),
    "hmmsort_channel_mix": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "hmmsort_seed_templates": (_int, [_vp, _int, _i64, _i64, _i64, C.POINTER(SeedOpt), C.POINTER(SeedOut)]),
    "hmmsort_seed_templates_device": (_int, [_vp, _i64, _i64, _i64, C.POINTER(SeedOpt), C.POINTER(SeedOut), _vp]),
    "hmmsort_forward": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp]),
    "hmmsort_backward": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp]),
    "hmmsort_update": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64,
                              _vp, _vp, _i64, _pi64, _vp]),
    "hmmsort_em_step": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp,
                               _i64, _pi64, _vp]),
    "hmmsort_viterbi_step": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp,
                                    _i64, _pi64, _vp, _vp, _vp]),
    "hmmsort_reconstruct": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "hmmsort_unroll_mlseq": (_int, [_vp, _i64, _vp, _i64, _i64, _vp]),
    "hmmsort_extract_spiketimes": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    "hmmsort_plan_create": (_int, [C.POINTER(_vp), _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp,
                                   _f64]),
    "hmmsort_plan_set_model": (_int, [_vp, _vp, _i64, _vp, _f64]),
    "hmmsort_plan_create_batched": (_int, [C.POINTER(_vp), _i64, _i64, _vp, _i64, _i64, _i64, _vp, _i64,
                                           _vp, _vp]),
    "hmmsort_plan_channels": (_i64, [_vp]),
    "hmmsort_plan_set_model_channel": (_int, [_vp, _i64, _vp, _i64, _vp, _f64]),
    "hmmsort_plan_destroy": (_int, [_vp]),
    "hmmsort_plan_info": (_int, [_vp, _pi64, _pi64, _pi64, _pi64, _pi64]),
    "hmmsort_plan_overlap_sweep": (_i64, [_vp]),
    "hmmsort_plan_bind": (_int, [_vp, _vp, _vp]),
    "hmmsort_plan_unbind": (_int, [_vp]),
    "hmmsort_plan_viterbi": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "hmmsort_plan_estep": (_int, [_vp, _vp, _vp, _vp]),
    "hmmsort_plan_decode_estep": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "hmmsort_plan_stats_len": (_i64, [_vp]),
    "hmmsort_plan_set_shard": (_int, [_vp, _i64, _i64, _int, _int]),
    "hmmsort_plan_mstep": (_int, [_vp, _vp, _vp, _vp]),
    "hmmsort_plan_mstep_len": (_i64, [_vp]),
    "hmmsort_plan_path_update": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "hmmsort_plan_path_stats_len": (_i64, [_vp]),
    "hmmsort_plan_path_stats": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _vp]),
    "hmmsort_plan_path_finish": (_int, [_vp, _vp, _vp, _vp, _vp]),
    "hmmsort_stats_sum": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "hmmsort_plan_diagnostics": (_int, [_vp, _vp, _pi64]),
    "hmmsort_plan_tie_stats": (_int, [_vp, _vp, _pi64]),
    "hmmsort_plan_extract_spiketimes": (_int, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "hmmsort_plan_reconstruct": (_int, [_vp, _vp, _vp, _vp]),
    "hmmsort_plan_unroll_mlseq": (_int, [_vp, _vp, _vp, _vp]),
    "hmmsort_plan_posteriors": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hmmsort_plan_posterior_decode": (_int, [_vp, _vp, _vp]),
    "hmmsort_plan_spike_confidence": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "hmmsort_plan_expected_counts": (_int, [_vp, _vp, _vp]),
    "hmmsort_posteriors": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _vp, _vp, _vp, _vp,
                                  _vp]),
    "hmmsort_spike_fit": (_int, [_vp, _int, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp,
                                 C.POINTER(SpikeFitOut)]),
    "hmmsort_plan_spike_fit": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, C.POINTER(SpikeFitOut), _vp]),
    "hmmsort_correlograms": (_int, [_i64, C.POINTER(_vp), _vp, C.POINTER(CcgOpt), C.POINTER(CcgOut)]),
    "hmmsort_plan_correlograms": (_int, [_vp, _vp, C.POINTER(CcgOpt), C.POINTER(CcgOut), _vp]),
    "hmmsort_footprints": (_int, [_vp, _int, _i64, _i64, _i64, C.POINTER(_vp), _vp, C.POINTER(FpOpt),
                                  C.POINTER(FpOut)]),
    "hmmsort_footprints_device": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.POINTER(FpOpt), C.POINTER(FpOut), _vp]),
    "hmmsort_plan_footprints": (_int, [_vp, _vp, _vp, _i64, C.POINTER(FpOpt), C.POINTER(FpOut), _vp]),
    "hmmsort_snippet_features": (_int, [_vp, _int, _i64, _i64, _i64, C.POINTER(_vp), _vp, C.POINTER(FeatOpt),
                                        C.POINTER(FeatOut)]),
    "hmmsort_snippet_features_device": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, C.POINTER(FeatOpt), C.POINTER(FeatOut),
                                               _vp]),
    "hmmsort_plan_snippet_features": (_int, [_vp, _vp, _vp, _i64, C.POINTER(FeatOpt), C.POINTER(FeatOut), _vp]),
    "hmmsort_cluster_isolation": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, C.POINTER(IsoOut)]),
    "hmmsort_cluster_isolation_device": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, C.POINTER(IsoOut), _vp]),
    "hmmsort_unit_stability": (_int, [_i64, C.POINTER(_vp), C.POINTER(_vp), _vp, C.POINTER(StabOpt),
                                      C.POINTER(StabOut)]),
    "hmmsort_unit_stability_device": (_int, [_i64, _vp, _vp, _vp, C.POINTER(StabOpt), C.POINTER(StabOut), _vp]),
    "hmmsort_plan_unit_stability": (_int, [_vp, _vp, _vp, C.POINTER(StabOpt), C.POINTER(StabOut), _vp]),
    "hmmsort_plan_profile": (_int, [_vp, _int]),
    "hmmsort_plan_profile_read": (_int, [_vp, _vp, C.c_char_p, _i64, C.POINTER(_f64), _pi64, _i64,
                                         _pi64]),
}

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libhmmsort_hip.so is not built (%s). Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C %s/csrc`; "
                "there is no CPU fallback." % (LIB_PATH, _HERE))
        # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 and fails to
        # find the GPU if the system copy (same soname) was mapped first.  Importing torch first
        # makes this library bind to the runtime torch uses; without torch the system ROCm copy
        # (RUNPATH /opt/rocm/lib) is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError here == header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def last_error():
    return lib().hmmsort_last_error().decode("utf-8", "replace")


def check(rc):
    if rc != 0:
        raise HmmsortError(rc, last_error())


def ptr(a):
    """void* of a numpy array (or None)."""
    if a is None:
        return None
    return a.ctypes.data_as(C.c_void_p)


def device_count():
    n = C.c_int(0)
    check(lib().hmmsort_device_count(C.byref(n)))
    return n.value


def set_option(key, value):
    check(lib().hmmsort_set_option(key.encode(), int(value)))


def shutdown():
    """hmmsort_shutdown: free the idle plans and device buffers the host-buffer entry points keep"""
    check(lib().hmmsort_shutdown())


def get_option(key):
    v = C.c_int64(0)
    check(lib().hmmsort_get_option(key.encode(), C.byref(v)))
    return v.value
