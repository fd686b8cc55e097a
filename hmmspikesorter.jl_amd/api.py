"""Host-side mirror of the reference's API for the hot path.

Julia is not available in the build image, so the host side above the C ABI is written in Python
with the reference's names, argument meaning and error behaviour; julia/HMMSpikeSorterHIP.jl holds
the equivalent `ccall` overrides for a Julia host.  Everything numeric happens behind
libhmmsort_hip.so on the GPU; this module only marshals arrays (column-major, 1-based ids, as
Julia lays them out).

Reference methods mirrored (file:line relative to the reference root):
  StateMatrix(N,K,lp,allow_overlaps) / StateMatrix(states,pp,K,lp)   src/types.jl:135-151
  forward / backward / update / train_model                           src/baumwelch.jl:25,73,205,311-370
  viterbi                                                             src/viterbi.jl:44
  reconstruct_signal                                                  src/reconstruction.jl:1
  unroll_mlseq                                                        src/extraction.jl:4
  fit(HMMSpikingModel, templates, X, chunksize)                       src/fit.jl:11-42
Extensions (no counterpart in the reference): posteriors, posterior_decode, spike_confidence, fit_step_channels, viterbi_step,
train_model(..., method="viterbi"), fit_adaptive, reconstruct_tracked, seed_templates, train_model(..., init="detect"),
spike_fit and unit_quality.  get_energy mirrors src/utils.jl:112-124 on the host.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import TRANS_DTYPE, HmmsortError, check, lib, ptr
from .synth import create_spike_template


@dataclass
class StateMatrix:
    """src/types.jl:1-9.  `transitions` is a structured array of (src, dst, lp) 24-byte records,
    binary-identical to Julia's Vector{Tuple{Int64,Int64,Float64}}."""
    states: np.ndarray        # N x S int16 (Fortran order), entry = 1-based row of mu
    transitions: np.ndarray   # R records, reference order
    pi: np.ndarray            # S float64, never read by the hot path
    K: int
    N: int
    nstates: int
    resolve_overlaps: bool = True

    def isempty(self):        # types.jl:13
        return self.states.size == 0

    @staticmethod
    def null():
        """StateMatrix()  types.jl:12: the null model, a single noise state"""
        tr = np.zeros(1, dtype=TRANS_DTYPE)
        tr[0] = (1, 1, 0.0)
        return StateMatrix(np.ones((1, 1), dtype=np.int16, order="F"), tr, np.array([1.0]), 0, 0, 1, False)

    @staticmethod
    def create(N, K, lp, allow_overlaps=True, pp=None):
        """StateMatrix(N, K, lp[, pp], allow_overlaps=true)  types.jl:135-146."""
        L = lib()
        S = L.hmmsort_generate_states(int(N), int(K), int(bool(allow_overlaps)), None)
        if S < 0:
            raise HmmsortError(int(S), _lib.last_error())
        states = np.zeros((N, S), dtype=np.int16, order="F")
        L.hmmsort_generate_states(int(N), int(K), int(bool(allow_overlaps)), ptr(states))
        if pp is None:
            pp = np.log(np.ones(S) / S)
        return StateMatrix.from_states(states, pp, K, lp, allow_overlaps)

    @staticmethod
    def from_states(states1, pp, K, lp, allow_overlaps=True):
        """StateMatrix(states, pp, K, lp; allow_overlaps)  types.jl:148-151, with the transition
        list produced in closed form (hmmsort_build_transitions) instead of the all-pairs scan.
        `states1` is the 1-based table (the reference passes `lA.states .- 1`, baumwelch.jl:265)."""
        L = lib()
        states1 = np.asfortranarray(states1, dtype=np.int16)
        N, S = states1.shape
        lp = np.ascontiguousarray(lp, dtype=np.float64)
        R = L.hmmsort_build_transitions(N, int(K), ptr(lp), len(lp), int(bool(allow_overlaps)),
                                        None, 0)
        if R < 0:
            raise HmmsortError(int(R), _lib.last_error())
        tr = np.zeros(R, dtype=TRANS_DTYPE)
        L.hmmsort_build_transitions(N, int(K), ptr(lp), len(lp), int(bool(allow_overlaps)),
                                    ptr(tr), R)
        return StateMatrix(states1, tr, np.array(pp, dtype=np.float64), int(K), int(N), int(S),
                           bool(allow_overlaps))


@dataclass
class HMMSpikeTemplateModel:   # types.jl:15-19
    state_matrix: StateMatrix
    mu: np.ndarray
    sigma: float


@dataclass
class HMMSpikingModel:         # types.jl:21-26
    template_model: HMMSpikeTemplateModel
    ml_seq: np.ndarray
    ll: float
    y: np.ndarray


def _model_args(lA, mu, sigma):
    mu = np.asfortranarray(mu, dtype=np.float64)
    if mu.ndim != 2 or mu.shape != (lA.K, lA.N):
        raise ValueError("mu must be K x N = %d x %d, got %s" % (lA.K, lA.N, mu.shape))
    tr = np.ascontiguousarray(lA.transitions, dtype=TRANS_DTYPE)
    st = np.asfortranarray(lA.states, dtype=np.int16)
    keep = (st, tr, mu)
    return keep, (ptr(st), lA.N, lA.K, lA.nstates, ptr(tr), len(tr), ptr(mu), float(sigma))


def _signal(y):
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 1:
        raise ValueError("signal must be one-dimensional")
    return y


def viterbi(y, lA, mu, sigma):
    """viterbi(y, lA::StateMatrix, mu, sigma) -> (x::Vector{Int16}, ll)   viterbi.jl:44-98."""
    raw = isinstance(y, np.ndarray) and y.dtype == np.int16 and y.ndim == 1
    # int16 acquisition samples cross PCIe as they are and are widened in HBM (hmmsort.jl:84-88)
    y = np.ascontiguousarray(y) if raw else _signal(y)
    keep, margs = _model_args(lA, mu, sigma)
    x = np.zeros(len(y), dtype=np.int16)
    ll = C.c_double(0.0)
    entry = lib().hmmsort_viterbi_i16 if raw else lib().hmmsort_viterbi
    check(entry(ptr(y), len(y), *margs, ptr(x), C.cast(C.byref(ll), C.c_void_p)))
    if _lib.get_option("last_escalations") < 0:
        import warnings
        warnings.warn(_lib.last_error())      # near-ties the strict sweep could not re-decide (table too large)
    return x, ll.value


def forward(V, lA, mu, sigma):
    """forward(V, lA, mu, sigma) -> alpha (S x T)   baumwelch.jl:25-51."""
    V = _signal(V)
    keep, margs = _model_args(lA, mu, sigma)
    a = np.empty((lA.nstates, len(V)), dtype=np.float64, order="F")
    check(lib().hmmsort_forward(ptr(V), len(V), *margs, ptr(a)))
    return a


def backward(V, lA, mu, sigma):
    """backward(V, lA, mu, sigma) -> beta (S x T)   baumwelch.jl:73-98."""
    V = _signal(V)
    keep, margs = _model_args(lA, mu, sigma)
    b = np.empty((lA.nstates, len(V)), dtype=np.float64, order="F")
    check(lib().hmmsort_backward(ptr(V), len(V), *margs, ptr(b)))
    return b


def _finish_step(lA, mu, sig, lp, nlp, pp):
    lp_new = lp[: nlp.value].copy()
    # baumwelch.jl:265: StateMatrix(lA.states .- 1, pp, K, xb[2:end]; allow_overlaps)
    lA_new = StateMatrix.from_states(lA.states, pp, lA.K, lp_new, lA.resolve_overlaps)
    return lA_new, mu, sig.value


def update(alpha, beta, lA, mu, sigma, x):
    """update(alpha, beta, lA, mu, sigma, x) -> (StateMatrix, mu, sigma)   baumwelch.jl:205-309.
    `mu` is overwritten in place (as the reference's fill!(mu, 0.0) does) when it is a
    Fortran-ordered float64 array; it is also returned."""
    x = _signal(x)
    alpha = np.asfortranarray(alpha, dtype=np.float64)
    beta = np.asfortranarray(beta, dtype=np.float64)
    if alpha.shape != (lA.nstates, len(x)) or beta.shape != alpha.shape:
        raise ValueError("alpha/beta must be S x T")
    mu_in = mu
    keep, margs = _model_args(lA, mu, sigma)
    st, tr, mu_f = keep
    mu_f = mu_f if mu_f is not mu_in else mu_in  # in place when the layout allows
    sig = C.c_double(0.0)
    nlp = C.c_int64(0)
    lp = np.zeros(len(tr), dtype=np.float64)
    pp = np.zeros(lA.nstates, dtype=np.float64)
    check(lib().hmmsort_update(ptr(alpha), ptr(beta), ptr(x), len(x), ptr(st), lA.N, lA.K,
                               lA.nstates, ptr(tr), len(tr), ptr(mu_f), float(sigma),
                               C.cast(C.byref(sig), C.c_void_p), ptr(lp), len(lp), C.byref(nlp),
                               ptr(pp)))
    if mu_f is not mu_in and isinstance(mu_in, np.ndarray) and mu_in.shape == mu_f.shape:
        mu_in[...] = mu_f
    return _finish_step(lA, mu_f, sig, lp, nlp, pp)


def train_step(X, state_matrix, mu0, sigma0, verbose=0):
    """train_model(X, state_matrix, mu0, sigma0) = forward -> backward -> update, one EM step
    baumwelch.jl:362-370.  One C-ABI call; alpha/beta never leave the GPU."""
    X = _signal(X)
    keep, margs = _model_args(state_matrix, mu0, sigma0)
    st, tr, mu_f = keep
    mu_f = np.array(mu_f, dtype=np.float64, order="F", copy=True) if mu_f is mu0 else mu_f
    sig = C.c_double(0.0)
    nlp = C.c_int64(0)
    lp = np.zeros(len(tr), dtype=np.float64)
    pp = np.zeros(state_matrix.nstates, dtype=np.float64)
    check(lib().hmmsort_em_step(ptr(X), len(X), ptr(st), state_matrix.N, state_matrix.K,
                                state_matrix.nstates, ptr(tr), len(tr), ptr(mu_f), float(sigma0),
                                C.cast(C.byref(sig), C.c_void_p), ptr(lp), len(lp), C.byref(nlp),
                                ptr(pp)))
    if isinstance(mu0, np.ndarray) and mu0.shape == mu_f.shape and mu0.dtype == np.float64:
        mu0[...] = mu_f  # the reference updates the caller's mu in place (baumwelch.jl:268)
    return _finish_step(state_matrix, mu_f, sig, lp, nlp, pp)


def viterbi_step(X, state_matrix, mu, sigma, return_path=False):
    """One step of Viterbi training (hard EM): decode X with the model, then re-estimate the model from the decoded
    path -- update() of baumwelch.jl:205-309 with gamma and xi the indicators of that path.  One C-ABI call
    (hmmsort_viterbi_step); signal and path stay on the GPU between the two halves.  Returns
    (state_matrix', mu', sigma'), plus the path and its log-likelihood under the OLD model with `return_path`.
    A template row no sample visits keeps its value; an entry transition the path never takes gets -Inf and
    leaves the new list (types.jl:121).  `mu` is updated in place like train_step's."""
    X = _signal(X)
    keep, margs = _model_args(state_matrix, mu, sigma)
    st, tr, mu_f = keep
    mu_f = np.array(mu_f, dtype=np.float64, order="F", copy=True) if mu_f is mu else mu_f
    sig = C.c_double(0.0)
    nlp = C.c_int64(0)
    lp = np.zeros(len(tr), dtype=np.float64)
    pp = np.zeros(state_matrix.nstates, dtype=np.float64)
    x = np.zeros(len(X), dtype=np.int16) if return_path else None
    ll = C.c_double(0.0)
    check(lib().hmmsort_viterbi_step(ptr(X), len(X), ptr(st), state_matrix.N, state_matrix.K,
                                     state_matrix.nstates, ptr(tr), len(tr), ptr(mu_f), float(sigma),
                                     C.cast(C.byref(sig), C.c_void_p), ptr(lp), len(lp), C.byref(nlp), ptr(pp),
                                     ptr(x), C.cast(C.byref(ll), C.c_void_p) if return_path else None))
    if isinstance(mu, np.ndarray) and mu.shape == mu_f.shape and mu.dtype == np.float64:
        mu[...] = mu_f
    out = _finish_step(state_matrix, mu_f, sig, lp, nlp, pp)
    return out + (x, ll.value) if return_path else out


class _EMSession:
    """EM steps on one signal that stays in HBM: the signal is uploaded once and one plan is
    re-armed with hmmsort_plan_set_model between steps (ring-engine models; anything else, a
    changed model shape or a failed warm-up certificate goes through train_step, which escalates).
    With `hard` every step is a Viterbi-training step (plan.viterbi + plan.path_update) and the signal
    stays resident for every engine; a failed boundary certificate or an open near-tie goes through
    viterbi_step, which escalates."""

    def __init__(self, X, hard=False):
        self.X = X
        self.dX = None
        self.plan = None
        self.key = None
        self.hard = hard

    def _hard_step(self, lA, mu, sigma):
        import torch
        from . import _lib
        from .device import Plan
        key = (lA.N, lA.K, lA.nstates, len(lA.transitions), lA.resolve_overlaps)
        try:
            if self.key != key or self.plan is None:
                self.close()
                self.key = key
                self.plan = Plan(len(self.X), lA, mu, sigma)
            else:
                self.plan.set_model(lA, mu, sigma)
        except _lib.HmmsortError:
            self.close()
            self.key = None
            return viterbi_step(self.X, lA, mu, sigma)
        if self.dX is None:
            self.dX = torch.from_numpy(self.X).cuda()
            self.dx = torch.zeros(len(self.X), dtype=torch.int16, device="cuda")
            self.dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        out = torch.zeros(self.plan.mstep_len(), dtype=torch.float64, device="cuda")
        self.plan.viterbi(self.dX, self.dx, self.dll)
        self.plan.path_update(self.dX, self.dx, out)
        d = self.plan.diagnostics()
        if d[0] != 0 or (self.plan.info()["engine"] in (_lib.ENGINE_BLOCKED, _lib.ENGINE_WAVE) and d[7] != 0):
            return viterbi_step(self.X, lA, mu, sigma)
        o = out.cpu().numpy()
        K, N, S = lA.K, lA.N, lA.nstates
        nlp = len(o) - K * N - 1 - S
        mu_n = np.asfortranarray(o[:K * N].reshape((K, N), order="F"))
        if isinstance(mu, np.ndarray) and mu.shape == mu_n.shape and mu.dtype == np.float64:
            mu[...] = mu_n
        lA_n = StateMatrix.from_states(lA.states, o[K * N + 1 + nlp:], K, o[K * N + 1:K * N + 1 + nlp].copy(),
                                       lA.resolve_overlaps)
        return lA_n, mu_n, float(o[K * N])

    def close(self):
        if self.plan is not None:
            self.plan.close()
            self.plan = None

    def step(self, lA, mu, sigma, verbose=0):
        if self.hard:
            return self._hard_step(lA, mu, sigma)
        import torch
        from . import _lib
        from .device import Plan
        key = (lA.N, lA.K, lA.nstates, len(lA.transitions), lA.resolve_overlaps)
        try:
            if self.key != key:                 # first step, or the model shape changed
                self.close()
                self.key = key
                self.plan = Plan(len(self.X), lA, mu, sigma)
                if self.plan.info()["engine"] not in (_lib.ENGINE_RING, _lib.ENGINE_WAVE):
                    self.close()                # remembered through self.key: not retried
            elif self.plan is not None:
                self.plan.set_model(lA, mu, sigma)
        except _lib.HmmsortError:
            self.close()
        if self.plan is None:
            return train_step(self.X, lA, mu, sigma, verbose=verbose)
        if self.dX is None:
            self.dX = torch.from_numpy(self.X).cuda()
            self.stats = torch.zeros(self.plan.stats_len(), dtype=torch.float64, device="cuda")
        out = torch.zeros(self.plan.mstep_len(), dtype=torch.float64, device="cuda")
        self.plan.estep(self.dX, self.stats)
        self.plan.mstep(self.stats, out)
        d = self.plan.diagnostics()
        if d[3] != 0 or d[5] != 0:
            return train_step(self.X, lA, mu, sigma, verbose=verbose)
        o = out.cpu().numpy()
        K, N = lA.K, lA.N
        mu_n = np.asfortranarray(o[:K * N].reshape((K, N), order="F"))
        if isinstance(mu, np.ndarray) and mu.shape == mu_n.shape and mu.dtype == np.float64:
            mu[...] = mu_n  # the reference updates the caller's mu in place (baumwelch.jl:268)
        lA_n = StateMatrix.from_states(lA.states, o[K * N + 1 + N:], K, o[K * N + 1:K * N + 1 + N],
                                       lA.resolve_overlaps)
        return lA_n, mu_n, float(o[K * N])


_SEED_OPTS = ("threshold", "sigma", "polarity", "align", "refractory", "max_iters")


def _seed_run(call, T, N, K, resolve_overlaps, opts):
    """hmmsort_seed_templates / _device through `call(opt, out)`; the part after the C ABI that both forms share:
    empty clusters are dropped and the state matrix is built from the kept entry log-probabilities."""
    bad = sorted(set(opts) - set(_SEED_OPTS))
    if bad:
        raise TypeError("seed_templates: unknown option(s) %s; known: %s" % (", ".join(bad), ", ".join(_SEED_OPTS)))
    T, N, K = int(T), int(N), int(K)
    thr = opts.get("threshold")
    opt = _lib.SeedOpt(float("nan") if thr is None else float(thr), float(opts.get("sigma") or 0.0),
                       int(opts.get("polarity") or 0), *[-1 if opts.get(k) is None else int(opts[k])
                                                         for k in ("align", "refractory", "max_iters")])
    R = opt.refractory if opt.refractory >= 0 else K - 1
    cap = T // (max(R, 0) + 1) + 1     # events are at least R + 1 apart
    mu = np.zeros((max(K, 0), max(N, 0)), order="F")
    sigma, lp, counts = np.zeros(1), np.zeros(max(N, 0)), np.zeros(max(N, 0), dtype=np.int64)
    ne, iters = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    times, labels = np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int16)
    out = _lib.SeedOut(*[a.ctypes.data for a in (mu, sigma, lp, counts, ne, iters, times, labels)], cap)
    check(call(C.byref(opt), C.byref(out)))
    E = int(ne[0])
    times, labels = times[:E].copy(), labels[:E].copy()
    info = {"n_events": E, "iters": int(iters[0]), "times": times, "raw_labels": labels,
            "raw": {"mu": mu, "lp": lp, "counts": counts}}
    kept = np.nonzero(counts > 0)[0]
    info["kept"] = kept
    info["counts"] = counts[kept].copy()
    renum = np.full(max(N, 1), -1, dtype=np.int16)
    renum[kept] = np.arange(len(kept), dtype=np.int16)
    info["labels"] = renum[labels] if E else labels
    if len(kept) == 0:
        return StateMatrix.null(), np.zeros((K, 0), order="F"), float(sigma[0]), info
    sm = StateMatrix.create(len(kept), K, lp[kept].copy(), resolve_overlaps)
    return sm, np.asfortranarray(mu[:, kept]), float(sigma[0]), info


def seed_templates(X, N=3, K=60, resolve_overlaps=False, **opts):
    """Templates from the recording alone (hmmsort_seed_templates; an extension, INTEGRATION.md "Template seed"):
    samples above `threshold` noise scales that are the extremum of their +-`refractory` window are events, the
    K - 1 samples around each (extremum at snippet index `align`) are clustered into N groups by Lloyd iterations
    started at amplitude quantiles.  Deterministic; detection and clustering run on the device.

    Options (defaults): threshold (4.0), sigma (0: the robust estimate median|X| / 0.6745), polarity (0: |X|; -1
    troughs, +1 peaks), align ((K-1)//3), refractory (K-1), max_iters (20).  X: float64 or int16 samples.

    Returns (StateMatrix, mu, sigma, info).  Empty clusters are dropped, so the model may hold fewer than N
    templates; entry log-probabilities are log(count / T).  No event at all gives StateMatrix.null() and a K x 0 mu.
    info: "counts", "times" (1-based event samples), "labels" (column of mu per event), "iters", "n_events", "kept"
    (which of the N clusters survived) and "raw" (mu, lp, counts of all N clusters, as the C ABI returns them)."""
    raw = isinstance(X, np.ndarray) and X.dtype == np.int16 and X.ndim == 1
    X = np.ascontiguousarray(X) if raw else _signal(X)
    st = _lib.SAMPLES_I16 if raw else _lib.SAMPLES_F64
    return _seed_run(lambda opt, out: lib().hmmsort_seed_templates(ptr(X), st, len(X), int(N), int(K), opt, out),
                     len(X), N, K, resolve_overlaps, opts)


def design_fir(fs, low=None, high=None, ntaps=257):
    """Linear-phase FIR filter for api.preprocess: the full, odd-length tap vector of a Hamming-windowed sinc scaled
    to unit gain, scipy.signal.firwin(ntaps, cutoffs, window="hamming", pass_zero=..., fs=fs) restated in numpy.
    `low` alone: high-pass above `low` Hz (unit gain at the Nyquist frequency); `high` alone: low-pass below `high` Hz
    (unit gain at 0 Hz); both: band-pass low..high (unit gain at the band centre)."""
    fs, ntaps = float(fs), int(ntaps)
    if low is None and high is None:
        raise ValueError("design_fir: give low (high-pass), high (low-pass) or both (band-pass)")
    if ntaps < 3 or ntaps % 2 == 0:
        raise ValueError("design_fir: ntaps = %d must be odd and at least 3" % ntaps)
    edges = np.array([f for f in (low, high) if f is not None], dtype=np.float64) / (0.5 * fs)
    if np.any(edges <= 0.0) or np.any(edges >= 1.0) or np.any(np.diff(edges) <= 0.0):
        raise ValueError("design_fir: cutoffs must lie strictly between 0 and fs / 2 = %g Hz, low below high"
                         % (0.5 * fs))
    if low is None:
        bands = [(0.0, edges[0])]
    elif high is None:
        bands = [(edges[0], 1.0)]
    else:
        bands = [(edges[0], edges[1])]
    m = np.arange(ntaps) - 0.5 * (ntaps - 1)
    h = np.zeros(ntaps)
    for left, right in bands:
        h += right * np.sinc(right * m)
        h -= left * np.sinc(left * m)
    h *= 0.54 + 0.46 * np.cos(np.linspace(-np.pi, np.pi, ntaps))           # symmetric Hamming window
    left, right = bands[0]
    gain_at = 0.0 if left == 0.0 else (1.0 if right == 1.0 else 0.5 * (left + right))
    return h / np.sum(h * np.cos(np.pi * m * gain_at))


_PRE_TYPES = {np.dtype(np.int16): _lib.SAMPLES_I16, np.dtype(np.int32): _lib.SAMPLES_I32,
              np.dtype(np.float32): _lib.SAMPLES_F32, np.dtype(np.float64): _lib.SAMPLES_F64}
_PRE_REFS = {None: _lib.REF_NONE, "none": _lib.REF_NONE, "median": _lib.REF_MEDIAN, "mean": _lib.REF_MEAN}


def _pre_opt(taps, reference, groups, keep):
    """struct hmmsort_pre_opt of api.preprocess / device.preprocess and the arrays it points into (keep them alive).
    `taps` is the full odd-length vector; its second half, centre first, is what goes over."""
    if reference not in _PRE_REFS:
        raise ValueError("preprocess: reference must be None, 'median' or 'mean' (got %r)" % (reference,))
    half = grp = kp = None
    if taps is not None:
        h = np.asarray(taps, dtype=np.float64).ravel()
        if len(h) % 2 == 0:
            raise ValueError("preprocess: taps must be the full filter of odd length (got %d)" % len(h))
        half = np.ascontiguousarray(h[len(h) // 2:])
    if groups is not None:
        grp = np.ascontiguousarray(groups, dtype=np.int32).ravel()
    if keep is not None:
        kp = np.ascontiguousarray(keep, dtype=np.int32).ravel()
    opt = _lib.PreOpt(None if half is None else half.ctypes.data, 0 if half is None else len(half) - 1,
                      _PRE_REFS[reference], None if grp is None else grp.ctypes.data,
                      None if kp is None else kp.ctypes.data, 0 if kp is None else len(kp))
    return opt, (half, grp, kp)


def preprocess(raw, taps=None, reference=None, groups=None, keep=None):
    """Front end for a raw recording block (hmmsort_preprocess; an extension, INTEGRATION.md "Front end"): a zero-phase
    FIR filter per channel (`taps`: the full odd-length symmetric vector, e.g. design_fir's; None: no filter), then a
    common reference per sample (`reference`: None, "median" or "mean") across the channels that share an id in
    `groups` (one int per channel; negative: filtered only; None: all channels in one group).  Deterministic, and
    equal bit for bit to tests/preprocess_model.py.

    raw: 1-D, or 2-D of shape (T, C) as the reference's data arrays are; int16, int32, float32 or float64 samples go
    over as they are (anything else as float64).  A C-contiguous array goes over as sample-major, a Fortran-contiguous
    one as channel-major; neither is copied.  Returns (C or len(keep), T) float64, row i being channel keep[i]."""
    raw = np.asarray(raw)
    if raw.ndim == 1:
        raw = raw[:, None]
    if raw.ndim != 2:
        raise ValueError("preprocess: raw must be 1-D or (T, C), got shape %s" % (raw.shape,))
    if raw.dtype not in _PRE_TYPES:
        raw = raw.astype(np.float64)
    if not (raw.flags.c_contiguous or raw.flags.f_contiguous):
        raw = np.ascontiguousarray(raw)
    layout = _lib.LAYOUT_SAMPLE_MAJOR if raw.flags.c_contiguous else _lib.LAYOUT_CHANNEL_MAJOR
    T, nC = raw.shape
    opt, alive = _pre_opt(taps, reference, groups, keep)
    if alive[1] is not None and len(alive[1]) != nC:
        raise ValueError("preprocess: groups has %d entries for %d channels" % (len(alive[1]), nC))
    out = np.empty((nC if keep is None else len(alive[2]), T), dtype=np.float64)
    check(lib().hmmsort_preprocess(ptr(raw), _PRE_TYPES[raw.dtype], layout, nC, T, C.byref(opt), ptr(out)))
    return out


def _noise_args(nC, threshold, guard, thr):
    """struct hmmsort_noise_opt / hmmsort_noise_out for a block of nC channels, and the arrays they point into"""
    th = None
    if thr is not None:
        th = np.ascontiguousarray(np.broadcast_to(np.asarray(thr, dtype=np.float64), (nC,)))
    opt = _lib.NoiseOpt(float("nan") if threshold is None else float(threshold), None if th is None else th.ctypes.data,
                        -1 if guard is None else int(guard))
    sigma, n = np.zeros(nC), np.zeros(1, dtype=np.int64)
    s1, s2 = np.zeros(nC), np.zeros((nC, nC))
    out = _lib.NoiseOut(sigma.ctypes.data, n.ctypes.data, s1.ctypes.data, s2.ctypes.data, None)
    return opt, out, (th, sigma, n, s1, s2)


def _noise_result(opt, alive):
    """(sigma or None, thr, n_quiet, s1, s2) of a finished noise call"""
    th, sigma, n, s1, s2 = alive
    if th is None:
        th = (4.0 if np.isnan(opt.threshold) else opt.threshold) * sigma
    else:
        sigma = None
    return sigma, th, int(n[0]), s1, s2


def _block(block, who):
    b = np.ascontiguousarray(block, dtype=np.float64)
    if b.ndim == 1:
        b = b[None, :]
    if b.ndim != 2:
        raise ValueError("%s: the block must be (C, T) float64 (1-D: one channel), got shape %s" % (who, b.shape))
    return b


def noise_sums(block, threshold=4.0, guard=30, thr=None):
    """Raw noise moments of a host block [C][T] (hmmsort_noise_cov; rules in include/hmmsort.h): the noise scale per
    channel, the mask of quiet samples (no channel beyond `threshold` noise scales, or beyond thr[c], within `guard`
    samples) and the sums over them.  Returns (sigma or None when thr is given, thr, n_quiet, s1 [C], s2 [C][C]);
    noise_covariance turns the last three into the covariance.  Equal bit for bit to tests/whiten_model.py."""
    b = _block(block, "noise_sums")
    opt, out, alive = _noise_args(b.shape[0], threshold, guard, thr)
    check(lib().hmmsort_noise_cov(ptr(b), b.shape[0], b.shape[1], C.byref(opt), C.byref(out)))
    return _noise_result(opt, alive)


def _mix_args(nbr, w, who):
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if nbr.ndim != 2 or nbr.shape != w.shape:
        raise ValueError("%s: nbr and w must both be (R, M), got %s and %s" % (who, nbr.shape, w.shape))
    return nbr, w


def channel_mix(block, nbr, w):
    """out[r] = sum over m (ascending, empty slots nbr[r][m] = -1 skipped) of w[r][m] * block[nbr[r][m]], on a host
    block [C][T] (hmmsort_channel_mix): global or local whitening, or any re-montage.  Returns (R, T) float64."""
    b = _block(block, "channel_mix")
    nbr, w = _mix_args(nbr, w, "channel_mix")
    out = np.empty((nbr.shape[0], b.shape[1]), dtype=np.float64)
    check(lib().hmmsort_channel_mix(ptr(b), b.shape[0], b.shape[1], nbr.shape[0], nbr.shape[1], ptr(nbr), ptr(w),
                                    ptr(out)))
    return out


def noise_covariance(n, s1, s2):
    """Covariance of the quiet samples from their raw sums: m = s1 / n; cov = s2 / n - outer(m, m), in that order."""
    if int(n) < 2:
        raise ValueError("noise_covariance: %d quiet samples; a covariance needs two at least (lower guard or raise "
                         "threshold)" % int(n))
    m = np.asarray(s1, dtype=np.float64) / float(n)
    return np.asarray(s2, dtype=np.float64) / float(n) - np.outer(m, m)


def _zca(cov, eps_rel):
    lam, V = np.linalg.eigh(cov)
    lam = np.maximum(lam, 0.0)
    return (V * (1.0 / np.sqrt(lam + eps_rel * lam.max()))) @ V.T


def whitening_matrix(cov, neighbors=None, eps_rel=1e-6):
    """The channel mix (nbr int32 [C][M], w [C][M]) that whitens noise of covariance `cov`.  neighbors=None: ZCA of the
    whole matrix, W = V diag(1 / sqrt(max(lam, 0) + eps_rel max(lam))) V^T with lam, V = eigh(cov), M = C.  With
    `neighbors`, the usual local whitening: per channel the ZCA of the sub-covariance of its neighbours, of which the
    row of the channel itself is kept.  neighbors is [C][M] channel ids (own channel included, -1 padding) or a pair
    (positions [C][d], M): the M nearest channels by distance, then by index."""
    cov = np.asarray(cov, dtype=np.float64)
    nC = cov.shape[0]
    if cov.shape != (nC, nC):
        raise ValueError("whitening_matrix: cov must be square, got %s" % (cov.shape,))
    if neighbors is None:
        return np.ascontiguousarray(np.tile(np.arange(nC, dtype=np.int32), (nC, 1))), _zca(cov, eps_rel)
    if isinstance(neighbors, tuple):
        pos, M = np.asarray(neighbors[0], dtype=np.float64).reshape(nC, -1), min(int(neighbors[1]), nC)
        d = np.sqrt(((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1))
        d[np.arange(nC), np.arange(nC)] = -1.0                                  # the channel itself comes first
        nbr = np.argsort(d, axis=1, kind="stable")[:, :M].astype(np.int32)
    else:
        nbr = np.array(neighbors, dtype=np.int32)
        if nbr.ndim != 2 or nbr.shape[0] != nC:
            raise ValueError("whitening_matrix: neighbors must be (C, M), got %s" % (nbr.shape,))
        if nbr.min() < -1 or nbr.max() >= nC:
            raise ValueError("whitening_matrix: a neighbour outside -1 .. C - 1")
    w = np.zeros(nbr.shape)
    for c in range(nC):
        slots = np.nonzero(nbr[c] >= 0)[0]
        ids = nbr[c, slots]
        own = np.nonzero(ids == c)[0]
        if len(own) != 1 or len(set(ids.tolist())) != len(ids):
            raise ValueError("whitening_matrix: neighbors[%d] must hold channel %d once and no channel twice" % (c, c))
        w[c, slots] = _zca(cov[np.ix_(ids, ids)], eps_rel)[own[0]]
    return np.ascontiguousarray(nbr), w


class Whitening:
    """What api.whiten estimated and applied: the noise scale `sigma` per channel (None when thresholds were given),
    the thresholds `thr` and `guard` of the quiet mask, `n_quiet`, the raw sums `s1`, `s2`, the covariance `cov` and the
    channel mix (`nbr`, `w`)."""

    def __init__(self, sigma, thr, guard, n_quiet, s1, s2, cov, nbr, w):
        self.sigma, self.thr, self.guard, self.n_quiet = sigma, thr, guard, n_quiet
        self.s1, self.s2, self.cov, self.nbr, self.w = s1, s2, cov, nbr, w

    @property
    def matrix(self):
        """the mix as a dense [C][C] matrix (repeated slots add)"""
        nC = self.nbr.shape[0]
        W = np.zeros((nC, nC))
        r, m = np.nonzero(self.nbr >= 0)
        np.add.at(W, (r, self.nbr[r, m]), self.w[r, m])
        return W

    def apply(self, block):
        """the mix on a host block [C][T] (api.channel_mix)"""
        return channel_mix(block, self.nbr, self.w)

    def scale_templates(self, mu, channel):
        """templates that live on `channel` alone and were learned before whitening, as they appear on the whitened
        channel: mu times the weight of the channel's own slot"""
        own = self.w[channel][self.nbr[channel] == channel].sum()
        return np.asarray(mu, dtype=np.float64) * own

    def as_dict(self):
        """the "whitening" entry of sort_data's and learn_templates' output"""
        return {"nbr": self.nbr, "w": self.w, "sigma": np.zeros(0) if self.sigma is None else self.sigma,
                "n_quiet": self.n_quiet}


def whiten(block, threshold=4.0, guard=30, thr=None, neighbors=None, eps_rel=1e-6, whitening=None):
    """Spatial whitening of a host block [C][T] (an extension, INTEGRATION.md "Front end"): one upload, the noise
    scale, quiet mask, sums and the channel mix on the device (device.whiten), the C x C matrix on the host in between,
    one download.  Returns (out [C][T], Whitening).  A given `whitening` is applied as it is, nothing is estimated."""
    import torch
    from . import device
    b = _block(block, "whiten")
    d = torch.from_numpy(b).cuda()
    d, wh = device.whiten(d, threshold, guard, thr, neighbors, eps_rel, whitening, inplace=True)
    return d.cpu().numpy(), wh


def train_model(X, *args, callback=None, verbose=0, p0=None, rng=None, postprocess="reference",
                method="baum-welch", init="random", seed_options=None):
    """The three `train_model` methods of baumwelch.jl:

      train_model(X, state_matrix, mu0, sigma0)                  one EM step         :362-370
      train_model(X, state_matrix, mu, sigma, nsteps[, callback]) EM loop             :324-354
      train_model(X, N=3, K=60, resolve_overlaps=False, nsteps=8[, callback])         :311-322

    The loop stays on the host exactly as in the reference (callback(mu) before every step, stop
    when the state matrix becomes empty); each step is one GPU call.  Between the two rounds of
    steps the reference merges and prunes templates (condense_templates, remove_sparse, remove_small,
    baumwelch.jl:340-349): `postprocess="reference"` (default) runs the restatement in postprocess.py,
    `None` skips the stage, a callable `postprocess(state_matrix, mu, sigma) -> (state_matrix, mu)`
    replaces it.

    `method="viterbi"` (an extension; the default "baum-welch" is the reference's loop) makes every step a step of
    Viterbi training (viterbi_step): the loop, the callbacks and the stage between the rounds are the same.  It
    refines a model and does not find one, so the random-start form refuses it.

    `init` chooses the start of the third form.  "random" (default) is the reference's: N random templates with
    p0 = 2^(-3K/2).  "detect" (an extension) seeds with seed_templates(X, N, K, resolve_overlaps, **seed_options)
    -- threshold crossings clustered on the device, sigma from the median absolute sample, entry probabilities
    from the cluster sizes -- and runs the same loop from there; clusters that stay empty are dropped, so the loop
    may start with fewer than N templates, and a recording without a single event returns the null model.  With a
    seed there is a model to refine, so "detect" is allowed with either method; p0 and rng are not used.
    """
    if method not in ("baum-welch", "viterbi"):
        raise ValueError("train_model: method must be \"baum-welch\" or \"viterbi\", got %r" % (method,))
    if init not in ("random", "detect"):
        raise ValueError("train_model: init must be \"random\" or \"detect\", got %r" % (init,))
    hard = method == "viterbi"
    X = _signal(X)
    if len(args) >= 1 and isinstance(args[0], StateMatrix):
        state_matrix, mu, sigma = args[0], args[1], float(args[2])
        if len(args) == 3:
            if hard:
                return viterbi_step(X, state_matrix, mu, sigma)
            return train_step(X, state_matrix, mu, sigma, verbose=verbose)
        nsteps = int(args[3])
        cb = args[4] if len(args) > 4 else callback
        mu = np.array(mu, dtype=np.float64, order="F", copy=True)
        em = _EMSession(X, hard)
        try:
            for _ in range(nsteps):
                if cb is not None:
                    cb(mu)
                state_matrix, mu, sigma = em.step(state_matrix, mu, sigma, verbose=verbose)
                if state_matrix.isempty():
                    break
            if postprocess == "reference":
                from .postprocess import reference_postprocess
                state_matrix, mu = reference_postprocess(state_matrix, mu, sigma, verbose=verbose)
            elif postprocess is not None:
                state_matrix, mu = postprocess(state_matrix, mu, sigma)
            if state_matrix.N == 0:
                return state_matrix, mu, sigma      # every template was pruned: the null model
            for _ in range(nsteps // 2):
                state_matrix, mu, sigma = em.step(state_matrix, mu, sigma, verbose=verbose)
        finally:
            em.close()
        return state_matrix, mu, sigma
    if init == "detect":
        N = int(args[0]) if len(args) > 0 else 3
        K = int(args[1]) if len(args) > 1 else 60
        resolve_overlaps = bool(args[2]) if len(args) > 2 else False
        nsteps = int(args[3]) if len(args) > 3 else 8
        cb = args[4] if len(args) > 4 else callback
        state_matrix, mu, sigma, _info = seed_templates(X, N, K, resolve_overlaps, **(seed_options or {}))
        if state_matrix.N == 0:
            return state_matrix, mu, sigma          # no event above threshold: the null model
        return train_model(X, state_matrix, mu, sigma, nsteps, cb, verbose=verbose, postprocess=postprocess,
                           method=method)
    # random initialisation, baumwelch.jl:311-322
    if hard:
        raise ValueError("train_model: method=\"viterbi\" needs a model to refine.  From the random start "
                         "(p0 = 2^(-3K/2)) the decoded path holds no spike, so every template would lose its "
                         "entry transition on the first step; start from templates, or run Baum-Welch first")
    N = int(args[0]) if len(args) > 0 else 3
    K = int(args[1]) if len(args) > 1 else 60
    resolve_overlaps = bool(args[2]) if len(args) > 2 else False
    nsteps = int(args[3]) if len(args) > 3 else 8
    cb = args[4] if len(args) > 4 else callback
    if p0 is None:
        p0 = 2.0 ** (-3 * K / 2)
    if rng is None:
        rng = np.random.default_rng()
    lp = np.log(np.full(N, p0))
    state_matrix = StateMatrix.create(N, K, lp, resolve_overlaps)
    sigma = float(np.std(X, ddof=1))          # Julia's std is the corrected estimator
    mu = np.ones((K, N), order="F")
    for i in range(N):
        mu[:, i] = create_spike_template(K, 3 * sigma * rng.random(), 0.5 + 0.1 * rng.standard_normal(),
                                         1.5 * rng.random())
    mu[0, :] = 0.0
    return train_model(X, state_matrix, mu, sigma, nsteps, cb, verbose=verbose,
                       postprocess=postprocess)


def reconstruct_signal(x, lA, mu, sigma=None):
    """reconstruct_signal(x, lA, mu, sigma) -> Y2 (sigma unused)   reconstruction.jl:1-10."""
    x = np.ascontiguousarray(x, dtype=np.int16)
    mu = np.asfortranarray(mu, dtype=np.float64)
    st = np.asfortranarray(lA.states, dtype=np.int16)
    out = np.zeros(len(x), dtype=np.float64)
    check(lib().hmmsort_reconstruct(ptr(x), len(x), ptr(st), lA.N, lA.nstates, ptr(mu),
                                    mu.shape[0], ptr(out)))
    return out


def unroll_mlseq(mlseq, state_matrix):
    """unroll_mlseq(mlseq, state_matrix) -> N x T Int16   extraction.jl:4-13."""
    mlseq = np.ascontiguousarray(mlseq, dtype=np.int16)
    st = np.asfortranarray(state_matrix.states, dtype=np.int16)
    out = np.zeros((state_matrix.N, len(mlseq)), dtype=np.int16, order="F")
    check(lib().hmmsort_unroll_mlseq(ptr(mlseq), len(mlseq), ptr(st), state_matrix.N,
                                     state_matrix.nstates, ptr(out)))
    return out


def fit(templates, X, chunksize=None):
    """fit(HMMSpikingModel, templates, X[, chunksize])   fit.jl:6-9 and :11-42.

    With `chunksize` the signal is decoded in sequentially dependent chunks with the reference's
    stitch rule (leading non-silent samples of a chunk are skipped, trailing ones are handed to
    the next chunk, which restarts at the last silent sample).  The reference's call to the
    removed `gc()` (fit.jl:19) is not reproduced."""
    raw = isinstance(X, np.ndarray) and X.dtype == np.int16 and X.ndim == 1
    X = np.ascontiguousarray(X) if raw else _signal(X)
    lA, mu, sigma = templates.state_matrix, templates.mu, templates.sigma
    if chunksize is None:
        x, ll = viterbi(X, lA, mu, sigma)
        return HMMSpikingModel(templates, x, ll, X)
    n = len(X)
    i = j = 1
    ml_seq = np.ones(n, dtype=np.int16)
    ll = 0.0
    # The chunks depend on each other (a chunk restarts where the previous decode was last silent),
    # so they run one after the other -- but on the device: the signal is uploaded once and one
    # plan per chunk length is reused (the host-buffer entry point would rebuild its plan and copy
    # the chunk for every call).
    import torch
    from .device import Plan
    # duplicate templates: which twin the reference decodes hangs on the last bit of its own sums
    # (DESIGN 3.2); the host-buffer entry point knows (strict engine), the plan API does not
    muf = np.asarray(mu, dtype=np.float64)
    twins = any(np.array_equal(muf[:, a], muf[:, b]) for a in range(lA.N) for b in range(a + 1, lA.N))
    dX = torch.from_numpy(X).cuda()
    if raw:
        # the acquisition's int16 samples: 2 bytes per sample over PCIe, widened in HBM (hmmsort.jl:84-88)
        draw, dX = dX, torch.empty(n, dtype=torch.float64, device="cuda")
        check(lib().hmmsort_samples_to_f64(draw.data_ptr(), 0, n, 1, dX.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
        del draw
    dx = torch.zeros(min(chunksize, n), dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    plans = {}
    try:
        while j < n:
            j = min(i + chunksize - 1, n)
            k = j - i + 1
            l = 1
            if k not in plans:
                plans[k] = Plan(k, lA, mu, sigma)
            plan = plans[k]
            if twins and plan.info()["engine"] == _lib.ENGINE_RING:
                # the lane-per-chain ring engine has no run-time near-tie detector (the wave and
                # blocked engines count near-ties in diag[7])
                x, _ll = viterbi(X[i - 1:j], lA, mu, sigma)
                plan = None
            else:
                plan.viterbi(dX.data_ptr() + (i - 1) * 8, dx, dll)
            dg = plan.diagnostics() if plan is not None else None
            if plan is None:
                pass
            elif dg[0] != 0 or (plan.info()["engine"] in (_lib.ENGINE_BLOCKED, _lib.ENGINE_WAVE) and dg[7] != 0):  # failed check / near-ties:
                x, _ll = viterbi(X[i - 1:j], lA, mu, sigma)   # the escalating entry point
            else:
                x, _ll = dx[:k].cpu().numpy(), float(dll.cpu()[0])
            if i > 1:
                while x[l - 1] > 1:
                    l += 1
            if j < n:
                while x[k - 1] > 1:
                    j -= 1
                    k -= 1
            ml_seq[i + l - 2:j] = x[l - 1:k]
            ll += _ll
            if j <= i:
                raise RuntimeError("chunk without a silent sample: the reference loops forever here")
            i = j
    finally:
        for pl in plans.values():
            pl.close()
    return HMMSpikingModel(templates, ml_seq, ll, X)


def fit_channels(templates, X, chunksize=None, devices=None):
    """The chunked decode of fit (fit.jl:11-42) for C recording channels in one native call
    (hmmsort_fit_channels): the chunk loop, the stitch and the per-channel state stay behind the C ABI, and
    channels on the same device are decoded in step on streams of their own (option "fit_streams").

    `templates`: one HMMSpikeTemplateModel for every channel, or a list of C of them (each channel its own
    templates, src/hmmsort.jl:79-83).  `X`: C x T (float64 or int16, rows C-contiguous) or a list of C
    one-dimensional arrays of equal length.  `chunksize=None`: every channel in one decode.  `devices`: list of
    device numbers, channel c runs on devices[c % len(devices)]; None = the current device.
    Returns a list of HMMSpikingModel.  A channel the reference would die on (no silent sample where the stitch
    needs one) raises HmmsortError naming the channel."""
    rows = [X[c] for c in range(len(X))]
    if not rows:
        raise ValueError("fit_channels: no channel")
    raw = all(isinstance(r, np.ndarray) and r.dtype == np.int16 for r in rows)
    rows = [np.ascontiguousarray(r) if raw else _signal(r) for r in rows]
    nch, n = len(rows), len(rows[0])
    if any(r.ndim != 1 or len(r) != n for r in rows):
        raise ValueError("fit_channels: channels must be one-dimensional and of equal length")
    tms = list(templates) if isinstance(templates, (list, tuple)) else [templates] * nch
    if len(tms) != nch:
        raise ValueError("fit_channels: %d template models for %d channels" % (len(tms), nch))
    keep = []
    models = (_lib.Model * nch)()
    for c, tm in enumerate(tms):
        k, m = _model_args(tm.state_matrix, tm.mu, tm.sigma)
        keep.append(k)
        models[c] = _lib.Model(*m)
    ml = [np.zeros(n, dtype=np.int16) for _ in range(nch)]
    ll = np.zeros(nch)
    status = (C.c_int * nch)()
    ys = (C.c_void_p * nch)(*[r.ctypes.data for r in rows])
    outs = (C.c_void_p * nch)(*[m.ctypes.data for m in ml])
    dev = (C.c_int * len(devices))(*devices) if devices else None
    rc = lib().hmmsort_fit_channels(nch, ys, _lib.SAMPLES_I16 if raw else _lib.SAMPLES_F64, n,
                                    0 if chunksize is None else int(chunksize), models, dev,
                                    len(devices) if devices else 0, outs, ptr(ll), status)
    check(rc)
    return [HMMSpikingModel(tms[c], ml[c], float(ll[c]), rows[c]) for c in range(nch)]


def fit_step_channels(templates, X, chunksize=None, devices=None, pooled=False):
    """One step of Viterbi training for C recording channels in one native call (hmmsort_fit_step_channels): every
    channel is decoded exactly as fit_channels decodes it, and the model is re-estimated from the statistics of
    its stitched path while signal and path are still on the GPU.  Arguments as fit_channels.  `pooled`: the
    channels' statistics are added in channel order and finished once with the first channel's model (all
    models must share their state table): one set of templates for all channels.

    Returns (models, steps): the list of HMMSpikingModel of the decode under the OLD models, and one
    (state_matrix', mu', sigma', counts) per channel, or a single one when pooled.  counts = [ids outside 1..S,
    pairs that are no transition, template rows that kept their mean]."""
    rows = [X[c] for c in range(len(X))]
    if not rows:
        raise ValueError("fit_step_channels: no channel")
    raw = all(isinstance(r, np.ndarray) and r.dtype == np.int16 for r in rows)
    rows = [np.ascontiguousarray(r) if raw else _signal(r) for r in rows]
    nch, n = len(rows), len(rows[0])
    if any(r.ndim != 1 or len(r) != n for r in rows):
        raise ValueError("fit_step_channels: channels must be one-dimensional and of equal length")
    tms = list(templates) if isinstance(templates, (list, tuple)) else [templates] * nch
    if len(tms) != nch:
        raise ValueError("fit_step_channels: %d template models for %d channels" % (len(tms), nch))
    keep = []
    models = (_lib.Model * nch)()
    for c, tm in enumerate(tms):
        k, m = _model_args(tm.state_matrix, tm.mu, tm.sigma)
        keep.append(k)
        models[c] = _lib.Model(*m)
    ml = [np.zeros(n, dtype=np.int16) for _ in range(nch)]
    ll = np.zeros(nch)
    status = (C.c_int * nch)()
    ys = (C.c_void_p * nch)(*[r.ctypes.data for r in rows])
    outs = (C.c_void_p * nch)(*[m.ctypes.data for m in ml])
    dev = (C.c_int * len(devices))(*devices) if devices else None
    nout = 1 if pooled else nch
    recs = (_lib.StepOut * nout)()
    bufs = []
    for c in range(nout):
        lA = tms[c].state_matrix
        b = dict(mu=np.zeros((lA.K, lA.N), order="F"), sigma=np.zeros(1), lp=np.zeros(len(keep[c][1])),
                 nlp=np.zeros(1, dtype=np.int64), pp=np.zeros(lA.nstates), counts=np.zeros(3, dtype=np.int64))
        bufs.append(b)
        # the first column of a pooled step is no channel's: the old one is kept
        recs[c] = _lib.StepOut(b["mu"].ctypes.data, b["sigma"].ctypes.data, b["lp"].ctypes.data, len(b["lp"]),
                               b["nlp"].ctypes.data, None if pooled else b["pp"].ctypes.data,
                               b["counts"].ctypes.data)
    rc = lib().hmmsort_fit_step_channels(nch, ys, _lib.SAMPLES_I16 if raw else _lib.SAMPLES_F64, n,
                                         0 if chunksize is None else int(chunksize), models, dev,
                                         len(devices) if devices else 0, int(bool(pooled)), outs, ptr(ll), recs,
                                         status)
    check(rc)
    steps = []
    for c, b in enumerate(bufs):
        lA = tms[c].state_matrix
        pp = np.asarray(lA.pi, dtype=np.float64) if pooled else b["pp"]
        lA_new = StateMatrix.from_states(lA.states, pp, lA.K, b["lp"][:int(b["nlp"][0])].copy(), lA.resolve_overlaps)
        steps.append((lA_new, b["mu"], float(b["sigma"][0]), b["counts"].tolist()))
    return [HMMSpikingModel(tms[c], ml[c], float(ll[c]), rows[c]) for c in range(nch)], steps


@dataclass
class ModelTrack:
    """What fit_adaptive's chunk loop did, one entry per decoded chunk (struct hmmsort_track)."""
    n: int               # chunks decoded
    first: np.ndarray    # n, fit.jl's i of each chunk (1-based)
    own: np.ndarray      # n x 2, the 0-based range [lo, hi) whose statistics the chunk contributed
    w: np.ndarray        # n, the weight the accumulator was multiplied by before the chunk's statistics were added
    mu: np.ndarray       # n x K x N, the templates each chunk was DECODED with
    sigma: np.ndarray    # n
    final: tuple = None  # (state_matrix', mu', sigma', counts): the full re-estimate after the last chunk


def _fit_adaptive_call(templates, X, chunksize, halflife, warmup, update_sigma, update_lp, cap=None, want_final=True):
    """hmmsort_fit_adaptive without raising: (rc, ml_seq, ll, ModelTrack of the first `cap` records, X as passed)"""
    raw = isinstance(X, np.ndarray) and X.dtype == np.int16 and X.ndim == 1
    X = np.ascontiguousarray(X) if raw else _signal(X)
    lA = templates.state_matrix
    keep, margs = _model_args(lA, templates.mu, templates.sigma)
    model = _lib.Model(*margs)
    n = len(X)
    cs = 0 if chunksize is None else int(chunksize)
    grow = cap is None   # a guessed capacity is corrected by a second run; a caller's own is kept
    if grow:
        cap = 2 * (n // cs + 1) + 2 if cs > 0 else 1
    K, N, S = lA.K, lA.N, lA.nstates
    while True:
        ml = np.zeros(n, dtype=np.int16)
        ll = np.zeros(1)
        b = dict(n=np.zeros(1, dtype=np.int64), first=np.zeros(cap, dtype=np.int64),
                 own=np.zeros((cap, 2), dtype=np.int64), w=np.zeros(cap), mu=np.zeros((cap, K * N)), sigma=np.zeros(cap))
        track = _lib.Track(cap, *[b[k].ctypes.data for k in ("n", "first", "own", "w", "mu", "sigma")])
        f = dict(mu=np.zeros((K, N), order="F"), sigma=np.zeros(1), lp=np.zeros(len(keep[1])),
                 nlp=np.zeros(1, dtype=np.int64), pp=np.zeros(S), counts=np.zeros(3, dtype=np.int64))
        rec = _lib.StepOut(f["mu"].ctypes.data, f["sigma"].ctypes.data, f["lp"].ctypes.data, len(f["lp"]),
                           f["nlp"].ctypes.data, f["pp"].ctypes.data, f["counts"].ctypes.data)
        opt = _lib.Adapt(float(halflife), int(warmup), int(bool(update_sigma)), int(bool(update_lp)))
        rc = lib().hmmsort_fit_adaptive(ptr(X), _lib.SAMPLES_I16 if raw else _lib.SAMPLES_F64, n, cs, C.byref(model),
                                        C.byref(opt), ptr(ml), ptr(ll), C.byref(track),
                                        C.byref(rec) if want_final else None)
        nrec = int(b["n"][0])
        if rc == 0 and nrec > cap and grow:   # more chunks than guessed: the loop is deterministic, run it again
            cap = nrec
            continue
        break
    m = min(nrec, cap)
    final = None
    if rc == 0 and want_final:
        lA_new = StateMatrix.from_states(lA.states, f["pp"], K, f["lp"][:int(f["nlp"][0])].copy(), lA.resolve_overlaps)
        final = (lA_new, f["mu"], float(f["sigma"][0]), f["counts"].tolist())
    tk = ModelTrack(nrec, b["first"][:m], b["own"][:m], b["w"][:m],
                    b["mu"][:m].reshape((m, N, K)).transpose(0, 2, 1), b["sigma"][:m], final)
    return rc, ml, float(ll[0]), tk, X


def fit_adaptive(templates, X, chunksize, halflife, warmup=0, update_sigma=True, update_lp=False):
    """Drift-tracking chunked decode (hmmsort_fit_adaptive; an extension, INTEGRATION.md "Drift tracking"): fit(...,
    chunksize) with the model re-estimated between chunks from exponentially weighted statistics of the decoded
    path, so that templates follow slow changes of the recording.  `halflife`: samples after which a statistic
    weighs one half (inf: never forget); `warmup`: samples that must have entered the statistics before the model
    is first replaced; `update_sigma` / `update_lp`: whether the noise level and the transition list follow too.
    With `update_lp` a template that does not fire within memory loses its entry transition and cannot come back:
    off by default.

    Returns (HMMSpikingModel, ModelTrack): the stitched path and the sum of the chunks' log-likelihoods, each under
    the model its chunk was decoded with, beside the caller's templates; and the model track (reconstruct_tracked
    gives the reconstruction that goes with it)."""
    rc, ml, ll, tk, X = _fit_adaptive_call(templates, X, chunksize, halflife, warmup, update_sigma, update_lp)
    check(rc)
    return HMMSpikingModel(templates, ml, ll, X), tk


def reconstruct_tracked(x, lA, track):
    """reconstruct_signal under a model track: sample t takes the templates of the last chunk of `track` whose
    first sample is <= t (hmmsort_reconstruct_tracked).  State ids outside 1..S give NaN."""
    x = np.ascontiguousarray(x, dtype=np.int16)
    st = np.asfortranarray(lA.states, dtype=np.int16)
    first = np.ascontiguousarray(track.first, dtype=np.int64)
    mu = np.ascontiguousarray(np.asarray(track.mu, dtype=np.float64).transpose(0, 2, 1))   # [n][K*N], column-major each
    if mu.ndim != 3 or mu.shape != (len(first), lA.N, lA.K):
        raise ValueError("reconstruct_tracked: track.mu must be n x K x N = %d x %d x %d" % (len(first), lA.K, lA.N))
    out = np.zeros(len(x), dtype=np.float64)
    check(lib().hmmsort_reconstruct_tracked(ptr(x), len(x), ptr(st), lA.N, lA.nstates, lA.K, len(first), ptr(first),
                                            ptr(mu), ptr(out)))
    return out


def predict(model):
    """StatsBase.predict(model)   fit.jl:54-56."""
    tm = model.template_model
    return reconstruct_signal(model.ml_seq, tm.state_matrix, tm.mu, tm.sigma)


def extract_spiketimes(model):
    """extract_spiketimes(model::HMMSpikingModel) -> one array of spike sample indices per neuron
    (1-based like the reference's findin result)   extraction.jl:15-24."""
    tm = model.template_model
    lA = tm.state_matrix
    x = np.ascontiguousarray(model.ml_seq, dtype=np.int16)
    mu = np.asfortranarray(tm.mu, dtype=np.float64)
    st = np.asfortranarray(lA.states, dtype=np.int16)
    cap = max(1, len(x) // 8)
    while True:
        times = np.zeros((lA.N, cap), dtype=np.int64)
        counts = np.zeros(lA.N, dtype=np.int64)
        check(lib().hmmsort_extract_spiketimes(ptr(x), len(x), ptr(st), lA.N, lA.nstates, ptr(mu),
                                               mu.shape[0], ptr(times), cap, ptr(counts)))
        if counts.max(initial=0) <= cap:
            return [times[i, :counts[i]].copy() for i in range(lA.N)]
        cap = int(counts.max())


@dataclass
class SpikeFit:
    """Per-spike fit of one template (hmmsort_spike_fit; definitions in include/hmmsort.h), aligned element for
    element with extract_spiketimes."""
    times: np.ndarray     # 1-based trough samples, ascending
    amp: np.ndarray       # least-squares amplitude of the template on the overlap-cleaned window (1 = as the template)
    rss: np.ndarray       # residual sum of squares at unit amplitude (at the fitted one: energy - amp^2 smm)
    energy: np.ndarray    # sum of squares of the overlap-cleaned window
    nused: np.ndarray     # phases of the window the path supports; K - 1 for a full event
    summary: np.ndarray   # 8 + 3 (K-1) doubles: n, n_full, sums over full events, smm, wsum / wsq / wcnt per phase


@dataclass
class UnitQuality:
    """What unit_quality derives from a template's summary and sigma."""
    n: int                   # events
    n_full: int              # events whose whole window the path supports; the figures below are over these
    mean_amp: float          # sum amp / n_full
    sd_amp: float            # sqrt(sum amp^2 / n_full - mean_amp^2), the spread around the mean
    sd_expected: float       # sigma / sqrt(smm): the spread noise alone gives
    chi2: float              # sum rss / (sigma^2 (K-1) n_full): 1 when the template explains its spikes
    energy: float            # smm / sigma^2
    waveform: np.ndarray     # K - 1: overlap-cleaned spike-triggered mean, wsum / wcnt (all events, used phases)
    waveform_sd: np.ndarray  # K - 1: its spread, sqrt(wsq / wcnt - waveform^2)


def _track_args(lA, track):
    """(nchunks, first, mu_track [n][K*N]) of a ModelTrack, or (0, None, None); the arrays must outlive the call"""
    if track is None:
        return 0, None, None
    first = np.ascontiguousarray(track.first, dtype=np.int64)
    mu = np.ascontiguousarray(np.asarray(track.mu, dtype=np.float64).transpose(0, 2, 1))   # column-major K x N each
    if mu.ndim != 3 or mu.shape != (len(first), lA.N, lA.K):
        raise ValueError("track.mu must be n x K x N = %d x %d x %d" % (len(first), lA.K, lA.N))
    return len(first), first, mu


def _spike_fit_run(call, nC, N, K, cap):
    """call(byref(hmmsort_spike_fit_out)) -> rc, repeated with a larger cap until every event fits: per channel a
    list of SpikeFit, one per template"""
    L = 8 + 3 * (K - 1)
    while True:
        b = dict(times=np.zeros((nC, N, cap), dtype=np.int64), amp=np.zeros((nC, N, cap)), rss=np.zeros((nC, N, cap)),
                 energy=np.zeros((nC, N, cap)), nused=np.zeros((nC, N, cap), dtype=np.int32),
                 counts=np.zeros((nC, N), dtype=np.int64), summary=np.zeros((nC, N, L)))
        out = _lib.SpikeFitOut(*[b[k].ctypes.data for k in ("times", "amp", "rss", "energy", "nused")], cap,
                               b["counts"].ctypes.data, b["summary"].ctypes.data)
        check(call(C.byref(out)))
        if b["counts"].max(initial=0) <= cap:
            break
        cap = int(b["counts"].max())
    cnt = b["counts"]
    return [[SpikeFit(*[b[k][c, a, :cnt[c, a]].copy() for k in ("times", "amp", "rss", "energy", "nused")],
                      b["summary"][c, a].copy()) for a in range(N)] for c in range(nC)]


def spike_fit(model, track=None):
    """spike_fit(model::HMMSpikingModel[, track::ModelTrack]) -> one SpikeFit per template (an extension,
    INTEGRATION.md "Spike fit"): for every spike extract_spiketimes reports, the least-squares amplitude of the
    template on the samples under it once the other templates the path says are active are subtracted, the residual
    at unit amplitude and the window's energy.  With fit_adaptive's `track` every spike is measured against the
    templates its chunk was decoded with.  int16 samples go to the device as they are."""
    tm = model.template_model
    lA = tm.state_matrix
    raw = isinstance(model.y, np.ndarray) and model.y.dtype == np.int16 and model.y.ndim == 1
    y = np.ascontiguousarray(model.y) if raw else _signal(model.y)
    x = np.ascontiguousarray(model.ml_seq, dtype=np.int16)
    if len(x) != len(y):
        raise ValueError("spike_fit: the path has %d samples, the signal %d" % (len(x), len(y)))
    mu = np.asfortranarray(tm.mu, dtype=np.float64)
    st = np.asfortranarray(lA.states, dtype=np.int16)
    nch, first, mut = _track_args(lA, track)
    stype = _lib.SAMPLES_I16 if raw else _lib.SAMPLES_F64
    return _spike_fit_run(lambda out: lib().hmmsort_spike_fit(ptr(y), stype, len(y), ptr(x), ptr(st), lA.N, lA.nstates,
                                                              ptr(mu), mu.shape[0], nch, ptr(first), ptr(mut), out),
                          1, lA.N, mu.shape[0], max(1, len(x) // 8))[0]


def quality_from_summary(summary, K, sigma):
    """UnitQuality of one template's summary vector (SpikeFit.summary)"""
    s = np.asarray(summary, dtype=np.float64)
    P = K - 1
    n, nf, sa, saa, srss, _sen, _snu, smm = s[:8]
    wsum, wsq, wcnt = s[8:8 + P], s[8 + P:8 + 2 * P], s[8 + 2 * P:8 + 3 * P]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = sa / nf
        sd = np.sqrt(np.maximum(saa / nf - mean * mean, 0.0))
        wf = wsum / wcnt
        wsd = np.sqrt(np.maximum(wsq / wcnt - wf * wf, 0.0))
        return UnitQuality(int(n), int(nf), float(mean), float(sd), float(sigma / np.sqrt(smm)),
                           float(srss / (sigma * sigma * P * nf)), float(smm / (sigma * sigma)), wf, wsd)


def unit_quality(model, track=None):
    """unit_quality(model[, track]) -> one UnitQuality per template, from spike_fit's summary and the model's sigma:
    do these templates fit this recording (chi2 near 1, mean_amp near 1, sd_amp near sd_expected), and what do the
    spikes the path found look like (waveform)?  Figures without events are NaN."""
    tm = model.template_model
    return [quality_from_summary(f.summary, tm.state_matrix.K, tm.sigma) for f in spike_fit(model, track)]


@dataclass
class Correlograms:
    """What hmmsort_correlograms counts for U units (definitions in include/hmmsort.h); all integers."""
    counts: np.ndarray          # [U, U, 2H]: counts[u, v, k] pairs with lag t_v - t_u in [lags[k], lags[k] + bin)
    lags: np.ndarray            # [2H]: left bin edges in samples, (k - H) * bin
    isi_violations: np.ndarray  # [U]: consecutive intervals shorter than `refractory`
    coincidence: np.ndarray     # [U, U]: spikes of u with a spike of v within +-`coincidence` samples
    n: np.ndarray               # [U]: spikes per unit


def _ccg_run(call, U, bin, half_bins, refractory, coincidence):
    """call(byref(hmmsort_ccg_opt), byref(hmmsort_ccg_out)) -> rc into a Correlograms of U units"""
    b, H = int(bin), int(half_bins)
    # sizes the library refuses get token arrays: it checks before it writes, and its message says what is wrong
    ok = 1 <= U <= _lib.CCG_MAX_UNITS and 1 <= H <= _lib.CCG_MAX_HALF_BINS and U * U * 2 * H <= 1 << 28
    Ua, Ha = (U, H) if ok else (1, 1)
    ccg, coinc = np.zeros((Ua, Ua, 2 * Ha), dtype=np.int64), np.zeros((Ua, Ua), dtype=np.int64)
    viol, n = np.zeros(Ua, dtype=np.int64), np.zeros(Ua, dtype=np.int64)
    opt = _lib.CcgOpt(b, H, int(refractory), int(coincidence))
    out = _lib.CcgOut(ccg.ctypes.data, viol.ctypes.data, coinc.ctypes.data, n.ctypes.data)
    check(call(C.byref(opt), C.byref(out)))
    return Correlograms(ccg, (np.arange(2 * H, dtype=np.int64) - H) * b, viol, coinc, n)


def correlograms(models_or_time_lists, bin=30, half_bins=50, refractory=30, coincidence=2):
    """correlograms(units; bin, half_bins, refractory, coincidence) -> Correlograms (an extension, INTEGRATION.md
    "Correlograms"): auto- and cross-correlograms of the spike trains, refractory violations per unit and, per ordered
    pair, how many spikes of one unit the other also has.  `units` is a list whose entries are spike-time arrays
    (1-based samples, strictly ascending) or HMMSpikingModels; a model contributes its extract_spiketimes lists in
    order, so a list of per-channel models (fit_channels) gives units channel by channel.  All options in samples."""
    lists = _time_lists(models_or_time_lists)
    U = len(lists)
    ptrs = (C.c_void_p * max(U, 1))(*[t.ctypes.data if len(t) else None for t in lists])
    cnt = np.array([len(t) for t in lists] + [0] * (U == 0), dtype=np.int64)
    return _ccg_run(lambda opt, out: lib().hmmsort_correlograms(U, ptrs, ptr(cnt), opt, out), U, bin, half_bins,
                    refractory, coincidence)


def duplicate_units(cg, min_fraction=0.5):
    """duplicate_units(cg::Correlograms; min_fraction) -> [(u, v, fraction)] for u != v with fraction =
    coincidence[u, v] / n[u] >= min_fraction, in ascending (u, v): v has that share of u's spikes too.  A neuron sorted
    twice shows up in both directions; a unit without spikes is in no pair.  Host code."""
    out = []
    n = np.asarray(cg.n)
    for u in range(len(n)):
        for v in range(len(n)):
            if u != v and n[u] > 0 and cg.coincidence[u, v] >= min_fraction * n[u]:
                out.append((u, v, float(cg.coincidence[u, v]) / float(n[u])))
    return out


@dataclass
class Footprints:
    """What hmmsort_footprints sums for U units over M channel slots and W window samples (definitions in
    include/hmmsort.h), and what follows from the sums on the host."""
    sum: np.ndarray       # [U, M, W]: sum of the used spikes' snippets
    sumsq: np.ndarray     # [U, M, W]: sum of their squares
    n_used: np.ndarray    # [U]: spikes whose window lies inside the block
    n: np.ndarray         # [U]: spikes per unit
    channels: np.ndarray  # [U, M] int32: block channel of every slot, -1 for an empty slot
    pre: int              # window samples before the spike time

    @property
    def mean(self):
        """[U, M, W]: sum / n_used, zeros for a unit without a used spike"""
        nu = np.asarray(self.n_used, dtype=np.float64)[:, None, None]
        return np.divide(self.sum, nu, out=np.zeros_like(self.sum), where=nu > 0)

    @property
    def std(self):
        """[U, M, W]: sample spread sqrt(max(0, sumsq - sum * mean) / (n_used - 1)), zeros below two used spikes"""
        nu = np.asarray(self.n_used, dtype=np.float64)[:, None, None]
        var = np.maximum(0.0, self.sumsq - self.sum * self.mean)
        return np.sqrt(np.divide(var, nu - 1.0, out=np.zeros_like(var), where=nu > 1))

    @property
    def ptp(self):
        """[U, M]: peak to peak of the mean over the window"""
        m = self.mean
        return m.max(axis=2) - m.min(axis=2)

    @property
    def peak_channel(self):
        """[U]: block channel of the slot with the largest ptp (ties to the lower slot, empty slots never), -1 for a
        unit without a used spike"""
        ch = np.asarray(self.channels)
        slot = np.argmax(np.where(ch >= 0, self.ptp, -1.0), axis=1)
        peak = ch[np.arange(len(ch)), slot]
        return np.where(np.asarray(self.n_used) > 0, peak, -1).astype(np.int64)


def _fp_run(call, U, nC, pre, W, channels):
    """call(byref(hmmsort_fp_opt), byref(hmmsort_fp_out)) -> rc into the Footprints of U units on a block of nC
    channels; `channels`: None (every channel in order), one list of block channels for all units, or a [U][M] table
    (-1: empty slot)"""
    pre, W = int(pre), int(W)
    if channels is None:
        chan, M = None, nC
        table = np.tile(np.arange(max(nC, 0), dtype=np.int32), (max(U, 0), 1))
    else:
        chan = np.asarray(channels, dtype=np.int32)
        if chan.ndim == 1:
            chan = np.tile(chan, (max(U, 1), 1))
        if chan.ndim != 2 or (U >= 1 and chan.shape[0] != U):
            raise ValueError("footprints: channels must be one list of channels or a table of %d rows" % U)
        table = chan = np.ascontiguousarray(chan)
        M = chan.shape[1]
    # sizes the library refuses get token arrays: it checks before it writes, and its message says what is wrong
    ok = (1 <= U <= _lib.FP_MAX_UNITS and 1 <= W <= _lib.FP_MAX_W and 1 <= M <= _lib.FP_MAX_SLOTS
          and U * M * W <= 1 << 28)
    Ua, Ma, Wa = (U, M, W) if ok else (1, 1, 1)
    s, q = np.zeros((Ua, Ma, Wa)), np.zeros((Ua, Ma, Wa))
    nused, n = np.zeros(Ua, dtype=np.int64), np.zeros(Ua, dtype=np.int64)
    opt = _lib.FpOpt(pre, W, M, chan.ctypes.data if chan is not None else None)
    out = _lib.FpOut(s.ctypes.data, q.ctypes.data, nused.ctypes.data, n.ctypes.data)
    check(call(C.byref(opt), C.byref(out)))
    return Footprints(s, q, nused, n, table, pre)


def _time_lists(models_or_time_lists):
    """the units of correlograms / footprints as contiguous int64 arrays: a model contributes its extract_spiketimes
    lists in order"""
    lists = []
    for item in models_or_time_lists:
        if isinstance(item, HMMSpikingModel):
            lists.extend(extract_spiketimes(item))
        else:
            lists.append(item)
    return [np.ascontiguousarray(t, dtype=np.int64).ravel() for t in lists]


def footprints(block, units, pre=20, W=60, channels=None):
    """footprints(block, units; pre, W, channels) -> Footprints (an extension, INTEGRATION.md "Footprints"): the
    spike-triggered sum and sum of squares of every unit on every channel of `block`, a [C, T] float64 or int16 array
    (1-D: one channel) -- typically api.preprocess's output.  `units` is a list of spike-time arrays (1-based samples,
    strictly ascending) or HMMSpikingModels, as correlograms takes them.  The window of a spike at t is samples
    t - 1 - pre .. t - 2 - pre + W (0-based); a spike whose window leaves the block is not used.  `channels`: None for
    all channels, one list of block channels for every unit, or a table [U][M] with -1 for empty slots."""
    y = np.asarray(block)
    if y.ndim == 1:
        y = y[None, :]
    if y.ndim != 2:
        raise ValueError("footprints: block must be channels x samples")
    raw = y.dtype == np.int16
    y = np.ascontiguousarray(y, dtype=np.int16 if raw else np.float64)
    lists = _time_lists(units)
    U = len(lists)
    ptrs = (C.c_void_p * max(U, 1))(*[t.ctypes.data if len(t) else None for t in lists])
    cnt = np.array([len(t) for t in lists] + [0] * (U == 0), dtype=np.int64)
    stype = _lib.SAMPLES_I16 if raw else _lib.SAMPLES_F64
    nC, T = y.shape
    return _fp_run(lambda opt, out: lib().hmmsort_footprints(ptr(y), stype, nC, T, U, ptrs, ptr(cnt), opt, out),
                   U, nC, pre, W, channels)


def unit_locations(fp, positions):
    """unit_locations(fp::Footprints, positions) -> [U, D]: per unit the centre of mass of positions[channel] (a [C]
    or [C, D] array of electrode coordinates) weighted by ptp^2 over the unit's listed slots.  NaN for a unit without
    a used spike (or without any amplitude).  Host code."""
    pos = np.asarray(positions, dtype=np.float64)
    flat = pos.ndim == 1
    if flat:
        pos = pos[:, None]
    ch = np.asarray(fp.channels)
    w = np.where(ch >= 0, fp.ptp, 0.0) ** 2
    w[np.asarray(fp.n_used) == 0] = 0.0
    num = np.einsum("um,umd->ud", w, pos[np.where(ch >= 0, ch, 0)])
    den = w.sum(axis=1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        loc = np.where(den > 0, num / den, np.nan)
    return loc[:, 0] if flat else loc


def footprint_similarity(fp, max_lag=10):
    """footprint_similarity(fp::Footprints; max_lag) -> (similarity [U, U], lag [U, U]).  For u != v the similarity is
    the maximum over l in -max_lag..max_lag of the cosine between mean_u[c][k] and mean_v[c][k + l], taken over the
    channels both units list (a channel listed twice counts once, by its first slot) and the k for which both indices
    lie in 0..W-1; lag[u, v] is the l that attains it (the smallest |l|, then the negative one, among equals), so
    lag[v, u] == -lag[u, v].  0 (and lag 0) without a common channel or when either norm is 0; the diagonal is 1.
    Host code."""
    mean, ch = fp.mean, np.asarray(fp.channels)
    U, _, W = mean.shape
    sim, lag = np.zeros((U, U)), np.zeros((U, U), dtype=np.int64)
    first = [{} for _ in range(U)]          # channel -> its first slot
    for u in range(U):
        for m, c in enumerate(ch[u]):
            if c >= 0:
                first[u].setdefault(int(c), m)
    lags = sorted(range(-int(max_lag), int(max_lag) + 1), key=lambda l: (abs(l), l))
    for u in range(U):
        sim[u, u] = 1.0
        for v in range(u + 1, U):
            common = sorted(set(first[u]) & set(first[v]))
            if not common:
                continue
            a = mean[u, [first[u][c] for c in common]]
            b = mean[v, [first[v][c] for c in common]]
            best, best_l = 0.0, 0
            for l in lags:
                if abs(l) >= W:
                    continue
                x, y = (a[:, :W - l], b[:, l:]) if l >= 0 else (a[:, -l:], b[:, :W + l])
                nx, ny = np.sqrt(np.sum(x * x)), np.sqrt(np.sum(y * y))
                if nx > 0 and ny > 0:
                    c = float(np.sum(x * y) / (nx * ny))
                    if c > best:
                        best, best_l = c, l
            sim[u, v] = sim[v, u] = best
            lag[u, v], lag[v, u] = best_l, -best_l
    return sim, lag


def resolve_duplicates(cg, fp, min_fraction=0.5, min_similarity=0.8, max_lag=10):
    """resolve_duplicates(cg::Correlograms, fp::Footprints; min_fraction, min_similarity, max_lag) -> (keep, pairs): a
    pair {u, v} is a duplicate when duplicate_units(cg, min_fraction) lists it in either direction and
    footprint_similarity is at least min_similarity -- a neuron seen twice has one shape across the channels, two
    neurons that fire together do not.  Pairs are taken in ascending (min, max) order and skipped when a member is
    already dropped; the member whose largest ptp is smaller is dropped, the higher index on a tie.  `keep` is the
    boolean mask over the units, `pairs` the list (kept, dropped, fraction, similarity, lag) with the larger of the two
    directions' fractions and lag = lag[kept, dropped].  Host code."""
    frac = {}
    for u, v, f in duplicate_units(cg, min_fraction):
        key = (min(u, v), max(u, v))
        frac[key] = max(f, frac.get(key, 0.0))
    sim, lag = footprint_similarity(fp, max_lag)
    amp = fp.ptp.max(axis=1)
    keep = np.ones(len(amp), dtype=bool)
    pairs = []
    for (u, v) in sorted(frac):
        if sim[u, v] < min_similarity or not (keep[u] and keep[v]):
            continue
        kept, dropped = (v, u) if amp[u] < amp[v] else (u, v)
        keep[dropped] = False
        pairs.append((kept, dropped, frac[(u, v)], float(sim[u, v]), int(lag[kept, dropped])))
    return keep, pairs


def get_energy(waveforms, cinv):
    """get_energy(waveforms::Array{Float64,2}, cinv::Float64) -> ee   utils.jl:112-124: per template (column) the sum
    over rows j ascending of w*cinv*w, folded from 0.0 in the reference's operation order.  Host code."""
    W = np.asarray(waveforms, dtype=np.float64)
    if W.ndim != 2:
        raise ValueError("get_energy: waveforms must be nstates x N")
    cinv = np.float64(cinv)
    ee = np.zeros(W.shape[1])
    for j in range(W.shape[0]):
        ee += (W[j] * cinv) * W[j]
    return ee


@dataclass
class Posteriors:
    """Smoothed state posteriors gamma_t(s) = P(state s at sample t | whole recording), reduced per template
    (INTEGRATION.md "Posteriors"; the reference keeps the decoded path only)."""
    onset: np.ndarray    # N x T: template a at its first phase (states[a, s] == 2)
    occ: np.ndarray      # N x T: template a mid-spike (states[a, s] > 1)
    silent: np.ndarray   # T: state 1
    logz: float          # log-likelihood of the recording


def _posteriors_host(y, lA, mu, sigma, want_xm, want_marginals=True):
    y = _signal(y)
    keep, margs = _model_args(lA, mu, sigma)
    T = len(y)
    onset = np.zeros((lA.N, T)) if want_marginals else None
    occ = np.zeros((lA.N, T)) if want_marginals else None
    silent = np.zeros(T) if want_marginals else None
    xm = np.zeros(T, dtype=np.int16) if want_xm else None
    logz = np.zeros(1)
    check(lib().hmmsort_posteriors(ptr(y), T, *margs, ptr(onset), ptr(occ), ptr(silent), ptr(xm), ptr(logz)))
    return onset, occ, silent, xm, float(logz[0])


def posteriors(y, lA, mu, sigma):
    """posteriors(y, lA, mu, sigma) -> Posteriors.  Ring models (no overlaps, up to 16 templates) run on the wave
    engine; any other model on the strict engine from materialised alpha/beta (2 x S x T doubles on the
    device: short signals only).  With option "engine" set to ENGINE_BLOCKED an overlap model whose two state
    columns fit the LDS (up to 4 templates) runs on the blocked engine instead: time-parallel, no S x T array,
    boundaries certified and escalated like em_step's.  With option "blocked_hbm_columns" = 1 as well, so does a
    model past that limit (3 x 60 and 4 x 60 with overlaps): its columns live in device memory."""
    onset, occ, silent, _, logz = _posteriors_host(y, lA, mu, sigma, False)
    return Posteriors(onset, occ, silent, logz)


def posterior_decode(y, lA, mu, sigma):
    """Maximum-posterior-marginal decode: x[t] = arg max_s gamma_t(s), 1-based like viterbi's path, ties to the
    lower state number."""
    return _posteriors_host(y, lA, mu, sigma, True, False)[3]


def _posterior_plan(T, lA, mu, sigma):
    """a plan that serves posteriors: the wave engine when it takes the model, else the strict engine -- or the
    blocked engine when option "engine" names it and the model fits (4 templates; the blocked E-step's LDS limit,
    or any size under option "blocked_hbm_columns": stats_len() > 0 says which)"""
    from .device import Plan
    plan = Plan(T, lA, mu, sigma)
    engine = plan.info()["engine"]
    if engine in (_lib.ENGINE_WAVE, _lib.ENGINE_STRICT):
        return plan
    if (engine == _lib.ENGINE_BLOCKED and _lib.get_option("engine") == _lib.ENGINE_BLOCKED
            and plan.stats_len() > 0 and lA.N <= 4):
        return plan
    plan.close()
    prev = _lib.get_option("engine")
    _lib.set_option("engine", _lib.ENGINE_STRICT)
    try:
        return Plan(T, lA, mu, sigma)
    finally:
        _lib.set_option("engine", prev)


def spike_confidence(model, jitter=2):
    """spike_confidence(model::HMMSpikingModel, jitter=2) -> per template (times, confidence), aligned element for
    element with extract_spiketimes(model): the posterior probability that the template fired (was in its trough
    state) within +-jitter samples of where the decoded path put the spike."""
    import torch
    tm = model.template_model
    y = np.ascontiguousarray(model.y, dtype=np.float64)
    x = np.ascontiguousarray(model.ml_seq, dtype=np.int16)
    plan = _posterior_plan(len(y), tm.state_matrix, tm.mu, tm.sigma)
    try:
        dy, dx = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()
        plan.posteriors(dy)
        d = plan.diagnostics()
        if d[3] != 0 or d[5] != 0:
            raise HmmsortError(_lib.ENOCONV, "spike_confidence: %d chain boundaries fail the warm-up check; set "
                               "option \"halo\" wider" % (d[3] + d[5]))
        return plan.spike_confidence(dx, jitter)
    finally:
        plan.close()


# ---- waveform features and cluster isolation (an extension; include/hmmsort.h) ------------------------

@dataclass
class SnippetFeatures:
    """What hmmsort_snippet_features returns for U units: one row of F features per list entry, rows in unit order
    (entry e of unit u is row offs[u] + e), and the moments the mode asked for."""
    features: object          # [n_total, F] (numpy; a device tensor from device.snippet_features) or None
    used: object              # [n_total] uint8, likewise, or None
    n: np.ndarray             # [U]: list entries per unit
    n_used: np.ndarray        # [U]: entries whose window lies inside the block
    b1: np.ndarray = None     # moments = 1: [U, M, P], [U, M, P, P]
    b2: np.ndarray = None
    g1: np.ndarray = None     # moments = 2: [U, F], [U, F, F]
    g2: np.ndarray = None

    @property
    def offs(self):
        return np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)


def _feat_args(U, nC, pre, W, channels, basis, centre, moments):
    """-> (hmmsort_feat_opt, hmmsort_feat_out, arrays, (M, P, F)): the option record and the host outputs of a features
    call on a block of nC channels.  Sizes the library refuses get token arrays: it checks before it writes, and its
    message says what is wrong."""
    pre, W, moments = int(pre), int(W), int(moments)
    chan = None if channels is None else np.ascontiguousarray(channels, dtype=np.int32).ravel()
    M = nC if chan is None else len(chan)
    P = W
    if basis is not None:
        basis = np.ascontiguousarray(basis, dtype=np.float64)
        if basis.ndim != 3 or basis.shape[0] != M or basis.shape[2] != W:
            raise ValueError("snippet_features: basis must be [M = %d][P][W = %d], got %s" % (M, W, basis.shape))
        P = basis.shape[1]
    if centre is not None:
        centre = np.ascontiguousarray(centre, dtype=np.float64)
        if centre.shape != (M, W):
            raise ValueError("snippet_features: centre must be [M = %d][W = %d], got %s" % (M, W, centre.shape))
    F = M * P
    ok = (1 <= U <= _lib.FP_MAX_UNITS and M >= 1 and W >= 1
          and (moments != 1 or (P <= _lib.FEAT_MAX_P1 and U * M * P * P <= 1 << 26))
          and (moments != 2 or (F <= _lib.FEAT_MAX_F2 and U * F * F <= 1 << 26)))
    Ua, Ma, Pa = (U, M, P) if ok else (1, 1, 1)
    arr = {"n": np.zeros(Ua, dtype=np.int64), "nused": np.zeros(Ua, dtype=np.int64)}
    if moments == 1:
        arr["b1"], arr["b2"] = np.zeros((Ua, Ma, Pa)), np.zeros((Ua, Ma, Pa, Pa))
    if moments == 2:
        arr["g1"], arr["g2"] = np.zeros((Ua, Ma * Pa)), np.zeros((Ua, Ma * Pa, Ma * Pa))
    opt = _lib.FeatOpt(pre, W, M, ptr(chan), max(P, 1) if basis is not None else 1, ptr(basis), ptr(centre), moments)
    out = _lib.FeatOut(None, None, 0, ptr(arr["n"]), ptr(arr["nused"]), ptr(arr.get("b1")), ptr(arr.get("b2")),
                       ptr(arr.get("g1")), ptr(arr.get("g2")))
    arr["_keep"] = (chan, basis, centre)
    return opt, out, arr, (M, P, F)


def _host_block(block, who):
    y = np.asarray(block)
    if y.ndim == 1:
        y = y[None, :]
    if y.ndim != 2:
        raise ValueError(who + ": block must be channels x samples")
    raw = y.dtype == np.int16
    return np.ascontiguousarray(y, dtype=np.int16 if raw else np.float64), \
        (_lib.SAMPLES_I16 if raw else _lib.SAMPLES_F64)


def snippet_features(block, units, pre=20, W=60, channels=None, basis=None, centre=None, moments=0, features=True):
    """snippet_features(block, units; pre, W, channels, basis, centre, moments, features) -> SnippetFeatures (an
    extension, INTEGRATION.md "Isolation"; hmmsort_snippet_features).  `block` and `units` as footprints takes them;
    `channels`: None for all channels or ONE list of block channels for every unit.  Without a basis a row is the
    spike's snippets on the listed channels minus `centre` (None: the snippets themselves -- the export); with
    `basis` [M][P][W] it is the P projections per channel.  `moments`: 0 none, 1 the per-channel sums b1 / b2 (what
    pca_basis takes), 2 the per-unit sums g1 / g2 over whole rows.  features=False skips the rows."""
    y, stype = _host_block(block, "snippet_features")
    lists = _time_lists(units)
    U = len(lists)
    nC, T = y.shape
    opt, out, arr, (M, P, F) = _feat_args(U, nC, pre, W, channels, basis, centre, moments)
    n_total = sum(len(t) for t in lists)
    feat = used = None
    if features:
        fits = n_total * F <= 1 << 31
        feat = np.zeros((n_total if fits else 1, F if fits else 1))
        used = np.zeros(n_total if fits else 1, dtype=np.uint8)
        out.feat, out.used = feat.ctypes.data, used.ctypes.data
    ptrs = (C.c_void_p * max(U, 1))(*[t.ctypes.data if len(t) else None for t in lists])
    cnt = np.array([len(t) for t in lists] + [0] * (U == 0), dtype=np.int64)
    check(lib().hmmsort_snippet_features(ptr(y), stype, nC, T, U, ptrs, ptr(cnt), C.byref(opt), C.byref(out)))
    return SnippetFeatures(feat, used, arr["n"], arr["nused"], arr.get("b1"), arr.get("b2"), arr.get("g1"),
                           arr.get("g2"))


def pca_basis(b1, b2, n_used, P=3):
    """pca_basis(b1 [U, M, W], b2 [U, M, W, W], n_used [U]; P) -> (basis [M, P, W], centre [M, W]): per channel slot
    the mean snippet and the top P principal axes of the snippets of all units pooled (the sums of
    snippet_features(..., moments=1) without a basis), by decreasing variance, each with the sign that makes its
    largest-magnitude component positive.  Host code (numpy.linalg.eigh of M matrices W x W)."""
    b1, b2 = np.asarray(b1, dtype=np.float64), np.asarray(b2, dtype=np.float64)
    n = float(np.sum(n_used))
    _, M, W = b1.shape
    P = int(P)
    if not 1 <= P <= W:
        raise ValueError("pca_basis: P = %d components of a window of %d samples" % (P, W))
    if n < 1:
        raise ValueError("pca_basis: no used spike")
    centre = b1.sum(axis=0) / n
    basis = np.zeros((M, P, W))
    for m in range(M):
        cov = b2[:, m].sum(axis=0) / n - np.outer(centre[m], centre[m])
        _, vec = np.linalg.eigh(0.5 * (cov + cov.T))
        for p in range(P):
            v = vec[:, W - 1 - p]
            basis[m, p] = v if v[np.argmax(np.abs(v))] > 0 else -v
    return basis, centre


def unit_gaussians(g1, g2, n_used):
    """unit_gaussians(g1 [U, F], g2 [U, F, F], n_used [U]) -> (mu [U, F], Vinv [U, F, F]): per unit the feature mean
    and the inverse of the sample covariance (g2 / n - mu mu') n / (n - 1).  A unit with n_used <= F or a singular
    covariance is marked not scored: Vinv[u, 0, 0] = NaN, the rest zeros (hmmsort_cluster_isolation's convention)."""
    g1, g2 = np.asarray(g1, dtype=np.float64), np.asarray(g2, dtype=np.float64)
    U, F = g1.shape
    mu, vinv = np.zeros((U, F)), np.zeros((U, F, F))
    for u in range(U):
        n = float(n_used[u])
        ok = n > F
        if ok:
            m = g1[u] / n
            cov = (g2[u] / n - np.outer(m, m)) * (n / (n - 1.0))
            try:
                inv = np.linalg.inv(cov)
                ok = bool(np.all(np.isfinite(inv))) and np.linalg.cond(cov) < 1.0 / np.finfo(np.float64).eps
            except np.linalg.LinAlgError:
                ok = False
        if ok:
            mu[u], vinv[u] = m, inv
        else:
            vinv[u, 0, 0] = np.nan
    return mu, vinv


def _iso_run(call, U):
    """call(byref(hmmsort_iso_out)) -> rc into (iso_d2 [U], closer [U, U], lpair [U, U])"""
    Ua = U if 1 <= U <= _lib.FP_MAX_UNITS else 1
    d2, closer, lpair = np.zeros(Ua), np.zeros((Ua, Ua), dtype=np.int64), np.zeros((Ua, Ua))
    out = _lib.IsoOut(ptr(d2), ptr(closer), ptr(lpair))
    check(call(C.byref(out)))
    return d2, closer, lpair


def isolation_scores(features, offs, mu, Vinv, used=None):
    """isolation_scores(features [n, F], offs [U + 1], mu [U, F], Vinv [U, F, F]; used [n]) -> (iso_d2 [U],
    closer [U, U], lpair [U, U]): hmmsort_cluster_isolation as it is, for rows and Gaussians the caller made."""
    f = np.ascontiguousarray(features, dtype=np.float64)
    offs = np.ascontiguousarray(offs, dtype=np.int64).ravel()
    mu, Vinv = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(Vinv, dtype=np.float64)
    U = len(offs) - 1
    n, F = (int(f.shape[0]), int(f.shape[1])) if f.ndim == 2 else (0, 0)
    if mu.shape != (U, F) or Vinv.shape != (U, F, F):
        raise ValueError("isolation_scores: mu must be [%d][%d] and Vinv [%d][%d][%d]" % (U, F, U, F, F))
    u8 = None if used is None else np.ascontiguousarray(used, dtype=np.uint8).ravel()
    if u8 is not None and len(u8) != n:
        raise ValueError("isolation_scores: used has %d entries, features %d rows" % (len(u8), n))
    return _iso_run(lambda out: lib().hmmsort_cluster_isolation(ptr(f), n, F, U, ptr(offs), ptr(u8), ptr(mu),
                                                                ptr(Vinv), out), U)


@dataclass
class Isolation:
    """cluster_isolation's result for U units in a space of F = M P features."""
    distance: np.ndarray      # [U]: isolation distance (squared Mahalanobis distance of the n_used-th nearest
                              # non-member spike); NaN for a unit that is not scored or has too few non-members
    l_ratio: np.ndarray       # [U]: sum over the non-member spikes of Q_F(d2) / n_used; NaN when not scored
    lpair: np.ndarray         # [U, U]: the L-ratio's sum, split by the unit the spikes belong to
    closer: np.ndarray        # [U, U] int64: spikes of v nearer to u than to v; -1 when either is not scored
    n_used: np.ndarray        # [U]
    basis: np.ndarray         # [M, P, W]
    centre: np.ndarray        # [M, W]
    features: object = None   # [n_total, F] when asked for


def _isolation_result(d2, closer, lpair, n_used, basis, centre, features):
    nu = np.asarray(n_used, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        lr = np.where(nu > 0, lpair.sum(axis=1) / nu, np.nan)
    return Isolation(d2, lr, lpair, closer, np.asarray(n_used), basis, centre, features)


def cluster_isolation(block, units, pre=20, W=60, channels=None, P=3, keep_features=False):
    """cluster_isolation(block, units; pre, W, channels, P) -> Isolation (an extension, INTEGRATION.md "Isolation"):
    isolation distance and L-ratio (Schmitzer-Torbert et al. 2005) of every unit against the spikes of all the other
    lists, in the space of the top P principal components of the snippets on each listed channel.  Pass the detected
    events no unit explains (unassigned_events) as one more list to give the units a noise cluster to be isolated
    from.  Two passes over the block on the device (snippet moments; projections and their moments), the PCA and the
    F x F inverses on the host, the distances, the order statistic and the sums on the device."""
    lists = _time_lists(units)
    p1 = snippet_features(block, lists, pre, W, channels, moments=1, features=False)
    basis, centre = pca_basis(p1.b1, p1.b2, p1.n_used, P)
    p2 = snippet_features(block, lists, pre, W, channels, basis, centre, moments=2)
    mu, vinv = unit_gaussians(p2.g1, p2.g2, p2.n_used)
    d2, closer, lpair = isolation_scores(p2.features, p2.offs, mu, vinv, p2.used)
    return _isolation_result(d2, closer, lpair, p2.n_used, basis, centre, p2.features if keep_features else None)


def unassigned_events(events, units, tol=10):
    """unassigned_events(events, units, tol) -> the entries of `events` (sample numbers, e.g. seed_templates' detected
    events) that lie within `tol` samples of no spike of any unit, ascending and without repeats.  Host numpy."""
    ev = np.unique(np.asarray(events, dtype=np.int64).ravel())
    lists = _time_lists(units)
    spikes = np.sort(np.concatenate(lists + [np.zeros(0, dtype=np.int64)]))
    if len(spikes) == 0 or len(ev) == 0:
        return ev
    i = np.searchsorted(spikes, ev)
    left = np.abs(ev - spikes[np.maximum(i - 1, 0)])
    right = np.abs(spikes[np.minimum(i, len(spikes) - 1)] - ev)
    return ev[np.minimum(left, right) > int(tol)]


_STAB_SMOOTH = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


@dataclass
class UnitStability:
    """The tables of hmmsort_unit_stability for U units and B time bins (definitions in include/hmmsort.h) and the
    figures that follow from them on the host.  Without values only n and count are filled, the rest is None."""
    n: np.ndarray        # [U]: spikes per unit
    count: np.ndarray    # [U, B]: spikes per unit and time bin
    valid: np.ndarray    # [U, B]: of them with a value (not NaN)
    quant: np.ndarray    # [U, B, nq]: exact order statistics of the values of a bin, NaN where valid == 0
    sum: np.ndarray      # [U, B]: sum of the values
    sumsq: np.ndarray    # [U, B]: sum of their squares
    uvalid: np.ndarray   # [U]: values per unit over the whole recording
    uquant: np.ndarray   # [U, nq]: their order statistics
    umin: np.ndarray     # [U]
    umax: np.ndarray     # [U]
    usum: np.ndarray     # [U]: the bin sums folded in bin order
    usumsq: np.ndarray   # [U]
    hist: np.ndarray     # [U, HB]: values with floor((v - hist_lo) * hist_scale) == k
    under: np.ndarray    # [U]: values below bin 0
    over: np.ndarray     # [U]: values at or beyond bin HB
    T: int               # recording length in samples
    bin: int             # samples per time bin
    q_num: tuple         # the quantiles are q_num[k] / q_den
    q_den: int
    hist_lo: float
    hist_scale: float

    @property
    def bin_samples(self):
        """[B]: samples per time bin; the last one may be short"""
        B = self.count.shape[1]
        return np.minimum(self.bin, self.T - np.arange(B, dtype=np.int64) * self.bin)

    def firing_rate(self, fs):
        """[U, B]: spikes per second in every time bin at the sampling rate fs"""
        return self.count / (self.bin_samples / float(fs))

    def presence_ratio(self, min_count=1):
        """[U]: the share of full-length bins with at least min_count spikes; the short last bin is left out unless
        it is the only bin"""
        full = self.bin_samples == self.bin
        if not full.any():
            full[:] = True
        return np.sum(self.count[:, full] >= int(min_count), axis=1) / float(np.sum(full))

    def _median_index(self):
        for k, q in enumerate(self.q_num):
            if 2 * q == self.q_den:
                return k
        raise ValueError("amplitude_drift needs the quantile 1/2 among the quantiles")

    def amplitude_drift(self, min_valid=20):
        """[U]: (largest - smallest per-bin median) / overall median, over the bins with at least min_valid values;
        NaN for a unit without such a bin"""
        k = self._median_index()
        out = np.full(len(self.n), np.nan)
        for u in range(len(self.n)):
            med = self.quant[u, self.valid[u] >= int(min_valid), k]
            if len(med):
                with np.errstate(divide="ignore", invalid="ignore"):
                    out[u] = (med.max() - med.min()) / self.uquant[u, k]
        return out

    def amplitude_cutoff(self):
        """[U]: the estimated share of spikes lost below the detection floor (Hill et al. 2011), from the histogram:
        the counts smoothed with the binomial kernel (1, 4, 6, 4, 1) / 16 (zero padded), the peak at the first largest
        smoothed bin, the low edge at the first non-empty bin (bin 0 when `under` counts anything); the mass of the
        smoothed bins at or above the mirror image of the low edge about the peak, plus `over`, over the total count,
        capped at 0.5.  NaN for a unit without a value or without a histogram."""
        HB = self.hist.shape[1]
        out = np.full(len(self.n), np.nan)
        for u in range(len(self.n)):
            h = self.hist[u].astype(np.float64)
            total = float(self.under[u] + self.hist[u].sum() + self.over[u])
            if total == 0 or HB == 0:
                continue
            sm = np.convolve(h, _STAB_SMOOTH, mode="same") if HB >= len(_STAB_SMOOTH) else h
            peak = int(np.argmax(sm))
            nz = np.nonzero(self.hist[u])[0]
            low = 0 if self.under[u] > 0 or len(nz) == 0 else int(nz[0])
            mirror = 2 * peak - low
            mass = float(sm[mirror:].sum()) if mirror < HB else 0.0
            out[u] = min(0.5, (mass + float(self.over[u])) / total)
        return out


def quantile_fractions(quantiles):
    """(q_num, q_den) of float quantiles, the integers hmmsort_unit_stability ranks with: every q becomes the closest
    fraction with a denominator of at most 4096 (Fraction.limit_denominator, so 1/4, 1/3 or 0.9 are exact) and q_den
    is the least common multiple of the denominators; should that exceed 2^20, q_den = 2^20 and
    q_num = floor(q 2^20 + 1/2) instead."""
    from fractions import Fraction
    from math import lcm
    fr = [Fraction(float(q)).limit_denominator(4096) for q in quantiles]
    den = lcm(*[f.denominator for f in fr]) if fr else 1
    if den <= _lib.STAB_MAX_QDEN:
        return tuple(int(f.numerator * (den // f.denominator)) for f in fr), int(den)
    den = _lib.STAB_MAX_QDEN
    return tuple(int(np.floor(float(q) * den + 0.5)) for q in quantiles), den


def _stab_run(call, U, T, bin, quantiles, hist, with_values):
    """call(byref(hmmsort_stab_opt), byref(hmmsort_stab_out)) -> rc into the UnitStability of U units; hist: None or
    (bins, lo, hi), the histogram's bin k being [lo + k w, lo + (k + 1) w) with 1 / w = bins / (hi - lo)"""
    T, bin = int(T), int(bin)
    q_num, q_den = quantile_fractions(quantiles)
    nq = len(q_num)
    HB, lo, scale = 0, 0.0, 1.0
    if hist is not None:
        HB, lo, hi = int(hist[0]), float(hist[1]), float(hist[2])
        with np.errstate(divide="ignore", invalid="ignore"):
            scale = float(np.float64(HB) / (np.float64(hi) - np.float64(lo)))
    # sizes the library refuses get token arrays: it checks before it writes, and its message says what is wrong
    B = (T + bin - 1) // bin if bin >= 1 else 0
    ok = (1 <= U <= _lib.STAB_MAX_UNITS and 1 <= B <= _lib.STAB_MAX_BINS and U * B <= _lib.STAB_MAX_BINS
          and nq <= _lib.STAB_MAX_Q and 0 <= HB <= _lib.STAB_MAX_HIST)
    Ua, Ba, qa, Ha = (U, B, nq, HB) if ok else (1, 1, min(nq, _lib.STAB_MAX_Q), 0)
    i64 = dict(n=(Ua,), count=(Ua, Ba), valid=(Ua, Ba), uvalid=(Ua,), hist=(Ua, Ha), under=(Ua,), over=(Ua,))
    f64 = dict(quant=(Ua, Ba, qa), sum=(Ua, Ba), sumsq=(Ua, Ba), uquant=(Ua, qa), umin=(Ua,), umax=(Ua,), usum=(Ua,),
               usumsq=(Ua,))
    a = {k: np.zeros(s, dtype=np.int64) for k, s in i64.items()}
    a.update({k: np.zeros(s) for k, s in f64.items()})
    opt = _lib.StabOpt(T, bin, nq, (C.c_int64 * 8)(*q_num[:8]), q_den, HB, lo, scale)
    out = _lib.StabOut(*[a[k].ctypes.data for k, _ in _lib.StabOut._fields_])
    check(call(C.byref(opt), C.byref(out)))
    if not with_values:
        a.update({k: None for k in a if k not in ("n", "count")})
    return UnitStability(*[a[k] for k, _ in _lib.StabOut._fields_], T, bin, q_num, q_den, lo, scale)


def unit_stability(times, values=None, T=None, bin=None, quantiles=(1 / 4, 1 / 2, 3 / 4), hist=None):
    """unit_stability(units[, values]; T, bin, quantiles, hist) -> UnitStability (an extension, INTEGRATION.md
    "Stability"): per unit and time bin of `bin` samples the spike count and, of one value per spike, exact order
    statistics, sums and a histogram -- was the unit there the whole time, and did its amplitude sink?  `units` is a
    list of spike-time arrays (1-based samples, strictly ascending, at most T) or HMMSpikingModels, as correlograms
    takes them; `values` a list of float64 arrays of the same lengths (NaN: no value) or None for the counts alone.
    `quantiles` are floats in 0..1 turned into integer fractions by quantile_fractions; a quantile is the value of
    rank floor(q (m - 1)) among the m values of a bin, never interpolated.  `hist`: None or (bins, lo, hi)."""
    lists = _time_lists(times)
    U = len(lists)
    if T is None or bin is None:
        raise ValueError("unit_stability: T and bin are required")
    ptrs = (C.c_void_p * max(U, 1))(*[t.ctypes.data if len(t) else None for t in lists])
    cnt = np.array([len(t) for t in lists] + [0] * (U == 0), dtype=np.int64)
    vptrs = None
    if values is not None:
        vals = [np.ascontiguousarray(v, dtype=np.float64).ravel() for v in values]
        if [len(v) for v in vals] != [len(t) for t in lists]:
            raise ValueError("unit_stability: values must hold one array per unit, as long as its times")
        vptrs = (C.c_void_p * max(U, 1))(*[v.ctypes.data if len(v) else None for v in vals])
    return _stab_run(lambda opt, out: lib().hmmsort_unit_stability(U, ptrs, vptrs, ptr(cnt), opt, out), U, T, bin,
                     quantiles, hist, values is not None)
