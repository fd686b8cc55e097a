"""ctypes front-end of the extended-precision references: the E-step (oracle/hp_estep.c) and the
maximum-a-posteriori path (oracle/hp_viterbi.c, second half of this file).

TEST INFRASTRUCTURE ONLY.  The C routine turns (y, transition list, per-state means, sigma) into
the sufficient statistics of one Baum-Welch step in long double; this module forms the M-step
from them, still in long double (numpy's longdouble is the C type), and rounds once to double.
A machine whose long double has fewer than 64 mantissa bits fails here; nothing falls back to
double.
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
LD = np.longdouble


def build(force=False, name="hp_estep"):
    so = os.path.join(_HERE, "lib%s.so" % name)
    src = os.path.join(_HERE, name + ".c")
    if force or not os.path.exists(so) or (
            os.path.exists(src) and os.path.getmtime(so) < os.path.getmtime(src)):
        subprocess.check_call(["make", "-C", _HERE, "lib%s.so" % name], stdout=subprocess.DEVNULL)
    return so


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(build())
        L.hp_mant_dig.restype = C.c_int
        if L.hp_mant_dig() < 64 or np.finfo(LD).nmant < 63 or C.sizeof(C.c_longdouble) != LD().itemsize:
            raise RuntimeError("the extended-precision reference needs a long double with a 64-bit "
                               "mantissa shared by C and numpy; this machine has none")
        vp, i64 = C.c_void_p, C.c_int64
        L.hp_estep.restype = C.c_int
        L.hp_estep.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, C.c_double, i64, C.c_int,
                               i64, vp, vp] + [vp] * 8
        _LIB = L
    return _LIB


def state_means(states1, mu, dtype=np.float64):
    """m_j = sum over templates l of mu[states1[l, j] - 1, l] (row 0 of mu is the silent phase).
    The model's means are doubles added in template order, as every implementation forms them."""
    states1 = np.asarray(states1)
    N, S = states1.shape
    m = np.zeros(S, dtype)
    for l in range(N):
        m += np.asarray(mu, dtype)[states1[l].astype(np.int64) - 1, l]
    return m


@dataclass
class Estep:
    """Long-double sufficient statistics of one E-step (arrays of numpy longdouble)."""
    sg: np.ndarray      # S   sum_t gamma_t(j)
    sgy: np.ndarray     # S   sum_t gamma_t(j) y_t
    sgd: np.ndarray     # S   sum_t gamma_t(j) (y_t - m_j)
    sgd2: np.ndarray    # S   sum_t gamma_t(j) (y_t - m_j)^2
    sxi: np.ndarray     # R   sum_{t<T-1} xi_t(r)
    g0: np.ndarray      # S   gamma_0
    gl: np.ndarray      # S   gamma_{T-1}
    loglik: LD
    defect: LD          # max_t |sum_j gamma_t(j) - 1|
    mean: np.ndarray    # S   the per-state means used (double, as handed to C)
    windows: list       # per window: (hi - lo) x S float64 gamma


def estep(y, src, dst, lp, mean, sigma, block=1024, threads=1, windows=()):
    """src/dst 1-based as the state matrices store them; mean: S doubles."""
    L = lib()
    y = np.ascontiguousarray(y, np.float64)
    src0 = np.ascontiguousarray(np.asarray(src, np.int64) - 1)
    dst0 = np.ascontiguousarray(np.asarray(dst, np.int64) - 1)
    lp = np.ascontiguousarray(lp, np.float64)
    mean = np.ascontiguousarray(mean, np.float64)
    S, R, T = len(mean), len(lp), len(y)
    win = np.ascontiguousarray(np.asarray(windows, np.int64).reshape(-1, 2))
    nw = int((win[:, 1] - win[:, 0]).sum()) if len(win) else 0
    gwin = np.zeros((max(nw, 1), S), np.float64)
    out = [np.zeros(n, LD) for n in (S, S, S, R, S, S, 1, 1)]
    rc = L.hp_estep(y.ctypes.data, T, S, R, src0.ctypes.data, dst0.ctypes.data, lp.ctypes.data,
                    mean.ctypes.data, float(sigma), int(block), int(threads), len(win),
                    win.ctypes.data, gwin.ctypes.data, *[o.ctypes.data for o in out])
    if rc != 0:
        raise RuntimeError("hp_estep failed with code %d" % rc)
    sg, sgd, sgd2, sxi, g0, gl, ll, df = out
    ws, o = [], 0
    for lo, hi in win:
        ws.append(gwin[o:o + hi - lo])
        o += hi - lo
    return Estep(sg, sgd + mean.astype(LD) * sg, sgd, sgd2, sxi, g0, gl, ll[0], df[0], mean, ws)


@dataclass
class Mstep:
    mu: np.ndarray      # K x N float64 (Fortran order)
    sigma: float
    lp_new: np.ndarray  # new log p of the transitions leaving state 1, all but the first
    pp: np.ndarray      # S   log gamma_0


def mstep(E, states1, src, K):
    """The reference's update (baumwelch.jl:205-309) from the statistics, in long double:
      lp_new(1->j) = log( sum_{t<T-1} xi_t(1->j) / sum_{t<T-1} gamma_t(1) )   (:226-265, all but the first)
      pp           = log gamma_0                                              (:263)
      mu[k, l]     = sum_t gamma_t(j) y_t / sum_t gamma_t(j) over the states j in which template l
                     alone is active, at phase k                              (:266-287)
      sigma^2      = sum_{t,j} gamma_t(j) (y_t - m_j')^2 / sum_{t,j} gamma_t(j), m' from the new mu (:288-307)
    """
    states1 = np.asarray(states1)
    N, S = states1.shape
    first = np.nonzero(np.asarray(src) == 1)[0]
    with np.errstate(all="ignore"):
        lp_new = np.log(E.sxi[first[1:]] / (E.sg[0] - E.gl[0]))
        pp = np.log(E.g0)
        num = np.zeros((K, N), LD)
        den = np.zeros((K, N), LD)
        single = ((states1 >= 2).sum(0) == 1)
        for j in np.nonzero(single)[0]:
            l = int(np.argmax(states1[:, j] >= 2))
            num[states1[l, j] - 1, l] += E.sgy[j]
            den[states1[l, j] - 1, l] += E.sg[j]
        mu = num / den
        mu[0, :] = 0
        d = state_means(states1, mu, LD) - E.mean.astype(LD)
        # sum gamma (y - m')^2 with m' = m + d:  sgd2 - 2 d sgd + d^2 sg
        sig = np.sqrt((E.sgd2 - 2 * d * E.sgd + d * d * E.sg).sum() / E.sg.sum())
    return Mstep(np.asfortranarray(mu.astype(np.float64)), float(sig), lp_new.astype(np.float64),
                 pp.astype(np.float64))


def train_step(y, sm, mu, sigma, block=1024, threads=1, windows=()):
    """One EM step on an oracle-style StateMatrix (states 1-based N x S, src/dst/val lists)."""
    mean = state_means(sm.states, mu)
    E = estep(y, sm.src, sm.dst, sm.val, mean, sigma, block, threads, windows)
    return E, mstep(E, sm.states, sm.src, sm.K)


# ---------------------------------------------------------------------------------------------------------
# The maximum-a-posteriori path (oracle/hp_viterbi.c) and the rule by which a decode is accepted against it
# ---------------------------------------------------------------------------------------------------------
_VLIB = None
U64 = 2.0 ** -53        # unit roundoff of double
ULD = LD(2.0) ** -64    # unit roundoff of the 64-bit-mantissa long double


def vlib():
    global _VLIB
    if _VLIB is None:
        L = C.CDLL(build(name="hp_viterbi"))
        L.hpv_mant_dig.restype = C.c_int
        if L.hpv_mant_dig() < 64 or np.finfo(LD).nmant < 63 or C.sizeof(C.c_longdouble) != LD().itemsize:
            raise RuntimeError("the extended-precision reference needs a long double with a 64-bit "
                               "mantissa shared by C and numpy; this machine has none")
        vp, i64 = C.c_void_p, C.c_int64
        L.hp_viterbi.restype = C.c_int
        L.hp_viterbi.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, C.c_double, i64, C.c_int, i64, vp] + [vp] * 5
        _VLIB = L
    return _VLIB


@dataclass
class Map:
    """The reference's maximum-a-posteriori path and its scores (long double)."""
    x: np.ndarray       # T int32, 1-based states
    score: LD           # delta_{T-1}(x_{T-1}): log-probability of the path (first-sample rule included)
    ll: LD              # sum_{t>=1} delta_t(x_t), the reference implementation's "ll" (viterbi.jl:92-96)
    idx: np.ndarray     # the sample indices asked for (ascending)
    cum: np.ndarray     # delta_t(x_t) at those samples
    dmax: LD            # max_t |delta_t(x_t) - max_j delta_t(j)|


def viterbi_mean(y, src, dst, lp, mean, sigma, block=1024, threads=1, idx=()):
    """src/dst 1-based as the state matrices store them; mean: S doubles."""
    L = vlib()
    y = np.ascontiguousarray(y, np.float64)
    src0 = np.ascontiguousarray(np.asarray(src, np.int64) - 1)
    dst0 = np.ascontiguousarray(np.asarray(dst, np.int64) - 1)
    lp = np.ascontiguousarray(lp, np.float64)
    mean = np.ascontiguousarray(mean, np.float64)
    idx = np.ascontiguousarray(np.sort(np.asarray(idx, np.int64).ravel()))
    x = np.zeros(len(y), np.int32)
    sc, ll, dm = np.zeros(1, LD), np.zeros(1, LD), np.zeros(1, LD)
    cum = np.zeros(max(len(idx), 1), LD)
    rc = L.hp_viterbi(y.ctypes.data, len(y), len(mean), len(lp), src0.ctypes.data, dst0.ctypes.data,
                      lp.ctypes.data, mean.ctypes.data, float(sigma), int(block), int(threads), len(idx),
                      idx.ctypes.data, x.ctypes.data, sc.ctypes.data, ll.ctypes.data, cum.ctypes.data,
                      dm.ctypes.data)
    if rc != 0:
        raise RuntimeError("hp_viterbi failed with code %d" % rc)
    return Map(x, sc[0], ll[0], idx, cum[:len(idx)], dm[0])


def viterbi(y, sm, mu, sigma, block=1024, threads=1, idx=()):
    """The reference path of an oracle-style StateMatrix (states 1-based N x S, src/dst/val lists)."""
    return viterbi_mean(y, sm.src, sm.dst, sm.val, state_means(sm.states, mu), sigma, block, threads, idx)


def _pi_ld():
    return LD(4) * np.arctan(LD(1))


class _Model:
    """What path_score needs of a model: long-double means and emission constants, and the transition list
    as a sorted (src, dst) -> lp table.  Of a pair listed more than once the largest lp counts (what the
    maximisation over the list picks)."""

    def __init__(self, sm, mu, sigma):
        self.S = int(np.asarray(sm.states).shape[1])
        self.m = state_means(sm.states, mu).astype(LD)
        s = LD(float(sigma))
        self.c0 = -LD(0.5) * np.log(LD(2) * _pi_ld()) - np.log(s)
        self.two_s2 = LD(2) * s * s
        src, dst, lp = np.asarray(sm.src, np.int64), np.asarray(sm.dst, np.int64), np.asarray(sm.val, np.float64)
        key = src * (self.S + 1) + dst
        o = np.lexsort((-lp, key))
        key, lp = key[o], lp[o]
        first = np.r_[True, key[1:] != key[:-1]]
        self.key, self.lp = key[first], lp[first]
        self.indeg = np.bincount(dst, minlength=self.S + 1)     # by 1-based state; listed transitions

    def trans(self, a, b):
        """lp of the steps a[i] -> b[i] (1-based states); raises on a step that is not in the list"""
        k = np.asarray(a, np.int64) * (self.S + 1) + np.asarray(b, np.int64)
        i = np.minimum(np.searchsorted(self.key, k), len(self.key) - 1)
        bad = np.nonzero(self.key[i] != k)[0]
        if len(bad):
            raise ValueError("the path uses a transition that is not in the list: %d -> %d (step %d of the range)"
                             % (np.asarray(a)[bad[0]], np.asarray(b)[bad[0]], bad[0]))
        return self.lp[i].astype(LD)

    def emis(self, y, x, lo):
        """q_{x_t}(y_t) for the samples of a range that starts at sample lo (first-sample rule at sample 0)"""
        d = np.asarray(y, np.float64).astype(LD) - self.m[np.asarray(x, np.int64) - 1]
        q = self.c0 - d * d / self.two_s2
        if lo == 0 and len(q) and x[0] == 1:
            q[0] = 0
        return q


def path_terms(model, y, x, lo, hi):
    """(emission terms of samples lo..hi-1, transition terms of the steps into lo+1..hi-1), long double"""
    x = np.asarray(x)
    if not (0 <= lo < hi <= len(y)) or len(x) != len(y):
        raise ValueError("bad range")
    if x[lo:hi].min() < 1 or x[lo:hi].max() > model.S:
        raise ValueError("the path leaves the state space")
    return model.emis(y[lo:hi], x[lo:hi], lo), model.trans(x[lo:hi - 1], x[lo + 1:hi])


def path_score(y, sm, mu, sigma, x, lo, hi):
    """Score of the valid path x on the samples [lo, hi): sum of q_{x_t}(y_t) over the range (the silent state
    does not emit at sample 0) and of lp(x_{t-1} -> x_t) for lo < t < hi, in long double, summed over that range
    only.  With lo = 0 and hi = t + 1 it is delta_t(x_t) of the path.  Raises ValueError if x uses a transition that
    is not in the list."""
    model = sm if isinstance(sm, _Model) else _Model(sm, mu, sigma)
    q, a = path_terms(model, y, x, lo, hi)
    return q.sum() + a.sum()


def path_is_valid(model, x):
    try:
        model.trans(np.asarray(x)[:-1], np.asarray(x)[1:])
    except ValueError:
        return False
    return bool(np.asarray(x).min() >= 1 and np.asarray(x).max() <= model.S)


@dataclass
class Run:
    s: int              # first and last sample on which the two paths differ
    e: int
    delta: float        # score(reference on the run) - score(x on the run)
    tau: float          # what the fp64 reference implementation's own rounding can turn
    eps: float          # long-double rounding of the reference's own decisions and of the two sums
    J: int              # decisions inside the run
    V: float            # cumulative score at the later end of the run

    @property
    def ratio(self):
        return self.delta / self.tau


def compare_paths(y, sm, mu, sigma, x_ref, x, cum_idx=(), cum_val=(), dmax=0.0):
    """The maximal runs [s, e] on which the valid path x differs from the reference path x_ref, as a list of Run.

    Delta of a run is the score of x_ref minus the score of x over what differs: the emissions of s..e, the steps
    into s+1..e, the step into s (if s > 0; both leave the common state x[s-1]) and the step out of e (if e < T-1;
    both enter the common state x[e+1]); when s = 0 the silent state's emission at sample 0 counts as 0.  Outside
    the runs the two paths collect identical terms, so sum of Delta = score(x_ref) - score(x).

    ACCEPTANCE RULE.  x passes against x_ref when it is a valid path and  -eps <= Delta <= tau  on every run.

    tau: what the fp64 reference implementation (viterbi.jl:65-88) can decide against the exact arithmetic.
    Its T1[j,i] is a cumulative score of magnitude V (~ 2 T at the headline model).  Per step and path it rounds
    twice at that magnitude: t = T1[k,i-1] + lp and T1[j,i] += q, each by at most 1/2 ulp64(V).  Two candidate
    histories that meet in a state share every rounding made before they separated; if they separated n steps
    earlier, each carries at most n ulp64(V) of roundings of its own, so the comparison t > T1[j,i] can go against an
    exact gap of at most 2 n ulp64(V).  The reference path and x separate at s and meet again at e+1 (or never, if
    e = T-1: then the final arg-max compares them), so n <= m + 1 with m = e - s + 1.  Between s and e+1 the fp64
    implementation can have preferred a piece of x to a piece of x_ref only where a comparison took place: at a
    sample at which one of the two paths sits in a state with more than one incoming transition, and at the final
    arg-max.  Let J be the number of such samples in [s, min(e+1, T-1)], plus one if e = T-1.  Each of the J
    comparisons turns at most 2 (m+1) ulp64(V):
        tau_T1 = 2 (m+1) J ulp64(V),   V = max(|delta_{s-1}(x_ref)|, |delta_{min(e+1,T-1)}(x_ref)|),
    the larger of the exact cumulative scores at the two ends (the larger binade; the cumulative score of x at the
    same samples differs by Delta at most).  To that the fp64 evaluation of the emission itself is added
    (utils.jl:4: dd = x - mu, dd*dd, sigma2 = sigma*sigma, 2*sigma2, the quotient, -log2pi - lsigma, the final
    difference: the mean is formed from the same doubles in the same order, so it is the model's): relative to the
    quadratic term e = dd^2 / (2 sigma^2) at most (2 + 1 + 1 + 1 + 1) u64 = 6 u64 (dd enters squared), and
    1/2 ulp64 <= u64 |q| for the final difference; the rounded constants log2pi, lsigma are common to both paths
    except at sample 0 under the first-sample rule.  With e <= |q| + |c0|:
        tau_q = sum over both paths and the samples s..e of  7 u64 (|q_t| + |c0|)   (+ 2 u64 |c0| if s = 0),
        tau = tau_T1 + tau_q.
    No constant in it is measured.

    eps: the same argument for the long-double routine itself, whose values have the magnitude
    B = dmax + sum of |terms| of the run (dmax = max_t |dh_t(x_t)| as hp_viterbi reports it; a competitor inside
    the run is at most the run's terms away from it) and which rounds three times per step (+ lp, + q, - c_t):
        eps = 6 (m+1) max(J, 1) uLD B  +  (number of terms) uLD (sum of |terms|)     (the two sums formed here).
    Delta < -eps means x beats the "reference": the reference is wrong, not x.

    cum_idx/cum_val: cumulative scores delta_t(x_ref) at some samples (ascending), as hp.viterbi returns them;
    the cumulative score at a run's ends is the nearest earlier one plus the path's terms in between."""
    model = sm if isinstance(sm, _Model) else _Model(sm, mu, sigma)
    x_ref, x = np.asarray(x_ref), np.asarray(x)
    T = len(y)
    if len(x_ref) != T or len(x) != T:
        raise ValueError("paths and signal differ in length")
    diff = np.nonzero(x_ref != x)[0]
    if len(diff) == 0:
        return []
    cut = np.nonzero(np.diff(diff) > 1)[0]
    starts, ends = diff[np.r_[0, cut + 1]], diff[np.r_[cut, len(diff) - 1]]
    cum_idx = np.asarray(cum_idx, np.int64)
    cum_val = np.asarray(cum_val, LD)

    def cum_at(t):
        """delta_t(x_ref) in long double"""
        if t < 0:
            return LD(0)
        i = int(np.searchsorted(cum_idx, t, side="right")) - 1
        if i >= 0 and cum_idx[i] == t:
            return cum_val[i]
        lo = int(cum_idx[i]) if i >= 0 else 0
        q, a = path_terms(model, y, x_ref, lo, t + 1)
        return (cum_val[i] - q[0] if i >= 0 else LD(0)) + q.sum() + a.sum()

    runs = []
    absc0 = float(abs(model.c0))
    for s, e in zip(starts.tolist(), ends.tolist()):
        lo, hi = max(s - 1, 0), min(e + 1, T - 1)            # the common samples around the run, if any
        terms, tot = [], []
        for p in (x_ref, x):
            q, a = path_terms(model, y, p, lo, hi + 1)
            q = q[(1 if s > 0 else 0):(len(q) - 1 if e < T - 1 else len(q))]      # common samples emit alike
            terms.append((q, a))
            tot.append(q.sum() + a.sum())
        delta = tot[0] - tot[1]
        m = e - s + 1
        sl = slice(s, hi + 1)
        J = int(((model.indeg[x_ref[sl]] > 1) | (model.indeg[x[sl]] > 1)).sum()) + (1 if e == T - 1 else 0)
        V = float(max(abs(cum_at(s - 1)), abs(cum_at(hi))))
        sabs = sum(float(np.abs(q).sum() + np.abs(a).sum()) for q, a in terms)
        nterms = sum(len(q) + len(a) for q, a in terms)
        tau_q = sum(float(7 * U64 * (np.abs(q).sum() + len(q) * absc0)) for q, _ in terms) \
            + (2 * U64 * absc0 if s == 0 else 0.0)
        tau = 2.0 * (m + 1) * J * float(np.spacing(V)) + tau_q
        eps = float(ULD) * (6.0 * (m + 1) * max(J, 1) * (float(dmax) + sabs) + nterms * sabs)
        runs.append(Run(s, e, float(delta), tau, eps, J, V))
    return runs


def judge(runs):
    """(number of differing samples, largest Delta/tau, runs with Delta > tau, runs with Delta < -eps)"""
    n = sum(r.e - r.s + 1 for r in runs)
    worst = max((r.ratio for r in runs), default=0.0)
    return n, worst, [r for r in runs if r.delta > r.tau], [r for r in runs if r.delta < -r.eps]
