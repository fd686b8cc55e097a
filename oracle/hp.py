"""ctypes front-end of the extended-precision E-step reference (oracle/hp_estep.c).

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


def build(force=False):
    so = os.path.join(_HERE, "libhp_estep.so")
    src = os.path.join(_HERE, "hp_estep.c")
    if force or not os.path.exists(so) or (
            os.path.exists(src) and os.path.getmtime(so) < os.path.getmtime(src)):
        subprocess.check_call(["make", "-C", _HERE, "libhp_estep.so"], stdout=subprocess.DEVNULL)
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
