"""Generates tests/golden/blocked_post_at_size/<case>.npz FROM THE EXTENDED-PRECISION REFERENCE
(oracle/hp_estep.c through oracle/hp.py, hp.train_step(..., windows=...)): the posterior marginals of
overlap models at 10^6 samples on windows that hold block boundaries of the blocked engine, for
tests/test_gpu_blocked_posteriors_at_size.py.  CPU only.

Each fixture holds the case's parameters, SHA-256 of y and of the model arrays, and per window: onset, occ,
trough mass per template, silent, the reference's arg-max state and the gap between its two largest posteriors;
the log-likelihood and sum_t gamma_t(j) of every state.  The GPU test regenerates the inputs from the seed,
compares the hashes, and recomputes the reference live on a mismatch.

Windows: the two ends and 1 024 samples around three interior multiples of the blocked plan's block length
(block_length() below restates blocked_geometry of csrc/generic_blocked.hip for the default options; the test
reads the length from plan.info() and asserts that a boundary lies inside a window).

The generator asserts on the reference alone that at most 1e-3 of the window samples have a top-two gap <= 1e-6
(the decode is compared with the reference's arg max everywhere else) and stores the share.

Usage:  python tests/golden/make_blocked_post_at_size.py [--threads N] [case ...]     (default: all cases)
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_estep_at_size as G  # noqa: E402  (model family, hashes; puts the repository root on sys.path)
from oracle import oracle as O  # noqa: E402
from oracle import hp  # noqa: E402
import hmmsort_amd as H  # noqa: E402  (synthetic generator only)
import posterior_model as PM  # noqa: E402

OUT = os.path.join(HERE, "blocked_post_at_size")
W = 1024
GAP = 1e-6

# name: (N, K, T, sigma of the signal, seed)
CASES = {
    "P20a": (2, 20, 1_000_000, 0.3, 201),
    "P20b": (2, 20, 1_000_000, 1.0, 202),
    "P60": (2, 60, 1_000_000, 1.0, 203),
}


def block_length(T, K):
    """blocked_geometry with options block = halo = 0: halo = max(256, 4 (K - 1)) rounded up to 64 samples,
    block = max(2 halo, ceil(T / 1280)) rounded up to 64"""
    h = (max(256, 4 * (K - 1)) + 63) // 64 * 64
    return (max(2 * h, (T + 1279) // 1280) + 63) // 64 * 64


def windows(T, K):
    B = block_length(T, K)
    nb = (T + B - 1) // B
    centres = [B * (nb // 4), B * (nb // 2), B * (3 * nb // 4)]
    return np.array([(0, W), (T - W, T)] + [(c - W // 2, c + W // 2) for c in centres], np.int64)


def inputs(name):
    """(y, oracle StateMatrix, model mu, model sigma, pp, windows): make_estep_at_size.overlap_model, the model
    is 0.9 x the truth with sigma 1.15 x the signal's"""
    N, K, T, sig, seed = CASES[name]
    temps, pp = G.overlap_model(N, K)
    y = H.create_signal(T, sig, pp, temps, seed=seed)
    sm = O.state_matrix(N, K, np.log(pp), True)
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    return y, sm, mu, 1.15 * sig, pp, windows(T, K)


def reference(y, sm, mu, sigma, win, threads=1):
    E, _ = hp.train_step(y, sm, mu, sigma, block=1024, threads=threads, windows=win)
    f = np.float64
    out = dict(sg=E.sg.astype(f), loglik=f(E.loglik), defect=f(E.defect), windows=np.asarray(win, np.int64))
    q = PM.trough_values(mu)
    close = total = 0
    gmin = np.inf
    for i, g in enumerate(E.windows):
        g = g.T                                              # S x W
        on, oc, si = PM.marginals(g, sm.states)
        tr = np.stack([g[sm.states[a] == q[a]].sum(0) for a in range(sm.N)])
        top = np.sort(np.partition(g, -2, axis=0)[-2:], axis=0)
        gap = top[1] - top[0]
        out.update({"w%d_onset" % i: on, "w%d_occ" % i: oc, "w%d_trough" % i: tr, "w%d_silent" % i: si,
                    "w%d_xm" % i: PM.decode(g), "w%d_gap" % i: gap})
        close += int((gap <= GAP).sum())
        total += gap.size
        gmin = min(gmin, float(gap.min()))
    out["close_share"], out["gap_min"] = f(close / total), f(gmin)
    assert close / total <= 1e-3, "reference: %d of %d window samples have a top-two gap <= 1e-6" % (close, total)
    return out


def make(name, threads=1):
    N, K, T, sig, seed = CASES[name]
    y, sm, mu, sigma, pp, win = inputs(name)
    t0 = time.time()
    out = reference(y, sm, mu, sigma, win, threads)
    out.update(G.hashes(y, sm, mu, sigma))
    out.update(N=N, K=K, T=T, sigma_signal=sig, sigma_model=sigma, seed=seed, pp=np.array(pp))
    print("%s: S=%d T=%d  %.0f s  defect=%.3g  share of window samples with gap <= 1e-6: %.3g (min gap %.3g)" % (
        name, sm.nstates, T, time.time() - t0, out["defect"], out["close_share"], out["gap_min"]), flush=True)
    return out


def load(name):
    with np.load(os.path.join(OUT, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def main(argv):
    threads = 1
    if "--threads" in argv:
        i = argv.index("--threads")
        threads = int(argv[i + 1])
        del argv[i:i + 2]
    os.makedirs(OUT, exist_ok=True)
    for name in (argv or list(CASES)):
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **make(name, threads))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
