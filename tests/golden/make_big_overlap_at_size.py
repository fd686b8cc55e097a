"""Generates tests/golden/big_overlap_at_size/<case>.npz FROM THE EXTENDED-PRECISION REFERENCE
(oracle/hp_estep.c through oracle/hp.py): one Baum-Welch step and the posterior marginals of the three- and
four-template overlap models at K = 60 (10 621 and 21 123 states) on 200 000 samples, for
tests/test_gpu_blocked_big.py.  These models do not fit the LDS columns of the blocked E-step; they run on its
device-memory-column kernels (csrc/generic_estep_big.hip, option "blocked_hbm_columns").  CPU only; about 4 and 7
minutes with 8 threads.

Each fixture holds the case's parameters, SHA-256 of y and of the model arrays, sum_t gamma_t(j) of every state, the
log-likelihood, the reference's M-step (mu, sigma, lp), and per window: onset, occ, trough mass per template, silent,
the reference's arg-max state and the gap between its two largest posteriors (reference() and the window layout are
make_blocked_post_at_size's).  The GPU test regenerates the inputs from the seed, compares the hashes, and recomputes
the reference live on a mismatch.

Windows: 1 024 samples at each end and around the middle one of make_blocked_post_at_size's three interior block
boundaries: three windows, not five, keep the four-template fixture (13 marginals per sample and 21 123 state sums)
under the 600 KB of the largest fixture committed before it; main() asserts the size.

The generator asserts on the reference alone that at most 1e-3 of the window samples have a top-two gap <= 1e-6 and
stores the share (make_blocked_post_at_size.reference).

Usage:  python tests/golden/make_big_overlap_at_size.py [--threads N] [case ...]     (default: all cases)
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_estep_at_size as G  # noqa: E402  (template family, hashes; puts the repository root on sys.path)
import make_blocked_post_at_size as P  # noqa: E402  (reference(), windows())
from oracle import oracle as O  # noqa: E402
from oracle import hp  # noqa: E402
import hmmsort_amd as H  # noqa: E402  (synthetic generator only)

OUT = os.path.join(HERE, "big_overlap_at_size")
MAX_BYTES = 600 * 1024
RATES = [0.012, 0.008, 0.006, 0.005]      # make_estep_at_size.overlap_model has three; the fourth template its own

# name: (N, K, T, sigma of the signal, seed)
CASES = {
    "M3": (3, 60, 200_000, 1.0, 301),
    "M4": (4, 60, 200_000, 1.0, 302),
}


def overlap_model(N, K):
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *G.BASE[i]) for i in range(N)], 1))
    return temps, RATES[:N]


def windows(T, K):
    w = P.windows(T, K)
    return w[[0, 3, 1]].copy()            # start, the middle interior block boundary, end


def inputs(name):
    """(y, oracle StateMatrix, model mu, model sigma, pp, windows); the model is 0.9 x the truth with sigma
    1.15 x the signal's, as in the other at-size fixtures"""
    N, K, T, sig, seed = CASES[name]
    temps, pp = overlap_model(N, K)
    y = H.create_signal(T, sig, pp, temps, seed=seed)
    sm = O.state_matrix(N, K, np.log(pp), True)
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    return y, sm, mu, 1.15 * sig, pp, windows(T, K)


def reference(y, sm, mu, sigma, win, threads=1):
    """make_blocked_post_at_size.reference plus the reference's M-step; one sweep of the reference serves both"""
    keep = {}
    inner = hp.train_step

    def once(*a, **k):
        keep["EM"] = inner(*a, **k)
        return keep["EM"]
    hp.train_step = once
    try:
        out = P.reference(y, sm, mu, sigma, win, threads)
    finally:
        hp.train_step = inner
    M = keep["EM"][1]
    out.update(mu_new=M.mu, sigma_new=np.float64(M.sigma), lp_new=M.lp_new)
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
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **make(name, threads))
        size = os.path.getsize(path)
        print("%s: %d bytes" % (path, size), flush=True)
        assert size <= MAX_BYTES, "%s is %d bytes, over the %d allowed" % (path, size, MAX_BYTES)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
