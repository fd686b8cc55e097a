"""Generates tests/golden/estep_at_size/<case>.npz FROM THE EXTENDED-PRECISION REFERENCE
(oracle/hp_estep.c through oracle/hp.py): one Baum-Welch step at the sizes the headline numbers
are quoted at, too slow to recompute in every test run (~1 min of CPU per million samples at
237 states).  CPU only: the signal generator is pure numpy and the state space is the oracle's.

Each fixture holds the seed/shape/model parameters, SHA-256 of y and of the model arrays, the
reference's statistics and M-step output rounded once to double, and -- for the cases with
windows -- the posterior marginals on those windows (1 024 samples each, one of 5 120 at 10 M).  The GPU tests regenerate the
inputs from the seed, compare the hashes, and recompute the reference live on a mismatch.

Usage:  python tests/golden/make_estep_at_size.py [--threads N] [case ...]     (default: all cases)
        python tests/golden/make_estep_at_size.py --check <case>      recompute, compare bit for bit
"""
import hashlib
import os
import resource
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from oracle import oracle as O  # noqa: E402
from oracle import hp  # noqa: E402
import hmmsort_amd as H  # noqa: E402  (synthetic generator only)
import posterior_model as PM  # noqa: E402

OUT = os.path.join(HERE, "estep_at_size")
M20 = 1 << 20
BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
W = 1024


def ring_model(N, K):
    """bench.py's model family (4 x 60 = the headline model; 8 x 128, 16 x 256 = configs 4, 5)"""
    amps = [(BASE[i % 4][0] * (1 + 0.13 * (i // 4)), BASE[i % 4][1] + 0.03 * (i // 4), BASE[i % 4][2])
            for i in range(N)]
    pp = [[0.003, 0.001, 0.002, 0.0015][i % 4] * (60.0 / K) for i in range(N)]
    return np.asfortranarray(np.stack([H.create_spike_template(K, *a) for a in amps], 1)), pp


def overlap_model(N, K):
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *BASE[i]) for i in range(N)], 1))
    return temps, [0.012, 0.008, 0.006][:N]


def windows(T, centres):
    """the two ends and 1 024 samples around each centre.  The centres are multiples of every power-of-two chain
    length; the wave engine's chains are multiples of 64 samples, not powers of two (4 928 at 10 M samples), so at
    10 M a sixth window of 5 120 samples around 4 * 2^20 holds a chain boundary whatever length up to 5 120 the plan
    picks (at 1 M and below the chains are shorter than 1 024 samples)"""
    w = [(0, W), (T - W, T)] + [(c - W // 2, c + W // 2) for c in centres]
    if T >= 1 << 23:
        w.append((4 * M20 - 2560, 4 * M20 + 2560))
    return np.array(w, np.int64)


# name: (N, K, overlaps, T, sigma of the signal, seed, window centres or None, spikes cut by the edges)
CASES = {
    "A": (4, 60, False, 10_000_000, 0.3, 101, (1 * M20, 4 * M20, 7 * M20), False),
    "B": (4, 60, False, 10_000_000, 1.0, 102, (1 * M20, 4 * M20, 7 * M20), False),
    "C03": (4, 60, False, 1_000_000, 0.3, 103, None, False),
    "C10": (4, 60, False, 1_000_000, 1.0, 104, None, False),
    "C03odd": (4, 60, False, 1_000_001, 0.3, 105, None, False),
    "C10odd": (4, 60, False, 1_000_001, 1.0, 106, None, False),
    "D": (8, 128, False, 1_000_000, 0.3, 107, None, False),
    "E": (16, 256, False, 500_000, 0.3, 108, None, False),
    # T = 10^6 < 2^20: the interior windows sit on multiples of 2^18 instead
    "F": (4, 60, False, 1_000_000, 1.0, 109, (1 << 18, 2 << 18, 3 << 18), True),
    "G03": (4, 60, False, 200_000, 0.3, 110, (1 << 16, 1 << 17), False),
    "G10": (4, 60, False, 200_000, 1.0, 111, (1 << 16, 1 << 17), False),
    "H": (2, 20, True, 1_000_000, 0.3, 112, None, False),
}
LIVE = ("G03", "G10")          # cheap enough (~15 s) to be computed in the test run itself


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def inputs(name):
    """(y, oracle StateMatrix, model mu, model sigma, true templates, pp, windows) of a case.  The model is
    never the truth: mu = 0.9 x templates, sigma = 1.15 x the signal's, so wrong statistics move the M-step."""
    N, K, ov, T, sig, seed, centres, cut = CASES[name]
    temps, pp = overlap_model(N, K) if ov else ring_model(N, K)
    y = H.create_signal(T, sig, pp, temps, seed=seed)
    if cut:
        # the recording starts 25 samples into a spike of template 0 and ends 30 samples into one of template 2
        y[:K - 25] += temps[25:, 0]
        y[T - 30:] += temps[:30, 2]
    sm = O.state_matrix(N, K, np.log(pp), ov)
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    win = windows(T, centres) if centres is not None else np.zeros((0, 2), np.int64)
    return y, sm, mu, 1.15 * sig, temps, pp, win


def hashes(y, sm, mu, sigma):
    return dict(sha_y=sha(y), sha_model=sha(np.r_[sm.src, sm.dst].astype(np.int64)) + sha(sm.val) + sha(mu)
                + sha(np.array([sigma])))


def reference(y, sm, mu, sigma, win, threads=1, block=1024):
    """dict of the reference's outputs, rounded once to double"""
    E, M = hp.train_step(y, sm, mu, sigma, block=block, threads=threads, windows=win)
    f = np.float64
    out = dict(sg=E.sg.astype(f), sgy=E.sgy.astype(f), sgd2=E.sgd2.astype(f), sxi=E.sxi.astype(f),
               g0=E.g0.astype(f), gl=E.gl.astype(f), loglik=f(E.loglik), defect=f(E.defect),
               mass_minus_T=f(E.sg.sum() - len(y)), sum_y2=f((y.astype(hp.LD) ** 2).sum()),
               mu_new=M.mu, sigma_new=f(M.sigma), lp_new=M.lp_new, pp_new=M.pp, windows=win)
    for i, g in enumerate(E.windows):
        on, oc, si = PM.marginals(g.T, sm.states)
        out["w%d_onset" % i], out["w%d_occ" % i], out["w%d_silent" % i] = on, oc, si
    return out


def make(name, threads=1):
    N, K, ov, T, sig, seed, centres, cut = CASES[name]
    y, sm, mu, sigma, temps, pp, win = inputs(name)
    t0 = time.time()
    out = reference(y, sm, mu, sigma, win, threads)
    out.update(hashes(y, sm, mu, sigma))
    out.update(N=N, K=K, overlaps=int(ov), T=T, sigma_signal=sig, sigma_model=sigma, seed=seed, cut=int(cut),
               pp=np.array(pp), mu_model=mu)
    print("%s: S=%d T=%d  %.0f s  mass-T=%.3g defect=%.3g  peak RSS %.0f MB" % (
        name, sm.nstates, T, time.time() - t0, out["mass_minus_T"], out["defect"],
        resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0), flush=True)
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
    if argv and argv[0] == "--check":
        new, old = make(argv[1], threads), load(argv[1])
        bad = [k for k in old if not np.array_equal(np.asarray(new[k]), old[k], equal_nan=np.asarray(new[k]).dtype.kind == "f")]
        print("check %s: %s" % (argv[1], "bitwise equal" if not bad else "DIFFERS in %s" % bad))
        return 1 if bad else 0
    os.makedirs(OUT, exist_ok=True)
    for name in (argv or [c for c in CASES if c not in LIVE]):
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **make(name, threads))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
