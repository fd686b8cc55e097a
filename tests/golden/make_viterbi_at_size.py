"""Generates tests/golden/viterbi_at_size/<case>.npz FROM THE EXTENDED-PRECISION MAP REFERENCE
(oracle/hp_viterbi.c through oracle/hp.py): the maximum-a-posteriori path at the sizes the decode's headline
numbers are quoted at, too slow to recompute in every test run (~10 s of CPU per million samples at 237 states,
minutes at the overlap models).  CPU only: the signal generator is pure numpy and the state space is the oracle's.

Each fixture holds the seed/shape/model parameters, SHA-256 of y and of the model arrays, the reference's path in
run-length code, its score and ll (long double rounded once to double, and the residual of that rounding), and the
cumulative score at every stored sample.  The GPU tests regenerate the inputs from the seed, compare the hashes,
and recompute the reference live on a mismatch.

Run-length code of a path.  succ(j) is the destination of the first listed transition that leaves state j (silent
stays silent, a ring state advances, a ring's last state falls silent).  A sample t is stored, with its state, when
t = 0 or x_t != succ(x_{t-1}): one entry per spike and one per decision that is not the default.

Usage:  python tests/golden/make_viterbi_at_size.py [--threads N] [case ...]     (default: all cases)
        python tests/golden/make_viterbi_at_size.py --check <case>      recompute, compare bit for bit
"""
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
sys.path.insert(0, HERE)

from oracle import oracle as O  # noqa: E402
from oracle import hp  # noqa: E402
import hmmsort_amd as H  # noqa: E402  (synthetic generator only)
import make_estep_at_size as E  # noqa: E402

OUT = os.path.join(HERE, "viterbi_at_size")

# cases whose inputs are those of the E-step fixtures of the same name (model = 0.9 x truth, sigma x 1.15)
SHARED = ("A", "B", "C03odd", "C10odd", "D", "E", "F", "H")
# name: (N, K, overlaps, T, sigma, seed) of the cases defined here (model = truth)
OWN = {
    "P60": (2, 60, True, 2_000_000, 0.3, 77),       # tests/test_gpu_fullsize.py, overlap decode at 2 M
    "M3": (3, 20, True, 300_000, 0.3, 21),          # tests/test_gpu_blocked.py, _multi_case
    "CLI": (4, 60, True, 400_000, 0.3, 11),         # _multi_case(H, 4, 60, 400_000, 11): 21 123 states
    "DUP": (4, 60, False, 2_000_000, 0.3, 113),     # templates 1 = 2: every spike of theirs an exact tie
}
CASES = SHARED + tuple(OWN)
LIVE = ("G03", "G10")       # the E-step cases of that name: cheap enough to be computed in the test run itself
DUPLICATES = ("DUP",)       # exempt from the cap on differing samples, not from the acceptance rule


def shape(name):
    """(N, K, overlaps, T)"""
    return E.CASES[name][:4] if name in E.CASES else OWN[name][:4]


def _multi_signal(N, K, T, seed):
    """the signal of tests/test_gpu_blocked.py::_multi_case: overlapping pairs at random offsets, a third spike
    as the first ends"""
    rng = np.random.default_rng(seed)
    shapes = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15), (2.0, 0.4, 0.3)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *shapes[i]) for i in range(N)], 1))
    pp = [0.004, 0.002, 0.003, 0.0025, 0.002][:N]
    pp = [p * min(1.0, 30.0 / K) for p in pp]
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    L = K - 1
    for _ in range(max(6, T // 3000)):
        t0 = int(rng.integers(L, T - 4 * L))
        d = int(rng.integers(0, L))
        a, b = rng.choice(N, 2, replace=False)
        y[t0:t0 + L] += temps[1:, a]
        y[t0 + d:t0 + d + L] += temps[1:, b]
        if rng.random() < 0.5:
            c = int(rng.choice([q for q in range(N) if q != a]))
            y[t0 + L:t0 + 2 * L] += temps[1:, c]
    return y, temps, pp


def inputs(name):
    """(y, oracle StateMatrix, model mu, model sigma, pp) of a case"""
    if name in E.CASES:
        y, sm, mu, sigma, temps, pp, _ = E.inputs(name)
        return y, sm, mu, sigma, pp
    N, K, ov, T, sig, seed = OWN[name]
    if name == "P60":
        temps = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                            H.create_spike_template(K, 4.0, 0.3, 0.2)], 1))
        pp = [0.003, 0.001]
        y = H.create_signal(T, sig, pp, temps, seed=seed)
        rng = np.random.default_rng(5)
        for t0 in rng.integers(1000, T - 1000, 200):
            y[t0:t0 + K] += temps[:, 0]
            y[t0 + 17:t0 + 17 + K] += temps[:, 1]
    elif name in ("M3", "CLI"):
        y, temps, pp = _multi_signal(N, K, T, seed)
    elif name == "DUP":
        temps, pp = E.ring_model(N, K)
        temps[:, 1] = temps[:, 0]
        pp[1] = pp[0]
        temps = np.asfortranarray(temps)
        y = H.create_signal(T, sig, pp, temps, seed=seed)
    else:
        temps, pp = E.ring_model(N, K)
        y = H.create_signal(T, sig, pp, temps, seed=seed)
    sm = O.state_matrix(N, K, np.log(pp), ov)
    mu = temps.copy(order="F")
    if name in ("M3", "CLI"):
        mu[0, :] = 0.0
    return y, sm, mu, sig, pp


def hashes(y, sm, mu, sigma):
    return E.hashes(y, sm, mu, sigma)


def successor(sm):
    """succ[j] (1-based, entry 0 unused) = destination of the first listed transition that leaves j"""
    src, dst = np.asarray(sm.src, np.int64), np.asarray(sm.dst, np.int64)
    succ = np.zeros(sm.nstates + 1, np.int64)
    _, first = np.unique(src, return_index=True)
    succ[src[first]] = dst[first]
    return succ


def encode(x, sm):
    succ = successor(sm)
    x = np.asarray(x, np.int64)
    idx = np.r_[0, np.nonzero(x[1:] != succ[x[:-1]])[0] + 1]
    return idx.astype(np.int64), x[idx].astype(np.int32)


def decode(idx, st, T, sm):
    """the path of a run-length code; the orbit of every stored state under succ must reach a fixed point"""
    succ = successor(sm)
    idx, st = np.asarray(idx, np.int64), np.asarray(st, np.int64)
    seg = np.diff(np.r_[idx, T])
    rows, depth = [st], 0
    while True:
        nxt = succ[rows[-1]]
        rows.append(nxt)
        depth += 1
        if np.all((succ[nxt] == nxt) | (seg <= depth)):
            break
        if depth > 4 * sm.K + 4:
            raise ValueError("a stored state's orbit under succ does not settle: not a run-length code of this model")
    orb = np.stack(rows, 1)                         # orb[k, d] = succ^d(st[k]), constant beyond the last column
    k = np.repeat(np.arange(len(idx)), seg)
    d = np.minimum(np.arange(T) - idx[k], orb.shape[1] - 1)
    return orb[k, d].astype(np.int32)


def reference(y, sm, mu, sigma, threads=1, block=1024):
    """dict of the reference's outputs"""
    M = hp.viterbi(y, sm, mu, sigma, block=block, threads=threads, idx=np.arange(len(y)))
    idx, st = encode(M.x, sm)
    assert np.array_equal(decode(idx, st, len(y), sm), M.x), "the run-length code does not reproduce the path"
    f = np.float64
    return dict(idx=idx, state=st, cum=M.cum[idx].astype(f), score=f(M.score), score_lo=f(M.score - f(M.score)),
                ll=f(M.ll), ll_lo=f(M.ll - f(M.ll)), dmax=f(M.dmax))


def make(name, threads=1):
    N, K, ov, T = shape(name)
    y, sm, mu, sigma, pp = inputs(name)
    t0 = time.time()
    out = reference(y, sm, mu, sigma, threads)
    out.update(hashes(y, sm, mu, sigma))
    out.update(N=N, K=K, overlaps=int(ov), T=T, sigma_model=sigma, pp=np.array(pp), mu_model=mu)
    print("%s: S=%d T=%d  %.0f s  %d stored samples  score %.6f  peak RSS %.0f MB" % (
        name, sm.nstates, T, time.time() - t0, len(out["idx"]), out["score"],
        resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0), flush=True)
    return out


def load(name):
    with np.load(os.path.join(OUT, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def save(name, out):
    out = dict(out)
    out["didx"] = np.diff(np.r_[0, out.pop("idx")]).astype(np.uint32)      # gaps compress better than indices
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)


def unpack(z):
    z = dict(z)
    if "didx" in z:
        z["idx"] = np.cumsum(z.pop("didx").astype(np.int64))
    return z


def main(argv):
    threads = 1
    if "--threads" in argv:
        i = argv.index("--threads")
        threads = int(argv[i + 1])
        del argv[i:i + 2]
    if argv and argv[0] == "--check":
        new, old = make(argv[1], threads), unpack(load(argv[1]))
        bad = [k for k in old if not np.array_equal(np.asarray(new[k]), old[k])]
        print("check %s: %s" % (argv[1], "bitwise equal" if not bad else "DIFFERS in %s" % bad))
        return 1 if bad else 0
    os.makedirs(OUT, exist_ok=True)
    for name in (argv or CASES):
        save(name, make(name, threads))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
