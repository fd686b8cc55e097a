"""Shared cases of the ring-count tests (test_ring_cases_cpu.py, test_gpu_wave_dispatch.py, test_gpu_ring_counts.py):
one small no-overlap model per (number of rings N, templates of K samples, uniform or per-source exit -> entry
values), with its references.  Plain module; every case is built once per session (functools.lru_cache) and nothing
in it is changed afterwards.

Templates  the ring_model family of tests/golden/make_estep_at_size.py with the sign of every second pair of
           templates flipped (templates 2, 3, 6, 7, ... are negative), so that sixteen templates of eight samples stay
           distinguishable.
Signal     create_signal at a low rate (RATES x min(1, 4 / N) x min(1, 20 / K) per sample; the model's entry
           probabilities are the same numbers) at sigma 0.3, plus planted spikes: three per template in a shuffled
           order, every third of them (every second with two templates, which have six) followed directly by another
           template's spike, so that the decoded path takes at least three exit -> entry transitions; gaps of
           max(L / 2, 12) samples.  T is what that needs plus max(512, 4 L) plus 37.
           The wave engine's chains have at least 512 samples, so for the shorter models that T is one or two chains:
           T then grows (by widening every gap alike) until the plan has three chains, and by one more sample if it is
           a multiple of 64.  wave_geometry restates the engine's choice (wave_engine.hip, make_geometry, default
           options); the GPU tests assert that the plan's chain length is the one predicted here.
Model      never the truth: mu = 0.9 x templates, sigma = 1.15 x the signal's, as in the at-size cases.  The planted
           spikes have the model's amplitude, the background spikes the templates': templates i and i + 4 share a
           shape and differ by 13 % in amplitude, so a full-size spike of template i is nearer to the model's template
           i + 4 (0.9 x 1.13) than to its own (0.9), and at full size the lower templates never appear on the path.
per_source the exit -> entry log-probabilities are perturbed by source ring, exactly as
           test_gpu_wave_edges._per_source_list does.
References path and ll: the fp64 oracle (oracle.viterbi).  E-step and M-step: oracle/hp.py, long double
           (make_estep_at_size.reference, the dictionary test_gpu_estep_at_size.check_mstep reads).  Posteriors: the
           reference's gamma on windows -- both ends and 512 samples around every chain boundary -- as onset,
           occupancy and silent marginals.
"""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

SIGMA = 0.3
MODEL_SCALE = 0.9
RATES = [0.003, 0.001, 0.002, 0.0015]

# (N, K, per_source): every ring count at L = K - 1 in {8, 23, 64, 65}; 5..16 rings at L = 128, 129; the lengths at
# which one and two rings change their statistics tiles; two passes over rho; per-source lists for 2..8 rings.  The
# rows these reach are asserted by name in test_gpu_wave_dispatch.py.
# MORE_TILES: what that table leaves out of kw_gsum_mx<N, NT> for up to four rings, each with the shortest ring that
# reaches it: three and four accumulator tiles, and a second pass over rho (one ring: 256 lags per tile; two: 128;
# three and four: 64).
MORE_TILES = [(1, 514, False), (1, 770, False), (1, 1026, False), (2, 258, False), (2, 386, False), (2, 514, False),
              (3, 130, False), (4, 130, False), (3, 194, False), (4, 194, False), (3, 258, False), (4, 258, False)]
CASES = ([(N, K, False) for K in (9, 24, 65, 66) for N in range(1, 17)]
         + [(N, K, False) for K in (129, 130) for N in range(5, 17)]
         + [(1, 258, False), (2, 130, False), (9, 258, False)]
         + [(N, K, True) for K in (9, 24, 66) for N in range(2, 9)]
         + MORE_TILES)


def case_id(c):
    return "%dx%d%s" % (c[0], c[1], "-ps" if c[2] else "")


def templates(N, K):
    import make_estep_at_size as G
    temps, _ = G.ring_model(N, K)
    for i in range(N):
        if (i // 2) % 2:
            temps[:, i] = -temps[:, i]
    return temps


def uniform_entries(sm, N, L):
    """are the exit -> entry log-probabilities (b, L) -> (a, 1) of this list the same for every source ring b, bit for
    bit?  (What the wave engine asks before it takes its uniform kernels: wave_engine.hip, ring_uniform_cx.)"""
    tr = sm.transitions
    for a in range(N):
        v = [lp for s, d, lp in zip(tr["src"], tr["dst"], tr["lp"]) if d == 2 + a * L and s > 1]
        if len(set(v)) > 1:
            return False
    return True


@functools.lru_cache(maxsize=None)
def rates(N, K):
    """The list the reference builds sums the log-probabilities in template order, and for some rates the sums of two
    source rings differ in the last bit: such a list is a per-source list to the engine.  The uniform cases must
    reach the uniform kernels, so the rates are scaled by 1, 63/64, 62/64, ... until the list is uniform bit for bit."""
    import hmmsort_amd as H
    for j in range(32):
        pp = [RATES[i % 4] * min(1.0, 4.0 / N) * min(1.0, 20.0 / K) * (64 - j) / 64.0 for i in range(N)]
        if uniform_entries(H.StateMatrix.create(N, K, np.log(pp), False), N, K - 1):
            return pp
    raise AssertionError("no uniform list for %d x %d" % (N, K))


def wave_geometry(T, L):
    """(chain length, chains) of a one-channel wave plan with default options (wave_engine.hip, make_geometry)"""
    W = min(L, 64)
    H = max(256, 4 * L, L + 8)
    Hw = 1 + -(-H // W) * W
    B = max((T + 2047) // 2048, 2 * Hw, 512)
    B = -(-B // 64) * 64
    if B > T:
        B = -(-T // 64) * 64
    while True:
        nch = -(-T // B)
        if nch == 1 or T - (nch - 1) * B >= L:
            return B, nch
        B += 64


def planted(N, L, seed):
    """[(template, followed directly by this template or None)]: three spikes per template, shuffled"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(np.repeat(np.arange(N), 3)).tolist()
    out = []
    every = 3 if N >= 3 else 2            # two templates have six planted spikes: every second, for three pairs
    for i, a in enumerate(order):
        b = None
        if N > 1 and i % every == every - 1:
            b = (a + 1 + i // every) % N
            if b == a:
                b = (a + 1) % N
        out.append((a, b))
    return out


def signal(N, K, seed):
    """(y, templates, rates): the length is fixed by the planted spikes and the plan's geometry (module docstring)"""
    L = K - 1
    temps, pp = templates(N, K), rates(N, K)
    plan = planted(N, L, seed)
    gap = max(L // 2, 12)
    need = sum(L + (L if b is not None else 0) for _, b in plan)

    def length(gap):
        T = L + 16 + need + gap * len(plan) + max(512, 4 * L) + 37
        return T + (1 if T % 64 == 0 else 0)
    while wave_geometry(length(gap), L)[1] < 3:
        gap += 1
    T = length(gap)
    import hmmsort_amd as H
    y = H.create_signal(T, SIGMA, pp, temps, seed=seed)
    t = L + 16
    for a, b in plan:
        y[t:t + L] += MODEL_SCALE * temps[1:, a]
        t += L
        if b is not None:
            y[t:t + L] += MODEL_SCALE * temps[1:, b]
            t += L
        t += gap
    assert t + max(512, 4 * L) <= T
    return y, temps, pp


def windows(T, B):
    """disjoint sample ranges: both ends and 512 samples around every chain boundary"""
    w = [(0, min(512, T)), (max(T - 512, 0), T)] + [(b - 256, min(b + 256, T)) for b in range(B, T, B)]
    w.sort()
    out = [list(w[0])]
    for lo, hi in w[1:]:
        if lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return np.array(out, np.int64)


# (N, K, per_source) -> seed, where the default 1000 + 16 K + N does not meet test_ring_cases_cpu.py (a background
# spike on a planted pair: two exit -> entry transitions instead of three; a template without an onset)
SEEDS = {(2, 24, False): 1, (3, 24, False): 1, (6, 24, False): 1, (4, 65, False): 2, (5, 66, False): 1,
         (2, 24, True): 1, (3, 24, True): 1,
         # long smooth templates: a planted pair is often decoded with one silent sample between its spikes
         (2, 514, False): 3, (3, 194, False): 12, (4, 194, False): 1, (3, 258, False): 2}


@functools.lru_cache(maxsize=None)
def case(N, K, per_source=False):
    import hmmsort_amd as H
    import make_estep_at_size as G
    from conftest import to_oracle_sm
    from oracle import oracle as O
    O.build()
    seed = SEEDS.get((N, K, per_source), 1000 + 16 * K + N)
    y, temps, pp = signal(N, K, seed)
    T, L = len(y), K - 1
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    if per_source:
        from test_gpu_wave_edges import _per_source_list
        sm = _per_source_list(H, sm, N, K, np.random.default_rng(seed))
    osm = to_oracle_sm(O, sm)
    mu = np.asfortranarray(temps * MODEL_SCALE)
    mu[0, :] = 0
    sigma = 1.15 * SIGMA
    B, nch = wave_geometry(T, L)
    win = windows(T, B)
    xo, llo = O.viterbi(y, osm, mu, sigma)
    ref = G.reference(y, osm, mu, sigma, win, threads=16)
    for v in (y, mu, xo, win):
        v.setflags(write=False)
    return dict(N=N, K=K, L=L, T=T, per_source=per_source, y=y, temps=temps, pp=pp, sm=sm, osm=osm, mu=mu, sigma=sigma,
                block=B, nchains=nch, win=win, x=xo, ll=llo, ref=ref, uniform=uniform_entries(sm, N, L))


def lag_tile(N):
    """lags per accumulator tile of kw_gsum_mx by ring-count class (rings padded to 1, 2, 4, 8, 16)"""
    return 256 if N == 1 else 128 if N == 2 else 64 if N <= 4 else 32 if N <= 8 else 16


def expected_row(N, L, per_source, call, light=False, env=None, chains=3):
    """The row a wave plan of this shape is MEANT to run, as DESIGN section 3.10 words it, in the notation of
    hmmsort_selftest_wave_dispatch.  call: 1 decode, 2 E-step, 3 decode + E-step, 4 posteriors; light: the light
    backtrace (option "backtrace" = 2, or the automatic choice of a fused call); env: HMMSORT_GSUM_SEPARATE or
    HMMSORT_GSUM_GENERIC set.  Spot rows are pinned as literals in test_ring_cases_cpu.py."""
    # (with two rings every ring has ONE source: any such list is uniform, kw_*<2, false> cannot be reached)
    u = "ps" if per_source and N >= 3 else "uc"
    per_source = u == "ps"
    parts = ["prepass<%d>" % N]
    if call != 1:
        post = call == 4
        ft = 0
        if not post and env is None:
            if N in (3, 4) and L <= 64:
                ft = 1
            elif 5 <= N <= 8 and not per_source:
                ft = 2 if L <= 64 else 4 if L <= 128 else 0
        parts.append("fwd<%d,%s%s>" % (N, u, ",logdl" if N > 8 else ""))
        parts.append("bwd<%d,%s,ft%d%s>" % (N, u, ft, ",gs" if post else ""))
        if post:
            parts.append("gsum=none")
        elif ft:
            parts.append("gsum=bwd")
        elif env == "HMMSORT_GSUM_GENERIC":
            parts.append("gsum=generic")
        else:
            ntx = -(-L // lag_tile(N))
            nt = (4 if ntx <= 4 else 8 if ntx <= 8 else 16) if N > 8 else min(ntx, 4)
            parts.append("gsum=mx<%d,%d>x%d" % (N, nt, -(-ntx // nt)))
    if call in (1, 3):
        parts.append("vit<%d,%s>" % (N, u))
        parts.append("redo<%d,%s%s>" % (N, u, ",tight" if call == 3 and N <= 4 else "") if chains > 1 else "redo=none")
        # one word of back-pointers per sample up to 7 rings (8 entries of 4 bits): 32 segments per workgroup
        parts.append("backtrace=light<%d,%d>" % (N, 32 if N <= 7 else 64) if light else "backtrace=rows<%d>" % N)
    return " ".join(parts)


def onsets(c):
    """samples at which the oracle's path enters each ring, and the number of exit -> entry transitions on it"""
    x, L, N = c["x"].astype(np.int64), c["L"], c["N"]
    first = (x > 1) & ((x - 2) % L == 0)
    per_ring = [int(np.count_nonzero(first & ((x - 2) // L == a))) for a in range(N)]
    direct = int(np.count_nonzero((x[:-1] > 1) & ((x[:-1] - 2) % L == L - 1) & (x[1:] > 1)))
    return per_ring, direct
