"""Numpy model of the per-spike fit (hmmsort_spike_fit): a plain loop over events and phases plus the
two-level summary fold.  Test infrastructure: the CPU test pins its rules and the drift figures, the GPU tests ask the
library for the same bits.

Rules restated here from include/hmmsort.h (all arithmetic in IEEE doubles, product and sum rounded separately):
  events   template a at 0-based t when x[t] in 1..S and states[a, x[t]] == qv_a = first arg min of the BASE mu[:, a], + 1;
           qv_a == 1 is refused.
  model    M = mu, or M = track mu[c] for the last chunk c with first[c] <= t + 1; none: NaN event, nused = 0.
  window   k = 2..K ascending, u = t + (k - qv_a); used iff 0 <= u < T, x[u] in 1..S, states[a, x[u]] == k.
  phase    oth = 0.0, += M[states[b, x[u]] - 1, b] for b ascending, b != a;  r = y[u] - oth;  m = M[k - 1, a].
  event    srm += r*m, smm += m*m, energy += r*r, rss += (r - m)*(r - m), serial from 0.0;  amp = srm / smm.
  summary  [n, n_full, sum amp, sum amp*amp, sum rss, sum energy (full events), sum nused (all), smm of the base template,
           wsum (K-1), wsq (K-1), wcnt (K-1)]; per slot: events in blocks of 256, each block folded serially from 0.0 in
           event order, the block partials folded serially from 0.0 in block order."""
import numpy as np

BLOCK = 256


def trough_value(mu, a):
    return int(np.argmin(np.asarray(mu)[:, a])) + 1


def fold2(contrib):
    """the two-level fold of one slot: contrib[e] is event e's term, None where the event does not enter"""
    parts = []
    for b in range(0, len(contrib), BLOCK):
        v = 0.0
        for c in contrib[b:b + BLOCK]:
            if c is not None:
                v += c
        parts.append(v)
    tot = 0.0
    for p in parts:
        tot += p
    return tot


def events(x, states, qv, a):
    x = np.asarray(x).astype(np.int64)
    S = states.shape[1]
    ok = (x >= 1) & (x <= S)
    return np.flatnonzero(ok & (states[a, np.clip(x, 1, S) - 1] == qv))


def fit_template(y, x, states, mu, a, track=None):
    """dict(times (1-based), amp, rss, energy, nused, summary) of template a"""
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x).astype(np.int64)
    states = np.asarray(states).astype(np.int64)
    mu = np.asarray(mu, dtype=np.float64)
    (N, S), K, T = states.shape, mu.shape[0], len(x)
    P = K - 1
    qv = trough_value(mu, a)
    if qv == 1:
        raise ValueError("template %d has its minimum in the silent row" % a)
    ts = events(x, states, qv, a)
    n = len(ts)
    amp, rss, energy = np.zeros(n), np.zeros(n), np.zeros(n)
    nused = np.zeros(n, dtype=np.int32)
    R = [[None] * n for _ in range(P)]          # r per (phase, event), None where unused
    for e, t in enumerate(ts):
        M = mu
        if track is not None:
            first, mus = track
            c = int(np.searchsorted(np.asarray(first), t + 1, side="right")) - 1
            if c < 0:
                amp[e] = rss[e] = energy[e] = np.nan
                continue
            M = np.asarray(mus[c], dtype=np.float64)
        srm = smm = en = rs = 0.0
        for k in range(2, K + 1):
            u = int(t) + (k - qv)
            if not (0 <= u < T) or not (1 <= x[u] <= S) or states[a, x[u] - 1] != k:
                continue
            oth = 0.0
            for b in range(N):
                if b != a:
                    oth += float(M[states[b, x[u] - 1] - 1, b])
            r = float(y[u]) - oth
            m = float(M[k - 1, a])
            d = r - m
            srm += r * m
            smm += m * m
            en += r * r
            rs += d * d
            nused[e] += 1
            R[k - 2][e] = r
        with np.errstate(divide="ignore", invalid="ignore"):
            amp[e] = np.float64(srm) / np.float64(smm)
        rss[e], energy[e] = rs, en
    full = nused == P
    pick = lambda v: [float(q) if f else None for q, f in zip(v, full)]  # noqa: E731
    base = 0.0
    for k in range(2, K + 1):
        base += float(mu[k - 1, a]) * float(mu[k - 1, a])
    head = [fold2([1.0] * n), fold2(pick(np.ones(n))), fold2(pick(amp)), fold2(pick(amp * amp)), fold2(pick(rss)),
            fold2(pick(energy)), fold2([float(q) for q in nused]), base]
    wsum = [fold2(R[j]) for j in range(P)]
    wsq = [fold2([None if r is None else r * r for r in R[j]]) for j in range(P)]
    wcnt = [fold2([None if r is None else 1.0 for r in R[j]]) for j in range(P)]
    return dict(times=ts + 1, amp=amp, rss=rss, energy=energy, nused=nused,
                summary=np.array(head + wsum + wsq + wcnt, dtype=np.float64), R=R)


def spike_fit(y, x, states, mu, track=None):
    """one fit_template result per template"""
    return [fit_template(y, x, states, mu, a, track) for a in range(np.asarray(states).shape[0])]


def get_energy(waveforms, cinv):
    """utils.jl:112-124 as a literal loop"""
    W = np.asarray(waveforms, dtype=np.float64)
    ee = np.zeros(W.shape[1])
    for i in range(W.shape[1]):
        s = 0.0
        for j in range(W.shape[0]):
            w = float(W[j, i])
            s += w * float(cinv) * w
        ee[i] = s
    return ee
