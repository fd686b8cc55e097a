"""Numpy model of the drift-tracking chunk loop (hmmsort_fit_adaptive): fit.jl:11-42 over the CPU oracle's
viterbi, with the model re-estimated after every chunk from exponentially weighted path statistics
(tests/path_stats_model.py).  Test infrastructure: the CPU test pins its rules and the recall figures, the GPU tests
check the library against its pieces.

Rules restated here from include/hmmsort.h:
  chunk [i, j] (1-based) with trim points l, kk owns the 0-based range [i + l - 2, i + kk - 2), or up to T when it ends
  the recording; w = 2^(-(hi - lo) / halflife); acc <- w acc + new in two rounded steps on all slots but the last three
  (x0, bad0, bad1), which add; once the undecayed owned samples reach `warmup` the accumulator is finished under the
  current model and mu (sigma when asked and finite and > 0; the list when asked) is replaced."""
import numpy as np

import path_stats_model as PS

K_D, SIGMA_D, PP_D, T_D = 16, 0.3, (0.01, 0.006), 48_000


def templates_d(H, K=K_D):
    return np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                       H.create_spike_template(K, 4.0, 0.3, 0.2)], axis=1))


def drifting(H, seed, g, T=T_D, K=K_D):
    """the drifting recording D(seed, g): noise and onsets of create_signal with zero templates, every spike scaled by
    linspace(1, g, T) at its onset.  Returns (y, onsets [(t, template)], templates)."""
    temps = templates_d(H, K)
    y, onsets = H.create_signal(T, SIGMA_D, PP_D, 0 * temps, seed, return_states=True)
    y = y.copy()
    gain = np.linspace(1.0, g, T)
    for t, a in onsets:
        m = min(K, T - t)
        y[t:t + m] += gain[t] * temps[:m, a]
    return y, onsets, temps


def trim(x, lead, trail):
    """fit.jl:24-36 on one decoded chunk: (l, kk), 1-based; l = k + 1 / kk = 0 when no sample is silent"""
    k = len(x)
    silent = np.flatnonzero(np.asarray(x) <= 1)
    l = (int(silent[0]) + 1 if len(silent) else k + 1) if lead else 1
    kk = (int(silent[-1]) + 1 if len(silent) else 0) if trail else k
    return l, kk


def owned(i, l, kk, last, T):
    """the 0-based range [lo, hi) whose statistics the chunk that starts at fit.jl's i contributes"""
    return i + l - 2, (T if last else i + kk - 2)


def blend(acc, w, new, plain_tail=3):
    """hmmsort_stats_blend: the product rounded, then the sum rounded; the last plain_tail entries add"""
    acc, new = np.asarray(acc, dtype=np.float64), np.asarray(new, dtype=np.float64)
    n = len(acc) - plain_tail
    out = acc + new
    prod = np.float64(w) * acc[:n]
    out[:n] = prod + new[:n]
    return out


def weight(n, halflife):
    return float(np.exp2(-np.float64(n) / np.float64(halflife)))


def finish(vec, states, mu):
    """hmmsort_plan_path_finish on a (weighted) statistics vector, from the definitions: dict(mu, sigma, lp, pp, counts).
    Sums in plain numpy order: sigma' agrees with the library within the rounding of the four sums."""
    states = np.asarray(states)
    mu = np.asarray(mu, dtype=np.float64)
    (N, S), K = states.shape, mu.shape[0]
    L = K - 1
    st = PS.split_vector(vec, N, K, S)
    c, s, sm = (np.asarray(st[k]).reshape(N, L).T for k in ("c", "s", "sm"))      # [k-2, l]
    mu_n = np.zeros((K, N), order="F")
    hit = c > 0
    mu_n[1:] = np.where(hit, s / np.where(hit, c, 1.0), mu[1:])
    M = np.zeros(S)
    for l in range(N):
        M += mu_n[states[l] - 1, l]
    tot = st["sum_y2"] - 2.0 * np.sum(mu_n[1:] * (s + sm)) + np.sum(c * mu_n[1:] ** 2) + np.sum(st["nj"] * M * M)
    with np.errstate(divide="ignore", invalid="ignore"):
        sigma = float(np.sqrt(max(tot, 0.0) / st["n"])) if st["n"] else float("nan")
        ent, b = np.asarray(st["ent"]), st["b"]
        lp = np.where((ent == 0) | (b == 0), -np.inf, np.log(np.where(ent > 0, ent, 1.0)) - np.log(b if b > 0 else 1.0))
    pp = np.full(S, -np.inf)
    if 1 <= int(st["x0"]) <= S:
        pp[int(st["x0"]) - 1] = 0.0
    return dict(mu=mu_n, sigma=sigma, lp=lp, pp=pp, counts=[int(st["bad0"]), int(st["bad1"]), int(np.sum(~hit))])


def walk(decode, T, chunksize):
    """fit.jl:11-42 with decode(i, j, c) -> (x, ll) for the chunk [i, j] (1-based) number c: yields
    (c, i, j, x, ll, l, kk, last) for every chunk that finishes, and writes nothing itself"""
    i = j = 1
    c = 0
    while j < T:
        j = min(i + chunksize - 1, T)
        k = j - i + 1
        x, ll = decode(i, j, c)
        l, kk = trim(x, i > 1, j < T)
        if l > k:
            return
        last = not (j < T)
        if i + kk - 1 <= i:
            return
        yield c, i, j, x, ll, l, kk, last
        j = i + kk - 1
        i = j
        c += 1


def fit_adaptive(O, to_oracle, H, y, sm, mu, sigma, chunksize, halflife, warmup=0, update_sigma=True, update_lp=False):
    """the loop.  sm: the product's StateMatrix (rebuilt through StateMatrix.from_states when update_lp); to_oracle:
    conftest.to_oracle_sm.  Returns dict(ml, ll, first, own, w, mu, sigma, lists, final) with one entry per chunk in the
    lists; halflife = inf and warmup = T give the fixed-model loop."""
    y = np.asarray(y, dtype=np.float64)
    T = len(y)
    mu = np.array(mu, dtype=np.float64, order="F", copy=True)
    ring = not sm.resolve_overlaps
    ml = np.ones(T, dtype=np.int16)
    out = dict(ml=ml, ll=0.0, first=[], own=[], w=[], mu=[], sigma=[], lists=[], final=None)
    state = dict(sm=sm, mu=mu, sigma=float(sigma), acc=None, n=0)

    def decode(i, j, c):
        return O.viterbi(y[i - 1:j], to_oracle(O, state["sm"]), state["mu"], state["sigma"])

    for c, i, j, x, ll, l, kk, last in walk(decode, T, chunksize):
        if l <= kk:
            ml[i + l - 2:i + kk - 1] = x[l - 1:kk]
        out["ll"] += ll
        lo, hi = owned(i, l, kk, last, T)
        w = weight(hi - lo, halflife)
        cur = state["sm"]
        out["first"].append(i), out["own"].append((lo, hi)), out["w"].append(w)
        out["mu"].append(state["mu"].copy()), out["sigma"].append(state["sigma"]), out["lists"].append(cur)
        new = PS.vector(PS.path_stats(y, ml, cur.states, cur.transitions, cur.K, by_template=ring, own_lo=lo, own_hi=hi,
                                      first=(i == 1)))
        state["acc"] = blend(np.zeros_like(new) if state["acc"] is None else state["acc"], w, new)
        state["n"] += hi - lo
        if last or state["n"] >= warmup:
            fin = finish(state["acc"], cur.states, state["mu"])
            if last:
                out["final"] = fin
                break
            state["mu"] = np.asfortranarray(fin["mu"])
            if update_sigma and np.isfinite(fin["sigma"]) and fin["sigma"] > 0:
                state["sigma"] = float(fin["sigma"])
            if update_lp:
                state["sm"] = H.StateMatrix.from_states(cur.states, cur.pi, cur.K, fin["lp"].copy(), cur.resolve_overlaps)
    return out


def recall(x, onsets, sm, lo, hi, slack=2):
    """(found, true, extra): onsets (t, a) with lo <= t <= hi that have a sample within +-slack decoded to template a's
    first phase (a state in which a is at row 2), the number of such onsets, and the first-phase samples in
    [lo - slack, hi + slack] that lie within +-slack of no onset of their template anywhere"""
    x = np.asarray(x)
    states = np.asarray(sm.states)
    N = states.shape[0]
    found = true = extra = 0
    for a in range(N):
        sid = np.flatnonzero(states[a] == 2) + 1
        det = np.flatnonzero(np.isin(x, sid))
        ons = np.array([t for t, b in onsets if b == a], dtype=np.int64)
        for t in ons[(ons >= lo) & (ons <= hi)]:
            true += 1
            found += bool(np.any(np.abs(det - t) <= slack))
        for d in det[(det >= lo - slack) & (det <= hi + slack)]:
            extra += not np.any(np.abs(ons - d) <= slack)
    return found, true, extra
