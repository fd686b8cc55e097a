"""Correlograms on resident paths (hmmsort_plan_correlograms) and on host lists (hmmsort_correlograms).

Shape 1, the plan form: BASELINE config 4's one-GPU share -- a batched wave plan of 8 channels x 10 M samples with the
headline 4 x 60 ring model, decoded once; then Plan.correlograms(d_x) with bin 30, half_bins 50, refractory 30,
coincidence 2 is timed with device events around the call (it synchronises its stream; the events cover compaction,
the three kernels and the copies of the counts), median of the timed calls after warm-up.  The result is compared with
a numpy searchsorted model on the same lists (every entry), and that model's host time is reported for context: the
one condition this script checks is that the device call is not slower than it.
Shape 2, the host form: 256 synthetic units at the same density (Poisson-like trains with a refractory gap), host
lists in, counts out, timed with a host clock (upload and the 52 MB of counts coming back included); the numpy model is
timed on a sample of the 65 536 ordered pairs and scaled.
Increments (pairs inside the window) are counted by the script from the lists and must equal the sum of the counts.
Per-kernel split: run this script under `rocprofv3 --kernel-trace --stats` with --reps 3 --no-numpy.

    python scripts/bench_correlograms.py [--channels 8] [--samples 10000000] [--reps 10] [--units 256] [--no-numpy]
"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hmmsort_amd as H  # noqa: E402

BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
PP = [0.003, 0.001, 0.002, 0.0015]
OPTS = dict(bin=30, half_bins=50, refractory=30, coincidence=2)


def numpy_pair(tu, tv, b, Hb, same):
    """one correlogram by searchsorted and an enumeration of the pairs inside the window"""
    W = Hb * b
    lo, hi = np.searchsorted(tv, tu - W, "left"), np.searchsorted(tv, tu + W, "left")
    cnt = hi - lo
    first = np.cumsum(cnt) - cnt
    j = np.arange(int(cnt.sum())) - np.repeat(first, cnt) + np.repeat(lo, cnt)
    d = tv[j] - np.repeat(tu, cnt)
    h = np.bincount((d + W) // b, minlength=2 * Hb)
    if same:
        h[Hb] -= len(tu)
    return h


def increments(lists, W):
    """pairs (i, j), i != j, over all units with -W <= t_j - t_i < W"""
    a = np.sort(np.concatenate(lists))
    return int(np.sum(np.searchsorted(a, a + W, "left") - np.searchsorted(a, a - W, "left")) - len(a))


def numpy_model(lists, pairs, b, Hb):
    t0 = time.perf_counter()
    out = {(u, v): numpy_pair(lists[u], lists[v], b, Hb, u == v) for u, v in pairs}
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--states", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--units", type=int, default=256)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_correlograms.py needs a GPU"
    nC, T, K, N = a.channels, a.samples, a.states, 4
    b, Hb = OPTS["bin"], OPTS["half_bins"]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p) for p in BASE], 1))
    temps[0, :] = 0.0
    sm = H.StateMatrix.create(N, K, np.log(PP), False)
    st = np.asarray(sm.states)
    res = {"what": "correlograms", "options": OPTS, "reps": a.reps}

    # ---- shape 1: the plan form ----
    dy = torch.empty((nC, T), dtype=torch.float64, device="cuda")
    for c in range(nC):
        dy[c] = torch.from_numpy(H.create_signal(T, 0.3, PP, temps, seed=1234 + c)).cuda()
    dx = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
    dll = torch.zeros(nC, dtype=torch.float64, device="cuda")
    H.set_option("engine", H.ENGINE_WAVE)
    plan = H.Plan.batched(T, [sm] * nC, [temps] * nC, [0.3] * nC)
    try:
        plan.viterbi(dy, dx, dll)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        ms = []
        for rep in range(2 + a.reps):          # two warm-up calls
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cg = plan.correlograms(dx, stream=stream, **OPTS)
            e1.record()
            e1.synchronize()
            if rep >= 2:
                ms.append(e0.elapsed_time(e1))
    finally:
        plan.close()
        H.set_option("engine", H.ENGINE_AUTO)
    # the same events on the host: trough states of each template along the decoded paths
    qv = temps.argmin(axis=0) + 1
    lists = []
    for c in range(nC):
        x = dx[c].cpu().numpy().astype(np.int64)
        lists += [np.flatnonzero(st[i, x - 1] == qv[i]).astype(np.int64) + 1 for i in range(N)]
    del dy
    assert cg.n.tolist() == [len(t) for t in lists]
    inc = increments(lists, Hb * b)
    assert int(cg.counts.sum()) == inc, (int(cg.counts.sum()), inc)
    med = statistics.median(ms)
    res["plan"] = {"channels": nC, "samples": T, "units": nC * N, "spikes": int(cg.n.sum()), "increments": inc,
                   "ms_call": round(med, 3), "min_max": [round(min(ms), 3), round(max(ms), 3)],
                   "increments_per_s": round(inc / (med * 1e-3), 0),
                   "isi_violations": int(cg.isi_violations.sum()), "coincident": int(cg.coincidence.sum())}
    if not a.no_numpy:
        U = nC * N
        model, secs = numpy_model(lists, [(u, v) for u in range(U) for v in range(U)], b, Hb)
        assert all(np.array_equal(cg.counts[u, v], h) for (u, v), h in model.items()), "device != numpy model"
        res["plan"]["ms_numpy_model"] = round(secs * 1e3, 1)
        res["plan"]["device_not_slower_than_numpy"] = bool(med <= secs * 1e3)

    # ---- shape 2: the host form on synthetic units at the same density ----
    U = a.units
    if U > 0:
        rng = np.random.default_rng(5)
        per_unit = max(1, int(cg.n.sum()) // (nC * N))
        lists = []
        for u in range(U):                     # distinct samples with a gap of at least K between neighbours
            g = np.sort(rng.choice(T - per_unit * K, per_unit, replace=False)).astype(np.int64)
            lists.append(g + np.arange(per_unit, dtype=np.int64) * K + 1)
        hs = []
        for rep in range(1 + max(3, a.reps // 2)):
            t0 = time.perf_counter()
            hg = H.correlograms(lists, **OPTS)
            if rep >= 1:
                hs.append((time.perf_counter() - t0) * 1e3)
        inc = increments(lists, Hb * b)
        assert int(hg.counts.sum()) == inc, (int(hg.counts.sum()), inc)
        med = statistics.median(hs)
        res["host"] = {"units": U, "spikes": int(hg.n.sum()), "increments": inc, "ms_call": round(med, 3),
                       "min_max": [round(min(hs), 3), round(max(hs), 3)],
                       "increments_per_s": round(inc / (med * 1e-3), 0)}
        if not a.no_numpy:
            pairs = [(int(u), int(v)) for u, v in rng.integers(0, U, (64, 2))] + [(0, 0)]
            model, secs = numpy_model(lists, pairs, b, Hb)
            assert all(np.array_equal(hg.counts[u, v], h) for (u, v), h in model.items()), "device != numpy model"
            res["host"]["ms_numpy_model_scaled_from_%d_pairs" % len(pairs)] = round(secs * 1e3 * U * U / len(pairs), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
