"""Footprints on the resident paths of a plan (hmmsort_plan_footprints) at the correlogram benchmark's size.

BASELINE config 4's one-GPU share: a batched wave plan of 8 channels x 10 M samples with the headline 4 x 60 ring model,
decoded once; then Plan.footprints(d_x, d_y) -- every unit on all 8 channels of the resident block, pre 20, W 60 -- is
timed with device events around the call (it synchronises its stream; the events cover the compaction, the two kernels
and the copies of the sums), median of the timed calls after two warm-up calls.  Reported beside it:
  * the gather's byte count, sum over units of nused * M * W * 8, and its time at the copy rate measured here in the
    same session the way scripts/bw_probe.py measures it (400 MB device copy, read + write bytes over time): the floor;
  * the device form on the same lists (no compaction), for the split between compaction and gather;
  * the host numpy model (a fancy-indexed gather and a sum per unit and channel; no tile order) on the same input, and
    the check that both agree to 1e-9 of the largest sum -- the bit-for-bit check is the test suite's.
The time of the gather kernel alone comes from a run of its own: this script under `rocprofv3 --kernel-trace --stats`
with --reps 3 --no-numpy (k_fp_gather, k_fp_fold and the compaction kernels are listed by name).

    python scripts/bench_footprints.py [--channels 8] [--samples 10000000] [--reps 10] [--no-numpy]
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
PRE, W = 20, 60


def copy_rate():
    """GB/s of a 400 MB device copy, read + write bytes counted (scripts/bw_probe.py's "copy" line)"""
    n = 400_000_000 // 8
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    y.copy_(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        y.copy_(x)
    torch.cuda.synchronize()
    return 2 * n * 8 / ((time.perf_counter() - t0) / 20) / 1e9


def numpy_model(block, lists):
    """sum and sumsq by a fancy-indexed gather per unit and channel (float64; the order of the adds is numpy's)"""
    nC, T = block.shape
    t0 = time.perf_counter()
    s, q = np.zeros((len(lists), nC, W)), np.zeros((len(lists), nC, W))
    nused = np.zeros(len(lists), dtype=np.int64)
    k = np.arange(W)
    for u, t in enumerate(lists):
        a = t - 1 - PRE
        a = a[(a >= 0) & (a + W <= T)]
        nused[u] = len(a)
        idx = a[:, None] + k[None, :]
        for c in range(nC):
            sn = block[c][idx]
            s[u, c], q[u, c] = sn.sum(axis=0), (sn * sn).sum(axis=0)
    return s, q, nused, time.perf_counter() - t0


def timed(call, reps):
    ms, out = [], None
    for rep in range(2 + reps):                # two warm-up calls
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        e1.synchronize()
        if rep >= 2:
            ms.append(e0.elapsed_time(e1))
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--states", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_footprints.py needs a GPU"
    nC, T, K, N = a.channels, a.samples, a.states, 4
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p) for p in BASE], 1))
    temps[0, :] = 0.0
    sm = H.StateMatrix.create(N, K, np.log(PP), False)
    st = np.asarray(sm.states)
    res = {"what": "footprints", "pre": PRE, "W": W, "reps": a.reps}
    rate = copy_rate()
    res["copy_GBps"] = round(rate, 0)

    dy = torch.empty((nC, T), dtype=torch.float64, device="cuda")
    for c in range(nC):
        dy[c] = torch.from_numpy(H.create_signal(T, 0.3, PP, temps, seed=1234 + c)).cuda()
    dx = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
    dll = torch.zeros(nC, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    H.set_option("engine", H.ENGINE_WAVE)
    plan = H.Plan.batched(T, [sm] * nC, [temps] * nC, [0.3] * nC)
    try:
        plan.viterbi(dy, dx, dll)
        torch.cuda.synchronize()
        fp, ms = timed(lambda: plan.footprints(dx, dy, pre=PRE, W=W, stream=stream), a.reps)
    finally:
        plan.close()
        H.set_option("engine", H.ENGINE_AUTO)
    # the same events on the host: trough states of each template along the decoded paths
    qv = temps.argmin(axis=0) + 1
    lists = []
    for c in range(nC):
        x = dx[c].cpu().numpy().astype(np.int64)
        lists += [np.flatnonzero(st[i, x - 1] == qv[i]).astype(np.int64) + 1 for i in range(N)]
    assert fp.n.tolist() == [len(t) for t in lists]
    offs = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    d_t = torch.from_numpy(np.concatenate(lists)).cuda()
    fd, msd = timed(lambda: H.device.footprints(dy, d_t, offs, pre=PRE, W=W, stream=stream), a.reps)
    assert fd.sum.tobytes() == fp.sum.tobytes() and fd.sumsq.tobytes() == fp.sumsq.tobytes()
    med, medd = statistics.median(ms), statistics.median(msd)
    nbytes = int(fp.n_used.sum()) * nC * W * 8
    floor_ms = nbytes / (rate * 1e9) * 1e3
    res["plan"] = {"channels": nC, "samples": T, "units": nC * N, "spikes": int(fp.n.sum()),
                   "used": int(fp.n_used.sum()), "gather_bytes": nbytes, "ms_floor_at_copy_rate": round(floor_ms, 3),
                   "ms_call": round(med, 3), "min_max": [round(min(ms), 3), round(max(ms), 3)],
                   "call_over_floor": round(med / floor_ms, 2),
                   "ms_device_form": round(medd, 3), "device_form_min_max": [round(min(msd), 3), round(max(msd), 3)],
                   "device_form_over_floor": round(medd / floor_ms, 2)}
    if not a.no_numpy:
        block = dy.cpu().numpy()
        s, q, nused, secs = numpy_model(block, lists)
        assert np.array_equal(nused, fp.n_used)
        assert np.abs(s - fp.sum).max() <= 1e-9 * np.abs(s).max() and np.abs(q - fp.sumsq).max() <= 1e-9 * q.max()
        res["plan"]["ms_numpy_model"] = round(secs * 1e3, 1)
        res["plan"]["device_not_slower_than_numpy"] = bool(med <= secs * 1e3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
