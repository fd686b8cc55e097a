"""Unit stability on the resident paths of a plan at the footprint benchmark's size: a batched wave plan of
8 channels x 10 M samples with the headline 4 x 60 ring model, decoded once (about 416 k spikes in 32 units), binned into
100 and into 10 000 time bins.  Timed with device events around the library calls (each synchronises its stream), median
of the timed calls after two warm-up calls:
  (a) plan form    hmmsort_plan_unit_stability: event compaction, the per-spike fit for the amplitudes, and the tables
                   (three quantiles, sums, a 512-bin histogram);
  (b) device form  hmmsort_unit_stability_device on the same events and amplitudes, resident: the tables alone.
There is no earlier implementation to compare with, so each time is reported as a multiple of a byte floor the script
computes from the shapes, at the copy rate measured in the same run the way scripts/bw_probe.py measures it:
  * device form: times and values read once (16 bytes per spike), keys and positions written (16), keys read by the
    select, the sums and the histogram (3 x 8), and the tables written (U B (3 x 8 + nq x 8));
  * plan form: that, plus the paths read once by the compaction (2 bytes per sample) and the fit's windows (K x 8 bytes
    per spike).
Beside them: the numpy model on the host on the same events (tests/stability_model.py's rules, without its tile loop:
a sort per segment and numpy's order of adds) and the check that counts and quantiles agree exactly -- the bit-for-bit
check of every table is the test suite's.  Kernel times come from a run of its own: this script under
`rocprofv3 --kernel-trace --stats` with --reps 3 --no-numpy.

    python scripts/bench_stability.py [--channels 8] [--samples 10000000] [--reps 10] [--no-numpy]
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
QUANTILES, HIST = (0.25, 0.5, 0.75), (512, 0.0, 4.0)


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


def entry(ms, floor_ms):
    med = statistics.median(ms)
    return {"ms": round(med, 3), "min_max": [round(min(ms), 3), round(max(ms), 3)], "byte_floor_ms": round(floor_ms, 4),
            "over_floor": round(med / floor_ms, 2)}


def host_model(times, amps, T, bin, q_num, q_den):
    """counts and quantiles per (unit, bin) with numpy on the host: bincount, and a sort per segment"""
    B = (T + bin - 1) // bin
    count = np.zeros((len(times), B), dtype=np.int64)
    quant = np.full((len(times), B, len(q_num)), np.nan)
    for u, (t, v) in enumerate(zip(times, amps)):
        b = (t - 1) // bin
        count[u] = np.bincount(b, minlength=B)
        edges = np.concatenate([[0], np.cumsum(count[u])])
        for k in np.flatnonzero(count[u]):
            seg = np.sort(v[edges[k]:edges[k + 1]])
            seg = seg[~np.isnan(seg)]
            if len(seg):
                quant[u, k] = [seg[q * (len(seg) - 1) // q_den] for q in q_num]
    return count, quant


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--states", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_stability.py needs a GPU"
    nC, T, K, N = a.channels, a.samples, a.states, 4
    U = nC * N
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p) for p in BASE], 1))
    temps[0, :] = 0.0
    sm = H.StateMatrix.create(N, K, np.log(PP), False)
    rate = copy_rate()
    res = {"what": "stability", "quantiles": len(QUANTILES), "hist_bins": HIST[0], "reps": a.reps,
           "copy_GBps": round(rate, 0)}
    byte_ms = lambda nbytes: nbytes / (rate * 1e9) * 1e3

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
        fits = plan.spike_fit(dy, dx)
        times = [f.times for ch in fits for f in ch]
        amps = [f.amp for ch in fits for f in ch]
        n = sum(len(t) for t in times)
        offs = np.concatenate([[0], np.cumsum([len(t) for t in times])]).astype(np.int64)
        d_t, d_v = torch.from_numpy(np.concatenate(times)).cuda(), torch.from_numpy(np.concatenate(amps)).cuda()
        res["spikes"], res["units"] = n, U
        q_num, q_den = H.quantile_fractions(QUANTILES)
        for nbins in (100, 10_000):
            bin = -(-T // nbins)
            B = -(-T // bin)
            tables = n * (16 + 16 + 24) + U * B * (24 + 8 * len(QUANTILES))
            got_p, ms_p = timed(lambda: plan.unit_stability(dy, dx, bin, QUANTILES, HIST, stream), a.reps)
            got_d, ms_d = timed(lambda: H.device.unit_stability(d_t, offs, d_v, T=T, bin=bin, quantiles=QUANTILES,
                                                                hist=HIST, stream=stream), a.reps)
            assert all(getattr(got_p, k).tobytes() == getattr(got_d, k).tobytes() for k in ("count", "quant", "sum"))
            r = {"bins": B, "plan_form": entry(ms_p, byte_ms(tables + nC * T * 2 + n * K * 8)),
                 "device_form": entry(ms_d, byte_ms(tables))}
            if not a.no_numpy:
                t0 = time.perf_counter()
                count, quant = host_model(times, amps, T, bin, q_num, q_den)
                r["ms_numpy_counts_and_quantiles"] = round((time.perf_counter() - t0) * 1e3, 1)
                assert np.array_equal(count, got_d.count) and np.array_equal(quant, got_d.quant, equal_nan=True)
            res["bins_%d" % nbins] = r
    finally:
        plan.close()
        H.set_option("engine", H.ENGINE_AUTO)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
