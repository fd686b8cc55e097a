"""Front end on a resident raw block (hmmsort_preprocess_device): C channels x T int16 samples, sample-major, through
the zero-phase FIR filter and the common reference.  The call synchronises its stream, so HIP events around it time all
of it: the kernels plus what every call pays for its own small buffers (two allocations, two blocking copies of a few
kilobytes, the final synchronisation).  That fixed part is measured on a block of one sample and reported, and taken
off in the `kernel_ms` figures.  Median of --reps calls after --warm warm-up calls.

Floors, neither taken from this code:
  bytes  2 C T read + 8 C T written for the filter, 16 C T for the in-place reference, at the rate of a 400 MB device
         copy measured in the same run (as scripts/bw_probe.py takes it, read + write bytes);
  issue  3 fp64 vector instructions per tap pair and output (add, multiply, add: the contract forbids the fused form,
         which would need 2) at the fp64 rate scripts/micro/fma_probe.hip sustains, --fp64-rate lane-operations per
         second (default: DESIGN section 8's calibration, 33e12).
For comparison the numpy model of tests/preprocess_model.py on the host, on --model-samples per channel, scaled to T.

    python scripts/bench_preprocess.py [--samples 10000000] [--channels 8] [--reps 20] [--warm 3]
"""
import argparse
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hmmsort_amd as H  # noqa: E402

LAYOUT_SAMPLE_MAJOR = H._lib.LAYOUT_SAMPLE_MAJOR


def timed(fn, reps, warm):
    """median, min, max milliseconds of fn() by HIP events"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def raw_block(T, C, seed=1):
    """(T, C) int16 on the device: noise, a common 50 Hz term and a ramp, in ADC counts"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.arange(T, device="cuda", dtype=torch.float32)
    common = 300.0 * torch.sin(2 * np.pi * 50.0 * t / 30000.0) + 200.0 * t / T
    x = 100.0 * torch.randn((T, C), generator=g, device="cuda") + common[:, None]
    return x.round().to(torch.int16).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--fp64-rate", type=float, default=33e12)
    ap.add_argument("--model-samples", type=int, default=500_000)
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_preprocess.py needs a GPU"
    T, nC = a.samples, a.channels

    n = 400_000_000 // 8
    src, dst = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    src.fill_(1.0)
    copy_ms = timed(lambda: dst.copy_(src), 20, 2)[0]
    copy_rate = 2 * n * 8 / (copy_ms * 1e-3)
    del src, dst

    tiny = torch.zeros((1, 1), dtype=torch.int16, device="cuda")
    fixed_ms = timed(lambda: H.device.preprocess(tiny, LAYOUT_SAMPLE_MAJOR), a.reps, a.warm)[0]

    taps = {nt: H.design_fir(30000.0, low=300.0, high=6000.0, ntaps=nt) for nt in (257, 513)}
    d8 = raw_block(T, nC)
    T64 = max(1, T * nC // 64)
    configs = [
        ("fir257+median", d8, taps[257], "median"), ("fir513+median", d8, taps[513], "median"),
        ("fir257", d8, taps[257], None), ("fir513", d8, taps[513], None),
        ("widen", d8, None, None), ("widen+median", d8, None, "median"), ("widen+mean", d8, None, "mean"),
    ]
    rows = []

    def measure(name, d, tp, ref):
        Tn, Cn = (int(v) for v in d.shape)
        med, lo, hi = timed(lambda: H.device.preprocess(d, LAYOUT_SAMPLE_MAJOR, tp, ref), a.reps, a.warm)
        P = 0 if tp is None else len(tp) // 2
        fir_bytes, ref_bytes = 10.0 * Cn * Tn, (16.0 * Cn * Tn if ref else 0.0)
        rows.append({"config": name, "channels": Cn, "samples": Tn, "taps": 2 * P + 1 if tp is not None else 0,
                     "reference": ref, "call_ms": round(med, 3), "call_ms_min_max": [round(lo, 3), round(hi, 3)],
                     "kernel_ms": round(med - fixed_ms, 3),
                     "fir_bytes_floor_ms": round(fir_bytes / copy_rate * 1e3, 3),
                     "ref_bytes_floor_ms": round(ref_bytes / copy_rate * 1e3, 3),
                     "fir_issue_floor_ms": round(3.0 * P * Cn * Tn / a.fp64_rate * 1e3, 3)})

    for cfg in configs:
        measure(*cfg)
    del d8
    d64 = raw_block(T64, 64, seed=2)
    measure("64ch fir257+median", d64, taps[257], "median")
    measure("64ch widen+median", d64, None, "median")
    measure("64ch widen", d64, None, None)
    del d64

    # by difference: the reference pass alone, the filter's arithmetic alone
    by = {r["config"]: r for r in rows}
    for r in rows:
        base = "64ch widen" if r["channels"] == 64 else "widen"
        r["minus_widen_ms"] = round(r["call_ms"] - by[base]["call_ms"], 3)

    import preprocess_model as PM
    Tm = min(a.model_samples, T)
    xm = (100.0 * np.random.default_rng(1).standard_normal((nC, Tm))).round().astype(np.int16)
    t0 = time.perf_counter()
    PM.preprocess(xm, taps[257][128:], "median")
    model_s = time.perf_counter() - t0

    print(json.dumps({"what": "preprocess_device", "layout": "sample-major int16", "reps": a.reps, "warm": a.warm,
                      "copy_rate_GBps": round(copy_rate / 1e9, 1), "fp64_rate_lane_ops_per_s": a.fp64_rate,
                      "fixed_call_ms": round(fixed_ms, 3), "rows": rows,
                      "numpy_model_fir257_median_s": round(model_s, 3), "numpy_model_samples": Tm,
                      "numpy_model_scaled_to_T_s": round(model_s * T / Tm, 2)}))


if __name__ == "__main__":
    main()
