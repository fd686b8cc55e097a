"""Spatial whitening on a resident fp64 block [C][T] (hmmsort_noise_scale_device, hmmsort_noise_cov_device,
hmmsort_channel_mix_device), stage by stage.  Every call synchronises its stream, so HIP events around it time all of
it: the kernels plus what the call pays for its own small buffers, copies and the final synchronisation.  That fixed
part is measured on a block of one sample and reported, and taken off in the `kernel_ms` figures.  Median of --reps
calls after --warm warm-up calls.

Floors, neither taken from this code:
  bytes  8 C T read for the mask and the sums together, 16 C T for the mix (read + write), 8 C T for the noise scale, at
         the rate of a 400 MB device copy measured in the same run (as scripts/bw_probe.py takes it, read + write bytes);
  issue  2 fp64 lane-operations (multiply, add: the contract forbids the fused form) per entry and quiet sample for the
         sums, C (C + 1) / 2 entries, and 2 per term for the mix, at the fp64 rate scripts/micro/fma_probe.hip sustains,
         --fp64-rate lane-operations per second (default: DESIGN section 8's calibration, 33e12).
Each stage is reported as a multiple of whichever floor binds.  For comparison the numpy model of tests/whiten_model.py
on the host, on --model-samples per channel, scaled to T.

    python scripts/bench_whiten.py [--samples 10000000] [--reps 20] [--warm 3]
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


def block(C, T, seed):
    """[C][T] float64 on the device: unit noise, a noise source shared by all channels, and sparse large events"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    y = torch.randn((C, T), generator=g, device="cuda", dtype=torch.float64)
    y += 2.0 * torch.randn((1, T), generator=g, device="cuda", dtype=torch.float64)
    spikes = torch.rand((1, T), generator=g, device="cuda") < 0.002
    y[0] += 40.0 * spikes[0].to(torch.float64)
    return y.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10_000_000, help="samples per channel of the 8-channel block")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--fp64-rate", type=float, default=33e12)
    ap.add_argument("--model-samples", type=int, default=100_000)
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_whiten.py needs a GPU"
    dv = H.device

    n = 400_000_000 // 8
    src, dst = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    src.fill_(1.0)
    copy_ms = timed(lambda: dst.copy_(src), 20, 2)[0]
    copy_rate = 2 * n * 8 / (copy_ms * 1e-3)
    del src, dst

    tiny = torch.zeros((1, 1), dtype=torch.float64, device="cuda")
    one_n, one_w = np.zeros((1, 1), dtype=np.int32), np.ones((1, 1))
    fixed = {"noise_scale": timed(lambda: dv.noise_scale(tiny), a.reps, a.warm)[0],
             "mask+sums": timed(lambda: dv.noise_covariance(tiny, thr=[1.0]), a.reps, a.warm)[0],
             "mix": timed(lambda: dv.channel_mix(tiny, one_n, one_w, tiny), a.reps, a.warm)[0]}
    rows = []

    def row(stage, name, C, T, med, lo, hi, nbytes, lane_ops, extra=None):
        kernel = med - fixed[stage]
        bf, jf = nbytes / copy_rate * 1e3, lane_ops / a.fp64_rate * 1e3
        r = {"stage": name, "channels": C, "samples": T, "call_ms": round(med, 3),
             "call_ms_min_max": [round(lo, 3), round(hi, 3)], "kernel_ms": round(kernel, 3),
             "bytes_floor_ms": round(bf, 3), "issue_floor_ms": round(jf, 3),
             "binding_floor": "bytes" if bf >= jf else "issue", "times_floor": round(kernel / max(bf, jf), 2)}
        r.update(extra or {})
        rows.append(r)

    for C, T, seed in ((8, a.samples, 1), (64, max(1, a.samples * 8 // 64), 2)):
        d = block(C, T, seed)
        sigma = dv.noise_scale(d)
        thr = 4.0 * sigma
        med, lo, hi = timed(lambda: dv.noise_scale(d), a.reps, a.warm)
        row("noise_scale", "noise_scale", C, T, med, lo, hi, 8.0 * C * T, 0.0, {"passes_over_the_block": 6})
        _, _, nq, s1, s2 = dv.noise_covariance(d, thr=thr, guard=30)
        med, lo, hi = timed(lambda: dv.noise_covariance(d, thr=thr, guard=30), a.reps, a.warm)
        row("mask+sums", "mask+sums", C, T, med, lo, hi, 8.0 * C * T, 2.0 * (C * (C + 1) / 2) * nq,
            {"n_quiet": nq, "quiet_fraction": round(nq / T, 3)})
        nbr, w = H.whitening_matrix(H.noise_covariance(nq, s1, s2))
        out = torch.empty_like(d)
        med, lo, hi = timed(lambda: dv.channel_mix(d, nbr, w, out), a.reps, a.warm)
        row("mix", "mix global", C, T, med, lo, hi, 16.0 * C * T, 2.0 * C * C * T)
        del out
        if C == 64:
            nbr, w = H.whitening_matrix(H.noise_covariance(nq, s1, s2), (np.arange(64.0)[:, None], 16))
            out = torch.empty_like(d)
            med, lo, hi = timed(lambda: dv.channel_mix(d, nbr, w, out), a.reps, a.warm)
            row("mix", "mix local M=16", C, T, med, lo, hi, 16.0 * C * T, 2.0 * C * 16 * T)
            del out
        nbr, w = H.whitening_matrix(H.noise_covariance(nq, s1, s2))
        med, lo, hi = timed(lambda: dv.channel_mix(d, nbr, w, d), a.reps, a.warm)   # in place: the values run away,
        row("mix", "mix global in place", C, T, med, lo, hi, 16.0 * C * T, 2.0 * C * C * T)   # the time does not
        del d

    import whiten_model as WM
    Tm = min(a.model_samples, a.samples)
    ym = np.random.default_rng(1).standard_normal((8, Tm))
    t0 = time.perf_counter()
    _, _, _, nq, s1, s2 = WM.noise_cov(ym)
    t1 = time.perf_counter()
    WM.mix(ym, *H.whitening_matrix(H.noise_covariance(nq, s1, s2)))
    t2 = time.perf_counter()

    print(json.dumps({"what": "whiten_device", "reps": a.reps, "warm": a.warm,
                      "copy_rate_GBps": round(copy_rate / 1e9, 1), "fp64_rate_lane_ops_per_s": a.fp64_rate,
                      "fixed_call_ms": {k: round(v, 3) for k, v in fixed.items()}, "rows": rows,
                      "numpy_model_8ch_samples": Tm, "numpy_model_noise_cov_s": round(t1 - t0, 3),
                      "numpy_model_mix_s": round(t2 - t1, 3),
                      "numpy_model_scaled_to_T_s": [round((t1 - t0) * a.samples / Tm, 1),
                                                    round((t2 - t1) * a.samples / Tm, 2)]}))


if __name__ == "__main__":
    main()
