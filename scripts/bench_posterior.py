#!/usr/bin/env python3
"""Posterior calls at the headline shape (4 templates x 60 states, 10 M samples, signal resident in HBM):
time of plan.posteriors, + posterior_decode, + spike_confidence, next to plan.estep on the same plan, with
device events around `--steps` calls after `--warmup` calls, and the per-kernel times of plan.profile() with
their design bytes over the 8 TB/s HBM peak.  Prints one JSON line.

  python scripts/bench_posterior.py --steps 20 --warmup 5
  PYTHONPATH=/path/to/an/older/checkout HMMSORT_GSUM_SEPARATE=1 python scripts/bench_posterior.py --estep-only

The second form is the yardstick: a posterior call runs the unfused backward sweep and no statistics kernels,
so it should cost what an older build's E-step with stand-alone statistics costs minus its kw_gsum time."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)      # behind PYTHONPATH: an older checkout's package can be timed with --estep-only
HBM_PEAK_GBS = 8000.0


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def design_bytes(kernel, N, T):
    """HBM bytes per launch by design (per sample: doubles read + written)"""
    per = {"kw_post_marginals": (N + 1) * 8 + (2 * N + 1) * 8, # rho + gamma(silent) in, onset + occ + silent out
           "kw_post_decode": (N + 1) * 8 + 2,                  # rho + gamma(silent) in, int16 state out
           "kw_bwd_post": (2 * N + 5) * 8 + (N + 1) * 8,       # y, y, W2, fref, la0, R, fv in; rho + gamma(silent) out
           "kw_fwd": (N + 1) * 8 + (N + 2) * 8}                # y, R in; la0, fref, fv out
    return per[kernel] * T if kernel in per else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=10_000_000)
    ap.add_argument("--N", type=int, default=4)
    ap.add_argument("--K", type=int, default=60)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--estep-only", action="store_true", help="time plan.estep only (works with older builds)")
    a = ap.parse_args()
    import torch
    import hmmsort_amd as H
    assert H.device_count() >= 1, "bench_posterior.py needs a GPU"
    N, K, T = a.N, a.K, a.T
    p4 = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p4[i % 4]) for i in range(N)], 1))
    pp = ([0.003, 0.001, 0.002, 0.0015] * 4)[:N]
    y = H.create_signal(T, 0.3, pp, temps, seed=1234)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    plan = H.Plan(T, sm, temps, 0.3)
    st = torch.cuda.current_stream().cuda_stream
    dy = torch.from_numpy(y).cuda()
    stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
    res = {"shape": "%dx%d" % (N, K), "T": T, "steps": a.steps, "warmup": a.warmup, "lib": H._lib.LIB_PATH,
           "gsum_separate": bool(os.environ.get("HMMSORT_GSUM_SEPARATE"))}

    def profile(fn):
        plan.profile(True)
        for _ in range(a.steps):
            fn()
        out = {k: round(ms / n, 5) for k, (ms, n) in plan.profile_read(st).items()}
        plan.profile(False)
        return out
    res["estep_ms"] = round(timed(lambda: plan.estep(dy, stats, st), a.steps, a.warmup), 5)
    res["estep_kernels_ms"] = profile(lambda: plan.estep(dy, stats, st))
    if not a.estep_only:
        on = torch.zeros((N, T), dtype=torch.float64, device="cuda")
        oc, si = torch.zeros_like(on), torch.zeros(T, dtype=torch.float64, device="cuda")
        lz = torch.zeros(1, dtype=torch.float64, device="cuda")
        xm = torch.zeros(T, dtype=torch.int16, device="cuda")
        dx, dll = torch.zeros(T, dtype=torch.int16, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(dy, dx, dll, st)

        def post():
            plan.posteriors(dy, on, oc, si, lz, st)

        def post_decode():
            post()
            plan.posterior_decode(xm, st)
        res["posteriors_ms"] = round(timed(post, a.steps, a.warmup), 5)
        res["posteriors_onset_only_ms"] = round(timed(lambda: plan.posteriors(dy, on, None, None, None, st),
                                                      a.steps, a.warmup), 5)
        res["posteriors_decode_ms"] = round(timed(post_decode, a.steps, a.warmup), 5)
        post()
        import time
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            conf = plan.spike_confidence(dx, 2, st)      # host outputs: wall clock around a synchronising call
        res["spike_confidence_ms"] = round((time.perf_counter() - t0) / 3 * 1e3, 3)
        res["events"] = int(sum(len(t) for t, _ in conf))
        res["posterior_kernels_ms"] = profile(post_decode)
        res["roofline"] = {}
        for k, ms in res["posterior_kernels_ms"].items():
            b = design_bytes(k, N, T)
            if b and ms > 0:
                res["roofline"][k] = {"design_bytes": b, "GBs": round(b / ms / 1e6, 1),
                                      "frac_hbm_peak": round(b / ms / 1e6 / HBM_PEAK_GBS, 3)}
        d = plan.diagnostics(st)
        res["certificates_failed"] = int(d[3] + d[5])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
