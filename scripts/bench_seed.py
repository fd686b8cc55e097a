"""Template seed on a resident signal (hmmsort_seed_templates_device): the 10 M-sample, 4 x 60 headline recording of
bench.py, seeded with N clusters.  The call synchronises its stream, so HIP events around it time all of it; median of
the timed calls after warm-up.  The stages are separate launches inside one C call, so they are separated by
difference: `detect` is the call with sigma given and a threshold nothing reaches (detection pass, scan, one read
back), `median` = full call - call with sigma given, `cluster` = call with sigma given - detect.

Two yardsticks measured in the same run: the time the passes over the signal need at the copy rate (six select passes
and one detection pass, 8 bytes per sample each; the rate is that of a 400 MB device copy, as scripts/bw_probe.py
takes it, read + write bytes), and one hard step (decode + path update) of the generating model at the same size.

    python scripts/bench_seed.py [--samples 10000000] [--clusters 7] [--reps 5]
"""
import argparse
import json
import statistics
import sys

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hmmsort_amd as H  # noqa: E402

BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
PP = [0.003, 0.001, 0.002, 0.0015]
SELECT_PASSES, DETECT_PASSES = 6, 1


def timed(fn, reps, warm=2):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--clusters", type=int, default=7)
    ap.add_argument("--states", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_seed.py needs a GPU"
    T, K, N = a.samples, a.states, a.clusters
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p) for p in BASE], 1))
    y = H.create_signal(T, 0.3, PP, temps, seed=1234)
    dy = torch.from_numpy(y).cuda()

    sm, mu, sigma, info = H.device.seed_templates(dy, N, K)
    full = timed(lambda: H.device.seed_templates(dy, N, K), a.reps)
    given = timed(lambda: H.device.seed_templates(dy, N, K, sigma=sigma), a.reps)
    detect = timed(lambda: H.device.seed_templates(dy, N, K, sigma=sigma, threshold=1e30), a.reps)

    n = 400_000_000 // 8
    src, dst = torch.empty(n, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    src.fill_(1.0)
    copy_ms = timed(lambda: dst.copy_(src), 20)[0]
    copy_rate = 2 * n * 8 / (copy_ms * 1e-3)
    del src, dst
    floor_ms = (SELECT_PASSES + DETECT_PASSES) * T * 8 / copy_rate * 1e3

    smg = H.StateMatrix.create(4, K, np.log(PP), False)
    tg = temps.copy(order="F")
    tg[0, :] = 0.0
    plan = H.Plan(T, smg, tg, 0.3)
    try:
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")

        def hard():
            plan.viterbi(dy, dx, dll)
            plan.path_update(dy, dx, out)
        hard_ms = timed(hard, a.reps)[0]
    finally:
        plan.close()

    print(json.dumps({
        "what": "seed_templates_device", "samples": T, "K": K, "clusters": N, "kept": int(sm.N),
        "events": info["n_events"], "iters": info["iters"], "counts": info["counts"].tolist(), "sigma": sigma,
        "ms_full": round(full[0], 3), "ms_full_min_max": [round(full[1], 3), round(full[2], 3)],
        "ms_sigma_given": round(given[0], 3), "ms_detect_only": round(detect[0], 3),
        "ms_median_by_difference": round(full[0] - given[0], 3),
        "ms_cluster_by_difference": round(given[0] - detect[0], 3),
        "gsamples_per_s": round(T / full[0] / 1e6, 3),
        "copy_rate_GBps": round(copy_rate / 1e9, 1), "passes": SELECT_PASSES + DETECT_PASSES,
        "ms_passes_at_copy_rate": round(floor_ms, 3), "times_the_pass_floor": round(full[0] / floor_ms, 2),
        "ms_hard_step_4x60": round(hard_ms, 3), "hard_step_gsamples_per_s": round(T / hard_ms / 1e6, 3),
        "seed_over_hard_step": round(full[0] / hard_ms, 3), "reps": a.reps}))


if __name__ == "__main__":
    main()
