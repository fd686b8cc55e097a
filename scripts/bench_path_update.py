"""Viterbi training, device-resident (plan API): per model the decode (hmmsort_plan_viterbi), the path update
(hmmsort_plan_path_update), the same update from additive statistics (hmmsort_plan_path_stats +
hmmsort_plan_path_finish: one pass over the signal) and, for comparison, the soft step of the same plan
(hmmsort_plan_estep + hmmsort_plan_mstep).  HIP events on the current stream, median of the timed calls after warm-up; one JSON line per
model.  The update's byte floor is two passes over 10 bytes per sample (8 of y, 2 of x).

    python scripts/bench_path_update.py [--samples 10000000] [--reps 11] [--soft-samples-big 200000] [--models ring4,ov2,ov4]
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
PP = [0.004, 0.003, 0.002, 0.002]
HBM_PEAK = 6.29e12     # bytes/s, measured copy rate of the MI355X


def timed(fn, reps, warm=2):
    """median milliseconds of fn() by HIP events"""
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


def model(name, K=60):
    N, overlaps = {"ring4": (4, False), "ov2": (2, True), "ov4": (4, True)}[name]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *BASE[i]) for i in range(N)], 1))
    temps[0, :] = 0.0
    return N, overlaps, temps, PP[:N]


def run(name, T, reps, soft_T):
    N, overlaps, temps, pp = model(name)
    sm = H.StateMatrix.create(N, 60, np.log(pp), overlaps)
    y = H.create_signal(T, 0.3, pp, temps, seed=3)
    H.set_option("engine", H.ENGINE_BLOCKED if overlaps else H.ENGINE_WAVE)
    H.set_option("blocked_hbm_columns", 1 if name == "ov4" else 0)
    res = dict(model=name, N=N, K=60, S=sm.nstates, T=T)
    plan = H.Plan(T, sm, temps, 0.3)
    try:
        dy = torch.from_numpy(y).cuda()
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
        cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
        res["viterbi_ms"] = timed(lambda: plan.viterbi(dy, dx, dll), reps)
        res["diag"] = plan.diagnostics()[:2] + plan.diagnostics()[7:]
        res["path_update_ms"] = timed(lambda: plan.path_update(dy, dx, out, cnt), reps)
        res["counts"] = cnt.cpu().numpy().tolist()
        med = res["path_update_ms"][0] * 1e-3
        res["update_bytes_floor"] = 2 * 10 * T
        res["update_fraction_of_floor"] = (2 * 10 * T / HBM_PEAK) / med
        res["update_over_decode"] = res["path_update_ms"][0] / res["viterbi_ms"][0]
        res["hard_step_Msamples_s"] = T / ((res["viterbi_ms"][0] + res["path_update_ms"][0]) * 1e-3) / 1e6
        # the statistics form: one pass over (y, x), then a finish that does not touch the signal
        stats = torch.zeros(plan.path_stats_len(), dtype=torch.float64, device="cuda")
        out2 = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")

        def stats_finish():
            plan.path_stats(dy, dx, T, 0, T, True, stats)
            plan.path_finish(stats, out2, cnt)
        res["path_stats_ms"] = timed(lambda: plan.path_stats(dy, dx, T, 0, T, True, stats), reps)
        res["path_finish_ms"] = timed(lambda: plan.path_finish(stats, out2, cnt), reps)
        res["stats_finish_ms"] = timed(stats_finish, reps)
        res["stats_finish_over_update"] = res["stats_finish_ms"][0] / res["path_update_ms"][0]
        K, nn = sm.K, sm.N
        res["same_mu_lp_pp"] = bool(torch.equal(out[:K * nn], out2[:K * nn]) and torch.equal(out[K * nn + 1:], out2[K * nn + 1:]))
        res["sigma_update_stats"] = [float(out[K * nn]), float(out2[K * nn])]
    finally:
        plan.close()
    # the soft step of the same plan; the 21 123-state model at a length that finishes
    Ts = soft_T if name == "ov4" else T
    plan = H.Plan(Ts, sm, temps, 0.3)
    try:
        dy = torch.from_numpy(y[:Ts].copy()).cuda()
        stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
        out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")

        def soft():
            plan.estep(dy, stats)
            plan.mstep(stats, out)
        soft_reps = reps if name == "ring4" else 3
        res["soft_T"] = Ts
        res["soft_step_ms"] = timed(soft, soft_reps, warm=1)
        res["soft_step_Msamples_s"] = Ts / (res["soft_step_ms"][0] * 1e-3) / 1e6
        res["hard_over_soft_rate"] = res["hard_step_Msamples_s"] / res["soft_step_Msamples_s"]
    finally:
        plan.close()
        H.set_option("engine", H.ENGINE_AUTO)
        H.set_option("blocked_hbm_columns", 0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--soft-samples-big", type=int, default=200_000)
    ap.add_argument("--models", default="ring4,ov2,ov4")
    a = ap.parse_args()
    assert H.device_count() >= 1, "needs a GPU: a timing taken anywhere else says nothing"
    for name in a.models.split(","):
        print(json.dumps(run(name, a.samples, max(a.reps, 10), a.soft_samples_big)), flush=True)


if __name__ == "__main__":
    main()
