"""Per-spike fit on a resident recording (hmmsort_plan_spike_fit): the 10 M-sample, 4 x 60 ring recording of bench.py,
decoded once; then the fit of the resident signal and path is timed with cap = 0 (counts and summary only) and with
full per-spike arrays, and beside it, in the same run, hmmsort_plan_extract_spiketimes on the same path -- the
existing call the fit contains (its two compaction passes are the fit's first step).  Every call synchronises its
stream, so a host clock around it times all of it, copies to the host included; median of the timed calls after
warm-up, the three kinds of call alternating.

    python scripts/bench_spike_fit.py [--samples 10000000] [--reps 12]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hmmsort_amd as H  # noqa: E402
from hmmsort_amd import _lib  # noqa: E402

BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
PP = [0.003, 0.001, 0.002, 0.0015]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--states", type=int, default=60)
    ap.add_argument("--reps", type=int, default=12)
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_spike_fit.py needs a GPU"
    T, K, N = a.samples, a.states, 4
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p) for p in BASE], 1))
    temps[0, :] = 0.0
    y = H.create_signal(T, 0.3, PP, temps, seed=1234)
    sm = H.StateMatrix.create(N, K, np.log(PP), False)
    dy = torch.from_numpy(y).cuda()
    dx = torch.zeros(T, dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    plan = H.Plan(T, sm, temps, 0.3)
    L = _lib.lib()
    try:
        plan.viterbi(dy, dx, dll)
        torch.cuda.synchronize()
        counts = np.zeros(N, dtype=np.int64)
        _lib.check(L.hmmsort_plan_extract_spiketimes(plan._h, dx.data_ptr(), None, 0, _lib.ptr(counts), None))
        cap = int(counts.max())
        times = np.zeros((N, cap), dtype=np.int64)
        arr = [np.zeros((N, cap), dtype=dt) for dt in (np.int64, np.float64, np.float64, np.float64, np.int32)]
        cnt2, summ = np.zeros(N, dtype=np.int64), np.zeros((N, 8 + 3 * (K - 1)))
        full = _lib.SpikeFitOut(*[q.ctypes.data for q in arr], cap, cnt2.ctypes.data, summ.ctypes.data)
        brief = _lib.SpikeFitOut(None, None, None, None, None, 0, cnt2.ctypes.data, summ.ctypes.data)

        calls = {
            "extract": lambda: L.hmmsort_plan_extract_spiketimes(plan._h, dx.data_ptr(), _lib.ptr(times), cap,
                                                                 _lib.ptr(counts), None),
            "fit_cap0": lambda: L.hmmsort_plan_spike_fit(plan._h, dy.data_ptr(), dx.data_ptr(), 0, None, None,
                                                         C.byref(brief), None),
            "fit_full": lambda: L.hmmsort_plan_spike_fit(plan._h, dy.data_ptr(), dx.data_ptr(), 0, None, None,
                                                         C.byref(full), None),
        }
        ms = {k: [] for k in calls}
        for rep in range(2 + a.reps):          # two warm-up rounds
            for k, fn in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _lib.check(fn())
                if rep >= 2:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(cnt2, counts) and np.array_equal(arr[0], times)
        med = {k: statistics.median(v) for k, v in ms.items()}
        uq = [H.quality_from_summary(summ[i], K, 0.3) for i in range(N)]
        print(json.dumps({
            "what": "plan_spike_fit", "samples": T, "K": K, "N": N, "events": counts.tolist(), "reps": a.reps,
            "ms_extract": round(med["extract"], 3), "ms_fit_cap0": round(med["fit_cap0"], 3),
            "ms_fit_full": round(med["fit_full"], 3),
            "min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            "fit_cap0_over_extract": round(med["fit_cap0"] / med["extract"], 2),
            "fit_full_over_extract": round(med["fit_full"] / med["extract"], 2),
            "mean_amp": [round(q.mean_amp, 4) for q in uq], "chi2": [round(q.chi2, 4) for q in uq],
            "sd_amp_over_expected": [round(q.sd_amp / q.sd_expected, 3) for q in uq]}))
    finally:
        plan.close()


if __name__ == "__main__":
    main()
