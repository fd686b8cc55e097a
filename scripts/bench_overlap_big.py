"""Blocked E-step and posteriors with the state columns in device memory (option "blocked_hbm_columns",
csrc/generic_estep_big.hip), device-resident through the plan API, timed with HIP events after warm-up, median of
the repeats with their spread:

  python scripts/bench_overlap_big.py [--samples T] [--repeats R] [--skip-strict]

  1  E-step + M-step and posteriors of 3 x 60 (10 621 states) and 4 x 60 (21 123) at T samples, default geometry,
     with the grid the library's rule gives and the plan's workspace;
  2  2 x 60 (3 600 states) at T samples forced onto the same kernels (option 2) against the LDS kernels (option 0):
     the ratio is the price of the device-memory columns; ps per state-sample for all three models;
  3  the strict hmmsort_em_step (materialised alpha / beta, 8.5 GB) on 3 x 60 at 50 000 samples against the new path
     on the same signal, both through the host entry, wall clock;
  4  --grid-scan: one round of blocks with 49, 98, 196 and 256 workgroups resident (signals of 49 ... 256 default
     blocks of 512 samples): the time of a sweep against the number of workgroups says whether fewer workgroups
     per XCD would run faster (time per step growing faster than the workgroups) or not."""
import argparse
import statistics
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402
import hmmsort_amd as H  # noqa: E402

KEY = "blocked_hbm_columns"
BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
RATES = [0.012, 0.008, 0.006, 0.005]


def model(N, K, T, seed):
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *BASE[i]) for i in range(N)], 1))
    pp = RATES[:N]
    y = H.create_signal(T, 1.0, pp, temps, seed=seed)
    sm = H.StateMatrix.create(N, K, np.log(pp), True)
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    return y, sm, mu, 1.15


def events(fn, repeats, warm=2):
    """median and (min, max) of `repeats` timings of fn in ms, HIP events on the current stream"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def grid_of(plan, before, sm):
    """resident workgroups the library chose, from what the plan's first E-step added to workspace_bytes:
    grid x (window B x S + two columns) + boundary records, block statistics, weights, packed state records"""
    S, B, nb = sm.nstates, before["block"], before["nchains"]
    R, nsrc1 = len(sm.transitions), int((sm.transitions["src"] == 1).sum())
    fixed = (nb * 8 * S + nb * (nsrc1 + 2) + 2 * R + 4 + 2 * S + sm.K * sm.N) * 8 + S * 56
    grid, rest = divmod(plan.info()["workspace_bytes"] - before["workspace_bytes"] - fixed, (B * S + 2 * S) * 8)
    if rest:
        print("  (workspace leaves %d bytes unexplained: grid is rounded down)" % rest)
    return grid


def plan_times(N, K, T, mode, repeats, seed=3):
    y, sm, mu, sigma = model(N, K, T, seed)
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option(KEY, mode)
    plan = H.Plan(T, sm, mu, sigma)
    try:
        info = plan.info()
        S = sm.nstates
        dy = torch.from_numpy(y).cuda()
        stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
        out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
        on = torch.zeros((N, T), dtype=torch.float64, device="cuda")
        oc, si = torch.zeros_like(on), torch.zeros(T, dtype=torch.float64, device="cuda")
        lz = torch.zeros(1, dtype=torch.float64, device="cuda")

        def estep():
            plan.estep(dy, stats)
            plan.mstep(stats, out)

        def post():
            plan.posteriors(dy, on, oc, si, lz)
        estep()
        torch.cuda.synchronize()
        grid = grid_of(plan, info, sm) if mode else None     # before the posterior sweep adds its own buffers
        te = events(estep, repeats)
        de = plan.diagnostics()[3:7]
        tp = events(post, repeats)
        dp = plan.diagnostics()[3:7]
        ws = plan.info()["workspace_bytes"]
        ncu = torch.cuda.get_device_properties(0).multi_processor_count
        print("%d x %d  S=%d  T=%d  block %d  halo %d  blocks %d  option %d%s  workspace %.2f GB" % (
            N, K, S, T, info["block"], info["halo"], info["nchains"], mode,
            "  grid %d of %d CUs" % (grid, ncu) if grid else "", ws / 1e9))
        for name, (med, lo, hi), d in (("estep + mstep", te, de), ("posteriors", tp, dp)):
            print("  %-14s %9.2f ms  (min %.2f, max %.2f of %d)  %.3f Msamples/s  %.2f ps per state-sample  certificates %s" % (
                name, med, lo, hi, repeats, T / med / 1e3, med * 1e9 / (S * T), d))
        return te, tp, grid
    finally:
        plan.close()
        H.set_option(KEY, 0)
        H.set_option("engine", H.ENGINE_AUTO)


def host_em_step(T, repeats):
    y, sm, mu, sigma = model(3, 60, T, 5)
    res = {}
    for name, engine, mode in (("strict", H.ENGINE_STRICT, 0), ("device-memory columns", H.ENGINE_AUTO, 1)):
        H.set_option("engine", engine)
        H.set_option(KEY, mode)
        try:
            H.train_step(y, sm, mu.copy(order="F"), sigma)            # warm-up: plan and buffers
            ts = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                out = H.train_step(y, sm, mu.copy(order="F"), sigma)
                ts.append(time.perf_counter() - t0)
            res[name] = (statistics.median(ts), min(ts), max(ts), out, H.get_option("last_escalations"))
        finally:
            H.set_option(KEY, 0)
            H.set_option("engine", H.ENGINE_AUTO)
            H.shutdown()
    print("hmmsort_em_step, 3 x 60 (10 621 states), T=%d, host entry, wall clock:" % T)
    for name, (med, lo, hi, _, esc) in res.items():
        print("  %-22s %9.1f ms  (min %.1f, max %.1f of %d)  %.4f Msamples/s  escalations %d" % (
            name, med * 1e3, lo * 1e3, hi * 1e3, repeats, T / med / 1e6, esc))
    s, b = res["strict"], res["device-memory columns"]
    print("  ratio strict / new %.1f (slowest new against fastest strict: %.1f)  max |d mu| %.3g  rel d sigma %.3g" % (
        s[0] / b[0], s[1] / b[2], np.abs(s[3][1] - b[3][1]).max(), abs(s[3][2] - b[3][2]) / s[3][2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-strict", action="store_true")
    ap.add_argument("--grid-scan", action="store_true")
    a = ap.parse_args()
    if a.grid_scan:
        for N in (3, 4):
            for nblk in (49, 98, 196, 256):
                te, tp, grid = plan_times(N, 60, 512 * nblk, 1, a.repeats)
                steps = 2 * (512 + 256)
                print("  -> %d workgroups, one round of %d steps: %.2f us per step (E-step), %.2f (posteriors); "
                      "%.3f / %.3f workgroup-steps per us" % (grid, steps, te[0] * 1e3 / steps, tp[0] * 1e3 / steps,
                                                              grid * steps / te[0] / 1e3, grid * steps / tp[0] / 1e3))
        return
    for N in (3, 4):
        plan_times(N, 60, a.samples, 1, a.repeats)
    forced = plan_times(2, 60, a.samples, 2, a.repeats)
    lds = plan_times(2, 60, a.samples, 0, a.repeats)
    print("2 x 60: device-memory columns / LDS columns = %.2f (E-step), %.2f (posteriors)" % (
        forced[0][0] / lds[0][0], forced[1][0] / lds[1][0]))
    if not a.skip_strict:
        host_em_step(50_000, 3)


if __name__ == "__main__":
    main()
