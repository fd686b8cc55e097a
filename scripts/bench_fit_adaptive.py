"""Cost of drift tracking: hmmsort_fit_adaptive against hmmsort_fit_chunked, host array in, host array out, 4 M samples
in chunks of 100 000, median of 5 after one warm-up; and the per-chunk split of what the adaptive loop adds, timed on
the plan API with the same calls the loop makes (statistics + blend + finish on the device, copy-back of mu', sigma',
lp', the host rebuild of the list, set_model on a chunk plan).
    python scripts/bench_fit_adaptive.py [ring4|ov2|ov4 ...] [T=4000000]"""
import sys, time
sys.path.insert(0, ".")
import numpy as np
import hmmsort_amd as H
from hmmsort_amd.api import _fit_adaptive_call

K, CHUNK = 60, 100_000
MODELS = {"ring4": (4, False), "ov2": (2, True), "ov4": (4, True)}
names = [a for a in sys.argv[1:] if a in MODELS] or list(MODELS)
T = next((int(a[2:]) for a in sys.argv[1:] if a.startswith("T=")), 4_000_000)
shapes = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]


def median_of_5(f):
    f()
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), min(ts), max(ts), out


def split(sm, temps, y, ml):
    """per-chunk milliseconds of the added work, median of 20, on a plan of chunk length"""
    import torch
    from hmmsort_amd.device import Plan, stats_blend
    plan = Plan(CHUNK, sm, temps, 0.3)
    dy, dx = torch.from_numpy(y[:2 * CHUNK]).cuda(), torch.from_numpy(ml[:2 * CHUNK]).cuda()
    n, m = plan.path_stats_len(), plan.mstep_len()
    new, acc = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
    out = torch.zeros(m, dtype=torch.float64, device="cuda")
    nlp = m - sm.K * sm.N - 1 - sm.nstates
    keep = sm.K * sm.N + 1 + nlp
    host = torch.zeros(keep, dtype=torch.float64).pin_memory()
    dev, back, rebuild, setm = [], [], [], []
    for _ in range(21):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plan.path_stats(dy, dx, 2 * CHUNK, 100, CHUNK - 50, True, new)
        stats_blend(acc, 0.9, new, n, 3)
        plan.path_finish(acc, out)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host.copy_(out[:keep])
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        lp = host[sm.K * sm.N + 1:].numpy().copy()
        H.StateMatrix.from_states(sm.states, sm.pi, sm.K, lp, sm.resolve_overlaps)
        t3 = time.perf_counter()
        plan.set_model(sm, temps, 0.3)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        dev.append(t1 - t0), back.append(t2 - t1), rebuild.append(t3 - t2), setm.append(t4 - t3)
    engine = plan.info()["engine"]
    plan.close()
    med = lambda v: 1e3 * float(np.median(v[1:]))  # noqa: E731
    return engine, med(dev), med(back), med(rebuild), med(setm)


for name in names:
    N, ov = MODELS[name]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *shapes[i]) for i in range(N)], 1))
    pp = [0.003, 0.001, 0.002, 0.0015][:N]
    sm = H.StateMatrix.create(N, K, np.log(pp), ov)
    y = H.create_signal(T, 0.3, pp, temps, seed=3)
    tm = H.HMMSpikeTemplateModel(sm, temps, 0.3)
    d0, lo0, hi0, m0 = median_of_5(lambda: H.fit_channels(tm, [y], CHUNK)[0])
    d1, lo1, hi1, r = median_of_5(lambda: _fit_adaptive_call(tm, y, CHUNK, 1e6, 0, True, False))
    rc, ml, ll, tk, _ = r
    assert rc == 0
    nchunks = tk.n
    print("%s: N=%d K=60 %s (%d states), %d samples in %d chunks" % (name, N, "overlaps" if ov else "ring", sm.nstates, T, nchunks))
    print("  hmmsort_fit_chunked  %.1f ms (%.1f-%.1f) = %.1f Msamples/s" % (1e3 * d0, 1e3 * lo0, 1e3 * hi0, T / d0 / 1e6))
    print("  hmmsort_fit_adaptive %.1f ms (%.1f-%.1f) = %.1f Msamples/s: +%.2f ms per chunk; %d samples decoded "
          "differently on this stationary signal" % (1e3 * d1, 1e3 * lo1, 1e3 * hi1, T / d1 / 1e6,
                                                     1e3 * (d1 - d0) / nchunks, int(np.sum(ml != m0.ml_seq))))
    engine, dev, back, rebuild, setm = split(sm, temps, y, ml)
    print("  per chunk on a plan of engine %d: statistics + blend + finish %.3f ms, copy-back %.3f ms, list rebuild "
          "(update_lp only) %.3f ms, set_model %.3f ms" % (engine, dev, back, rebuild, setm))
    H.shutdown()
