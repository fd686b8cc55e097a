"""Posterior calls of the blocked engine on an overlap model, device-resident (plan API), next to the E-step of the
same build: python scripts/bench_overlap_posterior.py [N K T]      (shapes and timing as bench_overlap_estep.py)"""
import sys, time
sys.path.insert(0, ".")
import numpy as np, torch
import hmmsort_amd as H
N, K, T = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (2, 60, 1_000_000)
base = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25)]
temps = np.asfortranarray(np.stack([H.create_spike_template(K, *base[i]) for i in range(N)], 1))
pp = [0.012, 0.008, 0.006][:N]
y = H.create_signal(T, 0.3, pp, temps, seed=3)
sm = H.StateMatrix.create(N, K, np.log(pp), True)
H.set_option("engine", H.ENGINE_BLOCKED)
plan = H.Plan(T, sm, temps, 0.3)
dy = torch.from_numpy(y).cuda()
stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
on = torch.zeros((N, T), dtype=torch.float64, device="cuda")
oc, si = torch.zeros_like(on), torch.zeros(T, dtype=torch.float64, device="cuda")
lz = torch.zeros(1, dtype=torch.float64, device="cuda")
xm = torch.zeros(T, dtype=torch.int16, device="cuda")
dx = torch.zeros(T, dtype=torch.int16, device="cuda")
dll = torch.zeros(1, dtype=torch.float64, device="cuda")
plan.viterbi(dy, dx, dll)


def timed(fn, n=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def estep():
    plan.estep(dy, stats); plan.mstep(stats, out)


def post():
    plan.posteriors(dy, on, oc, si, lz)


def post_decode():
    plan.posteriors(dy, on, oc, si, lz); plan.posterior_decode(xm)


t_e = timed(estep)
d_e = plan.diagnostics()[3:7]
t_p = timed(post)
d_p = plan.diagnostics()[3:7]
t_pd = timed(post_decode)
t_c = timed(lambda: plan.spike_confidence(dx, 2))
nsp = sum(len(t) for t, _ in plan.spike_confidence(dx, 2))
print("blocked N=%d K=%d S=%d T=%d block %d halo %d" % (N, K, sm.nstates, T, plan.info()["block"], plan.info()["halo"]))
print("  estep + mstep        %9.2f ms  diag %s" % (t_e * 1e3, d_e))
print("  posteriors           %9.2f ms  diag %s  = %.2f x the E-step, %.1f Msamples/s" % (t_p * 1e3, d_p, t_p / t_e, T / t_p / 1e6))
print("  posteriors + decode  %9.2f ms" % (t_pd * 1e3))
print("  spike_confidence     %9.2f ms  (%d spikes, jitter 2)" % (t_c * 1e3, nsp))
print("  logz %.6f  workspace %.2f GB" % (float(lz.cpu()[0]), plan.info()["workspace_bytes"] / 1e9))
