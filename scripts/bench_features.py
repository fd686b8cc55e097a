"""Waveform features and cluster isolation on the resident paths of a plan at the footprint benchmark's
size: a batched wave plan of 8 channels x 10 M samples with the headline 4 x 60 ring model, decoded once (about 416 k
spikes in 32 units).  Timed with device events around the library calls (each synchronises its stream), median of the
timed calls after two warm-up calls:
  (a) pass 1   hmmsort_plan_snippet_features, no basis, no rows, moments = 1 on all 8 channels, W = 60;
  (b) pass 2   the same call with the PCA basis of (a) (P = 3, F = 24), rows and moments = 2;
  (c) export   no basis, rows only (F = 480: the snippets themselves);
  (d) the isolation of the 32 units on the rows of (b) (hmmsort_cluster_isolation_device, F = 24);
  (e) the isolation of one channel's 4 units at F = 12 (4 channels x 3 components).
There is no earlier implementation to compare with, so each time is reported as a multiple of a floor the script
computes from the shapes:
  * bytes: the gathered samples (used rows x M x W x 8), plus the rows written where rows are written, at the copy rate
    measured in the same run the way scripts/bw_probe.py measures it; for (d) and (e) six passes of the select over U n
    keys of 8 bytes;
  * fp64: three instructions per (row, m, p, k) of a projection, two per (row, a, b >= a) of the moments, two per
    (u, row, a, b) of the distances, at the rate scripts/micro/fma_probe (built from fma_probe.hip) prints for 16
    chains, when that program is there (else --fp64-gops, else the fp64 floor is left out).
The larger of the two is the floor that binds.  Beside them: the host numpy model of (b) and (d) on the same input
(gather, matrix product, einsum; numpy's order of adds) and the check that both agree to 1e-9 -- the bit-for-bit check
is the test suite's.  Kernel times come from a run of its own: this script under `rocprofv3 --kernel-trace --stats`
with --reps 3 --no-numpy.

    python scripts/bench_features.py [--channels 8] [--samples 10000000] [--reps 10] [--no-numpy] [--fp64-gops G]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, ".")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import hmmsort_amd as H  # noqa: E402

BASE = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
PP = [0.003, 0.001, 0.002, 0.0015]
PRE, W, P = 20, 60, 3
L = H._lib


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


def fp64_rate(given):
    """G instruction-lanes per second of independent fp64 chains: scripts/micro/fma_probe's "fma 16 chains" line"""
    if given:
        return float(given)
    exe = os.path.join("scripts", "micro", "fma_probe")
    if not os.path.exists(exe):
        return None
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    m = re.search(r"fma 16 chains\s+[\d.]+ ms\s+([\d.]+) Gop/s", out)
    return float(m.group(1)) if m else None


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


def plan_call(plan, dx, dy, U, M, basis, centre, moments, d_feat, d_used, stream):
    """hmmsort_plan_snippet_features into preallocated rows -> (n, nused, m1, m2)"""
    Pc = W if basis is None else basis.shape[1]
    F = M * Pc
    n, nused = np.zeros(U, dtype=np.int64), np.zeros(U, dtype=np.int64)
    G, groups = (Pc, M) if moments == 1 else (F, 1)
    m1 = np.zeros((U, groups, G)) if moments else None
    m2 = np.zeros((U, groups, G, G)) if moments else None
    opt = L.FeatOpt(PRE, W, 0, None, Pc if basis is not None else 1, L.ptr(basis), L.ptr(centre), moments)
    mp = [L.ptr(m1), L.ptr(m2)]
    out = L.FeatOut(None if d_feat is None else d_feat.data_ptr(), None if d_used is None else d_used.data_ptr(),
                    0 if d_feat is None else d_feat.shape[0], L.ptr(n), L.ptr(nused),
                    *(mp if moments == 1 else [None, None]), *(mp if moments == 2 else [None, None]))
    L.check(L.lib().hmmsort_plan_snippet_features(plan._h, C.c_void_p(dx.data_ptr()), C.c_void_p(dy.data_ptr()),
                                                  dy.shape[0], C.byref(opt), C.byref(out), C.c_void_p(stream)))
    return n, nused, m1, m2


def entry(ms, floors):
    """a time against its floors (ms): which binds, and the multiple"""
    med = statistics.median(ms)
    known = {k: v for k, v in floors.items() if v is not None}
    bind = max(known, key=known.get)
    return {"ms": round(med, 3), "min_max": [round(min(ms), 3), round(max(ms), 3)],
            "floors_ms": {k: round(v, 4) for k, v in known.items()}, "binding_floor": bind,
            "over_floor": round(med / known[bind], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--samples", type=int, default=10_000_000)
    ap.add_argument("--states", type=int, default=60)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--fp64-gops", type=float, default=None)
    a = ap.parse_args()
    assert H.device_count() >= 1, "bench_features.py needs a GPU"
    nC, T, K, N = a.channels, a.samples, a.states, 4
    U, M = nC * N, nC
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p) for p in BASE], 1))
    temps[0, :] = 0.0
    sm = H.StateMatrix.create(N, K, np.log(PP), False)
    rate, gops = copy_rate(), fp64_rate(a.fp64_gops)
    res = {"what": "features", "pre": PRE, "W": W, "P": P, "reps": a.reps, "copy_GBps": round(rate, 0),
           "fp64_Gops": gops}
    byte_ms = lambda nbytes: nbytes / (rate * 1e9) * 1e3
    flop_ms = lambda instr: None if gops is None else instr / (gops * 1e9) * 1e3

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
        (n, nused, b1, b2), ms_a = timed(lambda: plan_call(plan, dx, dy, U, M, None, None, 1, None, None, stream),
                                         a.reps)
        basis, centre = H.pca_basis(b1, b2, nused, P)
        rows, used_rows, F = int(n.sum()), int(nused.sum()), M * P
        d_feat = torch.zeros((rows, F), dtype=torch.float64, device="cuda")
        d_used = torch.zeros(rows, dtype=torch.uint8, device="cuda")
        (_, _, g1, g2), ms_b = timed(lambda: plan_call(plan, dx, dy, U, M, basis, centre, 2, d_feat, d_used, stream),
                                     a.reps)
        d_exp = torch.zeros((rows, M * W), dtype=torch.float64, device="cuda")
        _, ms_c = timed(lambda: plan_call(plan, dx, dy, U, M, None, None, 0, d_exp, None, stream), a.reps)
        del d_exp
    finally:
        plan.close()
        H.set_option("engine", H.ENGINE_AUTO)
    gather = used_rows * M * W * 8
    res["spikes"], res["used"], res["units"] = rows, used_rows, U
    res["a_pass1_moments"] = entry(ms_a, {"bytes": byte_ms(gather), "fp64": flop_ms(used_rows * M * W * (W + 1))})
    res["b_pass2_rows_and_moments"] = entry(ms_b, {"bytes": byte_ms(gather + rows * F * 8),
                                                  "fp64": flop_ms(used_rows * (3 * M * P * W + F * (F + 1)))})
    res["c_export"] = entry(ms_c, {"bytes": byte_ms(gather + rows * M * W * 8)})

    offs = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    mu, vinv = H.unit_gaussians(g1[:, 0], g2[:, 0], nused)
    iso, ms_d = timed(lambda: H.device.isolation_scores(d_feat, offs, mu, vinv, d_used=d_used, stream=stream), a.reps)
    res["d_isolation_32_units"] = entry(ms_d, {"bytes": byte_ms(6 * U * rows * 8),
                                               "fp64": flop_ms(2 * U * rows * F * F)})
    res["d_isolation_32_units"]["scored"] = int(np.count_nonzero(~np.isnan(vinv[:, 0, 0])))

    # one channel's four units on four channels
    lists = plan_lists(dx, sm, temps, 1)
    o4 = np.concatenate([[0], np.cumsum([len(t) for t in lists])]).astype(np.int64)
    d_t = torch.from_numpy(np.concatenate(lists)).cuda()
    p1 = H.device.snippet_features(dy, d_t, o4, pre=PRE, W=W, channels=[0, 1, 2, 3], moments=1, features=False)
    b4, c4 = H.pca_basis(p1.b1, p1.b2, p1.n_used, P)
    p2 = H.device.snippet_features(dy, d_t, o4, pre=PRE, W=W, channels=[0, 1, 2, 3], basis=b4, centre=c4, moments=2)
    mu4, vinv4 = H.unit_gaussians(p2.g1, p2.g2, p2.n_used)
    _, ms_e = timed(lambda: H.device.isolation_scores(p2.features, o4, mu4, vinv4, d_used=p2.used, stream=stream),
                    a.reps)
    r4 = int(o4[-1])
    res["e_isolation_4_units"] = entry(ms_e, {"bytes": byte_ms(6 * N * r4 * 8), "fp64": flop_ms(2 * N * r4 * 144)})

    if not a.no_numpy:
        block = dy.cpu().numpy()
        all_lists = plan_lists(dx, sm, temps, nC)
        t = np.concatenate(all_lists)
        t0 = time.perf_counter()
        start = t - 1 - PRE
        ok = (start >= 0) & (start + W <= T)
        idx = np.where(ok, start, 0)[:, None] + np.arange(W)[None, :]
        f = np.concatenate([(block[m][idx] - centre[m]) @ basis[m].T for m in range(M)], axis=1)
        f[~ok] = 0.0
        secs_b = time.perf_counter() - t0
        got = d_feat.cpu().numpy()
        assert np.abs(f - got).max() <= 1e-9 * np.abs(f).max()
        t0 = time.perf_counter()
        d2 = np.stack([np.einsum("ra,ab,rb->r", got - mu[u], vinv[u], got - mu[u]) for u in range(U)])
        secs_d = time.perf_counter() - t0
        unit = np.repeat(np.arange(U), n)
        want = np.array([np.sort(d2[u][(unit != u) & ok])[nused[u] - 1] if 0 < nused[u] <= (ok & (unit != u)).sum()
                         else np.nan for u in range(U)])
        both = ~np.isnan(want)
        assert np.array_equal(np.isnan(iso[0]), np.isnan(want))
        assert np.allclose(iso[0][both], want[both], rtol=1e-9)
        res["b_pass2_rows_and_moments"]["ms_numpy_rows_only"] = round(secs_b * 1e3, 1)
        res["d_isolation_32_units"]["ms_numpy_distances_only"] = round(secs_d * 1e3, 1)
    print(json.dumps(res))


def plan_lists(dx, sm, temps, channels):
    """the events of the first `channels` channels on the host: trough states of each template along the decoded paths"""
    st = np.asarray(sm.states)
    qv = temps.argmin(axis=0) + 1
    lists = []
    for c in range(channels):
        x = dx[c].cpu().numpy().astype(np.int64)
        lists += [np.flatnonzero(st[i, x - 1] == qv[i]).astype(np.int64) + 1 for i in range(temps.shape[1])]
    return lists


if __name__ == "__main__":
    main()
