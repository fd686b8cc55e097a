"""The choice of test_gpu_fused_tail.py's certificate case with a warm-up that is too short, checked on the CPU with
tests/wave_model.py: the forward half of kw_fb_check's certificate at one boundary between chains of 320 samples
whose warm-up is 119 samples (what the engine makes of the options block = 128, halo = 64 for rings of 59 states).
Chain c's warm-up state (la0 at tc - 1, the onset masses of the last L samples) against chain c - 1's own, up to the
frame constant of the entry with the largest posterior weight; the error is the posterior-weighted relative
mismatch, the tolerance 1e-9."""
import numpy as np

import wave_model as M
from test_gpu_fused_tail import CERT_CASES, busy_signal

B, HW, BOUNDARY, TOL = 320, 119, 3, 1e-9


def forward_certificate(y, m, c):
    T, N, L = len(y), m.N, m.L
    Rf, V = M.ring_scores(y, m)
    tc = c * B
    la_c, fv_c, fr_c = M.fwd_chain(y, Rf, V, m, T, B, HW, c)
    la_p, fv_p, fr_p = M.fwd_chain(y, Rf, V, m, T, B, HW, c - 1)
    rho = M.bwd_chain(y, Rf, m, T, B, HW, c - 1, la_p, fv_p, fr_p, la_p.get((c - 1) * B - 1, 0.0))[1]
    ringmass = sum(rho[tc - 1 - k].sum() for k in range(L) if tc - 1 - k in rho)
    ws, ds = [max(1.0 - ringmass, 0.0)], [la_c[tc - 1] - la_p[tc - 1]]
    for e in range(L):
        t = tc - 1 - e
        if t not in rho:
            continue
        for a in range(N):
            hv, mv = fv_c[t][a], fv_p[t][a]
            if (hv == mv and fr_c[t] == fr_p[t]) or (not hv > 0 and not mv > 0):
                d = 0.0
            else:
                with np.errstate(divide="ignore"):
                    d = (fr_c[t] - fr_p[t]) + (np.log(hv) - np.log(mv))
            ws.append(rho[t][a])
            ds.append(d)
    ws, ds = np.array(ws), np.array(ds)
    D = ds[np.argmax(ws)]
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.nansum(np.where(ws > 0, ws * np.abs(np.exp(np.minimum(ds - D, 700.0)) - 1.0), 0.0)))


def test_the_short_warmup_fails_on_the_noisy_signal_and_not_on_the_quiet_one(H):
    errs = {}
    for name in ("short_halo", "clean"):      # the clean case's signal and model, under the SHORT warm-up
        _, _, noise, sigma = CERT_CASES[name]
        y, sm, mu, sigma = busy_signal(H, noise, sigma, T=(BOUNDARY + 1) * B + HW)
        errs[name] = forward_certificate(y, M.Ring(sm, mu, sigma), BOUNDARY)
    print(errs)
    assert errs["short_halo"] > TOL, errs       # 8.2e-9
    assert errs["clean"] < 1e-3 * TOL, errs     # the busy signal at noise 0.3 would not have failed
