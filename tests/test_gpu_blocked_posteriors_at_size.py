"""Posteriors of the blocked engine at 10^6 samples against the extended-precision reference (oracle/hp_estep.c
through oracle/hp.py), on windows that hold block boundaries of the plan.

Reference values come from tests/golden/blocked_post_at_size/<case>.npz (tests/golden/make_blocked_post_at_size.py;
about half a minute of CPU for 400 states, several minutes for 3 600, with 8 threads).  The inputs are regenerated
from the seed and hashed: on a mismatch the reference is recomputed live, and the test says so; it never compares
against a stale fixture.

Bars (the project's own, none derived from what the device produced):
  marginals (onset, occ, trough, silent)   1e-8 absolute on every window sample
  log-likelihood                           1e-10 relative
  sum_t of the marginals                   1e-8 relative against the reference's sum_t gamma_t(j) over the same states
  decode                                   equal to the reference's arg max wherever the reference's top-two gap
                                           exceeds 1e-6; the share of closer samples is capped at 1e-3 (asserted by
                                           the generator on the reference alone, stored, and asserted again here)
Largest errors measured on the MI355X: DESIGN.md section 3.5.
"""
import functools
import os
import sys

import numpy as np
import pytest

import posterior_model as PM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_options(H):
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)
    yield
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)


@functools.lru_cache(maxsize=None)
def case(name):
    import make_blocked_post_at_size as G
    import make_estep_at_size as G0
    y, osm, mu, sigma, pp, win = G.inputs(name)
    h = G0.hashes(y, osm, mu, sigma)
    path = os.path.join(G.OUT, name + ".npz")
    assert os.path.exists(path), "fixture %s is missing" % path
    ref = G.load(name)
    if str(ref["sha_y"]) != h["sha_y"] or str(ref["sha_model"]) != h["sha_model"] or \
            not np.array_equal(ref["windows"], win):
        print("case %s: the regenerated inputs do not hash to the fixture's (another random stream?): "
              "recomputing the reference live" % name)
        ref = G.reference(y, osm, mu, sigma, win, threads=16)
    N, K = G.CASES[name][:2]
    return dict(name=name, y=y, osm=osm, mu=mu, sigma=sigma, pp=pp, win=win, ref=ref, N=N, K=K)


@pytest.mark.parametrize("name", ["P20a", "P20b", "P60"])
def test_blocked_posteriors_on_windows_against_reference(H, name):
    import torch
    c = case(name)
    r, N, T = c["ref"], c["N"], len(c["y"])
    sm = H.StateMatrix.create(N, c["K"], np.log(c["pp"]), True)
    tr = sm.transitions
    assert np.array_equal(tr["src"], c["osm"].src) and np.array_equal(tr["dst"], c["osm"].dst)
    assert np.array_equal(tr["lp"], c["osm"].val) and np.array_equal(sm.states, c["osm"].states)
    H.set_option("engine", H.ENGINE_BLOCKED)
    dy = torch.from_numpy(c["y"]).cuda()
    on = torch.full((N, T), np.nan, dtype=torch.float64, device="cuda")
    oc = torch.full_like(on, np.nan)
    si = torch.full((T,), np.nan, dtype=torch.float64, device="cuda")
    lz = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
    xm = torch.zeros(T, dtype=torch.int16, device="cuda")
    # a plan-API caller reads the certificates and widens the warm-up when one fails, as hmmsort_posteriors does by
    # itself (the default 256 samples leave 1.8e-9 against the certificate's 1e-9 at one boundary of P60)
    plan, first_diag = None, None
    for halo in (0, 512, 1024):
        H.set_option("halo", halo)
        plan = H.Plan(T, sm, c["mu"], c["sigma"])
        plan.posteriors(dy, on, oc, si, lz)
        plan.posterior_decode(xm)
        torch.cuda.synchronize()
        diag = plan.diagnostics()
        first_diag = first_diag or diag
        if diag[3] == 0 and diag[5] == 0:
            break
        print("%s: warm-up %d: certificates %s, widening" % (name, plan.info()["halo"], diag[3:7]), flush=True)
        plan.close()
        plan = None
    assert plan is not None, ("certificates still fail at a warm-up of 1 024 samples", first_diag, diag)
    try:
        info = plan.info()
        assert info["engine"] == H.ENGINE_BLOCKED
        counts = plan.expected_counts()
        # trough mass has no output of its own: spike_confidence at jitter 0 returns it at the events of a path, so
        # hand it a path that sits in template a's trough state (every other template silent) across the window
        q = PM.trough_values(c["mu"])
        tsum = [oc[a].sum().item() for a in range(N)]
        ssum = si.sum().item()
        osum = [on[a].sum().item() for a in range(N)]
        won = [on[:, lo:hi].cpu().numpy() for lo, hi in c["win"]]
        woc = [oc[:, lo:hi].cpu().numpy() for lo, hi in c["win"]]
        wsi = [si[lo:hi].cpu().numpy() for lo, hi in c["win"]]
        wxm = [xm[lo:hi].cpu().numpy() for lo, hi in c["win"]]
        st = c["osm"].states
        wtr = []
        for lo, hi in c["win"]:
            rows = []
            for a in range(N):
                others = np.ones(st.shape[1], bool)
                for b in range(N):
                    if b != a:
                        others &= st[b] == 1
                s_a = int(np.nonzero((st[a] == q[a]) & others)[0][0]) + 1
                x = np.ones(T, np.int16)
                x[lo:hi] = s_a
                got = plan.spike_confidence(torch.from_numpy(x).cuda(), 0)[a]
                assert np.array_equal(got[0], np.arange(lo + 1, hi + 1))
                rows.append(got[1])
            wtr.append(np.stack(rows))
    finally:
        plan.close()
    blk = info["block"]
    straddle = [(hi - 1) // blk > lo // blk for lo, hi in c["win"]]
    assert any(straddle[2:]), ("no interior window holds a block boundary", blk, c["win"])
    worst = dict(onset=0.0, occ=0.0, trough=0.0, silent=0.0)
    differ = close = total = 0
    for i in range(len(c["win"])):
        worst["onset"] = max(worst["onset"], float(np.abs(won[i] - r["w%d_onset" % i]).max()))
        worst["occ"] = max(worst["occ"], float(np.abs(woc[i] - r["w%d_occ" % i]).max()))
        worst["silent"] = max(worst["silent"], float(np.abs(wsi[i] - r["w%d_silent" % i]).max()))
        worst["trough"] = max(worst["trough"], float(np.abs(wtr[i] - np.minimum(r["w%d_trough" % i], 1.0)).max()))
        clear = r["w%d_gap" % i] > 1e-6
        differ += int((wxm[i][clear] != r["w%d_xm" % i][clear]).sum())
        close += int((~clear).sum())
        total += clear.size
    sg = r["sg"]
    sums = dict(silent=abs(ssum - sg[0]) / sg[0])
    for a in range(N):
        sums["occ%d" % a] = abs(tsum[a] - sg[st[a] > 1].sum()) / sg[st[a] > 1].sum()
        sums["onset%d" % a] = abs(osum[a] - sg[st[a] == 2].sum()) / sg[st[a] == 2].sum()
        sums["counts%d" % a] = abs(counts[a] - sg[st[a] == 2].sum()) / sg[st[a] == 2].sum()
    ez = abs(float(lz.cpu()[0]) - r["loglik"]) / abs(r["loglik"])
    print("%s blocked posteriors (S %d, block %d, halo %d, %d blocks; %d of %d windows hold a boundary): " % (
        name, sm.nstates, blk, info["halo"], info["nchains"], sum(straddle), len(straddle))
        + "  ".join("%s %.3g" % kv for kv in worst.items()) + "  logz rel %.3g  sums rel %.3g" % (ez, max(sums.values()))
        + "  decode differs at %d of %d clear samples (%d within 1e-6, share %.3g)" % (
            differ, total - close, close, close / total) + "  certificates %s" % (diag[3:7],), flush=True)
    assert max(worst.values()) <= 1e-8, worst
    assert ez <= 1e-10
    assert max(sums.values()) <= 1e-8, sums
    assert close / total <= 1e-3 and float(r["close_share"]) <= 1e-3
    assert differ == 0
