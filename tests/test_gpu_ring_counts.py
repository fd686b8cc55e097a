"""Every ring count on the frozen second implementation (ring_*.hip, ENGINE_RING), which instantiates its kernels
through the same dispatch_N as the wave engine: the cases of ring_cases.py with 16 <= L <= 304 (what the engine takes),
decode against the fp64 oracle's path and ll, E-step + M-step against the long-double reference under the bars of
test_gpu_estep_at_size.check_mstep, as test_ring_engine_against_reference does at size.  A refusal must name its
reason and fails the test."""
import numpy as np
import pytest

import ring_cases as RC
from test_gpu_estep_at_size import check_mstep

pytestmark = pytest.mark.gpu

CASES = [c for c in RC.CASES if 16 <= c[1] - 1 <= 304]


@pytest.fixture(autouse=True)
def _engine(H):
    for k in ("block", "halo"):
        H.set_option(k, 0)
    H.set_option("engine", H.ENGINE_RING)
    try:
        yield
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
        for k in ("block", "halo"):
            H.set_option(k, 0)


def test_every_ring_count_has_a_case():
    assert {c[0] for c in CASES} == set(range(1, 17))
    assert {c[0] for c in CASES if c[2]} == set(range(2, 9))


@pytest.mark.parametrize("N,K,per_source", CASES, ids=[RC.case_id(c) for c in CASES])
def test_ring_engine_every_ring_count(H, N, K, per_source):
    import torch
    c = RC.case(N, K, per_source)
    name, T = RC.case_id((N, K, per_source)), c["T"]
    # The plan API flags a warm-up certificate it cannot pass and leaves the remedy, a longer warm-up, to its caller
    # (the host ladder).  So does this test, like test_gpu_wave_dispatch.py: the E-step runs at the first of the default
    # warm-up, 2 x and 4 x it that leaves no flag, and every bar below holds there (9x65: 2 x).
    halo0 = None
    for widen in (1, 2, 4):
        if widen > 1:
            H.set_option("halo", widen * halo0)
        try:
            plan = H.Plan(T, c["sm"], c["mu"], c["sigma"])
        except H.HmmsortError as e:
            assert "ring engine unavailable" in str(e), str(e)       # a refusal names its reason (ring_supported)
            pytest.fail("ring engine refused case %s: %s" % (name, e))
        try:
            info = plan.info()
            assert info["engine"] == H.ENGINE_RING
            halo0 = halo0 or info["halo"]
            dy = torch.from_numpy(np.array(c["y"])).cuda()
            dx = torch.zeros(T, dtype=torch.int16, device="cuda")
            dll = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
            plan.viterbi(dy, dx, dll)
            dv = plan.diagnostics()
            stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
            out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
            plan.estep(dy, stats)
            plan.mstep(stats, out)
            de = plan.diagnostics()
            torch.cuda.synchronize()
            x, ll, o = dx.cpu().numpy(), float(dll.cpu()[0]), out.cpu().numpy()
        finally:
            plan.close()
        if de[3] == 0 and de[5] == 0:
            break
        print("%s ring: warm-up %d leaves E-step flags %s, widening" % (name, info["halo"], de[3:7]), flush=True)
    nbad = int(np.count_nonzero(x != c["x"]))
    ell = abs(ll - c["ll"]) / abs(c["ll"])
    print("%s ring: S=%d T=%d  %d chains of %d, warm-up %d (default %d)  differing samples %d  ll rel err %.3g  "
          "diag %s / %s" % (name, c["osm"].nstates, T, info["nchains"], info["block"], info["halo"], halo0, nbad, ell,
                            list(dv), list(de)), flush=True)
    assert nbad == 0, "%s: path differs at %d samples, first at %d (diag %s)" % (name, nbad, int(np.argmax(x != c["x"])), dv)
    assert ell <= 1e-9
    check_mstep("%s ring (%d chains)" % (name, info["nchains"]), o, c, N)
    assert de[3] == 0 and de[5] == 0, de
