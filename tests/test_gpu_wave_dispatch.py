"""Every ring count (1..16) and every dispatch row of the wave engine (csrc/wave_common.h, wave_pick) against the
references of ring_cases.py: the path and ll of the fp64 oracle, the E-step / M-step and the posteriors of the
long-double reference (oracle/hp.py).

The row is never worked out by the library's own thresholds here: the library says which kernels a call of a plan
launches (the undeclared test aid hmmsort_selftest_wave_dispatch, read before the call), and each case asserts that
answer against the row its shape is meant to pin (ring_cases.expected_row, whose spot rows are literals in
test_ring_cases_cpu.py).  A shape that drifts to another row after a change of thresholds fails instead of silently
testing something else: move the shape, not the expectation.

Every case runs through the plan API on the wave engine (no ladder that could end elsewhere): a decode in both
backtrace forms, an E-step + M-step, the fused decode + E-step call and a posterior call.  Bars: path equal to the
oracle's at every sample, ll within 1e-9 relative, every boundary certified and no near-tie block (diag[0], diag[7]);
M-step under test_gpu_estep_at_size.check_mstep (1e-8 relative, the project's E-step bar) with diag[3] == diag[5] ==
0; fused call bit-equal to the separate calls; posterior marginals within 1e-8 absolute on the windows (both ends, 512
samples around every chain boundary of the default geometry), logz within 1e-10 relative.  The plan API only flags
what it cannot certify; the calls run at the first of the default warm-up, 2 x and 4 x it that leaves no flag, and
every bar holds there (printed per case).

Found by this file and fixed with it: logz of a posterior call 2-3 % off where a chain
boundary falls inside a certain spike (9x65, 13x65); the E-step of one ring of more than 512 states (1x514, 1x770,
1x1026: kw_gsum_mx<1, 3> and <1, 4> staged 512 of their 594 / 850 rows of y and the ring's last lags summed stale LDS,
the last phase of mu 0.392 against -0.0173 at L = 513, NaN under HMMSORT_POISON at L = 769 and 1 025).  Largest errors measured on the MI355X: DESIGN.md
section 3.10."""
import ctypes as C
import time

import numpy as np
import pytest

import ring_cases as RC
from test_gpu_estep_at_size import check_mstep

pytestmark = pytest.mark.gpu

OPTIONS = ("block", "halo", "backtrace")
POST_MAX_L = 257    # hmmsort_plan_posteriors takes rings of up to 257 states on the wave engine


@pytest.fixture(autouse=True)
def _engine(H):
    H.set_option("engine", H.ENGINE_WAVE)
    for k in OPTIONS:
        H.set_option(k, 0)
    try:
        yield
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
        for k in OPTIONS:
            H.set_option(k, 0)


def _aid(H):
    fn = H._lib.lib().hmmsort_selftest_wave_dispatch
    fn.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int64]
    fn.restype = C.c_int
    return fn


def dispatch(H, plan, call):
    """(row, [chains listed by certificate rounds 0 and 1 of the last decode] or None) as the library words them"""
    buf = C.create_string_buffer(512)
    assert _aid(H)(plan._h, call, buf, len(buf)) == 0
    row, _, listed = buf.value.decode().partition(" | listed=")
    return row, ([int(v) for v in listed.split(",")] if listed else None)


def assert_row(H, plan, c, call, **kw):
    want = RC.expected_row(c["N"], c["L"], c["per_source"], call, **kw)
    got = dispatch(H, plan, call)[0]
    assert got == want, "%s call %d: the library runs '%s', this case is meant to pin '%s': move the shape" % (
        RC.case_id((c["N"], c["K"], c["per_source"])), call, got, want)
    return got


class Run:
    """one plan of a case: the device buffers and the calls"""

    def __init__(self, H, c, y=None, sm=None):
        import torch
        self.torch, self.H, self.c = torch, H, c
        self.y = c["y"] if y is None else y
        self.T = len(self.y)
        self.plan = H.Plan(self.T, c["sm"] if sm is None else sm, c["mu"], c["sigma"])
        self.info = self.plan.info()
        self.dy = torch.from_numpy(np.array(self.y)).cuda()

    def decode(self, stats=False):
        t = self.torch
        dx = t.zeros(self.T, dtype=t.int16, device="cuda")
        dll = t.full((1,), np.nan, dtype=t.float64, device="cuda")
        ds = t.zeros(self.plan.stats_len(), dtype=t.float64, device="cuda") if stats else None
        if stats:
            self.plan.decode_estep(self.dy, dx, dll, ds)
        else:
            self.plan.viterbi(self.dy, dx, dll)
        d = self.plan.diagnostics()
        return dx.cpu().numpy(), float(dll.cpu()[0]), d, (ds.cpu().numpy() if stats else None)

    def estep(self):
        t = self.torch
        ds = t.zeros(self.plan.stats_len(), dtype=t.float64, device="cuda")
        out = t.zeros(self.plan.mstep_len(), dtype=t.float64, device="cuda")
        self.plan.estep(self.dy, ds)
        self.plan.mstep(ds, out)
        d = self.plan.diagnostics()
        return ds.cpu().numpy(), out.cpu().numpy(), d

    def posteriors(self, win):
        t, N = self.torch, self.c["N"]
        on = t.full((N, self.T), np.nan, dtype=t.float64, device="cuda")
        oc = t.full_like(on, np.nan)
        si = t.full((self.T,), np.nan, dtype=t.float64, device="cuda")
        lz = t.full((1,), np.nan, dtype=t.float64, device="cuda")
        self.plan.posteriors(self.dy, on, oc, si, lz)
        d = self.plan.diagnostics()
        w = [(on[:, lo:hi].cpu().numpy(), oc[:, lo:hi].cpu().numpy(), si[lo:hi].cpu().numpy()) for lo, hi in win]
        return w, float(lz.cpu()[0]), d

    def close(self):
        self.plan.close()


def check_decode(c, tag, x, ll, d, xo=None, llo=None):
    xo, llo = (c["x"], c["ll"]) if xo is None else (xo, llo)
    nbad = int(np.count_nonzero(x != xo))
    ell = abs(ll - llo) / abs(llo)
    print("%-22s differing samples %d  ll rel err %.3g  diag %s" % (tag, nbad, ell, list(d)), flush=True)
    assert nbad == 0, "%s: path differs at %d samples, first at %d (diag %s)" % (tag, nbad, int(np.argmax(x != xo)), d)
    assert ell <= 1e-9
    assert d[0] == 0 and d[7] == 0, d
    return ell


@pytest.mark.parametrize("N,K,per_source", RC.CASES, ids=[RC.case_id(c) for c in RC.CASES])
def test_every_ring_count_and_row(H, N, K, per_source):
    c = RC.case(N, K, per_source)
    name, r = RC.case_id((N, K, per_source)), c["ref"]
    t0 = time.time()
    # The plan API flags a boundary it cannot certify and leaves the remedy, a longer warm-up, to its caller (the host
    # ladder).  So does this test, like test_gpu_blocked_dispatch.py: every call runs at the first of the default
    # warm-up, 2 x and 4 x it at which no call leaves a flag, and every bar below holds at that warm-up.  The planted
    # signals are dense (a spike runs at most warm-up starts); which cases needed more is in DESIGN.md section 3.10.
    halo0 = None
    for widen in (1, 2, 4):
        if widen > 1:
            H.set_option("halo", widen * halo0)
        got = _all_calls(H, c, check_geometry=widen == 1)
        halo0 = halo0 or got["info"]["halo"]
        if not any(got["flags"]):
            break
        print("%s: warm-up %d leaves flags %s, widening" % (name, got["info"]["halo"], got["flags"]), flush=True)
    dec, info = got["dec"], got["info"]
    # decode, both backtrace forms
    for form in (1, 2):
        x, ll, d, listed, row = dec[form]
        check_decode(c, "%s %s" % (name, row.split()[-1]), x, ll, d)
    assert dec[1][1] == dec[2][1]
    # E-step + M-step
    s, o, d = got["estep"]
    em = check_mstep("%s (%d chains)" % (name, info["nchains"]), o, c, N)
    assert d[3] == 0 and d[5] == 0, d
    # fused call: bit-equal to the separate calls
    x, ll, d, sf = got["fused"]
    assert np.array_equal(x, dec[1][0]) and ll == dec[1][1], (int(np.count_nonzero(x != dec[1][0])), ll, dec[1][1])
    assert np.array_equal(sf, s), float(np.abs(sf - s).max())
    assert d[0] == 0 and d[7] == 0 and d[3] == 0 and d[5] == 0, d
    # posteriors on the windows (rings of up to POST_MAX_L states; longer ones were refused by name in _all_calls)
    worst = dict(onset=0.0, occ=0.0, silent=0.0)
    w, logz, d = got["post"] or ([], float(r["loglik"]), None)
    assert d is None or (d[3] == 0 and d[5] == 0), d
    for i, (on, oc, si) in enumerate(w):
        worst["onset"] = max(worst["onset"], float(np.abs(on - r["w%d_onset" % i]).max()))
        worst["occ"] = max(worst["occ"], float(np.abs(oc - r["w%d_occ" % i]).max()))
        worst["silent"] = max(worst["silent"], float(np.abs(si - r["w%d_silent" % i]).max()))
    ez = abs(logz - r["loglik"]) / abs(r["loglik"])
    rows = got["rows"]
    print("%s: S=%d T=%d  %d chains of %d, warm-up %d (default %d)  %s | %s | %s  listed %s  M-step mu_abs %.3g mu_rel %.3g "
          "sigma %.3g lp %.3g  posteriors %s  logz rel %.3g  %.2f s" % (
              name, c["osm"].nstates, c["T"], info["nchains"], info["block"], info["halo"], halo0, rows[0],
              rows[1].split("vit")[1], rows[2].split(" ", 2)[2], dec[1][3], em["mu_abs"], em["mu_rel"], em["sigma"],
              em["lp"], "  ".join("%s %.3g" % kv for kv in worst.items()), ez, time.time() - t0), flush=True)
    assert max(worst.values()) <= 1e-8, worst
    assert ez <= 1e-10


def _all_calls(H, c, check_geometry):
    """the four calls of a case at the warm-up the options ask for; the rows are asserted before each call"""
    dec = {}
    for form in (1, 2):
        H.set_option("backtrace", form)
        p = Run(H, c)
        try:
            assert p.info["engine"] == H.ENGINE_WAVE and p.info["nchains"] >= 3 and c["T"] % 64 != 0, p.info
            if check_geometry:
                assert p.info["block"] == c["block"] and p.info["nchains"] == c["nchains"], (p.info, c["block"])
            row = assert_row(H, p.plan, c, 1, light=form == 2)
            x, ll, d, _ = p.decode()
            dec[form] = (x, ll, d, dispatch(H, p.plan, 1)[1], row)
        finally:
            p.close()
    H.set_option("backtrace", 0)
    p = Run(H, c)
    try:
        rows = [assert_row(H, p.plan, c, 2), assert_row(H, p.plan, c, 3, light=True), assert_row(H, p.plan, c, 4)]
        estep = p.estep()
        fused = p.decode(stats=True)
        if c["L"] <= POST_MAX_L:
            post = p.posteriors(c["win"])
        else:       # refused by name (wave_post.hip: the staged window of kw_post_marginals); the sweeps ran in the E-step
            with pytest.raises(H.HmmsortError, match="plan_posteriors: rings longer than %d states" % POST_MAX_L):
                p.posteriors(c["win"])
            post = None
        info = p.info
    finally:
        p.close()
    flags = [dec[1][2][0], dec[2][2][0], estep[2][3], estep[2][5], fused[2][0], fused[2][3], fused[2][5]] \
        + ([post[2][3], post[2][5]] if post else [])
    return dict(dec=dec, rows=rows, estep=estep, fused=fused, post=post, info=info, flags=flags)


# 3-8 rings of at most 64 states fuse the statistics into the backward sweep; HMMSORT_GSUM_SEPARATE sends them to
# kw_gsum_mx<N, 1> (N = 3, 4, and 5-8 up to 32 states) and kw_gsum_mx<N, 2> (5-8 rings of 33-64 states)
SEPARATE = [(N, K) for K in (9, 24, 65) for N in range(3, 9)]


def _mstep_under(H, monkeypatch, c, env):
    monkeypatch.setenv(env, "1")
    p = Run(H, c)
    try:
        row = assert_row(H, p.plan, c, 2, env=env)
        _, o, d = p.estep()
    finally:
        p.close()
    check_mstep("%s %s" % (RC.case_id((c["N"], c["K"], c["per_source"])), row.split()[-1]), o, c, c["N"])
    assert d[3] == 0 and d[5] == 0, d


@pytest.mark.parametrize("N,K", SEPARATE, ids=["%dx%d" % c for c in SEPARATE])
def test_separate_statistics_kernel(H, monkeypatch, N, K):
    _mstep_under(H, monkeypatch, RC.case(N, K, False), "HMMSORT_GSUM_SEPARATE")


def test_generic_statistics_kernel(H, monkeypatch):
    _mstep_under(H, monkeypatch, RC.case(11, 66, False), "HMMSORT_GSUM_GENERIC")


def test_switches_are_read_at_the_call(H, monkeypatch):
    c = RC.case(4, 24, False)
    p = Run(H, c)
    try:
        assert dispatch(H, p.plan, 2)[0].endswith("bwd<4,uc,ft1> gsum=bwd")
        monkeypatch.setenv("HMMSORT_GSUM_SEPARATE", "1")
        assert dispatch(H, p.plan, 2)[0].endswith("bwd<4,uc,ft0> gsum=mx<4,1>x1")
        monkeypatch.setenv("HMMSORT_GSUM_GENERIC", "1")
        assert dispatch(H, p.plan, 2)[0].endswith("bwd<4,uc,ft0> gsum=generic")
    finally:
        p.close()


def test_one_chain_runs_no_certificate_round(H):
    # a plan of one chain has no boundary: no kw_vit_redo launch
    c = RC.case(2, 24, False)
    T = 560                                   # less than one chain of 576 samples
    y = np.array(c["y"][:T])
    from oracle import oracle as O
    xo, llo = O.viterbi(y, c["osm"], c["mu"], c["sigma"])
    p = Run(H, c, y=y)
    try:
        assert p.info["nchains"] == 1
        assert dispatch(H, p.plan, 1)[0] == RC.expected_row(2, 23, False, 1, chains=1) \
            == "prepass<2> vit<2,uc> redo=none backtrace=rows<2>"
        x, ll, d, _ = p.decode()
    finally:
        p.close()
    check_decode(c, "2x24 one chain", x, ll, d, xo, llo)


def test_dispatch_refuses_other_engines_and_calls(H):
    c = RC.case(2, 24, False)
    buf = C.create_string_buffer(512)
    fn = _aid(H)
    H.set_option("engine", H.ENGINE_RING)
    plan = H.Plan(c["T"], c["sm"], c["mu"], c["sigma"])
    assert plan.info()["engine"] == H.ENGINE_RING
    assert fn(plan._h, 1, buf, len(buf)) == H._lib.EINVAL
    assert fn(None, 1, buf, len(buf)) == H._lib.EINVAL
    plan.close()
    H.set_option("engine", H.ENGINE_WAVE)
    plan = H.Plan(c["T"], c["sm"], c["mu"], c["sigma"])
    assert fn(plan._h, 0, buf, len(buf)) == H._lib.EINVAL and fn(plan._h, 5, buf, len(buf)) == H._lib.EINVAL
    assert fn(plan._h, 2, buf, 8) == H._lib.EINVAL                # a buffer too small for the answer
    plan.close()


# ---- the re-sweep kernels --------------------------------------------------------------------------------------
# kw_vit_redo runs in every decode of more than one chain, but sweeps a chain only when a certificate round lists it.
# Here the warm-up is the shortest the engine takes (option "halo" = 1 is clamped to L + 8 samples, two super-steps)
# and a train of five abutting spikes lies across two of the six chain boundaries (the second and the fifth), so that
# a spike is running where those warm-ups start: the warm-up (from "silent, rings empty") cannot hold that spike, its
# state at the boundary differs from the previous chain's end state by more than one constant, round 0 lists the chain
# and kw_vit_redo sweeps it again from the exact hand-off.  The decode must still be the oracle's with every boundary
# certified.  (A train across EVERY boundary is more than two rounds repair: each round lists only a failing chain
# whose predecessor passes; measured, round 0 and 1 listed one chain each and four boundaries stayed flagged.)
RESWEEP = [(4, 24, False), (4, 24, True), (8, 24, False), (8, 24, True), (12, 24, False)]


@pytest.mark.parametrize("N,K,per_source", RESWEEP, ids=[RC.case_id(c) for c in RESWEEP])
def test_resweep_kernels_sweep_listed_chains(H, N, K, per_source):
    from oracle import oracle as O
    c = RC.case(N, K, per_source)
    L = c["L"]
    H.set_option("halo", 1)
    H.set_option("block", 512)
    probe = H.Plan(4096, c["sm"], c["mu"], c["sigma"])
    B, halo = probe.info()["block"], probe.info()["halo"]
    probe.close()
    assert halo <= 2 * L + 1, (halo, L)
    T = 6 * B + 37
    # noise, one spike of every template in mid-chain (far from any warm-up), and the two trains
    y = np.random.default_rng(77 + N).normal(0.0, RC.SIGMA, T)
    for a in range(N):
        t = (a % 6) * B + B // 4 + (a // 6) * 3 * L
        y[t:t + L] += RC.MODEL_SCALE * c["temps"][1:, a]
    for j, b in enumerate((2 * B, 5 * B)):
        t = b - 2 * L - L // 2
        for i in range(5):
            y[t:t + L] += RC.MODEL_SCALE * c["temps"][1:, (j + i) % N]      # consecutive templates
            t += L
    xo, llo = O.viterbi(y, c["osm"], c["mu"], c["sigma"])
    calls = [(1, False)] + ([(3, True)] if N <= 4 else [])
    for call, fused in calls:
        p = Run(H, c, y=y)
        try:
            assert p.info["nchains"] == 7 and p.info["halo"] == halo
            row = dispatch(H, p.plan, call)[0]
            assert ("redo<%d,%s%s>" % (N, "ps" if per_source else "uc", ",tight" if fused else "")) in row, row
            x, ll, d, _ = p.decode(stats=fused)
            listed = dispatch(H, p.plan, call)[1]
        finally:
            p.close()
        print("%s re-sweep, call %d: %s  warm-up %d, chains of %d  listed %s  diag %s" % (
            RC.case_id((N, K, per_source)), call, row, halo, B, listed, list(d)), flush=True)
        nbad = int(np.count_nonzero(x != xo))
        assert nbad == 0, (nbad, int(np.argmax(x != xo)), d)
        assert abs(ll - llo) <= 1e-9 * abs(llo)
        assert d[0] == 0 and d[7] == 0, d
        assert listed[0] >= 1, listed
