"""The light backtrace's event walk (csrc/wave_viterbi.hip, HS_BT_EVENTS) on the device: it walks junction
decisions instead of samples, so every case here is chosen for what the jumps meet -- nothing but silence, rings
without silence between them (ring lengths 8, 59 and 255: the ramp bound of a tile row, a ring inside a tile, a
ring over four tiles), the headline rates, walks that start and end inside a ring, planes off 16 bytes, every
back-pointer row width, and hundreds of flagged decisions.

For every case the register-row kernel ("backtrace" = 1) is the independent reference: x sample for sample, ll bit
for bit, diagnostics and tie counters equal, all equal to the oracle path; the fused decode + E-step call gives the
same and its statistics equal a separate E-step's bit for bit.  Each case also asserts on the oracle path that the
feature it is there for is present (the CPU statement of the two walks is tests/test_backtrace_model_cpu.py).

Recordings are 3 to 6 backtrace segments long with chains of 128 samples (the dense case with rings of 255 states
runs as one chain), so every case has several chains, a walk that starts at T, inner segments and the segment that
holds recording sample 0.
"""
import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm

pytestmark = pytest.mark.gpu

OPTIONS = (("engine", 0), ("block", 0), ("halo", 0), ("tie_scale", 1), ("tie_debug", 0), ("backtrace", 0))


@pytest.fixture(autouse=True)
def options(H):
    yield
    for k, v in OPTIONS:
        H.set_option(k, H.ENGINE_AUTO if k == "engine" else v)


def seg_geometry(L):
    """make_geometry's backtrace segments: length Bb and walk-in Hb"""
    Bb, Hb = 512, 128
    while Hb < 2 * L + 64:
        Hb += 64
    return max(Bb, 2 * Hb), Hb


def templates(H, N, K):
    base = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    amps = [(base[i % 4][0] * (1 + 0.13 * (i // 4)), base[i % 4][1] + 0.03 * (i // 4), base[i % 4][2])
            for i in range(N)]
    return np.asfortranarray(np.stack([H.create_spike_template(K, *a) for a in amps], 1))


class Run:
    """one plan (C channels), its buffers, and the three calls"""

    def __init__(self, H, ys, sms, mus, sigmas):
        import torch
        self.C, self.T = len(ys), len(ys[0])
        self.st = torch.cuda.current_stream().cuda_stream
        if self.C == 1:
            self.plan = H.Plan(self.T, sms[0], mus[0], sigmas[0])
        else:
            self.plan = H.Plan.batched(self.T, sms, mus, sigmas)
        self.dy = torch.from_numpy(np.ascontiguousarray(np.stack(ys))).cuda()
        self.dx = torch.zeros((self.C, self.T), dtype=torch.int16, device="cuda")
        self.dll = torch.zeros(self.C, dtype=torch.float64, device="cuda")
        self.stats = torch.zeros(self.C * self.plan.stats_len() if self.C > 1 else self.plan.stats_len(),
                                 dtype=torch.float64, device="cuda")

    def _out(self):
        return self.dx.cpu().numpy().copy(), self.dll.cpu().numpy().copy()

    def viterbi(self):
        self.dx.fill_(-1)
        self.plan.viterbi(self.dy, self.dx, self.dll, self.st)
        return self._out() + (self.plan.diagnostics(self.st), self.plan.tie_stats(self.st))

    def estep(self):
        self.stats.fill_(0)
        self.plan.estep(self.dy, self.stats, self.st)
        return self.stats.cpu().numpy().copy()

    def decode_estep(self):
        self.dx.fill_(-1)
        self.stats.fill_(0)
        self.plan.decode_estep(self.dy, self.dx, self.dll, self.stats, self.st)
        return self._out() + (self.stats.cpu().numpy().copy(), self.plan.diagnostics(self.st),
                              self.plan.tie_stats(self.st))

    def close(self):
        self.plan.close()


def forms(H, ys, sms, mus, sigmas):
    """decode with the register rows, the light form, and through the fused call (the light form); the fused
    call's statistics against a separate E-step"""
    got = {}
    for mode in (1, 2):
        H.set_option("backtrace", mode)      # read when the plan is created
        r = Run(H, ys, sms, mus, sigmas)
        try:
            assert r.plan.info()["engine"] == H.ENGINE_WAVE, r.plan.info()
            got[mode] = r.viterbi()
            if mode == 2:
                st = r.estep()
                got["fused"] = r.decode_estep()
                assert np.array_equal(got["fused"][2], st), "fused statistics differ from a separate E-step's"
        finally:
            r.close()
    return got


def check(O, H, ys, sms, mus, sigmas, name, block=128):
    """All bars of the file for one case.  A dense case whose default warm-up leaves a boundary uncertified runs
    again at 2 x and 4 x the warm-up (the remedy the plan API leaves to its caller) and says so."""
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", block)
    H.set_option("halo", 128)
    xo = [np.asarray(O.viterbi(y, to_oracle_sm(O, sm), mu, s)[0]) for y, sm, mu, s in zip(ys, sms, mus, sigmas)]
    for widen in (1, 2, 4):
        if widen > 1:
            H.set_option("halo", 128 * widen)
        got = forms(H, ys, sms, mus, sigmas)
        if got[1][2][0] == 0:
            break
        print("%s: warm-up option %d leaves diag %s, widening" % (name, 128 * widen, list(got[1][2])), flush=True)
    x1, ll1, d1, t1 = got[1]
    print("%s: T=%d diag %s ties %s" % (name, len(ys[0]), list(d1), t1), flush=True)
    assert d1[0] == 0, d1
    for c in range(len(ys)):
        bad = np.flatnonzero(x1[c] != xo[c])
        assert bad.size == 0, "register rows, channel %d: %d samples differ from the oracle, first %d" % (c, bad.size, bad[0])
    x2, ll2, d2, t2 = got[2]
    bad = np.flatnonzero(x2 != x1)
    assert bad.size == 0, "light form: %d samples differ from the register rows, first at %d" % (bad.size, bad[0])
    assert np.array_equal(ll2, ll1), (ll2, ll1)
    assert list(d2) == list(d1), (d2, d1)
    assert t2 == t1, (t2, t1)
    xf, llf, _, df, tf = got["fused"]
    bad = np.flatnonzero(xf != x1)
    assert bad.size == 0, "fused call: %d samples differ from the register rows, first at %d" % (bad.size, bad[0])
    assert np.array_equal(llf, ll1), (llf, ll1)
    assert list(df[:3]) == list(d1[:3]) and df[7] == d1[7] and df[0] == 0, (df, d1)
    assert tf == t1, (tf, t1)
    return xo, t1


def rings_across(x, edges):
    """how many of the samples `edges` have a ring state on both sides"""
    return sum(1 for e in edges if 0 < e < len(x) and x[e - 1] > 1 and x[e] > 1)


def silent_share(x):
    return float(np.mean(np.asarray(x) == 1))


def test_pure_noise(O, H):
    """no spike anywhere: the whole walk is mask scanning"""
    N, K, T = 4, 60, 5 * 512 + 37
    temps = four_templates(H, K)
    pp = [0.002, 0.0015, 0.0025, 0.0015]
    y = 0.3 * np.random.default_rng(13).standard_normal(T)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, _ = check(O, H, [y], [sm], [temps], [0.3], "noise")
    assert (xo[0] == 1).all()


@pytest.mark.parametrize("K,p1,nsegs", [(9, 0.2, 5), (60, 0.1, 5), (256, 0.05, 3)])
def test_dense_rings(O, H, K, p1, nsegs):
    """rings follow each other with little or no silence.  L = 8: up to ten ramps in a tile row; L = 59: a ring
    inside a tile and across its edges; L = 255: a ring spans four tiles.  The generated signal leaves one silent
    sample between two spikes; a planted train of spikes L samples apart over the first segment edge has none, so
    there the path goes from a ring's last state straight into another ring."""
    N, L = 4, K - 1
    Bb, Hb = seg_geometry(L)
    T = nsegs * Bb + Hb // 2 + 29
    temps = four_templates(H, K) if K >= 20 else templates(H, N, K)
    pp = [p1] * N
    y = H.create_signal(T, 0.3, pp, temps, seed=300 + K)
    n = max(6, 200 // L)
    s0 = Bb - (n // 2) * L - L // 3
    y[s0:s0 + n * L] = 0.3 * np.random.default_rng(K).standard_normal(n * L)
    for i in range(n):
        y[s0 + i * L:s0 + (i + 1) * L] += temps[1:K, i % N]
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    # rings of 255 states this dense leave chains of a few hundred samples uncertified at any warm-up the
    # recording has room for: that case runs as one chain (as the stitch cases of test_gpu_decode_tail.py do);
    # its segments, which are what this file is about, are as many
    xo, _ = check(O, H, [y], [sm], [temps], [0.3], "dense L=%d" % L, block=T if L > 128 else 128)
    x = xo[0]
    back_to_back = int(np.count_nonzero((x[:-1] > 1) & (x[1:] > 1) & ((x[1:] - 2) % L == 0)))   # a ring's first state after a ring state
    print("dense L=%d: silent share %.3f, %d rings follow a ring directly" % (L, silent_share(x), back_to_back))
    assert silent_share(x) < 0.5 and back_to_back >= 3
    assert rings_across(x, range(Bb, T, Bb)) > 0, "no ring crosses a segment edge"
    assert rings_across(x, range(64, T, 64)) > 0, "no ring crosses a tile edge"


def test_headline_rates(O, H):
    N, K, T = 4, 60, 6 * 512 + 5
    temps = four_templates(H, K)
    pp = [0.002, 0.0015, 0.0025, 0.0015]       # 0.0075 onsets per sample
    y = H.create_signal(T, 0.3, pp, temps, seed=41)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, _ = check(O, H, [y], [sm], [temps], [0.3], "headline")
    assert 0.3 < silent_share(xo[0]) < 1.0


def test_recording_ends_and_begins_inside_a_spike(O, H):
    """the walk from T starts inside a ring (bt_start); the first segment's walk runs down a ring to sample 0"""
    N, K = 2, 20
    T = 3 * seg_geometry(K - 1)[0] + 1
    temps = templates(H, N, K)
    pp = [0.004, 0.003]
    y = H.create_signal(T, 0.3, pp, temps, seed=61)
    cut = 11
    y[T - cut:] += temps[1:cut + 1, 1]
    y[:cut] += temps[K - cut:, 0]
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, _ = check(O, H, [y], [sm], [temps], [0.3], "ends and begins in a spike")
    assert xo[0][-1] > 1, "the oracle should end inside a spike"
    assert xo[0][0] > 1, "the oracle should begin inside a spike"


def test_two_channels_at_odd_length(O, H):
    """a batched plan: the second channel's x and psi planes start off 4 and 16 bytes, which is the dword staging
    path and the unaligned x stores"""
    N, K = 4, 20
    T = 4 * seg_geometry(K - 1)[0] + 67
    t1 = templates(H, N, K)
    t2 = np.asfortranarray(t1 * 1.2)
    p1, p2 = [0.004, 0.003, 0.005, 0.002], [0.003, 0.005, 0.002, 0.004]
    ys = [H.create_signal(T, 0.3, p1, t1, seed=811), H.create_signal(T, 0.35, p2, t2, seed=812)]
    sms = [H.StateMatrix.create(N, K, np.log(p), False) for p in (p1, p2)]
    xo, _ = check(O, H, ys, sms, [t1, t2], [0.3, 0.35], "two channels")
    assert T % 2 == 1 and all((x > 1).any() for x in xo)


@pytest.mark.parametrize("N", [1, 4, 8, 16])
def test_every_row_width(O, H, N):
    """1, 1, 2 and 4 words per sample; 32 segments per workgroup for one word, 64 for more"""
    K = 20
    T = 3 * seg_geometry(K - 1)[0] + 131 + N
    temps = templates(H, N, K)
    pp = np.full(N, 0.016 / N)
    y = H.create_signal(T, 0.3, pp, temps, seed=13 * N + 1)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, _ = check(O, H, [y], [sm], [temps], [0.3], "N=%d" % N)
    assert len(set(int(v - 2) // (K - 1) for v in xo[0][xo[0] > 1])) >= min(N, 2), "spikes of more than one ring"


def test_hundreds_of_flagged_decisions(O, H):
    """the near-tie threshold raised until ordinary decisions are flagged: the counts the walk takes from the flag
    masks (silent stretches) and from the junction entries (ring starts) trigger and feed the resolver"""
    N, K, T = 4, 60, 6 * 512 + 77
    temps = four_templates(H, K)
    pp = [0.01, 0.008, 0.012, 0.008]
    y = H.create_signal(T, 1.0, pp, temps, seed=2)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    # a threshold of about 50: tests/wave_model.py (vit_decode with the kernels' threshold formula) counts about
    # 300 flagged decisions on this path; at the 300 000 000 of test_gpu_ties.py a recording this short has one
    H.set_option("tie_scale", 10_000_000_000)
    _, ties = check(O, H, [y], [sm], [temps], [1.0], "flagged")
    assert ties["flagged"] > 100, ties
    assert ties["trigger"] >= ties["flagged"], ties     # what the walks counted covers what the resolver listed
