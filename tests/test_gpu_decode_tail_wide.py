"""The decode tail with the light backtrace staging its tiles through 16-byte loads.

The light backtrace (option "backtrace" = 2, and the fused decode + E-step call) stages a plane of back-pointers
with 16-byte loads when the plane starts on 16 bytes, and with dword loads otherwise.  A plane starts at
psi + (w C + ch) T words, so T decides which planes (w > 0) and channels (ch > 0) are aligned, and the one group of
four samples that T cuts always comes in by dwords.  Every case compares the path with oracle.viterbi and ll, diag
and the tie counters between backtrace = 1, 2 and the fused call bit for bit (check_all_forms, as in
test_gpu_decode_tail.py; the helpers are copies of that file's).

K = 20 gives segments of Bb = 512 samples with a walk-in of Hb = 128 (seg_geometry).

The resolver cases run the exact near-tie resolver behind the light backtrace of the fused call, with decisions
to re-decide; the ll cases pin ll to the value recorded before the backtrace changed
(tests/golden/decode_tail_wide/ll_parent.json, recorded once on an MI355X from the parent build: T, seed and the
8 bytes of ll), at lengths below one pass of kw_ll_partial's grid, with a ragged last pass, and of several passes.
"""
import json
import os

import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_tail_wide", "ll_parent.json")


@pytest.fixture(autouse=True)
def options(H):
    yield
    for k, v in (("engine", H.ENGINE_AUTO), ("block", 0), ("halo", 0), ("tie_scale", 1), ("tie_debug", 0),
                 ("backtrace", 0)):
        H.set_option(k, v)


def seg_geometry(L):
    """make_geometry's backtrace segments: length Bb and walk-in Hb"""
    Bb, Hb = 512, 128
    while Hb < 2 * L + 64:
        Hb += 64
    return max(Bb, 2 * Hb), Hb


def family(H, N, K, seed):
    base = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    amps = [(base[i % 4][0] * (1 + 0.13 * (i // 4)), base[i % 4][1] + 0.03 * (i // 4), base[i % 4][2])
            for i in range(N)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *a) for a in amps], 1))
    rng = np.random.default_rng(seed)
    pp = rng.uniform(2e-3, 6e-3, N) * min(1.0, 4.0 / N)
    return temps, pp


class Run:
    """one plan (C channels), its buffers, and the three calls"""

    def __init__(self, H, ys, sms, mus, sigmas):
        import torch
        self.torch, self.H = torch, H
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
        return self.stats.cpu().numpy().copy(), self.plan.diagnostics(self.st)

    def decode_estep(self):
        self.dx.fill_(-1)
        self.stats.fill_(0)
        self.plan.decode_estep(self.dy, self.dx, self.dll, self.stats, self.st)
        return self._out() + (self.stats.cpu().numpy().copy(), self.plan.diagnostics(self.st),
                              self.plan.tie_stats(self.st))

    def close(self):
        self.plan.close()


def check_all_forms(O, H, ys, sms, mus, sigmas, wave=True, xo=None):
    """path == oracle for backtrace = 1 and 2 with equal diag and tie_stats; the fused call (backtrace = 0: the
    light form) equals viterbi + estep bit for bit"""
    H.set_option("engine", H.ENGINE_WAVE if wave else H.ENGINE_AUTO)
    if xo is None:
        xo = [O.viterbi(y, to_oracle_sm(O, sm), mu, s)[0] for y, sm, mu, s in zip(ys, sms, mus, sigmas)]
    got = {}
    for mode in (1, 2, 0):
        H.set_option("backtrace", mode)      # read when the plan is created
        r = Run(H, ys, sms, mus, sigmas)
        try:
            x, ll, dv, ties = r.viterbi()
            for c in range(r.C):
                nbad = int(np.count_nonzero(x[c] != xo[c]))
                assert nbad == 0, "backtrace=%d channel %d: path differs at %d samples, first at %d" % (
                    mode, c, nbad, int(np.argmax(x[c] != xo[c])))
            got[mode] = (x, ll, dv, ties)
            if mode == 0 and wave:
                st, de = r.estep()
                assert r.plan.tie_stats(r.st) == ties, "an E-step must leave the decode's tie counters alone"
                xf, llf, stf, df, tf = r.decode_estep()
                assert np.array_equal(xf, x) and np.array_equal(llf, ll), "fused path / ll differ"
                assert np.array_equal(stf, st), "fused statistics differ"
                assert list(df) == list(dv[:3]) + list(de[3:7]) + list(dv[7:8]), (df, dv, de)
                assert tf == ties, (tf, ties)
        finally:
            r.close()
    for mode in (2, 0):
        assert np.array_equal(got[mode][1], got[1][1])
        assert list(got[mode][2]) == list(got[1][2]), (mode, got[mode][2], got[1][2])
        assert got[mode][3] == got[1][3], (mode, got[mode][3], got[1][3])
    return xo, got[1]


# ---------------------------------------------------------------- alignment of planes and channels

@pytest.mark.parametrize("N", [4, 8, 12, 16])     # 1, 2, 3, 4 words per back-pointer row
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_plane_alignment_one_channel(O, H, N, r):
    """T = 64 Bb + r: with r != 0 the planes w > 0 start off 16 bytes and take the dword path beside plane 0"""
    K = 20
    T = 64 * seg_geometry(K - 1)[0] + r
    temps, pp = family(H, N, K, 200 + N)
    y = H.create_signal(T, 0.3, pp, temps, seed=11 * N + r)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    check_all_forms(O, H, [y], [sm], [temps], [0.3])


@pytest.mark.parametrize("N", [4, 8])
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_plane_alignment_two_channels_with_different_models(O, H, N, r):
    """the second channel's planes and its x start at ch T: off 16 bytes (planes) and off 4 bytes (x, odd r)"""
    K = 20
    T = 64 * seg_geometry(K - 1)[0] + r
    t1, p1 = family(H, N, K, 21)
    t2, p2 = family(H, N, K, 22)
    t2 = np.asfortranarray(t2 * 1.2)
    ys = [H.create_signal(T, 0.3, p1, t1, seed=300 + 4 * N + r), H.create_signal(T, 0.35, p2, t2, seed=400 + 4 * N + r)]
    sms = [H.StateMatrix.create(N, K, np.log(p), False) for p in (p1, p2)]
    check_all_forms(O, H, ys, sms, [t1, t2], [0.3, 0.35])


@pytest.mark.parametrize("d", [1, 2, 3, 5, 61, 67])
def test_data_ends_inside_a_group_and_inside_a_tile(O, H, d):
    """T = 63 Bb + d: the last segment is d samples long; the last group of four crosses T unless d is a
    multiple of four, and d = 67 ends in the second tile of the segment"""
    N, K = 4, 20
    T = 63 * seg_geometry(K - 1)[0] + d
    temps, pp = family(H, N, K, 31)
    y = H.create_signal(T, 0.3, pp, temps, seed=500 + d)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    check_all_forms(O, H, [y], [sm], [temps], [0.3])


# ---------------------------------------------------------------- stitch repairs

# the shapes of test_gpu_decode_tail.py's STITCH_CASES, with the ranges of diag[1] the CPU model gives there
STITCH_CASES = [(0.1, 2.5, 5, 2, 2), (0.2, 1.5, 5, 6, 7)]


@pytest.mark.parametrize("pp1,sigma,seed,lo,hi", STITCH_CASES)
def test_stitch_repairs_still_happen_and_are_counted(O, H, pp1, sigma, seed, lo, hi):
    K, N, T = 256, 4, 48_000
    temps = four_templates(H, K)
    pp = [pp1] * N
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    H.set_option("block", T)
    xo, (x, ll, diag, ties) = check_all_forms(O, H, [y], [sm], [temps], [sigma])
    print("stitch pp=%g sigma=%g: diag %s" % (pp1, sigma, list(diag)))
    assert diag[0] == 0, diag
    assert lo <= diag[1] <= hi, diag
    assert x[0][0] == xo[0][0]


# ---------------------------------------------------------------- the resolver beside the E-step

# (N, K, T, family seed, signal seed): the signals of test_gpu_decode_tail.py's resolver cases, whose decodes
# flag decisions at tie_scale = 30 000 000 (asserted below as well: without flagged decisions the case proves nothing)
RESOLVER_CASES = [(4, 60, 60_000, 9, 77), (2, 20, 255 * 512 - 3, 5, 255)]


@pytest.mark.parametrize("N,K,T,fseed,seed", RESOLVER_CASES)
def test_resolver_beside_the_estep(O, H, N, K, T, fseed, seed):
    temps, pp = family(H, N, K, fseed)
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("tie_scale", 30_000_000)
    r = Run(H, [y], [sm], [temps], [0.3])
    try:
        x, ll, dv, ties = r.viterbi()
        st, de = r.estep()
        xf, llf, stf, df, tf = r.decode_estep()
    finally:
        r.close()
    print("N=%d T=%d: %s" % (N, T, tf))
    assert tf["flagged"] > 0, tf
    assert tf["unresolved"] == 0 and df[7] == 0, (tf, df)
    assert np.array_equal(xf[0], xo), int(np.count_nonzero(xf[0] != xo))
    assert abs(llf[0] - llo) <= 1e-9 * abs(llo)
    assert np.array_equal(xf, x) and np.array_equal(llf, ll), "fused path / ll differ"
    assert np.array_equal(stf, st), "fused statistics differ"
    assert list(df) == list(dv[:3]) + list(de[3:7]) + list(dv[7:8]), (df, dv, de)
    assert tf == ties, (tf, ties)


# ---------------------------------------------------------------- ll, bit for bit

def ll_cases():
    return json.load(open(GOLDEN))["cases"]


def ll_signal(H, T, seed):
    N, K = 2, 20
    temps, pp = family(H, N, K, 41)
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    return y, sm, temps


# fewer samples than one pass of the grid (also fewer than the wave engine takes: the library chooses the engine),
# a ragged last pass, and several passes: one T above nparts x 256 x 8 (nparts = 1 024 partial sums per channel)
LL_T = [1 * 256 + 1, 7 * 256 * 4 + 3, 1024 * 256 * 8 + 1029]


@pytest.mark.parametrize("T", LL_T)
def test_ll_is_the_parents_to_the_bit(O, H, T):
    case = [c for c in ll_cases() if c["T"] == T]
    assert len(case) == 1, "no recorded value for T = %d" % T
    case = case[0]
    y, sm, temps = ll_signal(H, T, case["seed"])
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    wave = T >= max(512, 4 * (sm.K - 1))
    _, (x, ll, diag, ties) = check_all_forms(O, H, [y], [sm], [temps], [0.3], wave=wave, xo=[xo])
    print("T=%d ll=%r (%s) oracle %r" % (T, float(ll[0]), ll[0].tobytes().hex(), llo))
    assert abs(ll[0] - llo) <= 1e-9 * abs(llo)
    assert ll[0].tobytes().hex() == case["ll_bytes"], (ll[0].tobytes().hex(), case["ll_bytes"])
