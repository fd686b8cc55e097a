"""The tail of the wave engine's decode: both forms of the backtrace kernel (register rows / light, option
"backtrace" = 1 / 2), the final state found inside the backtrace, the re-sweep of failed chains over a compact
list, the stitch repair with the first state in one launch, the resolver's scans in 256-thread blocks, and the
tie counters that live next to diag.

The path oracle is oracle.viterbi.  Segment geometry (Bb, Hb) follows make_geometry (csrc/wave_engine.hip); the
wave engine takes recordings of at least max(512, 4 L) samples (wave_supported), so the shortest recordings of
the backtrace cases (T = 2, 3 and Bb - 1 with Bb = 512) are decoded by whichever engine the library chooses for
them -- they are kept as cases of the plan API, not of the backtrace kernel.

Signals of the certificate and stitch cases were chosen on the CPU with tests/wave_model.py (no GPU run):
* certificates: 4 x 60 states, 20 000 samples, pp = (0.03, 0.02, 0.025, 0.02), options block = 128, halo = 128
  (the engine makes chains of 320 samples with a warm-up of 178).  The model, run round by round like the kernels
  (check, re-sweep of the failed chains whose predecessor did not fail, check again), predicts:
  seed 22: chains 20, 25, 27, 35, 49, 51, 54 fail, none next to another: round 0 repairs them, diag[1] = 7.
  seed 26: chains 1, 11, 20, 40, 43, 47, 48, 62 fail in round 0; 48 stands behind 47, so round 0 leaves it and
  only round 1 can sweep it again: diag[1] = 8 + 1 = 9.  Both end with every certificate met (diag[0] = 0).
* stitch: see STITCH_CASES.
"""
import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm

pytestmark = pytest.mark.gpu


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


def check_all_forms(O, H, ys, sms, mus, sigmas, wave=True):
    """path == oracle for backtrace = 1 and 2 with equal diag and tie_stats; the fused call (backtrace = 0: the
    light form) equals viterbi + estep bit for bit"""
    H.set_option("engine", H.ENGINE_WAVE if wave else H.ENGINE_AUTO)
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


# one N per back-pointer row width (1, 2, 3, 4 words: wpsi_words_c), and the N = 2 / 4 of the issue
SHAPES = [(2, 20), (4, 20), (8, 20), (12, 20), (16, 20)]


def _t_values(L):
    Bb, _ = seg_geometry(L)
    return [2, 3, Bb - 1, Bb, Bb + 1, 64 * Bb - 1, 64 * Bb, 64 * Bb + 1]


@pytest.mark.parametrize("N,K", SHAPES)
@pytest.mark.parametrize("ti", range(8))
def test_both_backtrace_forms(O, H, N, K, ti):
    L = K - 1
    T = _t_values(L)[ti]
    temps, pp = family(H, N, K, 100 + N)
    y = H.create_signal(T, 0.3, pp, temps, seed=7 * N + ti)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    check_all_forms(O, H, [y], [sm], [temps], [0.3], wave=T >= max(512, 4 * L))


def test_odd_length_two_channels_with_different_models(O, H):
    """odd T puts the second channel of x on an odd sample: the unaligned int16-pair stores"""
    N, K = 4, 20
    T = 64 * seg_geometry(K - 1)[0] + 1
    t1, p1 = family(H, N, K, 1)
    t2, p2 = family(H, N, K, 2)
    t2 = np.asfortranarray(t2 * 1.2)
    ys = [H.create_signal(T, 0.3, p1, t1, seed=51), H.create_signal(T, 0.35, p2, t2, seed=52)]
    sms = [H.StateMatrix.create(N, K, np.log(p), False) for p in (p1, p2)]
    check_all_forms(O, H, ys, sms, [t1, t2], [0.3, 0.35])


def test_recording_that_ends_inside_a_spike(O, H):
    """the final state is inside a ring: found by the backtrace workgroup of the last segment"""
    N, K = 2, 20
    T = 64 * seg_geometry(K - 1)[0] + 1
    temps, pp = family(H, N, K, 3)
    y = H.create_signal(T, 0.3, pp, temps, seed=61)
    cut = 11
    y[T - cut:] += temps[1:cut + 1, 1]
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, _ = check_all_forms(O, H, [y], [sm], [temps], [0.3])
    assert xo[0][-1] > 1, "the oracle should end inside the spike"


@pytest.mark.parametrize("seed,swept", [(22, 7), (26, 9)])
def test_failed_certificates_are_repaired_from_the_list(O, H, seed, swept):
    K, N, T = 60, 4, 20_000
    temps = four_templates(H, K)
    pp = [0.03, 0.02, 0.025, 0.02]
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    H.set_option("block", 128)
    H.set_option("halo", 128)
    xo, (x, ll, diag, ties) = check_all_forms(O, H, [y], [sm], [temps], [0.3])
    print("seed %d: diag %s" % (seed, list(diag)))
    assert diag[0] == 0, diag         # every certificate holds in the end
    assert diag[1] == swept, diag     # failed checks of rounds 0 and 1, as the CPU model counts them


# (pp of each template, sigma, seed) -> what the CPU model predicts (tests/wave_model.py's back-pointers, one lane per
# segment, then the check / parallel repair / second check / serial repair in the kernels' order):
#   (0.1, 2.5, 5): first list [35, 36]; the parallel repair leaves 35 alone (its successor is queued) and re-walks
#                  36; the second check lists 35 and the serial repair re-walks it: 1 + 1 fixes.
#   (0.2, 1.5, 5): first list [10, 12, 18, 19, 20, 21, 30]; 4 parallel fixes (10, 12, 21, 30); second list [18, 19];
#                  the serial repair fixes 19 and 18, and 18 a second time when the list is walked in ascending
#                  order (its successor's first sample changes under it): 2 or 3 serial fixes.
STITCH_CASES = [(0.1, 2.5, 5, 2, 2), (0.2, 1.5, 5, 6, 7)]


@pytest.mark.parametrize("pp1,sigma,seed,lo,hi", STITCH_CASES)
def test_stitch_repair_and_first_state(O, H, pp1, sigma, seed, lo, hi):
    """long rings (4 x 256 states), busy and noisy: segments' walks that have not merged with the path when they
    reach their segment, alone and next to each other, so that the parallel repair, the second check inside
    kw_stitch_fix and its serial repair all do work.  One chain (option block = T), so that diag[1] counts
    stitch repairs only."""
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


@pytest.mark.parametrize("count", [255, 257, 1023, 1025])
@pytest.mark.parametrize("which", ["nblk", "ntile"])
def test_resolver_scans_around_their_partition_counts(O, H, which, count):
    """kw_tie_offsets scans ntile = ceil(T / 4096) counts, kw_tie_bscan nblk = ceil(T / 512) block sums, each in
    1 024 partitions handled by 256 threads: counts just below and above 256 and 1 024"""
    N, K = 2, 20
    unit = 512 if which == "nblk" else 4096
    T = count * unit - 3
    assert (T + unit - 1) // unit == count
    temps, pp = family(H, N, K, 5)
    y = H.create_signal(T, 0.3, pp, temps, seed=count)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("tie_scale", 30_000_000)
    r = Run(H, [y], [sm], [temps], [0.3])
    try:
        x, ll, diag, ties = r.viterbi()
    finally:
        r.close()
    print("%s = %d: %s" % (which, count, ties))
    assert ties["flagged"] > 0, ties
    assert ties["unresolved"] == 0 and diag[7] == 0, (ties, diag)
    assert np.array_equal(x[0], xo), int(np.count_nonzero(x[0] != xo))
    assert abs(ll[0] - llo) <= 1e-9 * abs(llo)


def test_tie_statistics_survive_an_estep(H):
    N, K, T = 4, 60, 60_000
    temps, pp = family(H, N, K, 9)
    y = H.create_signal(T, 0.3, pp, temps, seed=77)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("tie_scale", 30_000_000)
    r = Run(H, [y], [sm], [temps], [0.3])
    try:
        _, _, _, ties = r.viterbi()
        assert ties["flagged"] > 0, ties
        r.estep()
        assert r.plan.tie_stats(r.st) == ties
    finally:
        r.close()
