"""The decode branch of the fused call, short enough to end under the backward sweep.

Three things changed in the wave engine's decode tail, and every case here holds one of them to the oracle and to
the unchanged kernels:

* the light backtrace (option "backtrace" = 2, and the fused decode + E-step call) gives a workgroup SPW = 16, 32
  or 64 segments instead of always 64, so the number of segments around multiples of those group sizes, the rows
  that do not exist in the last workgroup and the lanes that hold no row are what can go wrong;
* a certificate round that would repeat the round before it returns at once (option "cert_rounds" = 0, the
  default); "cert_rounds" = 1 runs every round in full, which is the code path from before;
* the path likelihood of the fused call runs behind the near-tie resolver on the decode's own stream again.

check_all_forms compares the path with oracle.viterbi and ll, diag and the tie counters between backtrace = 1 (the
register-row kernel, unchanged: the comparator), 2 and the fused call bit for bit.  The helpers are copies of
tests/test_gpu_decode_tail_wide.py's.  K = 20 gives segments of Bb = 512 samples with a walk-in of Hb = 128.
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
        H.set_option(k, v)          # ("cert_rounds" is set and put back by the cases that use it: both_cert_rounds)


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


# ---------------------------------------------------------------- segments per workgroup

@pytest.mark.parametrize("d", [0, 1, 3, 67])
@pytest.mark.parametrize("k", [15, 16, 17, 31, 33, 63, 65])
def test_segment_counts_around_the_group_sizes(O, H, k, d):
    """T = k Bb + d: k (d = 0) or k + 1 segments, one short of, equal to and one past a multiple of 16, 32 and 64;
    the last segment is d samples long (d = 3 ends inside a group of four, d = 67 in the second tile)"""
    N, K = 4, 20
    T = k * seg_geometry(K - 1)[0] + d
    temps, pp = family(H, N, K, 31)
    y = H.create_signal(T, 0.3, pp, temps, seed=700 + 8 * k + d)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    check_all_forms(O, H, [y], [sm], [temps], [0.3])


@pytest.mark.parametrize("N", [4, 8, 12, 16])     # 1, 2, 3, 4 words per back-pointer row
def test_every_row_width(O, H, N):
    K = 20
    T = 17 * seg_geometry(K - 1)[0] + 1
    temps, pp = family(H, N, K, 200 + N)
    y = H.create_signal(T, 0.3, pp, temps, seed=13 * N + 1)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    check_all_forms(O, H, [y], [sm], [temps], [0.3])


def test_two_channels_with_different_models_at_odd_length(O, H):
    """the second channel's planes start off 16 bytes (dword staging) and its x off 4 bytes"""
    N, K = 4, 20
    T = 17 * seg_geometry(K - 1)[0] + 3
    t1, p1 = family(H, N, K, 21)
    t2, p2 = family(H, N, K, 22)
    t2 = np.asfortranarray(t2 * 1.2)
    ys = [H.create_signal(T, 0.3, p1, t1, seed=811), H.create_signal(T, 0.35, p2, t2, seed=812)]
    sms = [H.StateMatrix.create(N, K, np.log(p), False) for p in (p1, p2)]
    check_all_forms(O, H, ys, sms, [t1, t2], [0.3, 0.35])


def test_recording_ends_inside_a_spike(O, H):
    """the walks that start at the last sample start inside a ring (bt_start), in a workgroup of one segment"""
    N, K = 2, 20
    T = 64 * seg_geometry(K - 1)[0] + 1
    temps, pp = family(H, N, K, 3)
    y = H.create_signal(T, 0.3, pp, temps, seed=61)
    cut = 11
    y[T - cut:] += temps[1:cut + 1, 1]
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo, _ = check_all_forms(O, H, [y], [sm], [temps], [0.3])
    assert xo[0][-1] > 1, "the oracle should end inside the spike"


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


# ---------------------------------------------------------------- certificate rounds

def both_cert_rounds(H, ys, sms, mus, sigmas, fused):
    """the decode (fused: the decode + E-step call) of the WAVE engine with cert_rounds = 0 and 1: x, ll and all
    eight diag entries, bit for bit"""
    out = {}
    try:
        for cr in (0, 1):
            H.set_option("cert_rounds", cr)      # read when the plan is created
            r = Run(H, ys, sms, mus, sigmas)
            try:
                assert r.plan.info()["engine"] == H.ENGINE_WAVE, r.plan.info()   # no other engine has these rounds
                r.dx.fill_(-1)
                if fused:
                    r.plan.decode_estep(r.dy, r.dx, r.dll, r.stats, r.st)
                else:
                    r.plan.viterbi(r.dy, r.dx, r.dll, r.st)
                (x, ll), d = r._out(), r.plan.diagnostics(r.st)
            finally:
                r.close()
            out[cr] = (x, ll, [v.hex() if isinstance(v, float) else int(v) for v in d])   # entries 2, 4, 6 are doubles
    finally:
        H.set_option("cert_rounds", 0)
    print("cert_rounds 0: diag %s\ncert_rounds 1: diag %s" % (out[0][2], out[1][2]))
    assert len(out[0][2]) == 8 and out[0][2] == out[1][2], (out[0][2], out[1][2])
    assert np.array_equal(out[0][0], out[1][0]), "path differs between cert_rounds 0 and 1"
    assert out[0][1].tobytes() == out[1][1].tobytes(), "ll differs between cert_rounds 0 and 1"
    return out[0]


@pytest.mark.parametrize("fused", [False, True])
def test_no_failed_certificate_rounds_return_at_once(O, H, fused):
    N, K = 4, 20
    T = 17 * 512 + 1
    temps, pp = family(H, N, K, 31)
    y = H.create_signal(T, 0.3, pp, temps, seed=901)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", 512)
    H.set_option("halo", 256)
    x, ll, diag = both_cert_rounds(H, [y], [sm], [temps], [0.3], fused)
    assert diag[0] == 0 and diag[1] == 0, diag
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    assert np.array_equal(x[0], xo) and abs(ll[0] - llo) <= 1e-9 * abs(llo)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("seed,swept", [(22, 7), (26, 9)])
def test_failed_certificates_run_every_round(O, H, seed, swept, fused):
    """the signals of test_gpu_decode_tail.py::test_failed_certificates_are_repaired_from_the_list"""
    K, N, T = 60, 4, 20_000
    temps = four_templates(H, K)
    pp = [0.03, 0.02, 0.025, 0.02]
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", 128)
    H.set_option("halo", 128)
    x, ll, diag = both_cert_rounds(H, [y], [sm], [temps], [0.3], fused)
    assert diag[0] == 0 and diag[1] == swept, diag
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    assert np.array_equal(x[0], xo) and abs(ll[0] - llo) <= 1e-9 * abs(llo)


@pytest.mark.parametrize("fused", [False, True])
def test_certificates_still_failing_in_the_final_round(H, fused):
    """The signal and the options of tests/test_gpu_host_ladder.py's short-warm-up decode (block 256, halo 64: a
    warm-up of two ring lengths), as a ring model on the wave engine, one attempt through the plan API.  The
    geometry gives 63 chains of 320 samples with a warm-up of 119; tests/wave_model.py's chain sweep, run through
    the rounds as the kernels run them (certificate at 1e-9, list = failed with a passing predecessor, exact
    re-sweep of the listed chains), counts 24 failed checks in rounds 1 and 2 and leaves runs of consecutive
    failures that two rounds do not reach: 2 certificates still fail in the final round.  Every round lists
    something, so every round must run in full with cert_rounds = 0 as well."""
    par = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(60, a, b, c) for a, b, c in par], 1))
    pp = [0.02, 0.02]
    sm = H.StateMatrix.create(2, 60, np.log(pp), False)
    y = H.create_signal(20000, 0.3, pp, temps, seed=13)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", 256)
    H.set_option("halo", 64)
    x, ll, diag = both_cert_rounds(H, [y], [sm], [temps], [0.3], fused)
    print("diag[0], diag[1] = %s, %s (CPU model: 2, 24)" % (diag[0], diag[1]))
    assert diag[0] > 0 and diag[1] > 0, diag


# ---------------------------------------------------------------- ll behind the resolver in the fused call

def test_resolver_then_ll_in_the_fused_call(O, H):
    """test_gpu_decode_tail_wide.py's first RESOLVER_CASES signal: decisions to re-decide, then ll of the final path"""
    N, K, T, fseed, seed = 4, 60, 60_000, 9, 77
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
