"""The tail of the fused decode + E-step call: for one channel of up to four rings the path likelihood runs on
the E-step's stream beside the near-tie resolver and is computed again, behind the resolver, if the resolver rewrote
the path (kw_ll_partial, wave_viterbi_post); batched plans and the decode on its own keep the serial order, and are
compared with it here; kw_fb_check leaves the largest error alone when it cannot rise.

Nothing a call returns may change by a bit.  ll is pinned to bytes recorded once on an MI355X from the parent build:
tests/golden/decode_tail_wide/ll_parent.json for decodes the resolver leaves alone, tests/golden/fused_tail/
ll_parent.json for decodes in which it rewrites the path (with the resolver on, tie_debug = 0, and off,
tie_debug = 2: the two paths differ, and so do the two values of ll), and the same file for diag[3..6] of the
E-step cases.  Every case runs with plain launches (plan.profile(True)) and as a captured graph (HMMSORT_GRAPHS=1
on a stream that is not the null stream), the two launch paths of wave_graphed.

Helpers and signal families are those of test_gpu_decode_tail_wide.py.

The certificate case with a warm-up that is too short (options block = 128, halo = 64, for which the engine makes
chains of 320 samples with warm-ups of two super-steps = 118 samples, the shortest it makes for rings of 59 states)
was chosen with tests/wave_model.py on the CPU (fwd_chain of both chains of a boundary, weights from bwd_chain,
kw_fb_check's formula, chains of 320 samples and 119 of warm-up).  On the busy signal of
test_gpu_boundary_certificates.py (noise 0.3, model sigma 0.35) such a warm-up does NOT fail: the forward errors at
boundaries 1..8 are below 1e-19.  With noise 2.0 and model sigma 2.0 the samples say little, the rings remember, and
the model gives 9.9e-11, 4.0e-13, 8.2e-9, 1.6e-12, 5.4e-15, 9.0e-15, 2.0e-11, 1.7e-14 there: boundary 3 fails the
tolerance of 1e-9 in the forward direction alone (on the GPU 31 of the 62 forward and 32 of the backward
certificates fail).  tests/test_fused_tail_model.py repeats that computation for boundary 3.
"""
import json
import os

import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm
from test_gpu_decode_tail_wide import Run, family, ll_cases, ll_signal

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fused_tail", "ll_parent.json")
TIE_SCALE = 30_000_000
MODES = ("graph", "plain")


@pytest.fixture(autouse=True)
def options(H):
    yield
    for k, v in (("engine", H.ENGINE_AUTO), ("block", 0), ("halo", 0), ("tie_scale", 1), ("tie_debug", 0),
                 ("backtrace", 0)):
        H.set_option(k, v)


def golden():
    return json.load(open(GOLDEN))


def hexbytes(v):
    return np.float64(v).tobytes().hex()


class TailRun(Run):
    """Run on a stream of its own: mode "graph" replays each call as a captured graph (the plan reads HMMSORT_GRAPHS
    when it is created), mode "plain" brackets every launch with profiling events, which means plain launches"""

    def __init__(self, H, ys, sms, mus, sigmas, mode):
        import torch
        old = os.environ.get("HMMSORT_GRAPHS")
        os.environ["HMMSORT_GRAPHS"] = "1" if mode == "graph" else "0"
        try:
            super().__init__(H, ys, sms, mus, sigmas)
        finally:
            if old is None:
                del os.environ["HMMSORT_GRAPHS"]
            else:
                os.environ["HMMSORT_GRAPHS"] = old
        self.stream = torch.cuda.Stream()
        self.st = self.stream.cuda_stream
        if mode == "plain":
            self.plan.profile(True)
        torch.cuda.synchronize()      # the uploads were made on another stream

    def viterbi(self):
        with self.torch.cuda.stream(self.stream):
            return super().viterbi()

    def estep(self):
        with self.torch.cuda.stream(self.stream):
            return super().estep()

    def decode_estep(self):
        with self.torch.cuda.stream(self.stream):
            return super().decode_estep()

    def close(self):
        self.stream.synchronize()
        super().close()


def resolver_signal(H, case):
    """a recorded resolver case -> y, sm, temps.  kind "family": the signals of test_gpu_decode_tail_wide.py's
    RESOLVER_CASES (family seed, signal seed).  kind "twins": two copies of one template, as in test_gpu_ties.py,
    spikes from the first only, so that every spike is a tie the rounding of the reference's sums settles and the
    resolver does change back-pointers; the twins' rates differ by pp_ratio - 1 = 1e-12, below that rounding,
    so that the two paths have different likelihoods."""
    N, K, T = case["N"], case["K"], case["T"]
    if case["kind"] == "twins":
        t1 = H.create_spike_template(K, 3.0, 0.8, 0.2)
        temps = np.asfortranarray(np.stack([t1, t1.copy()], 1))
        pp = np.array([0.002, 0.002 * case["pp_ratio"]])
        y = H.create_signal(T, 0.3, [0.003, 0.0], temps, seed=case["seed"])
    else:
        temps, pp = family(H, N, K, case["fseed"])
        y = H.create_signal(T, 0.3, pp, temps, seed=case["seed"])
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    return y, sm, temps


def busy_signal(H, noise, sigma, T=20_000):
    """the busy signal of test_gpu_boundary_certificates.py, half as long, with a model off the signal's"""
    K, N = 60, 4
    temps = four_templates(H, K)
    pp = [0.03, 0.02, 0.025, 0.02]
    y = H.create_signal(T, noise, pp, temps, seed=21)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    return y, sm, mu, sigma


# block, halo, noise of the signal, sigma of the model: chains of 320 samples (62 boundaries) behind the default
# warm-up of 295 samples, and behind one of 118 that is too short for a signal this noisy (module docstring)
CERT_CASES = {"clean": (128, 0, 0.3, 0.35), "short_halo": (128, 64, 2.0, 2.0)}


# ---------------------------------------------------------------- 1. ll to the bit, resolver idle

def wave_takes(T, K):
    return T >= max(512, 4 * (K - 1))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [c["T"] for c in ll_cases() if wave_takes(c["T"], 20)])
def test_ll_unflagged_is_the_recorded_value(H, T, mode):
    """a ragged pass and several passes of kw_ll_partial's grid, decode alone and fused call"""
    case = [c for c in ll_cases() if c["T"] == T][0]
    y, sm, temps = ll_signal(H, T, case["seed"])
    H.set_option("engine", H.ENGINE_WAVE)
    r = TailRun(H, [y], [sm], [temps], [0.3], mode)
    try:
        x, ll, dv, ties = r.viterbi()
        xf, llf = r.decode_estep()[:2]
    finally:
        r.close()
    print("T=%d %s: decode %s fused %s recorded %s ties %s" % (T, mode, hexbytes(ll[0]), hexbytes(llf[0]),
                                                              case["ll_bytes"], ties))
    assert ties["flips"] == 0, ties
    assert hexbytes(ll[0]) == case["ll_bytes"]
    assert hexbytes(llf[0]) == case["ll_bytes"]
    assert np.array_equal(xf, x)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("T", [c["T"] for c in ll_cases() if not wave_takes(c["T"], 20)])
def test_ll_below_the_wave_engine_is_the_recorded_value(H, T, mode):
    """T = 257, fewer samples than one pass of the grid, is also fewer than the wave engine takes: the library
    gives the plan another engine, which has no fused call, so this covers the library's engine choice and the
    decode alone only"""
    case = [c for c in ll_cases() if c["T"] == T][0]
    y, sm, temps = ll_signal(H, T, case["seed"])
    H.set_option("engine", H.ENGINE_AUTO)
    r = TailRun(H, [y], [sm], [temps], [0.3], mode)
    try:
        assert r.plan.info()["engine"] != H.ENGINE_WAVE
        x, ll, dv, ties = r.viterbi()
    finally:
        r.close()
    assert hexbytes(ll[0]) == case["ll_bytes"]


# ---------------------------------------------------------------- 2. ll when the resolver rewrites x

def resolver_cases():
    return golden()["resolver_cases"]


_ORACLE = {}      # the oracle's path and ll of a resolver case, computed once for both launch modes


def test_a_recorded_case_exercises_the_second_launch():
    """flips > 0, the path differs between resolver on and off, and so do the recorded bytes of ll"""
    q = [c for c in resolver_cases()
         if c["flips"] > 0 and c["x_differs_at"] > 0 and c["ll_bytes"] != c["ll_bytes_resolver_off"]]
    assert q, resolver_cases()


@pytest.mark.parametrize("mode", MODES)
# 0, 1: test_gpu_decode_tail_wide.py's RESOLVER_CASES, which flag decisions but flip none (nor did any of 40 other
# signal seeds at either shape: the sweep's decisions are the reference's unless rounding settles them); 2: twins at
# the second shape, where the resolver rewrites the path
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_ll_with_the_resolver_rewriting_the_path(O, H, idx, mode):
    case = resolver_cases()[idx]
    y, sm, temps = resolver_signal(H, case)
    if idx not in _ORACLE:
        _ORACLE[idx] = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    xo, llo = _ORACLE[idx]
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("tie_scale", TIE_SCALE)
    res = {}
    for dbg in (0, 2):
        H.set_option("tie_debug", dbg)          # read when the plan is created
        r = TailRun(H, [y], [sm], [temps], [0.3], mode)
        try:
            x, ll, dv, ties = r.viterbi()
            st, de = r.estep()
            xf, llf, stf, df, tf = r.decode_estep()
        finally:
            r.close()
        print("case %d %s tie_debug=%d: ll %s fused %s %s" % (idx, mode, dbg, hexbytes(ll[0]), hexbytes(llf[0]), tf))
        assert np.array_equal(xf, x) and hexbytes(llf[0]) == hexbytes(ll[0]), "fused path / ll differ"
        assert np.array_equal(stf, st), "fused statistics differ"
        assert list(df) == list(dv[:3]) + list(de[3:7]) + list(dv[7:8]), (df, dv, de)
        assert tf == ties, (tf, ties)
        res[dbg] = (x, ll, ties)
    x, ll, ties = res[0]
    assert ties["flagged"] > 0 and ties["unresolved"] == 0, ties
    assert ties["flips"] == case["flips"] and ties["flagged"] == case["flagged"], (ties, case)
    assert np.array_equal(x[0], xo), int(np.count_nonzero(x[0] != xo))
    assert abs(ll[0] - llo) <= 1e-9 * abs(llo)
    assert hexbytes(ll[0]) == case["ll_bytes"]
    assert hexbytes(res[2][1][0]) == case["ll_bytes_resolver_off"]
    assert int(np.count_nonzero(res[2][0] != x)) == case["x_differs_at"]


# ---------------------------------------------------------------- 3. one channel with flips beside one without

@pytest.mark.parametrize("mode", MODES)
def test_two_channels_one_with_flips_one_without(H, mode):
    b = golden()["batch"]
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("tie_scale", TIE_SCALE)
    sig = [resolver_signal(H, c) for c in b["channels"]]
    assert not np.array_equal(sig[0][2], sig[1][2]) or not np.array_equal(sig[0][1].transitions["lp"],
                                                                          sig[1][1].transitions["lp"])
    single = []
    for y, sm, temps in sig:
        r = TailRun(H, [y], [sm], [temps], [0.3], mode)
        try:
            single.append(r.viterbi())
        finally:
            r.close()
    flips = [s[3]["flips"] for s in single]
    print("flips per channel:", flips)
    assert flips[0] > 0 and flips[1] == 0, flips
    for order in ((0, 1), (1, 0)):
        r = TailRun(H, [sig[i][0] for i in order], [sig[i][1] for i in order], [sig[i][2] for i in order],
                    [0.3, 0.3], mode)
        try:
            x, ll, dv, ties = r.viterbi()
            xf, llf, stf, df, tf = r.decode_estep()
        finally:
            r.close()
        assert ties["flips"] == flips[0] and tf == ties, (ties, tf)
        for pos, i in enumerate(order):
            assert np.array_equal(x[pos], single[i][0][0]) and np.array_equal(xf[pos], single[i][0][0])
            assert hexbytes(ll[pos]) == hexbytes(single[i][1][0]) == b["channels"][i]["ll_bytes"]
            assert hexbytes(llf[pos]) == hexbytes(single[i][1][0])


# ---------------------------------------------------------------- 4. certificates of the forward/backward sweeps

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CERT_CASES))
def test_fb_certificates_are_the_recorded_ones(H, name, mode):
    block, halo, noise, sigma = CERT_CASES[name]
    rec = golden()["certificates"][name]
    y, sm, mu, sigma = busy_signal(H, noise, sigma)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", block)
    H.set_option("halo", halo)
    r = TailRun(H, [y], [sm], [mu], [sigma], mode)
    try:
        info = r.plan.info()
        st, de = r.estep()
        xf, llf, stf, df, tf = r.decode_estep()
        st2, de2 = r.estep()
    finally:
        r.close()
    print("%s %s: %s estep %s fused %s" % (name, mode, info, de[3:7], df[3:7]))
    assert info["nchains"] - 1 >= 32, info
    got = [int(de[3]), hexbytes(de[4]), int(de[5]), hexbytes(de[6])]
    assert got == [int(df[3]), hexbytes(df[4]), int(df[5]), hexbytes(df[6])], (de, df)
    assert got == [int(de2[3]), hexbytes(de2[4]), int(de2[5]), hexbytes(de2[6])], (de, de2)
    assert got == rec["diag_3_6"], (got, rec)
    assert np.array_equal(st, stf) and np.array_equal(st, st2)
    if name == "short_halo":
        assert de[3] + de[5] > 0 and max(de[4], de[6]) > 1e-9, de      # the failing branch and the maximum
    else:
        assert de[3] + de[5] == 0 and 0.0 <= max(de[4], de[6]) <= 1e-9, de


# ---------------------------------------------------------------- 5. call after call on the same plan and buffers

@pytest.mark.parametrize("mode", MODES)
def test_calls_repeat_on_the_same_plan_and_buffers(H, mode):
    case = [c for c in resolver_cases() if c["flips"] > 0][0]
    y, sm, temps = resolver_signal(H, case)
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("tie_scale", TIE_SCALE)
    r = TailRun(H, [y], [sm], [temps], [0.3], mode)
    try:
        first = r.viterbi()
        second = r.viterbi()
        fused = r.decode_estep()
        third = r.viterbi()
        fused2 = r.decode_estep()
    finally:
        r.close()
    assert hexbytes(first[1][0]) == case["ll_bytes"]
    for other in (second, third):
        assert np.array_equal(other[0], first[0]) and hexbytes(other[1][0]) == hexbytes(first[1][0])
        assert list(other[2]) == list(first[2]) and other[3] == first[3], (other[2:], first[2:])
    for f in (fused, fused2):
        assert np.array_equal(f[0], first[0]) and hexbytes(f[1][0]) == hexbytes(first[1][0])
        assert f[4] == first[3], (f[4], first[3])
    assert np.array_equal(fused[2], fused2[2]) and list(fused[3]) == list(fused2[3])
