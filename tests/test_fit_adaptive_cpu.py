"""The drift-tracking chunk loop on the CPU (tests/fit_adaptive_model.py over the oracle): the owned-range rule on a
hand-made path, the two-step blend, and the recall figures the GPU test asserts for hmmsort_fit_adaptive against
hmmsort_fit_chunked on the drifting recording D(seed, 0.4).  No GPU: the state space helpers of the library run on the
host."""
import numpy as np
import pytest

import fit_adaptive_model as FA
from conftest import to_oracle_sm


def test_owned_range_rule_on_a_hand_made_path():
    """T = 40, chunks of 16.  Chunk 0 = [1, 16] ends in a spike: its last silent sample is its 12th, so it writes
    samples 1..12 and owns [0, 11): sample 12 (0-based 11) is the next chunk's first.  Chunk 1 = [12, 27] starts inside
    nothing (l = 1) but chunk 2 = [22, 37] is made to start with two busy samples: l = 3, they belong to nobody."""
    T, cs = 40, 16
    paths = {0: np.array([1] * 12 + [2, 3, 4, 5], dtype=np.int16)}                          # i = 1:  l = 1, kk = 12
    paths[1] = np.array([1, 2, 3, 4, 5, 1, 1, 1, 1, 1, 1, 2, 3, 4, 5, 6], dtype=np.int16)   # i = 12: l = 1, kk = 11
    paths[2] = np.array([7, 8, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4, 5], dtype=np.int16)   # i = 22: l = 3, kk = 12
    paths[3] = np.array([1, 1, 2, 3, 4, 5, 1, 1], dtype=np.int16)                           # i = 33: the last, 8 samples
    got = []
    for c, i, j, x, ll, l, kk, last in FA.walk(lambda i, j, c: (paths[c][:j - i + 1], 0.0), T, cs):
        got.append((i, j, l, kk, last, FA.owned(i, l, kk, last, T)))
    assert got == [(1, 16, 1, 12, False, (0, 11)),
                   (12, 27, 1, 11, False, (11, 21)),
                   (22, 37, 3, 12, False, (23, 32)),      # samples 21, 22 (0-based) belong to nobody
                   (33, 40, 1, 8, True, (32, 40))]
    owned = np.zeros(T, dtype=int)
    for g in got:
        owned[g[5][0]:g[5][1]] += 1
    assert owned.max() == 1 and np.flatnonzero(owned == 0).tolist() == [21, 22]


def test_trim_edges():
    assert FA.trim(np.array([2, 3, 4]), True, True) == (4, 0)      # no silent sample: fit.jl:26 runs off the chunk
    assert FA.trim(np.array([2, 3, 4]), False, False) == (1, 3)
    assert FA.trim(np.array([1, 3, 4]), True, True) == (1, 1)      # would not advance (fit.jl:41)


def test_blend_is_two_rounded_steps():
    rng = np.random.default_rng(5)
    acc, new = rng.standard_normal(1000) * 1e3, rng.standard_normal(1000)
    out = FA.blend(acc, 0.3, new, 3)
    assert np.array_equal(out[:-3], np.float64(0.3) * acc[:-3] + new[:-3]) and np.array_equal(out[-3:], acc[-3:] + new[-3:])
    # a fused multiply-add would differ somewhere on 997 random entries
    import math
    fused = np.array([math.fma(0.3, a, b) for a, b in zip(acc[:-3], new[:-3])]) if hasattr(math, "fma") else None
    assert fused is None or np.any(fused != out[:-3])
    assert abs(FA.weight(4000, 8000) - 2.0 ** -0.5) <= 4 * np.spacing(2.0 ** -0.5) and FA.weight(10, np.inf) == 1.0


def ring_model(H, temps):
    return H.StateMatrix.create(temps.shape[1], temps.shape[0], np.log(FA.PP_D), False)


@pytest.fixture(scope="module")
def runs(O, H):
    """seed -> (onsets, sm, fixed loop, adaptive loop) on D(seed, 0.4), computed once"""
    out = {}
    for seed in (1, 2, 3):
        y, onsets, temps = FA.drifting(H, seed, 0.4)
        sm = ring_model(H, temps)
        fixed = FA.fit_adaptive(O, to_oracle_sm, H, y, sm, temps, FA.SIGMA_D, 4000, np.inf, warmup=len(y) + 1)
        adapt = FA.fit_adaptive(O, to_oracle_sm, H, y, sm, temps, FA.SIGMA_D, 4000, 8000.0)
        out[seed] = (y, onsets, sm, temps, fixed, adapt)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_recall_on_the_drifting_recording(O, H, runs, seed):
    y, onsets, sm, temps, fixed, adapt = runs[seed]
    T = len(y)
    # the fixed-model loop of the model is the oracle's fit_chunked
    rc, oml, oll = O.fit_chunked(y, to_oracle_sm(O, sm), temps, FA.SIGMA_D, 4000)
    assert rc == 0 and np.array_equal(fixed["ml"], oml) and fixed["ll"] == oll
    f, n, fx = FA.recall(fixed["ml"], onsets, sm, 32_000, T - 16)
    a, n2, ax = FA.recall(adapt["ml"], onsets, sm, 32_000, T - 16)
    print("seed %d: fixed %d/%d (+%d), adaptive %d/%d (+%d)" % (seed, f, n, fx, a, n2, ax))
    assert n == n2 and n > 150
    assert f <= 0.55 * n
    assert a >= 0.95 * n and ax <= 3
    # the track moves towards the shrunken spikes: the trough of template 0 ends well above where it started
    assert adapt["mu"][-1][:, 0].min() > 0.7 * temps[:, 0].min()


def test_stationary_recording_decodes_alike(O, H):
    y, onsets, temps = FA.drifting(H, 1, 1.0)
    sm = ring_model(H, temps)
    rc, oml, oll = O.fit_chunked(y, to_oracle_sm(O, sm), temps, FA.SIGMA_D, 4000)
    adapt = FA.fit_adaptive(O, to_oracle_sm, H, y, sm, temps, FA.SIGMA_D, 4000, 8000.0)
    differ = int(np.sum(adapt["ml"] != oml))
    print("stationary: %d of %d samples differ" % (differ, len(y)))
    assert rc == 0 and differ <= len(y) // 1000
    # a chunk's decode starts without context and usually opens with a few busy samples, which nobody owns
    own = np.array(adapt["own"])
    assert own[0, 0] == 0 and own[-1, 1] == len(y) and np.all(own[1:, 0] >= own[:-1, 1])
    assert np.any(own[1:, 0] > own[:-1, 1])


def test_tiling_fixture_of_the_gpu_test(O, H):
    """D(2, 1.0) cut to 12 000 samples in chunks of 4 400: three chunks whose owned ranges tile [0, T), so the
    undecayed statistics are those of the whole path (what the GPU test compares with hmmsort_fit_step_channels)"""
    y, onsets, temps = FA.drifting(H, 2, 1.0, T=12_000)
    r = FA.fit_adaptive(O, to_oracle_sm, H, y, ring_model(H, temps), temps, FA.SIGMA_D, 4400, np.inf, warmup=len(y))
    assert r["own"] == [(0, r["own"][0][1]), (r["own"][0][1], r["own"][1][1]), (r["own"][1][1], 12_000)]
    assert r["w"] == [1.0, 1.0, 1.0] and all(np.array_equal(m, temps) for m in r["mu"])
