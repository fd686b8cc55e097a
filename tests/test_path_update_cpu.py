"""Viterbi training's update, without a GPU: the numpy model (path_update_model.py) is update() of
baumwelch.jl:205-309 fed the indicators of a path, and the C ABI declares the two entry points."""
import math
import os
import re

import numpy as np
import pytest

import path_update_model as PU
from conftest import to_oracle_sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", PU.SHAPES)
def test_model_equals_update_on_path_indicators(O, H, name):
    y, sm, temps, sigma = PU.shape(H, name)
    osm = to_oracle_sm(O, sm)
    x, _ = O.viterbi(y, osm, temps, sigma)
    T, S = len(y), sm.nstates
    # alpha = beta = 0 on the path and -1e300 off it; -Inf would make logsumexp(-Inf, -Inf) a NaN
    alpha = np.full((S, T), -1e300, order="F")
    alpha[x.astype(np.int64) - 1, np.arange(T)] = 0.0
    _, omu, osig, olp, opp = O.update(alpha, alpha.copy(order="F"), osm, temps.copy(order="F"), sigma, y)
    m = PU.path_update(y, x, sm.states, sm.transitions, temps)
    assert m["counts"] == [0, 0, 0] and m["n"] == T
    assert np.array_equal(m["mu"], omu)
    assert abs(m["sigma"] - osig) <= T * 2.0 ** -52 * osig, (m["sigma"], osig)
    assert len(m["lp"]) == len(olp)
    for a, b in zip(m["lp"], olp):
        if a == PU.NEG_INF:
            assert b < -1e299          # log of a sum of exp(-1e300) terms
        else:
            assert abs(a - b) <= 1e-11, (a, b)
    on = m["pp"] == 0.0
    assert on.sum() == 1 and on[x[0] - 1] and np.all(opp[on] == 0.0) and np.all(opp[~on] <= -1e300)
    if name == "2x12o":
        tab = PU.single_table(sm.states)
        pairs = sum(1 for s in x if s > 1 and tab[s - 1] is None)
        assert pairs > 0                                   # samples in pair states: absent from mu
        assert m["c"][1:].sum() + pairs + int((x == 1).sum()) == T
        assert len(m["lp"]) == 3 and np.isinf(m["lp"]).sum() == 1   # the joint onset never happens


def test_fsum_variant_stays_within_the_summing_bound(H):
    y, sm, temps, sigma = PU.shape(H, "3x20")
    rng = np.random.default_rng(5)
    # any path serves: this compares two ways of adding the same terms
    x = np.ones(len(y), dtype=np.int16)
    t = 3
    while t + 25 < len(y):
        a = int(rng.integers(0, 3))
        x[t:t + 19] = 2 + a * 19 + np.arange(19)
        t += 19 + 1 + int(rng.integers(0, 60))
    a = PU.path_update(y, x, sm.states, sm.transitions, temps)
    b = PU.path_update(y, x, sm.states, sm.transitions, temps, exact=True)
    bound = a["c"] * 2.0 ** -52 * np.abs(y).max() + np.spacing(np.abs(b["mu"]))
    assert np.all(np.abs(a["mu"] - b["mu"]) <= bound)
    assert a["counts"] == b["counts"] == [0, 0, 0] and np.array_equal(a["lp"], b["lp"])
    assert math.isclose(a["sigma"], b["sigma"], rel_tol=len(y) * 2.0 ** -52)


def test_both_symbols_are_declared(H):
    src = open(os.path.join(ROOT, "include", "hmmsort.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("hmmsort_plan_path_update", "hmmsort_viterbi_step"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in H._lib.SIGNATURES
    assert len(H._lib.SIGNATURES["hmmsort_plan_path_update"][1]) == 6
    assert len(H._lib.SIGNATURES["hmmsort_viterbi_step"][1]) == 17


def test_random_start_refuses_viterbi_training(H):
    with pytest.raises(ValueError, match="refine"):
        H.train_model(np.zeros(100), 3, 20, False, 4, method="viterbi")
    with pytest.raises(ValueError, match="method"):
        H.train_model(np.zeros(100), 3, 20, False, 4, method="hard")
