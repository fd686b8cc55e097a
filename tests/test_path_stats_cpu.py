"""Viterbi training from additive path statistics, without a GPU: the numpy model of the statistics vector and of its
finish (path_stats_model.py) reproduces the two-pass model (path_update_model.py), the integer slots of a partition
add up exactly to the whole, and the C ABI declares the calls."""
import os
import re

import numpy as np
import pytest

import path_stats_model as PS
import path_update_model as PU
from conftest import to_oracle_sm
from test_gpu_path_update import K_HAND, N_HAND, T_HAND, hand_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTS = (4099, 8209)   # both primes: the first inside a spike of the hand path, the second on the second silent
                      # sample after one (the spike ends at 8207)


def onset_cut(x, lo, hi):
    """the first t in (lo, hi) with x[t-1] silent and x[t] an onset (phase 1 of a ring of K_HAND - 1)"""
    for t in range(lo + 1, hi):
        if x[t - 1] == 1 and x[t] > 1 and (x[t] - 2) % (K_HAND - 1) == 0:
            return t
    raise AssertionError("no onset between the cuts")


def hand_case(H):
    temps = PU.templates(H, N_HAND, K_HAND)
    sm = H.StateMatrix.create(N_HAND, K_HAND, np.log([0.01, 0.01, 0.01]), False)
    y = np.random.default_rng(7).standard_normal(T_HAND) * 2.0
    x, sid = hand_path()
    return y, x, sm, temps, sid


def same(f, m, T):
    assert np.array_equal(f["mu"], m["mu"])
    assert np.array_equal(f["lp"], m["lp"]) and np.array_equal(f["pp"], m["pp"])
    assert f["counts"] == m["counts"] and f["n"] == m["n"] and np.array_equal(f["c"], m["c"])
    assert abs(f["sigma"] - m["sigma"]) <= PS.sigma_bound(f, T) * m["sigma"], (f["sigma"], m["sigma"])


@pytest.mark.parametrize("name", PU.SHAPES)
def test_finish_of_the_whole_reproduces_the_two_pass_model(O, H, name):
    y, sm, temps, sigma = PU.shape(H, name)
    x, _ = O.viterbi(y, to_oracle_sm(O, sm), temps, sigma)
    mu0 = np.asfortranarray(temps * 0.9)
    by_template = name != "2x12o"
    st = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, by_template)
    if name == "2x12o":
        assert st["nj"].sum() > 0 and np.abs(st["sm"]).sum() > 0
    else:
        assert st["nj"].sum() == 0 and not st["sm"].any()
    f = PS.finish(st, sm.states, mu0)
    same(f, PU.path_update(y, x, sm.states, sm.transitions, mu0, by_template=by_template, exact=True), len(y))
    v = PS.vector(st)
    assert len(v) == 3 * sm.N * (sm.K - 1) + sm.nstates + len(f["lp"]) + 6
    back = PS.split_vector(v, sm.N, sm.K, sm.nstates)
    assert all(np.array_equal(np.asarray(back[k]), np.asarray(st[k], dtype=np.float64)) for k in PS.ORDER)


@pytest.mark.parametrize("by_template", [True, False])
def test_hand_path_whole_and_partition(H, by_template):
    y, x, sm, temps, sid = hand_case(H)
    whole = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, by_template)
    f = PS.finish(whole, sm.states, temps)
    m = PU.path_update(y, x, sm.states, sm.transitions, temps, by_template=by_template, exact=True)
    assert m["counts"] == [0, 0, K_HAND - 1]
    same(f, m, T_HAND)
    assert x[CUTS[0] - 1] > 1 and x[CUTS[0]] > 1 and x[CUTS[1] - 2] > 1 and x[CUTS[1]] == 1
    c3 = onset_cut(x, CUTS[0], CUTS[1])
    assert x[c3 - 1] == 1 and x[c3] > 1
    edges = [0, CUTS[0], c3, CUTS[1], T_HAND]
    parts = [PS.path_stats(y, x, sm.states, sm.transitions, sm.K, by_template, lo, hi, first=lo == 0)
             for lo, hi in zip(edges[:-1], edges[1:])]
    tot = PS.add(parts)
    for k in PS.INT_SLOTS:
        assert np.array_equal(np.asarray(tot[k]), np.asarray(whole[k])), k
    # the shard that ends on the silent sample owns the pair into the onset
    onset_slot = PS.slots(sm.states, sm.transitions, by_template)[1][int(x[c3])]
    alone = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, by_template, c3 - 1, c3, first=False)
    assert alone["b"] == 1 and alone["ent"][onset_slot] == 1 and alone["ent"].sum() == 1
    assert [p["x0"] for p in parts] == [int(x[0]), 0, 0, 0]
    # slices with halos see the same owned samples: T is then the slice's length
    lo, hi = CUTS[0], c3
    a, b = lo - 64, hi + 64
    sl = PS.path_stats(y[a:b], x[a:b], sm.states, sm.transitions, sm.K, by_template, lo - a, hi - a, first=False)
    for k in PS.INT_SLOTS:
        assert np.array_equal(np.asarray(sl[k]), np.asarray(parts[1][k])), k
    # the float slots of the parts are rounded sums: mu' of their sum is within the summing bound, the rest equal
    ft = PS.finish(tot, sm.states, temps)
    bound = m["c"] * 2.0 ** -52 * np.abs(y).max() + np.spacing(np.abs(m["mu"]))
    assert np.all(np.abs(ft["mu"] - m["mu"]) <= bound)
    assert np.array_equal(ft["lp"], m["lp"]) and np.array_equal(ft["pp"], m["pp"]) and ft["counts"] == m["counts"]
    assert abs(ft["sigma"] - m["sigma"]) <= PS.sigma_bound(ft, T_HAND) * m["sigma"]
    empty = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, by_template, 500, 500)
    assert not PS.vector(empty).any()


def test_bad_ids_and_pairs_land_in_the_shard_that_owns_them(H):
    y, x, sm, temps, sid = hand_case(H)
    bad = x.copy()
    bad[9100], bad[9200], bad[9300], bad[9400] = 0, sm.nstates + 1, sm.nstates + 1, sid(0, 5)
    edges = [0, 9150, 9399, T_HAND]
    parts = [PS.path_stats(y, bad, sm.states, sm.transitions, sm.K, True, lo, hi, first=lo == 0)
             for lo, hi in zip(edges[:-1], edges[1:])]
    assert [p["bad0"] for p in parts] == [1, 2, 0]
    assert parts[0]["bad1"] == 0 and parts[1]["bad1"] == 0 and parts[2]["bad1"] >= 1   # 1 -> (0,5) at 9399 -> 9400
    whole = PS.path_stats(y, bad, sm.states, sm.transitions, sm.K, True)
    assert PS.add(parts)["bad1"] == whole["bad1"] and whole["bad0"] == 3 and whole["n"] == T_HAND - 3


def test_pooled_model_is_the_finish_of_the_sum(H):
    y, x, sm, temps, _ = hand_case(H)
    y2 = np.random.default_rng(8).standard_normal(T_HAND)
    f, st = PS.pooled([(y, x), (y2, x)], sm.states, sm.transitions, temps, True)
    one = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, True)
    assert np.array_equal(st["c"], 2 * one["c"]) and st["n"] == 2 * T_HAND and st["b"] == 2 * one["b"]
    seen = one["c"] > 0
    mean = ((one["s"] + PS.path_stats(y2, x, sm.states, sm.transitions, sm.K, True)["s"])[seen] / st["c"][seen])
    got = f["mu"][1:].ravel(order="F")[seen]
    assert np.all(np.abs(got - mean) <= 2 * np.spacing(np.abs(mean)))
    assert np.array_equal(f["lp"], PS.finish(one, sm.states, temps)["lp"])          # same path twice: same ratios


def test_the_symbols_are_declared(H):
    src = open(os.path.join(ROOT, "include", "hmmsort.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    nargs = dict(hmmsort_plan_path_stats_len=1, hmmsort_plan_path_stats=9, hmmsort_plan_path_finish=5,
                 hmmsort_stats_sum=5, hmmsort_fit_step_channels=13)
    for name, n in nargs.items():
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in H._lib.SIGNATURES and len(H._lib.SIGNATURES[name][1]) == n, name
    assert "hmmsort_step_out" in src and len(H._lib.StepOut._fields_) == 7
    for name in ("fit_step_channels", "stats_sum"):
        assert hasattr(H, name)
    for name in ("path_stats_len", "path_stats", "path_finish"):
        assert hasattr(H.Plan, name)
