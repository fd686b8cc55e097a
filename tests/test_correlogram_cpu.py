"""The numpy model of the correlograms (tests/correlogram_model.py) against itself and the definitions, and
api.duplicate_units on hand-made arrays.  No GPU."""
import numpy as np
import pytest

import correlogram_model as CM


@pytest.mark.parametrize("b", [1, 3, 30])
def test_the_two_model_forms_agree(b):
    rng = np.random.default_rng(100 + b)
    for trial in range(4):
        U, H = int(rng.integers(1, 7)), int(rng.integers(1, 9))
        lists = CM.random_lists(rng, U, 200, int(rng.integers(200, 4000)))
        r, c = int(rng.integers(0, 40)), int(rng.integers(0, 6))
        for got, want in zip(CM.fast(lists, b, H, r, c), CM.brute(lists, b, H, r, c)):
            assert got.dtype == want.dtype == np.int64 and np.array_equal(got, want), (trial, U, H, r, c)


def test_mirror_symmetry_at_unit_bin_width():
    rng = np.random.default_rng(7)
    H = 12
    lists = CM.random_lists(rng, 4, 150, 900)
    ccg = CM.fast(lists, 1, H, 0, 0)[0]
    for u in range(4):
        for v in range(4):
            for k in range(1, 2 * H):
                assert ccg[u, v, k] == ccg[v, u, 2 * H - k]


@pytest.mark.parametrize("b,H", [(1, 7), (3, 5), (30, 2)])
def test_bins_sum_to_the_pairs_in_the_window(b, H):
    rng = np.random.default_rng(b * 10 + H)
    lists = CM.random_lists(rng, 3, 200, 1500)
    ccg = CM.fast(lists, b, H, 0, 0)[0]
    for u in range(3):
        for v in range(3):
            assert ccg[u, v].sum() == CM.pairs_in_window(lists, u, v, H * b)


def test_duplicate_units(H):
    n = np.array([10, 8, 0, 4], dtype=np.int64)
    coinc = np.array([[9, 5, 0, 4],      # the diagonal is never a duplicate
                      [5, 8, 0, 3],
                      [0, 0, 0, 0],      # no spikes: in no pair, no division by zero
                      [4, 2, 0, 0]], dtype=np.int64)
    cg = H.Correlograms(np.zeros((4, 4, 2), dtype=np.int64), np.array([-1, 0]), np.zeros(4, dtype=np.int64), coinc, n)
    assert H.duplicate_units(cg) == [(0, 1, 0.5), (1, 0, 0.625), (3, 0, 1.0), (3, 1, 0.5)]
    assert H.duplicate_units(cg, min_fraction=0.6) == [(1, 0, 0.625), (3, 0, 1.0)]
    assert H.duplicate_units(cg, min_fraction=1.0) == [(3, 0, 1.0)]
    got = H.duplicate_units(cg, min_fraction=0.0)
    assert len(got) == 9 and all(u != v and u != 2 for u, v, _ in got)   # every ordered pair of a unit with spikes
    assert [p[:2] for p in got] == sorted(p[:2] for p in got)
