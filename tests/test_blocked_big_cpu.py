"""Option "blocked_hbm_columns" (the blocked E-step and posteriors with their state columns in device memory,
csrc/generic_estep_big.hip) and the fixtures of tests/test_gpu_blocked_big.py, without a GPU: the option table of
the library needs no device, and the fixtures' inputs are pure numpy plus the oracle's state space."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

KEY = "blocked_hbm_columns"


def test_option_round_trips_and_defaults_to_off(H):
    assert H._lib.OPT_BLOCKED_HBM_COLUMNS == KEY
    assert (H._lib.HBM_COLUMNS_OFF, H._lib.HBM_COLUMNS_AUTO, H._lib.HBM_COLUMNS_FORCE) == (0, 1, 2)
    assert H.get_option(KEY) == 0
    try:
        for v in (1, 2, 0):
            H.set_option(KEY, v)
            assert H.get_option(KEY) == v
        H.set_option(KEY, 1)
        for bad in (-1, 3, 1 << 40):
            with pytest.raises(H.HmmsortError) as e:
                H.set_option(KEY, bad)
            assert e.value.code == H._lib.EINVAL and KEY in str(e.value)
            assert H.get_option(KEY) == 1                   # a refused value changes nothing
    finally:
        H.set_option(KEY, 0)
    # the other options are where they were
    assert H.get_option("engine") == H.ENGINE_AUTO and H.get_option("halo") == 0


@pytest.mark.parametrize("name", ["M3", "M4"])
def test_fixture_hashes_match_the_regenerated_inputs(O, name):
    import make_big_overlap_at_size as G
    import make_estep_at_size as G0
    path = os.path.join(G.OUT, name + ".npz")
    assert os.path.exists(path), "fixture %s is missing" % path
    assert os.path.getsize(path) <= G.MAX_BYTES
    ref = G.load(name)
    y, osm, mu, sigma, pp, win = G.inputs(name)
    N, K, T = G.CASES[name][:3]
    assert osm.nstates == {3: 10_621, 4: 21_123}[N] and len(y) == T == int(ref["T"])
    assert len(pp) == N and len(set(pp)) == N                # every template its own rate
    h = G0.hashes(y, osm, mu, sigma)
    assert str(ref["sha_y"]) == h["sha_y"] and str(ref["sha_model"]) == h["sha_model"]
    assert np.array_equal(ref["windows"], win)
    # what the GPU test reads is there, of the right shape, and self-consistent
    S = osm.nstates
    assert ref["sg"].shape == (S,) and abs(ref["sg"].sum() - T) <= 1e-6 * T
    assert ref["mu_new"].shape == (K, N) and ref["lp_new"].shape == (int((osm.src == 1).sum()) - 1,)
    assert float(ref["close_share"]) <= 1e-3
    for i, (lo, hi) in enumerate(win):
        assert ref["w%d_onset" % i].shape == (N, hi - lo) and ref["w%d_trough" % i].shape == (N, hi - lo)
        assert ref["w%d_xm" % i].shape == (hi - lo,) and ref["w%d_gap" % i].shape == (hi - lo,)
    # the middle window holds a boundary of the default geometry
    import make_blocked_post_at_size as P
    blk = P.block_length(T, K)
    assert (win[1][1] - 1) // blk > win[1][0] // blk
