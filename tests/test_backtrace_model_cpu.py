"""The event walk of the light backtrace against the per-sample walk, on the CPU model (tests/backtrace_model.py).

The two must give the same x, bstate and flag count for ANY back-pointer table: a wrong jump is a wrong path, and
the device tests only see the tables real data produce.  So most tables here are random.
"""
import numpy as np
import pytest

import backtrace_model as M

NS = [1, 4, 7, 8, 16]            # one, one, one, two and four words per sample (PW)
LS = [8, 59, 127, 255]


def _same(psi, T, N, L, fs=0, geom=None):
    Bb, Hb = geom or M.seg_geometry(L)
    a = M.walk_samples(psi, T, N, L, Bb, Hb, fs)
    b = M.walk_events(psi, T, N, L, Bb, Hb, fs)
    bad = np.flatnonzero(a[0] != b[0])
    assert bad.size == 0, "x differs at %d samples, first at %d (N=%d L=%d T=%d fs=%d)" % (bad.size, bad[0], N, L, T, fs)
    assert np.array_equal(a[1], b[1]), ("bstate", a[1], b[1])
    assert a[2] == b[2], ("nflag", a[2], b[2])
    assert (a[0] >= 1).all(), "every sample below T is stored"
    return a


def _length(L, k):
    """T of 2 to 4 segments that is no multiple of 4, of the tile or of Bb; k picks one"""
    Bb, Hb = M.seg_geometry(L)
    return [2 * Bb + Hb + 37, 3 * Bb + 1, 2 * Bb + 63, 3 * Bb - 2, 2 * Bb + Hb - 1][k % 5]


def _random_table(rng, N, T, p_onset=None, p_flag=0.3, lo=0):
    pred = rng.integers(lo, N + 1, size=(N + 1, T))
    if p_onset is not None:      # entry 0 names a ring only now and then: silence to scan
        pred[0] = np.where(rng.random(T) < p_onset, pred[0], 0)
    flag = (rng.random((N + 1, T)) < p_flag).astype(np.int64)
    return M.pack_table(N, pred, flag)


def test_packing_matches_the_kernels_constants():
    assert [M.packing(N) for N in (1, 4, 7, 8, 11, 12, 15, 16)] == [
        (2, 16, 1), (4, 8, 1), (4, 8, 1), (5, 6, 2), (5, 6, 2), (5, 6, 3), (5, 6, 3), (6, 5, 4)]
    assert [M.tile_samples(N) for N in (4, 8, 12, 16)] == [64, 32, 32, 16]


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("N", NS)
def test_random_tables(N, L):
    rng = np.random.default_rng(1000 * N + L)
    T = _length(L, N + L)
    _same(_random_table(rng, N, T), T, N, L)                       # uniform predecessors: mostly rings
    x, _, nflag = _same(_random_table(rng, N, T, p_onset=0.02), T, N, L)   # rings and silence
    assert (x == 1).any() and (x > 1).any() and nflag > 0


@pytest.mark.parametrize("N", NS)
def test_all_silent_tables(N):
    L = 59
    rng = np.random.default_rng(N)
    for k in range(3):
        T = _length(L, k)
        flag = (rng.random((N + 1, T)) < 0.5).astype(np.int64)
        psi = M.pack_table(N, np.zeros((N + 1, T), dtype=np.int64), flag)
        x, bs, nflag = _same(psi, T, N, L)
        assert (x == 1).all() and (bs == 1).all()
        assert nflag == int(flag[0, 2:].sum()), "every silent decision from sample 2 on is counted once"


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("N", [1, 8, 16])
def test_every_junction_names_a_ring(N, L):
    """rings back to back, never silence: with L = 8 the ramps of a tile row reach their bound"""
    rng = np.random.default_rng(7 * N + L)
    T = _length(L, 2 * N + L)
    x, _, _ = _same(_random_table(rng, N, T, lo=1), T, N, L)
    assert (x[:-1] > 1).all() and x[-1] == 1     # the walk from T starts silent


@pytest.mark.parametrize("N,L", [(4, 8), (1, 8), (8, 8), (16, 8), (4, 59), (8, 59), (16, 59), (4, 127), (7, 255)])
def test_rings_across_every_edge(N, L):
    """Periodic spikes, a ring every L + gap samples.  The period is odd or 4 mod 8, so over a recording the rings
    meet the tile edges, the segment edge hi_rel and the walk start te_rel in many phases; the shifts move them
    over recording sample 0 and the end."""
    Bb, Hb = M.seg_geometry(L)
    seen_hi = seen_lo = 0
    for gap in (1, 5):
        period = L + gap
        for shift in range(0, period, max(1, period // 12)):
            T = _length(L, shift)
            pred = np.zeros((N + 1, T), dtype=np.int64)
            ring = 1 + (np.arange(T) // period) % N
            on = (np.arange(T) % period) == shift
            pred[0, on] = ring[on]
            flag = np.zeros((N + 1, T), dtype=np.int64)
            flag[:, ::3] = 1
            x, bs, _ = _same(M.pack_table(N, pred, flag), T, N, L)
            seen_hi += int(x[Bb - 1] > 1 and x[Bb] > 1)
            seen_lo += int(x[0] > 1)
            assert np.array_equal(x, M.walk_plain(M.pack_table(N, pred, flag), T, N, L)), "the segments' walks merge"
    assert seen_hi > 0, "no ring crossed the first segment edge"
    assert seen_lo > 0, "no ring reached recording sample 0"


@pytest.mark.parametrize("N,L", [(4, 8), (1, 59), (8, 59), (16, 127), (4, 255)])
def test_start_inside_a_ring(N, L):
    """bt_start: the walks that begin at T begin in state fs, every phase of the ring"""
    rng = np.random.default_rng(N + L)
    phases = range(1, L + 1) if L <= 59 else list(range(1, L + 1, 9)) + [L]
    for k0 in phases:
        a0 = k0 % N
        fs = a0 * L + k0
        T = _length(L, k0)
        psi = _random_table(rng, N, T, p_onset=0.01)
        x, _, _ = _same(psi, T, N, L, fs=fs)
        assert x[T - 1] == fs + 1
        if k0 > 1:
            assert x[T - 2] == fs


@pytest.mark.parametrize("N", [4, 8, 16])
def test_lengths_around_the_segment_and_tile_sizes(N):
    L = 20
    Bb, Hb = M.seg_geometry(L)
    rng = np.random.default_rng(N)
    for T in (Bb, Bb + 1, Bb - 1, Bb + Hb, Bb + Hb + 1, 2 * Bb, 2 * Bb + 2, 2 * Bb + Hb - 61, 33 * Bb + 5, 65 * Bb + 3):
        if T > 30 * Bb and N != 4:
            continue     # a second workgroup of segments: one row width is enough
        _same(_random_table(rng, N, T, p_onset=0.05), T, N, L)


def test_the_per_sample_walk_is_the_plain_walk_on_a_sweeps_table():
    """a table with silence everywhere: the segment walks merge within the walk-in, and both forms give the path
    of the whole table"""
    N, L = 4, 59
    rng = np.random.default_rng(3)
    T = 5 * 512 + 77
    pred = np.zeros((N + 1, T), dtype=np.int64)
    on = rng.random(T) < 0.01
    pred[0, on] = rng.integers(1, N + 1, size=int(on.sum()))
    psi = M.pack_table(N, pred, np.zeros((N + 1, T), dtype=np.int64))
    x, _, _ = _same(psi, T, N, L)
    assert np.array_equal(x, M.walk_plain(psi, T, N, L))
