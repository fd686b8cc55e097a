"""The posterior definitions (INTEGRATION.md "Posteriors") restated in numpy (tests/posterior_model.py), checked
on the CPU oracle alone, plus the host-side surface of the feature that needs no GPU."""
import inspect

import numpy as np
import pytest

import posterior_model as PM
from conftest import four_templates, to_oracle_sm, two_templates


def _case(O, H, N, K, T, sigma, seed):
    temps = (two_templates(H, K) if N == 2 else four_templates(H, K))[:, :N]
    pp = np.full(N, 0.003)
    y = H.create_signal(T, sigma, pp, temps, seed=seed)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    mu = np.asfortranarray(temps.copy())
    mu[0, :] = 0
    return y, sm, to_oracle_sm(O, sm), mu


@pytest.mark.parametrize("sigma", [0.3, 1.0])
def test_gamma_is_a_ring_posterior(O, H, sigma):
    N, K, T = 2, 20, 1500
    y, sm, osm, mu = _case(O, H, N, K, T, sigma, 3)
    g, z = PM.gamma(O, y, osm, mu, sigma)
    assert np.isfinite(z)
    assert PM.oracle_defect(g) < 1e-9
    L = K - 1
    # a ring runs deterministically: gamma_t(a, k) = gamma_{t+1}(a, k+1)
    for a in range(N):
        ring = g[1 + a * L:1 + (a + 1) * L]
        assert np.abs(ring[:-1, :-1] - ring[1:, 1:]).max() < 1e-10
    onset, occ, silent = PM.marginals(g, sm.states)
    assert np.abs(occ.sum(0) + silent - 1.0).max() < 1e-9
    # occ is the window sum of the onsets once the head has left the window
    for a in range(N):
        win = np.convolve(onset[a], np.ones(L))[:T]
        assert np.abs(win[L:] - occ[a, L:]).max() < 1e-9


def test_head_mass_sits_on_running_rings(O, H):
    # first column = emission only for every state (baumwelch.jl:36): at t = 0 the S - 1 ring states share the
    # uniform start with the one silent state, so almost all posterior mass of a quiet start is on running rings
    y, sm, osm, mu = _case(O, H, 4, 60, 2000, 1.0, 5)
    y[:80] = 0.0
    g, _ = PM.gamma(O, y, osm, mu, 1.0)
    onset, occ, silent = PM.marginals(g, sm.states)
    assert occ[:, 0].sum() > 0.9 and silent[0] < 0.1
    assert occ[:, 0].sum() - onset[:, 0].sum() > 0.85      # ... and not on rings that start at t = 0


def test_confidence_is_monotone_in_jitter_and_aligned(O, H):
    y, sm, osm, mu = _case(O, H, 2, 20, 3000, 1.0, 7)
    g, _ = PM.gamma(O, y, osm, mu, 1.0)
    x, _ = O.viterbi(y, osm, mu, 1.0)
    ref = O.extract_spiketimes(x, osm, mu)
    prev = None
    for J in (0, 1, 2, 5):
        c = PM.confidence(g, sm.states, mu, x, J)
        for a in range(2):
            assert np.array_equal(c[a][0], np.asarray(ref[a]).ravel())
            assert np.all(c[a][1] >= 0) and np.all(c[a][1] <= 1)
            if prev is not None:
                assert np.all(c[a][1] >= prev[a][1] - 1e-15)
        prev = c
    assert sum(len(c[a][0]) for a in range(2)) > 3
    assert min(c[a][1].min() for a in range(2) if len(c[a][1])) <= 1.0


def test_decode_picks_the_column_maximum(O, H):
    y, sm, osm, mu = _case(O, H, 2, 20, 800, 0.3, 9)
    g, _ = PM.gamma(O, y, osm, mu, 0.3)
    xm = PM.decode(g)
    assert xm.dtype == np.int16 and xm.min() >= 1 and xm.max() <= sm.nstates
    assert np.array_equal(g[xm.astype(int) - 1, np.arange(g.shape[1])], g.max(0))


def test_python_signatures(H):
    assert list(inspect.signature(H.posteriors).parameters) == ["y", "lA", "mu", "sigma"]
    assert list(inspect.signature(H.posterior_decode).parameters) == ["y", "lA", "mu", "sigma"]
    sig = inspect.signature(H.spike_confidence)
    assert list(sig.parameters) == ["model", "jitter"] and sig.parameters["jitter"].default == 2
    for name in ("posteriors", "posterior_decode", "spike_confidence", "expected_counts"):
        assert callable(getattr(H.Plan, name))
    assert inspect.signature(H.Plan.spike_confidence).parameters["jitter"].default == 2
    assert [f for f in H.Posteriors.__dataclass_fields__] == ["onset", "occ", "silent", "logz"]
    sd = inspect.signature(H.sort_data).parameters
    assert sd["confidence"].default is False and sd["jitter"].default == 2


def test_sort_data_too_many_templates_unchanged(H):
    # the early exit of hmmsort.jl:49-52 needs no device: the new keyword does not disturb it
    forms = np.zeros((20, 1, 5))
    assert H.sort_data(forms, [1.0], np.full(5, 0.01), np.zeros(100), dosave=False, confidence=False) == {}
    assert H.sort_data(forms, [1.0], np.full(5, 0.01), np.zeros(100), dosave=False) == {}


def test_new_symbols_declared_and_exported(H):
    import ctypes
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "hmmsort.h")).read()
    L = ctypes.CDLL(H._lib.LIB_PATH)
    for n in ("hmmsort_plan_posteriors", "hmmsort_plan_posterior_decode", "hmmsort_plan_spike_confidence",
              "hmmsort_plan_expected_counts", "hmmsort_posteriors"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert hasattr(L, n), "missing export: " + n
        assert n in H._lib.SIGNATURES
    L.hmmsort_version.restype = ctypes.c_int
    assert L.hmmsort_version() >= 110
