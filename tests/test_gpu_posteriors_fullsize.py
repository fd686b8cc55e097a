"""Posterior outputs at the headline size (N = 4, K = 60, 10 M samples) through the size-independent
properties of tests/test_gpu_posteriors.py: the CPU oracle cannot reach this size, the definitions are pinned
against it there."""
import numpy as np
import pytest

from conftest import four_templates
from test_gpu_posteriors import Dev, consistency

pytestmark = pytest.mark.gpu
T = 10_000_000


def test_posterior_consistency_at_10M(H):
    import torch
    K, N = 60, 4
    temps = four_templates(H, K)
    pp = [0.003, 0.001, 0.002, 0.0015]
    y = H.create_signal(T, 0.3, pp, temps, seed=1234)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)
    dev = Dev(H, y, sm, temps, 0.3)
    assert dev.plan.info()["engine"] == H.ENGINE_WAVE
    # expected counts: the sum of the onsets (read before the E-step of `consistency` discards the posteriors)
    cnt = dev.plan.expected_counts()
    assert np.allclose(cnt, dev.onset.sum(1), rtol=1e-12)
    consistency(H, dev, y, sm, temps, 0.3, 1e-8)
    # the decode is a valid labelling: silent where silent dominates, ring states inside 1..S
    assert dev.xm.min() >= 1 and dev.xm.max() <= sm.nstates
    assert np.all(dev.xm[dev.silent > 0.5] == 1)
    # ... and close to what the Viterbi path holds
    dx = torch.zeros(T, dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    dev.plan.viterbi(dev.dy, dx, dll)
    dev.plan.posteriors(dev.dy)                    # the E-step above discarded the posteriors: call again
    got = dev.plan.spike_confidence(dx, 2)
    nvit = np.array([len(t) for t, _ in got])
    print("expected counts", cnt, "Viterbi events", nvit)
    assert np.all(np.abs(cnt - nvit) <= 0.02 * nvit)
    allc = np.concatenate([c for _, c in got])
    assert np.all((allc >= 0) & (allc <= 1)) and np.median(allc) > 0.9
