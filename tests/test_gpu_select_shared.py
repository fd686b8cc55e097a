"""The one radix select (csrc/radix_select.hip) under its two callers: the template seed's noise scale and
device.noise_scale of the same signal as a one-row block are the same double, and both are seed_model.noise_scale.
The lengths cross one thread block (256), one whitening tile (2048) and odd and even ranks; the signals are heavy
ties, all-equal values, normal noise, signed zeros / denormals / infinities around a finite median, and int16 samples
through the seed's own upload.  A block of five rows exercises the per-slot row stride, a seed with four clusters the
side-by-side selects over one array (stride 0).  No NaN anywhere: neither model defines them."""
import numpy as np
import pytest

import seed_cases as SC
import seed_model as SM
from test_gpu_seed import run, same

pytestmark = pytest.mark.gpu

LENGTHS = (2, 3, 255, 256, 257, 2048, 2049, 20011)
SPECIALS = np.array([-0.0, 5e-324, -1.1e-308, np.inf, -np.inf])


def signals(T):
    """name -> signal; "i16" is int16, the rest float64"""
    rng = np.random.default_rng(7000 + T)
    special = rng.standard_normal(T)
    at = np.arange(1, T, 3)                       # a third of the samples, two fifths of them infinite
    special[at] = SPECIALS[(at // 3) % 5]
    out = {"ties": rng.integers(-3, 4, T).astype(np.float64), "equal": np.full(T, -2.5),
           "normal": rng.standard_normal(T), "special": special, "i16": rng.integers(-300, 301, T).astype(np.int16)}
    assert np.isfinite(SM.noise_scale(special)) and not np.isnan(special).any()
    return out


def seed_sigma(H, y):
    return H.seed_templates(y, 1, 2, sigma=0)[2]


def block_sigma(H, Y):
    import torch
    return H.device.noise_scale(torch.as_tensor(np.ascontiguousarray(Y, dtype=np.float64), device="cuda"))


@pytest.mark.parametrize("T", LENGTHS)
def test_seed_and_block_noise_scale_are_the_same_double(H, T):
    for name, y in signals(T).items():
        want = SM.noise_scale(y)
        s = seed_sigma(H, y)
        b = block_sigma(H, y.astype(np.float64)[None, :])
        assert b.shape == (1,) and s == want and b[0] == want, (T, name, s, b[0], want)
        if y.dtype == np.int16:
            assert seed_sigma(H, y.astype(np.float64)) == want, (T, name)


def test_rows_of_a_block_select_side_by_side(H):
    sig = signals(257)
    Y = np.stack([sig[k].astype(np.float64) for k in ("ties", "equal", "normal", "special", "i16")])
    rows = block_sigma(H, Y)
    single = np.array([block_sigma(H, row[None, :])[0] for row in Y])
    assert rows.shape == (5,) and np.array_equal(rows, single)
    assert np.array_equal(rows, [SM.noise_scale(row) for row in Y])


def test_quantile_selects_over_one_array(H):
    y = SC.adversarial(60, 20011)
    g = run(H, y, 4, 60, threshold=1.0, refractory=2)
    same(g, SM.seed_model(y, 4, 60, threshold=1.0, refractory=2), "four selects")
    assert g["n_events"] > 4
