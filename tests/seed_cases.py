"""Inputs the seed tests share (test_seed_cpu.py, test_gpu_seed.py): the three synthetic recordings of the DESIGN
table and the small integer signals that put ties and plateaux at every offset."""
import functools

import numpy as np

# (K, T, resolve_overlaps of the end-to-end run, generating counts)
REALISTIC = {"k60_long": (60, 200_000), "k60": (60, 60_000), "k20": (20, 30_000)}
GPU_REALISTIC = ("k60", "k20")
GPU_N = (2, 4, 7)
PARAMS = ((3.0, 0.8, 0.2), (4.0, 0.3, 0.2))
SIGMA, PP, SEED = 0.3, (0.003, 0.001), 1235


@functools.lru_cache(maxsize=None)
def realistic(name):
    """(y, generating templates K x 2, generating onset counts)"""
    import hmmsort_amd as H
    K, T = REALISTIC[name]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *p) for p in PARAMS], axis=1))
    y, onsets = H.create_signal(T, SIGMA, list(PP), temps, seed=SEED, return_states=True)
    y.setflags(write=False)
    return y, temps, np.bincount([j for _, j in onsets], minlength=2)


@functools.lru_cache(maxsize=None)
def realistic_model(name, N):
    import seed_model as SM
    y, _, _ = realistic(name)
    return SM.seed_model(y, N, REALISTIC[name][0])


ADV_K = (3, 20, 60, 257)


def adversarial_T(K):
    return (K, K + 1, 1000, 4097, 20011)


def adversarial(K, T):
    """int16 samples drawn from -8..8: equal neighbours, plateaux and ties between clusters wherever a tile ends"""
    rng = np.random.default_rng(1000 * K + T)
    return rng.integers(-8, 9, T).astype(np.int16)
