"""numpy model of the front end (hmmsort_preprocess, include/hmmsort.h): the authority the device result must equal
bit for bit.  Every numpy operation below rounds on its own, element by element, which is the contract: no fused
multiply-add, a fixed order of the lags and of the channels."""
import numpy as np


def mirror_index(T, P):
    """source index of every sample of the signal extended by P each side: mirrored about the end samples without
    repeating them (x[-i] = x[i], x[T-1+i] = x[T-1-i]); needs T >= P + 1"""
    assert T >= P + 1
    i = np.abs(np.arange(-P, T + P))
    return np.where(i >= T, 2 * (T - 1) - i, i)


def fir(x, half):
    """x: (C, T) float64; half: taps[0..P] (h[-j] = h[j] = taps[j]) or None for no filter.
    acc = taps[0] * x[t]; for j = 1..P ascending: acc = acc + taps[j] * (x[t-j] + x[t+j])"""
    x = np.asarray(x, dtype=np.float64)
    if half is None:
        return x.copy()
    half = np.asarray(half, dtype=np.float64)
    P, T = len(half) - 1, x.shape[1]
    xe = x[:, mirror_index(T, P)]
    acc = half[0] * x
    for j in range(1, P + 1):
        acc = acc + half[j] * (xe[:, P - j:P - j + T] + xe[:, P + j:P + j + T])
    return acc


def groups_of(C, group):
    """member channels (ascending) of every group, in ascending id; group None: all channels in group 0"""
    ids = np.zeros(C, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    assert len(ids) == C
    return [np.nonzero(ids == g)[0] for g in sorted(set(ids[ids >= 0].tolist()))]


def reference(f, mode, group=None):
    """f: (C, T) float64, mode None / "median" / "mean"; channels outside every group pass unchanged"""
    out = np.array(f, dtype=np.float64, copy=True)
    if mode is None:
        return out
    for mem in groups_of(f.shape[0], group):
        G, v = len(mem), f[mem]
        if mode == "median":
            s = np.sort(v, axis=0)
            m = s[G // 2] if G % 2 else (s[G // 2 - 1] + s[G // 2]) * 0.5
        elif mode == "mean":
            m = np.zeros(f.shape[1])
            for c in range(G):
                m = m + v[c]
            m = m / float(G)
        else:
            raise ValueError(mode)
        out[mem] = v - m
    return out


def preprocess(x, half=None, mode=None, group=None, keep=None):
    """x: (C, T), any of the four sample types (widening to float64 is exact); the whole front end"""
    out = reference(fir(np.asarray(x).astype(np.float64), half), mode, group)
    return out if keep is None else out[np.asarray(keep, dtype=np.int64)]
