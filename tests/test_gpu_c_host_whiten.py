"""The whitening stages from a C host (tests/c_host/whiten_host.c, gcc, no Python in the process): hmmsort_noise_cov
and hmmsort_channel_mix with plain pointers must give the bytes the ctypes binding gives for the same block."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("whiten_host") / "whiten_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "whiten_host.c"), "-o", path, "-L", lib,
                           "-lhmmsort_hip", "-Wl,-rpath," + lib])
    return path


def test_c_host_whitening_gets_the_same_bytes(H, exe, tmp_path):
    nC, T, R, M, guard, threshold = 5, 4097, 4, 3, 7, 3.5
    rng = np.random.default_rng(18)
    Y = rng.standard_normal((nC, T)) * np.array([1.0, 2.0, 0.5, 3.0, 1.5])[:, None]
    Y[1:3] += rng.standard_normal(T)
    nbr = np.array([[0, 1, -1], [4, 4, 2], [-1, -1, -1], [3, 0, 1]], dtype=np.int32)
    w = rng.standard_normal((R, M))
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qqqqqd", nC, T, R, M, guard, threshold))
        f.write(Y.astype("<f8").tobytes())
        f.write(nbr.astype("<i4").tobytes())
        f.write(w.astype("<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(fout, "rb").read()
    sigma, _thr, n, s1, s2 = H.noise_sums(Y, threshold, guard)
    mixed = H.channel_mix(Y, nbr, w)
    assert 0 < n < T and np.abs(mixed).max() > 0
    want = sigma.tobytes() + struct.pack("<q", n) + s1.tobytes() + s2.tobytes() + mixed.tobytes()
    assert buf == want
