"""The features and the isolation from a C host (tests/c_host/isolation_host.c, gcc, no Python in the process): both
host calls with plain pointers must give the bytes of the numpy model for the seam case (lists of 255, 256, 257 and 513
spikes, W = 60): rows, used bytes, counts, the per-unit moments, the isolation distance and the confusion counts."""
import os
import struct
import subprocess

import numpy as np
import pytest

import feature_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("isolation_host") / "isolation_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "isolation_host.c"), "-o", path, "-L", lib,
                           "-lhmmsort_hip", "-Wl,-rpath," + lib])
    return path


def test_c_host_isolation_gets_the_model_bytes(H, exe, tmp_path):
    y, lists, pre, W = M.seam_case(60)
    C, T = y.shape
    P = 2
    basis, centre = M.random_basis(np.random.default_rng(70), C, P, W, wide=False)
    f, use, n, nused = M.features(y, lists, pre, W, None, basis, centre)
    g1, g2 = M.moments(f, use, n, 1)
    mu, vinv = M.gaussians(g1[:, 0], g2[:, 0], nused)
    offs = np.concatenate([[0], np.cumsum(n)])
    iso, closer, _, _ = M.isolation(f, offs, use, mu, vinv)
    assert not np.isnan(iso).any() and nused.tolist() == [len(t) - 2 for t in lists]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<qqqqqq", C, T, len(lists), pre, W, P))
        fh.write(np.array([len(t) for t in lists], dtype="<i8").tobytes())
        for t in lists:
            fh.write(t.astype("<i8").tobytes())
        for a in (y, basis, centre, mu, vinv):
            fh.write(np.ascontiguousarray(a).astype("<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(fout, "rb").read()
    want = [f, use, nused, n, g1[:, 0], g2[:, 0], iso, closer]
    pos = 0
    for name, a in zip(("feat", "used", "nused", "n", "g1", "g2", "iso_d2", "closer"), want):
        b = np.ascontiguousarray(a).tobytes()
        assert buf[pos:pos + len(b)] == b, name
        pos += len(b)
    assert pos == len(buf)
