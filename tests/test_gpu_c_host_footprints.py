"""The footprints from a C host (tests/c_host/footprint_host.c, gcc, no Python in the process): hmmsort_footprints with
plain pointers must give the bytes of the numpy model for the seam case (lists of 255, 256, 257 and 513 spikes, W = 60)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import footprint_model as FM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("footprint_host") / "footprint_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "footprint_host.c"), "-o", path, "-L", lib,
                           "-lhmmsort_hip", "-Wl,-rpath," + lib])
    return path


def test_c_host_footprints_get_the_model_bytes(H, exe, tmp_path):
    y, lists, pre, W, _ = FM.seam_case(60)
    C, T = y.shape
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qqqqq", C, T, len(lists), pre, W))
        f.write(np.array([len(t) for t in lists], dtype="<i8").tobytes())
        for t in lists:
            f.write(t.astype("<i8").tobytes())
        f.write(np.ascontiguousarray(y).astype("<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(fout, "rb").read()
    s, q, nused, n = FM.model(y, lists, pre, W)
    assert nused.tolist() == [len(t) - 2 for t in lists] and np.abs(s).max() > 0
    assert buf == s.tobytes() + q.tobytes() + nused.tobytes() + n.tobytes()
