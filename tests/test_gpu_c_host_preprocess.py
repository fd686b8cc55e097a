"""The front end from a C host (tests/c_host/preprocess_host.c, gcc, no Python in the process): hmmsort_preprocess
with plain pointers must give the bytes the ctypes binding gives for the same int16 sample-major block."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("preprocess_host") / "preprocess_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "preprocess_host.c"), "-o", path, "-L", lib,
                           "-lhmmsort_hip", "-Wl,-rpath," + lib])
    return path


def test_c_host_preprocess_gets_the_same_bytes(H, exe, tmp_path):
    nC, T, P = 5, 4097, 64
    rng = np.random.default_rng(17)
    raw = np.round(rng.standard_normal((T, nC)) * 800.0).astype(np.int16)      # sample-major
    full = H.design_fir(30000.0, low=300.0, ntaps=2 * P + 1)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qqq", nC, T, P))
        f.write(full[P:].astype("<f8").tobytes())
        f.write(raw.astype("<i2").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(fout, "rb").read()
    want = H.preprocess(raw, full, "median")
    assert want.shape == (nC, T) and np.abs(want).max() > 0
    assert buf == want.tobytes()
