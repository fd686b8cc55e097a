"""The template seed from a C host (tests/c_host/seed_host.c, gcc, no Python in the process): hmmsort_seed_templates
with plain pointers must give what the ctypes binding gives for the same input, for float64 and for int16 samples."""
import os
import struct
import subprocess

import numpy as np
import pytest

import seed_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("seed_host") / "seed_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "seed_host.c"), "-o", path, "-L", lib,
                           "-lhmmsort_hip", "-Wl,-rpath," + lib])
    return path


@pytest.mark.parametrize("raw", (False, True))
def test_c_host_seed_gets_the_same_answers(H, exe, tmp_path, raw):
    if raw:
        N, K, threshold, y = 3, 20, 1.0, SC.adversarial(20, 4097)
    else:
        N, K, threshold, y = 4, 20, 4.0, np.array(SC.realistic("k20")[0])
    T = len(y)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qqqq", N, K, T, int(raw)))
        f.write(struct.pack("<d", threshold))
        f.write(y.astype("<i2" if raw else "<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(fout, "rb").read()
    E, iters, sigma = struct.unpack_from("<qqd", buf, 0)
    off = 24
    mu = np.frombuffer(buf, dtype="<f8", count=K * N, offset=off).reshape((K, N), order="F"); off += 8 * K * N
    lp = np.frombuffer(buf, dtype="<f8", count=N, offset=off); off += 8 * N
    counts = np.frombuffer(buf, dtype="<i8", count=N, offset=off); off += 8 * N
    times = np.frombuffer(buf, dtype="<i8", count=E, offset=off); off += 8 * E
    labels = np.frombuffer(buf, dtype="<i2", count=E, offset=off); off += 2 * E
    assert off == len(buf)

    _sm, _mu, sig_py, info = H.seed_templates(y, N, K, threshold=threshold)
    assert E == info["n_events"] > N and iters == info["iters"] and sigma == sig_py
    assert mu.tobytes() == info["raw"]["mu"].tobytes() and lp.tobytes() == info["raw"]["lp"].tobytes()
    assert np.array_equal(counts, info["raw"]["counts"]) and counts.sum() == E
    assert np.array_equal(times, info["times"]) and np.array_equal(labels, info["raw_labels"])
