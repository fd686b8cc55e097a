"""The chunked decode from a C host (tests/c_host/fit_host.c, gcc, no Python in the process): hmmsort_fit_chunked and
hmmsort_fit_channels with plain pointers must give what the ctypes binding gives for the same inputs."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import two_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_host_chunked_decode_gets_the_same_answers(H, tmp_path):
    N, K, T, cs = 2, 30, 6000, 1500
    temps = two_templates(H, K)
    pp = np.array([0.03, 0.03])
    y = H.create_signal(T, 0.3, pp, temps, seed=7)
    exe = str(tmp_path / "fit_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "fit_host.c"), "-o", exe, "-L", lib, "-lhmmsort_hip",
                           "-Wl,-rpath," + lib])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qqqq", N, K, T, cs))
        f.write(struct.pack("<d", 0.3))
        f.write(np.log(pp).astype("<f8").tobytes())
        f.write(temps.ravel(order="F").astype("<f8").tobytes())
        f.write(y.astype("<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = open(fout, "rb").read()
    nch, ll = struct.unpack_from("<qd", raw, 0)
    off = 16
    ml = np.frombuffer(raw, dtype="<i2", count=T, offset=off); off += 2 * T
    # the same through the Python binding
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    tm = H.HMMSpikeTemplateModel(sm, temps, 0.3)
    py = H.fit_channels(tm, [y], cs)[0]
    H.shutdown()
    assert py.ml_seq.max() > 1
    assert np.array_equal(ml, py.ml_seq) and ll == py.ll
    assert nch == 3
    for c in range(nch):
        st, llc = struct.unpack_from("<qd", raw, off); off += 16
        mlc = np.frombuffer(raw, dtype="<i2", count=T, offset=off); off += 2 * T
        assert st == 0 and llc == py.ll and np.array_equal(mlc, py.ml_seq), c
