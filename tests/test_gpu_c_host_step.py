"""Viterbi training over channels from a C host (tests/c_host/step_host.c, gcc, no Python in the process):
hmmsort_fit_step_channels with plain pointers must give what the ctypes binding gives for the same inputs."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import two_templates

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_host_hard_step_gets_the_same_answers(H, tmp_path):
    N, K, T, cs = 2, 30, 6000, 1500
    temps = two_templates(H, K)
    pp = np.array([0.03, 0.03])
    y = H.create_signal(T, 0.3, pp, temps, seed=7)
    exe = str(tmp_path / "step_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "step_host.c"), "-o", exe, "-L", lib, "-lhmmsort_hip",
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

    def record(off):
        mu = np.frombuffer(raw, dtype="<f8", count=K * N, offset=off).reshape((K, N), order="F"); off += 8 * K * N
        sigma, nlp = struct.unpack_from("<dq", raw, off); off += 16
        lp = np.frombuffer(raw, dtype="<f8", count=nlp, offset=off); off += 8 * nlp
        counts = list(struct.unpack_from("<qqq", raw, off)); off += 24
        return dict(mu=mu, sigma=sigma, lp=lp, counts=counts), off

    # the same through the Python binding
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    tm = H.HMMSpikeTemplateModel(sm, temps, 0.3)
    models, steps = H.fit_step_channels(tm, [y, y, y], cs, devices=[0, 0])
    _m, pooled = H.fit_step_channels(tm, [y, y, y], cs, devices=[0, 0], pooled=True)
    H.shutdown()
    assert models[0].ml_seq.max() > 1 and not np.array_equal(steps[0][1], temps)
    (nch,), off = struct.unpack_from("<q", raw, 0), 8
    assert nch == 3
    for c in range(nch):
        st, ll, ll2 = struct.unpack_from("<qdd", raw, off); off += 24
        ml = np.frombuffer(raw, dtype="<i2", count=T, offset=off); off += 2 * T
        rec, off = record(off)
        assert st == 0 and ll == ll2 == models[c].ll and np.array_equal(ml, models[c].ml_seq), c
        assert rec["mu"].tobytes() == steps[c][1].tobytes() and rec["sigma"] == steps[c][2], c
        assert rec["counts"] == steps[c][3] == [0, 0, 0], c
        assert len(rec["lp"]) == N and np.all(np.isfinite(rec["lp"])) and np.all(rec["lp"] < 0.0), c
    rec, off = record(off)
    assert off == len(raw)
    assert rec["mu"].tobytes() == pooled[0][1].tobytes() and rec["sigma"] == pooled[0][2]
    # three copies of one channel pool to that channel's templates (sums of three equal terms, then one division)
    assert np.allclose(rec["mu"], steps[0][1], rtol=1e-14, atol=1e-15) and abs(rec["sigma"] - steps[0][2]) <= 1e-13
