"""The unit stability from a C host (tests/c_host/stability_host.c, gcc, no Python in the process): the host call with
plain pointers must give the bytes of the numpy model, table after table, for three units whose bins hold 0 to 2 100
spikes (one wave, one workgroup in LDS, one workgroup re-reading) with NaNs among the values."""
import os
import struct
import subprocess

import numpy as np
import pytest

import stability_model as SM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES = ("n", "count", "valid", "quant", "sum", "sumsq", "uvalid", "uquant", "umin", "umax", "usum", "usumsq", "hist",
          "under", "over")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stability_host") / "stability_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "stability_host.c"), "-o", path, "-L", lib,
                           "-lhmmsort_hip", "-Wl,-rpath," + lib])
    return path


def test_c_host_stability_gets_the_model_bytes(H, exe, tmp_path):
    rng = np.random.default_rng(71)
    bin, lengths = 2500, ((3, 0, 64, 65, 2100, 257), (0, 0, 0, 0, 0, 0), (256, 1, 2049, 0, 700, 40))
    T = 6 * bin - 7
    times, values = [], []
    for row in lengths:
        t = np.concatenate([b * bin + 1 + np.sort(rng.choice(bin - 7, n, replace=False)) for b, n in enumerate(row)])
        v = np.round(rng.standard_t(3, len(t)), 2)
        v[rng.random(len(t)) < 0.1] = np.nan
        times.append(t.astype(np.int64)), values.append(v)
    q_num, q_den, hist = (0, 1, 3, 5, 6), 6, (32, -4.0, 4.0)
    want = SM.unit_stability(times, values, T, bin, q_num, q_den, hist)
    assert want.count.tolist() == [list(r) for r in lengths] and np.isnan(want.umin[1]) and want.under.sum() > 0
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<qqqqqq", len(times), T, bin, len(q_num), q_den, hist[0]))
        fh.write(np.array(q_num + (0,) * (8 - len(q_num)), dtype="<i8").tobytes())
        fh.write(struct.pack("<dd", hist[1], hist[2]))
        fh.write(np.array([len(t) for t in times], dtype="<i8").tobytes())
        for t in times:
            fh.write(t.astype("<i8").tobytes())
        for v in values:
            fh.write(v.astype("<f8").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(fout, "rb").read()
    pos = 0
    for name in TABLES:
        b = np.ascontiguousarray(getattr(want, name)).tobytes()
        assert buf[pos:pos + len(b)] == b, name
        pos += len(b)
    assert pos == len(buf)
