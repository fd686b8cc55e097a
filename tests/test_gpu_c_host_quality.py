"""The per-spike fit from a C host (tests/c_host/quality_host.c, gcc, no Python in the process): one call of
hmmsort_spike_fit under a model track and one of hmmsort_plan_spike_fit on device buffers the host made itself must
give what the Python wrappers give for the same input, bit for bit, for float64 and for int16 samples."""
import os
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_spike_fit import FIELDS, model_of, ring_path, signal_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("quality_host") / "quality_host")
    lib = os.path.join(ROOT, "hmmspikesorter.jl_amd")
    hip = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_host", "quality_host.c"), "-o", path, "-L", lib,
                           "-lhmmsort_hip", "-L", hip, "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + hip])
    return path


def read_fits(H, buf, off, N, L):
    counts = np.frombuffer(buf, dtype="<i8", count=N, offset=off); off += 8 * N
    summary = np.frombuffer(buf, dtype="<f8", count=N * L, offset=off).reshape(N, L); off += 8 * N * L
    fits = []
    for a in range(N):
        n, cols = int(counts[a]), []
        for dt in ("<i8", "<f8", "<f8", "<f8", "<i4"):
            cols.append(np.frombuffer(buf, dtype=dt, count=n, offset=off)); off += n * int(dt[2])
        fits.append(H.SpikeFit(*cols, summary[a]))
    return fits, off


@pytest.mark.parametrize("raw", (False, True))
def test_c_host_gets_the_same_answers(H, exe, tmp_path, raw):
    rng = np.random.default_rng(77 + raw)
    N, K, T, sigma = 2, 16, 12_000, 30.0
    lp = np.log([0.01, 0.006])
    sm = H.StateMatrix.create(N, K, lp, False)
    st = np.asarray(sm.states)
    mu = np.asfortranarray(np.stack([H.create_spike_template(K, 3.0, 0.8, 0.2),
                                     H.create_spike_template(K, 4.0, 0.3, 0.2)], 1) * 100.0)
    x = ring_path(st, (300, 200), T, rng, gap=12)
    y = signal_of(x, st, mu, sigma, rng)
    y = np.round(y).astype(np.int16) if raw else y
    first = np.array([400, 3000, 7000], dtype=np.int64)              # the first spikes lie before the track
    track = H.ModelTrack(3, first, None, None, np.stack([mu, 0.9 * mu, 0.8 * mu]), None)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<qqqqq", N, K, T, int(raw), len(first)))
        f.write(struct.pack("<d", sigma))
        f.write(lp.astype("<f8").tobytes() + mu.tobytes(order="F"))
        f.write(y.astype("<i2" if raw else "<f8").tobytes() + x.astype("<i2").tobytes() + first.tobytes())
        f.write(np.ascontiguousarray(track.mu.transpose(0, 2, 1)).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    buf = open(fout, "rb").read()
    L = 8 + 3 * (K - 1)
    host, off = read_fits(H, buf, 0, N, L)
    plan, off = read_fits(H, buf, off, N, L)
    assert off == len(buf)
    model = model_of(H, sm, mu, sigma, y, x)
    for got, want in ((host, H.spike_fit(model, track)), (plan, H.spike_fit(model))):
        for g, w in zip(got, want):
            for k in FIELDS:
                assert getattr(g, k).tobytes() == getattr(w, k).tobytes(), k
    assert [len(f.times) for f in host] == [300, 200]
    assert all(np.isnan(h.amp[0]) and not np.isnan(p.amp[0]) for h, p in zip(host, plan))
