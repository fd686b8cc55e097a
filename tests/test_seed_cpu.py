"""The template seed without a GPU: the numpy model of seed_model.py on the three recordings of the DESIGN table
(counts, error caps), the assignment margins that make exact label comparison on the GPU fair, and the C ABI's two
new symbols in the header and in the built library."""
import ctypes
import os
import re

import numpy as np
import pytest

import seed_cases as SC
import seed_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# seed counts per generating template, and the caps on the seed's best-shift error (measured 0.086 / 0.080, 0.086 /
# 0.057 and 0.244 / 0.117 on the CPU prototype; the caps leave room for another numpy build)
TABLE = {"k60_long": ((445, 179), (0.12, 0.12)), "k60": ((138, 43), (0.12, 0.12)), "k20": ((93, 30), (0.30, 0.15))}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_model_counts_and_seed_error(name):
    y, temps, true = SC.realistic(name)
    r = SC.realistic_model(name, 2)
    err, col = SM.match_errors(r["mu"], temps)
    print(name, "counts", r["counts"], "generating", true, "errors", err, "iters", r["iters"])
    assert sorted(col) == [0, 1]
    counts, caps = TABLE[name]
    assert tuple(int(r["counts"][c]) for c in col) == counts
    assert r["n_events"] == sum(counts) and len(r["times"]) == r["n_events"]
    assert err[0] <= caps[0] and err[1] <= caps[1]
    assert np.all(r["mu"][0] == 0)
    assert np.array_equal(r["lp"], np.log(r["counts"] / len(y)))


@pytest.mark.parametrize("N", SC.GPU_N)
@pytest.mark.parametrize("name", SC.GPU_REALISTIC + ("k60_long",))
def test_assignment_margins(name, N):
    """Exact label equality between two implementations whose centre sums are ordered differently needs every
    assignment to be decided by far more than rounding.  (The integer signals of the adversarial GPU tests need no
    margin: sums of small integers are exact in any order, so centres and distances agree bit for bit and ties
    fall the same way.)"""
    r = SC.realistic_model(name, N)
    print(name, N, "margin", r["margin"], "iters", r["iters"])
    assert r["margin"] >= 1e-9


def test_model_edge_rules():
    K, D = 8, 7
    y = np.zeros(50)
    y[[10, 11, 12]] = 5.0          # a plateau: its earliest sample
    y[30], y[33] = 4.0, 6.0        # within R of each other: the larger one
    r = SM.seed_model(y, 2, K, threshold=1.0, sigma=1.0, refractory=5, align=2)
    assert r["times"].tolist() == [11, 34]
    for t, ok in ((1, False), (2, True), (50 - D + 2 - 1, True), (50 - D + 2, True), (50 - D + 2 + 1, False)):
        y = np.zeros(50)
        y[t] = 5.0
        assert SM.seed_model(y, 1, K, threshold=1.0, sigma=1.0, align=2)["n_events"] == int(ok), t
    r = SM.seed_model(np.zeros(40), 3, K)
    assert r["n_events"] == 0 and np.all(r["mu"] == 0) and np.all(np.isneginf(r["lp"])) and r["sigma"] == 0.0


def test_header_declares_and_library_exports(H):
    src = open(os.path.join(ROOT, "include", "hmmsort.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = ctypes.CDLL(H._lib.LIB_PATH)
    for name in ("hmmsort_seed_templates", "hmmsort_seed_templates_device"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in H._lib.SIGNATURES, name
    for macro, v in (("HMMSORT_SEED_MAX_K", H._lib.SEED_MAX_K), ("HMMSORT_SEED_MAX_N", H._lib.SEED_MAX_N),
                     ("HMMSORT_SEED_MAX_R", H._lib.SEED_MAX_R)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == v
    assert H._lib.SEED_MAX_K >= 257 and H._lib.SEED_MAX_R >= 256 and H._lib.SEED_MAX_N >= 16
    # struct layouts as the header lays them out on LP64
    assert ctypes.sizeof(H._lib.SeedOpt) == 48 and ctypes.sizeof(H._lib.SeedOut) == 72


def test_bad_arguments_before_any_gpu_work(H):
    """EINVAL comes before the device is asked for, so these hold with and without a GPU"""
    y = np.zeros(100)
    for kw, N, K in ((dict(), 2, 101), (dict(), 0, 20), (dict(), 17, 20), (dict(), 2, 1), (dict(), 2, 1026),
                     (dict(align=19), 2, 20), (dict(polarity=2), 2, 20), (dict(polarity=-2), 2, 20),
                     (dict(refractory=0), 2, 20), (dict(refractory=1025), 2, 20)):
        with pytest.raises(H.HmmsortError) as e:
            H.seed_templates(y, N, K, **kw)
        assert e.value.code == H._lib.EINVAL, (kw, N, K)
    with pytest.raises(TypeError):
        H.seed_templates(y, 2, 20, treshold=3.0)
    with pytest.raises(ValueError):
        H.train_model(y, 2, 20, False, 2, init="guess")
    with pytest.raises(ValueError):      # the random start still refuses hard EM
        H.train_model(y, 2, 20, False, 2, method="viterbi")
