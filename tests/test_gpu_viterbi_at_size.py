"""Every engine's Viterbi decode at the sizes the headline numbers are quoted at, against the extended-precision
MAP reference (oracle/hp_viterbi.c: long double, delta renormalised per sample, pinned by exact enumeration and
compared with the fp64 oracle in test_hp_viterbi_cpu.py).  Above 2 M samples and on the large overlap models the
decode was so far checked device against device only, and by properties that a path with thousands of wrong
decisions satisfies; the engines share the state space, the emission code, the first-sample rule and the host glue.

Reference paths come from tests/golden/viterbi_at_size/<case>.npz (made by tests/golden/make_viterbi_at_size.py).
The inputs are regenerated from the seed and hashed: on a mismatch the reference is recomputed live, and the test
says so; it never compares against a stale fixture.

The acceptance rule (oracle/hp.py, compare_paths; tests/viterbi_rule.py): valid path; on every run where the decode
differs from the reference path, -eps <= Delta <= tau with tau what the fp64 reference implementation's own rounding
can turn (derived, not measured); differing samples <= 1e-5 T and no open near-tie on the device (diag[7] == 0,
last_escalations == 0) except that duplicate templates are exempt from the cap; |ll - ll*| <= 1e-9 |ll*|.
Each test prints the number of differing samples, the largest Delta/tau and the ll error before it asserts.
Measured on the MI355X: DESIGN.md section 3.7.
"""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

import viterbi_rule as VR  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_options(H, monkeypatch):
    monkeypatch.delenv("HMMSORT_PAIR", raising=False)
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)
    yield
    for k in ("engine", "block", "halo"):
        H.set_option(k, 0)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs of a case (regenerated from its seed) and the reference's path for exactly these inputs"""
    import make_viterbi_at_size as G
    from oracle import hp
    y, osm, mu, sigma, pp = G.inputs(name)
    h = G.hashes(y, osm, mu, sigma)
    path = os.path.join(G.OUT, name + ".npz")
    assert os.path.exists(path), "fixture %s is missing" % path
    z = G.unpack(G.load(name))
    if str(z["sha_y"]) != h["sha_y"] or str(z["sha_model"]) != h["sha_model"]:
        print("case %s: the regenerated inputs do not hash to the fixture's (another random stream?): "
              "recomputing the reference live" % name)
        z = G.reference(y, osm, mu, sigma, threads=16)
    x = G.decode(z["idx"], z["state"], len(y), osm)
    LD = hp.LD
    ref = VR.Ref(x, LD(z["ll"]) + LD(z["ll_lo"]), z["idx"], z["cum"].astype(LD), float(z["dmax"]),
                 LD(z["score"]) + LD(z["score_lo"]))
    N, K, ov, T = G.shape(name)
    return dict(name=name, y=y, osm=osm, mu=mu, sigma=sigma, pp=pp, ref=ref, N=N, K=K, ov=ov,
                model=hp._Model(osm, mu, sigma), dup=name in G.DUPLICATES)


def product_sm(H, c):
    """the product's state matrix of the case; its transition list is the one the reference was given"""
    sm = H.StateMatrix.create(c["N"], c["K"], np.log(c["pp"]), c["ov"])
    tr = sm.transitions
    assert np.array_equal(tr["src"], c["osm"].src) and np.array_equal(tr["dst"], c["osm"].dst)
    assert np.array_equal(tr["lp"], c["osm"].val) and np.array_equal(sm.states, c["osm"].states)
    return sm


def accept(tag, c, x, ll):
    return VR.accept(tag, c["y"], c["osm"], c["mu"], c["sigma"], c["ref"], x, ll, duplicates=c["dup"], model=c["model"])


def plan_decode(H, c, sm, fused=False):
    """one decode on a device-resident plan: (x, ll, diagnostics, info, overlap sweep)"""
    import torch
    T = len(c["y"])
    plan = H.Plan(T, sm, c["mu"], c["sigma"])
    try:
        info, sweep = plan.info(), plan.overlap_sweep()
        dy = torch.from_numpy(c["y"]).cuda()
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        if fused:
            stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
            plan.decode_estep(dy, dx, dll, stats)
        else:
            plan.viterbi(dy, dx, dll)
        diag = plan.diagnostics()
        torch.cuda.synchronize()
        return dx.cpu().numpy(), float(dll.cpu()[0]), diag, info, sweep
    finally:
        plan.close()


# ---- A, B: the headline model at 10 M samples -------------------------------------------------------------------

@pytest.mark.parametrize("engine", ["wave", "ring", "strict"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_host_decode_at_10M(H, name, engine):
    c = case(name)
    sm = product_sm(H, c)
    H.set_option("engine", {"wave": H.ENGINE_WAVE, "ring": H.ENGINE_RING, "strict": H.ENGINE_STRICT}[engine])
    x, ll = H.viterbi(c["y"], sm, c["mu"], c["sigma"])
    esc = H.get_option("last_escalations")
    accept("%s %s (host entry)" % (name, engine), c, x, ll)
    assert esc == 0, esc


def test_fused_decode_estep_at_10M(H):
    c = case("A")
    x, ll, diag, info, _ = plan_decode(H, c, product_sm(H, c), fused=True)
    assert info["engine"] == H.ENGINE_WAVE
    accept("A wave decode_estep (%d chains)" % info["nchains"], c, x, ll)
    assert diag[0] == 0 and diag[7] == 0, diag


def test_batched_plan_at_10M(H):
    """A and B as the two channels of one batched plan (per-channel models of one shape)"""
    import torch
    cs = [case("A"), case("B")]
    sms = [product_sm(H, c) for c in cs]
    T = len(cs[0]["y"])
    plan = H.Plan.batched(T, sms, [c["mu"] for c in cs], [c["sigma"] for c in cs])
    try:
        dy = torch.from_numpy(np.stack([c["y"] for c in cs])).cuda()
        dx = torch.zeros((2, T), dtype=torch.int16, device="cuda")
        dll = torch.zeros(2, dtype=torch.float64, device="cuda")
        plan.viterbi(dy, dx, dll)
        diag = plan.diagnostics()
        torch.cuda.synchronize()
        x, ll = dx.cpu().numpy(), dll.cpu().numpy()
    finally:
        plan.close()
    for i, c in enumerate(cs):
        accept("%s channel %d of a batched plan" % (c["name"], i), c, x[i], float(ll[i]))
    assert diag[0] == 0 and diag[7] == 0, diag


# ---- ring models on the wave engine -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["C03odd", "C10odd"])
def test_many_short_chains(H, name):
    """block 512 / halo 256 at 1 000 001 samples: ~2 000 short chains and a ragged end"""
    c = case(name)
    H.set_option("block", 512)
    H.set_option("halo", 256)
    x, ll, diag, info, _ = plan_decode(H, c, product_sm(H, c))
    assert info["engine"] == H.ENGINE_WAVE and info["nchains"] >= 1900, info
    accept("%s wave (%d chains)" % (name, info["nchains"]), c, x, ll)
    assert diag[0] == 0 and diag[7] == 0, diag


@pytest.mark.parametrize("name", ["D", "E", "F"])
def test_wave_engine_on_auto(H, name):
    """8 x 128 and 16 x 256 (configs 4, 5); F: a recording cut by both edges (first-sample rule, final arg-max)"""
    c = case(name)
    x, ll, diag, info, _ = plan_decode(H, c, product_sm(H, c))
    assert info["engine"] == H.ENGINE_WAVE, info
    if name == "F":
        assert c["ref"].x[0] > 1 and c["ref"].x[-1] > 1        # the reference starts and ends inside spikes
    accept("%s wave on AUTO (%d chains)" % (name, info["nchains"]), c, x, ll)
    assert diag[0] == 0 and diag[7] == 0, diag


def test_duplicate_templates_at_2M(H):
    """templates 1 = 2: every spike of theirs is an exact tie that list order settles; rules 2 and 5, no cap"""
    c = case("DUP")
    x, ll, diag, info, _ = plan_decode(H, c, product_sm(H, c))
    accept("DUP on AUTO (engine %d)" % info["engine"], c, x, ll)
    assert diag[7] == 0, diag


# ---- overlap models on the blocked engine -----------------------------------------------------------------------

def overlap_decode(H, c, mode, want, monkeypatch):
    if mode == "generic":
        monkeypatch.setenv("HMMSORT_PAIR", "0")
    x, ll, diag, info, sweep = plan_decode(H, c, product_sm(H, c))
    assert info["engine"] == H.ENGINE_BLOCKED, info
    assert sweep == (want if mode != "generic" else 0), sweep      # the sweep under test is the one that runs
    if c["name"] != "H":                        # (H's signal has no injected overlaps and its reference path none)
        assert np.count_nonzero(c["ref"].x > 1 + c["N"] * (c["K"] - 1)) > 0     # overlap states on the reference path
    accept("%s blocked, %s sweep" % (c["name"], mode), c, x, ll)
    assert diag[0] == 0 and diag[7] == 0, diag


@pytest.mark.parametrize("mode", ["pair", "generic"])
@pytest.mark.parametrize("name", ["H", "P60"])
def test_pair_models(H, name, mode, monkeypatch):
    overlap_decode(H, case(name), mode, 2, monkeypatch)


@pytest.mark.parametrize("mode", ["multi", "generic"])
@pytest.mark.parametrize("name", ["M3", "CLI"])
def test_multi_models(H, name, mode, monkeypatch):
    c = case(name)
    if name == "CLI":
        assert c["osm"].nstates == 21123
    overlap_decode(H, c, mode, c["N"], monkeypatch)


# ---- chunked decode ---------------------------------------------------------------------------------------------

def test_chunked_fit_against_reference_per_chunk(H):
    """fit(..., 100 000) on C03odd: the reference decodes each chunk and stitches by the reference implementation's
    own rule (fit.jl:11-42: a chunk's leading non-silent samples are skipped, its trailing ones handed to the next
    chunk, which restarts at the last silent sample).  The device's samples of a chunk's kept range are put into the
    chunk's reference path and that path is judged by the acceptance rule on the chunk's own signal (~10 s of
    reference time, computed live)."""
    from oracle import hp
    c = case("C03odd")
    sm = product_sm(H, c)
    y, n, cs = c["y"], len(c["y"]), 100_000
    fitted = H.fit(H.HMMSpikeTemplateModel(sm, c["mu"], c["sigma"]), y, chunksize=cs)
    i = j = 1                                   # 1-based, as fit.jl counts
    ll_ref, nchunks, ndiff, worst = hp.LD(0), 0, 0, 0.0
    stitched = np.ones(n, np.int64)
    while j < n:
        j = min(i + cs - 1, n)
        k, l = j - i + 1, 1
        yc = y[i - 1:j]
        ref = VR.Ref.live(yc, c["osm"], c["mu"], c["sigma"])
        x = ref.x
        if i > 1:
            while x[l - 1] > 1:
                l += 1
        if j < n:
            while x[k - 1] > 1:
                j -= 1
                k -= 1
        assert j > i, "chunk without a silent sample"
        stitched[i + l - 2:j] = x[l - 1:k]
        spliced = x.copy()
        spliced[l - 1:k] = fitted.ml_seq[i + l - 2:j]
        model = hp._Model(c["osm"], c["mu"], c["sigma"])
        assert hp.path_is_valid(model, spliced), "chunk %d: the device's samples do not fit the chunk's reference path" % nchunks
        runs = hp.compare_paths(yc, model, None, None, x, spliced, ref.idx, ref.cum, ref.dmax)
        nd, w, over, beaten = hp.judge(runs)
        assert not beaten and not over, (nchunks, [(r.s, r.e, r.delta, r.tau) for r in over + beaten][:5])
        ndiff, worst = ndiff + nd, max(worst, w)
        ll_ref += ref.ll
        nchunks += 1
        i = j
    ell = abs(float(hp.LD(fitted.ll) - ll_ref)) / abs(float(ll_ref))
    print("C03odd fit(chunksize=%d): %d chunks   differing samples %d   largest Delta/tau %.3g   ll error %.3g   "
          "samples outside the stitched reference %d" % (cs, nchunks, ndiff, worst, ell,
                                                         int(np.count_nonzero(stitched != fitted.ml_seq))), flush=True)
    assert nchunks >= 10 and ndiff <= VR.CAP * n
    assert np.count_nonzero(stitched != fitted.ml_seq) == ndiff      # skipped sections and seams are the reference's
    assert ell <= VR.LL_RTOL
