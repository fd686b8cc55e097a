"""Every row of the blocked engine's generic Viterbi dispatch (csrc/generic_blocked.hip, blocked_pick) against the
CPU oracle: one case per kernel instantiation a decode can be sent to -- the sweep (gen_vit_block<SPT,SPEC,GCOL,TLDS>,
gen_vit_block1<SPT>, gen_vit_blockG<SPT>), the backtrace (by segments or by block maps) and the ll sum (partial sums
staged in LDS or read from global memory).

The row is never worked out here: the library says which kernels a plan launches (the undeclared test aid
hmmsort_selftest_blocked_dispatch, read before the decode) and each case asserts that answer by name, so a shape that
drifts to another row after a change of thresholds fails instead of silently testing something else.  If that happens,
move the shape, not the expectation.

Bars as in test_gpu_blocked.py: path equal to the oracle's, ll within 1e-9 relative, every boundary certified
(diag[0] == 0) and no near-tie block (diag[7] == 0).  Every case runs through the plan API on the blocked engine (no
ladder that could end on the strict engine), on 3 blocks + 37 samples of the plan's own geometry: at least four
blocks, a ragged last one, warm-ups that start at sample 0 and warm-ups that do not.  The warm-up is the first of
default, 2x, 4x that certifies, and is printed with the row, the number of blocks, the count of differing samples and
the ll error.  Rows no accepted model reaches are listed in DESIGN.md section 3.5."""
import ctypes as C

import numpy as np
import pytest

from conftest import to_oracle_sm
from test_gpu_blocked import LL_RTOL, _multi_case, blocked_dispatch as dispatch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _engine(H):
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option("block", 0)
    H.set_option("halo", 0)
    try:
        yield
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
        H.set_option("block", 0)
        H.set_option("halo", 0)
        H.shutdown()


def overlap_model(H, N, K):
    """(build(T) -> (y, sm, mu), sigma, last state that is no overlap state): create_signal plus injected overlapping pairs, rates
    scaled by min(1, 30 / K) (test_gpu_blocked._multi_case, which takes two templates as well)"""
    return (lambda T: _multi_case(H, N, K, T, seed=100 + N * K)), 0.3, 1 + N * (K - 1)


def list_model(H, S, nrandom, seed):
    """an arbitrary list as in test_arbitrary_lists (b): state j reaches j + 1 and `nrandom` random states, so about
    S (1 - exp(-nrandom)) states have several incoming transitions and about nrandom * S transitions are 'tails'
    (incoming transitions after a state's first); more than 256 distinct log-probabilities (no dictionary)"""
    rng = np.random.default_rng(seed)
    tr = []
    for j in range(1, S + 1):
        for d in sorted(set(rng.integers(1, S - 50 + 1, nrandom).tolist() + [min(j + 1, S)])):
            tr.append((j, int(d), float(np.log(rng.uniform(0.05, 0.5)))))
    tr.sort(key=lambda e: (e[0], e[1]))
    states = np.asfortranarray(np.arange(1, S + 1, dtype=np.int16)[None, :])
    sm = H.StateMatrix(states, np.array(tr, dtype=H._lib.TRANS_DTYPE), np.zeros(S), S, 1, S, False)
    mu = np.asfortranarray(rng.normal(0, 1.5, (S, 1)))
    return (lambda T: (np.random.default_rng(seed + 1).normal(0, 1, T), sm, mu)), 0.7, None


def hub_model(H, S, nhub, seed):
    """few states with several incoming transitions in a large list: `nhub` hubs (state 1 among them), every other
    state on a chain of 2 .. 10 states that leaves one hub and ends in another.  Rows of nhub back-pointers, state
    codes past what the block-map backtrace keeps as int32 in LDS."""
    rng = np.random.default_rng(seed)
    tr = []
    j = nhub + 1
    while j <= S:
        n = int(min(rng.integers(2, 11), S - j + 1))
        tr.append((int(rng.integers(1, nhub + 1)), j, float(np.log(rng.uniform(0.05, 0.5)))))
        for q in range(j, j + n - 1):
            tr.append((q, q + 1, float(np.log(rng.uniform(0.5, 1.0)))))
        tr.append((j + n - 1, int(rng.integers(1, nhub + 1)), float(np.log(rng.uniform(0.05, 0.5)))))
        j += n
    tr.sort(key=lambda e: (e[0], e[1]))
    indeg = np.bincount([e[1] for e in tr], minlength=S + 1)
    assert indeg[1:nhub + 1].min() >= 2 and indeg.max() <= 256 and (indeg[nhub + 1:] == 1).all()
    states = np.asfortranarray(np.arange(1, S + 1, dtype=np.int16)[None, :])
    sm = H.StateMatrix(states, np.array(tr, dtype=H._lib.TRANS_DTYPE), np.zeros(S), S, 1, S, False)
    mu = np.asfortranarray(rng.normal(0, 1.5, (S, 1)))
    return (lambda T: (np.random.default_rng(seed + 1).normal(0, 1, T), sm, mu)), 0.7, None


def comb_model(H, S, seed):
    """no state with more than one incoming transition: state 1 with its self-loop, and a chain 1 -> 2 -> ... -> S that
    never returns.  After S samples every state descends from state 1, so the blocks do forget their start (a cycle
    or a forest, the other lists without a multi-source state, never do).  The signal ends in the head of the
    chain's means: the path leaves state 1 once, late."""
    rng = np.random.default_rng(seed)
    tr = [(1, 1, float(np.log(0.99))), (1, 2, float(np.log(0.01)))] + [(j, j + 1, 0.0) for j in range(2, S)]
    states = np.asfortranarray(np.arange(1, S + 1, dtype=np.int16)[None, :])
    sm = H.StateMatrix(states, np.array(tr, dtype=H._lib.TRANS_DTYPE), np.zeros(S), S, 1, S, False)
    mu = np.asfortranarray(rng.normal(0, 1.5, (S, 1)))
    mu[0, 0] = 0.0

    def build(T):
        y = np.random.default_rng(seed + 1).normal(0, 0.7, T)
        y[T - 100:] += mu[1:101, 0]
        return y, sm, mu
    return build, 0.7, 1


# (id, model, HMMSORT_PAIR=0?, options, T or None for 3 blocks + 37, overlap_sweep(), the library's answer)
# Overlap models of two templates with K > 64 are refused by the structured sweeps and reach the generic sweep by
# default; smaller ones reach it with HMMSORT_PAIR=0 (what the host ladder does after a near-tie).  Lists have K = S,
# so their geometry is set by option: blocks of 1 024 samples, a warm-up of 512 (a host-side max-plus sweep of these
# graphs forgets its start within 256 to 512 samples).
LIST_GEOM = {"block": 1024, "halo": 512}
CASES = [
    ("2x20", lambda H: overlap_model(H, 2, 20), True, {}, None, 0,
     "sweep=gen_vit_block<1,true,false,true> backtrace=map<1> ll=lds"),
    ("2x33", lambda H: overlap_model(H, 2, 33), True, {}, None, 0,
     "sweep=gen_vit_block<2,true,false,true> backtrace=seg ll=lds"),
    ("2x45", lambda H: overlap_model(H, 2, 45), True, {}, None, 0,
     "sweep=gen_vit_block<2,false,false,true> backtrace=seg ll=lds"),
    ("2x50", lambda H: overlap_model(H, 2, 50), True, {}, None, 0,
     "sweep=gen_vit_block<4,false,false,true> backtrace=seg ll=lds"),
    ("2x70", lambda H: overlap_model(H, 2, 70), False, {}, None, 0,
     "sweep=gen_vit_block1<6> backtrace=seg ll=lds"),
    ("2x85", lambda H: overlap_model(H, 2, 85), False, {}, None, 0,
     "sweep=gen_vit_block1<8> backtrace=seg ll=lds"),
    ("2x95", lambda H: overlap_model(H, 2, 95), False, {}, None, 0,
     "sweep=gen_vit_block1<10> backtrace=seg ll=lds"),
    ("2x104", lambda H: overlap_model(H, 2, 104), False, {}, None, 0,
     "sweep=gen_vit_block1<11> backtrace=seg ll=lds"),
    ("2x109", lambda H: overlap_model(H, 2, 109), False, {}, None, 0,
     "sweep=gen_vit_block1<12> backtrace=seg ll=lds"),
    ("2x115", lambda H: overlap_model(H, 2, 115), False, {}, None, 0,
     "sweep=gen_vit_blockG<14> backtrace=seg ll=lds"),
    ("2x140", lambda H: overlap_model(H, 2, 140), False, {}, None, 0,
     "sweep=gen_vit_blockG<21> backtrace=seg ll=lds"),
    ("2x160", lambda H: overlap_model(H, 2, 160), False, {}, None, 0,
     "sweep=gen_vit_block<0,false,true,true> backtrace=seg ll=lds"),
    ("2x181-int16-limit", lambda H: overlap_model(H, 2, 181), False, {}, None, 0,      # 32 761 of 32 767 state ids
     "sweep=gen_vit_block<0,false,true,true> backtrace=seg ll=lds"),
    ("list4500-1", lambda H: list_model(H, 4500, 1, 31), False, LIST_GEOM, None, 0,     # > 1 024 multi-source states
     "sweep=gen_vit_block<0,false,false,true> backtrace=seg ll=lds"),
    ("list4500-3", lambda H: list_model(H, 4500, 3, 32), False, LIST_GEOM, None, 0,     # tails past the LDS test
     "sweep=gen_vit_block<0,false,false,false> backtrace=seg ll=lds"),
    ("list10000-2", lambda H: list_model(H, 10000, 2, 33), False, LIST_GEOM, None, 0,   # columns and tails in global memory
     "sweep=gen_vit_block<0,false,true,false> backtrace=seg ll=lds"),
    ("hubs26000", lambda H: hub_model(H, 26000, 48, 34), False, LIST_GEOM, None, 0,     # rows of 48 < 64 pointers
     "sweep=gen_vit_block<0,false,true,true> backtrace=map<2> ll=lds"),
    ("comb300", lambda H: comb_model(H, 300, 35), False, {"block": 512, "halo": 512}, None, 0,   # no multi-source state
     "sweep=gen_vit_block<1,false,false,true> backtrace=map<1> ll=lds"),
    ("2x12-2657-blocks", lambda H: overlap_model(H, 2, 12), True, {"block": 64, "halo": 64}, 170_037, 0,
     "sweep=gen_vit_block<1,true,false,true> backtrace=map<1> ll=global"),
]


def run_case(O, H, name, build, sigma, beyond, options, T_fixed, sweep, row):
    """decode on a blocked plan whose dispatch is `row`; the warm-up is the first of default, 2x, 4x that certifies"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    for k, v in options.items():
        H.set_option(k, v)
    y, sm, mu = build(4096)                         # the model does not depend on the length
    halo0 = None
    for widen in (1, 2, 4):
        if widen > 1:
            H.set_option("halo", widen * halo0)
        probe = H.Plan(4096, sm, mu, sigma)         # the geometry the options and the model give
        g = probe.info()
        probe.close()
        halo0 = halo0 or g["halo"]
        T = T_fixed or 3 * g["block"] + 37
        if len(y) != T:
            y, sm, mu = build(T)
            xo, llo = O.viterbi(y, to_oracle_sm(O, sm), mu, sigma)
        plan = H.Plan(T, sm, mu, sigma)
        info = plan.info()
        assert info["engine"] == H.ENGINE_BLOCKED and info["nchains"] >= 4, info
        got = dispatch(H, plan)                     # asked before the decode
        assert got == row, "%s: the library runs '%s', this case is meant to pin '%s': move the shape" % (name, got, row)
        assert plan.overlap_sweep() == sweep
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
        plan.viterbi(torch.from_numpy(y).cuda(), dx, dll, st)
        d = plan.diagnostics(st)
        x, ll = dx.cpu().numpy(), float(dll.cpu()[0])
        plan.close()
        if d[0] == 0:
            break
        print("%s: warm-up %d leaves %d boundaries uncertified, widening" % (name, info["halo"], d[0]), flush=True)
    nbad = int(np.count_nonzero(x != xo))
    print("%s: S=%d T=%d  %s  %d blocks of %d, warm-up %d (default %d)  differing samples %d  ll rel err %.3g  diag %s"
          % (name, sm.nstates, T, got, info["nchains"], info["block"], info["halo"], halo0, nbad,
             abs(ll - llo) / abs(llo), list(d)), flush=True)
    if beyond is not None:
        assert np.count_nonzero(xo > beyond) > 0                 # overlap states (the chain) on the oracle's path
    assert d[0] == 0, d                                           # every boundary certified
    assert d[7] == 0, d                                           # no near-tie block
    assert nbad == 0, "%s: path differs at %d samples, first at %d (diag %s)" % (name, nbad, int(np.argmax(x != xo)), d)
    assert abs(ll - llo) <= LL_RTOL * abs(llo)


@pytest.mark.parametrize("name,model,pair_off,options,T,sweep,row", CASES, ids=[c[0] for c in CASES])
def test_every_viterbi_dispatch_row_matches_oracle(O, H, monkeypatch, name, model, pair_off, options, T, sweep, row):
    if pair_off:
        monkeypatch.setenv("HMMSORT_PAIR", "0")
    else:
        monkeypatch.delenv("HMMSORT_PAIR", raising=False)
    build, sigma, beyond = model(H)
    run_case(O, H, name, build, sigma, beyond, options, T, sweep, row)


def test_dispatch_names_the_structured_sweeps(H):
    # pair and multi sweep by name, with the backtrace and ll sum they share with the generic sweep
    for N, K, want in ((2, 20, "sweep=pair backtrace=map<1> ll=lds"), (4, 12, "sweep=multi<4> backtrace=seg ll=lds")):
        _, sm, mu = _multi_case(H, N, K, 6000, seed=3)
        plan = H.Plan(6000, sm, mu, 0.3)
        assert plan.overlap_sweep() == (N if N > 2 else 2)
        assert dispatch(H, plan) == want
        plan.close()


def test_dispatch_refuses_other_engines(H):
    _, sm, mu = _multi_case(H, 2, 12, 6000, seed=3)
    H.set_option("engine", H.ENGINE_STRICT)
    plan = H.Plan(6000, sm, mu, 0.3)
    assert plan.info()["engine"] == H.ENGINE_STRICT
    fn = H._lib.lib().hmmsort_selftest_blocked_dispatch
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    fn.restype = C.c_int
    buf = C.create_string_buffer(256)
    assert fn(plan._h, buf, len(buf)) == H._lib.EINVAL
    assert fn(None, buf, len(buf)) == H._lib.EINVAL
    plan.close()
    H.set_option("engine", H.ENGINE_BLOCKED)
    plan = H.Plan(6000, sm, mu, 0.3)
    assert fn(plan._h, buf, 8) == H._lib.EINVAL                   # a buffer too small for the answer
    plan.close()
