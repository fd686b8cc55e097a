"""Blocked engine (csrc/generic_blocked.hip): the strict Viterbi recursion run time-parallel over an
arbitrary transition list -- the overlap-resolving models of reference types.jl:78-90 that the
reference's decode path uses (hmmsort.jl:54, test/runtests.jl:24).  Bar: path bit-identical to the
oracle, ll within 1e-9 relative (per-block partial sums are combined in a different order)."""
import numpy as np
import pytest

from conftest import to_oracle_sm

pytestmark = pytest.mark.gpu
LL_RTOL = 1e-9


@pytest.fixture(autouse=True)
def _engine(H):
    H.set_option("engine", H.ENGINE_BLOCKED)
    H.set_option("block", 0)
    H.set_option("halo", 0)
    yield
    H.set_option("engine", H.ENGINE_AUTO)
    H.set_option("block", 0)
    H.set_option("halo", 0)
    H.set_option("escalate", 1)


def _templates(H, K, n):
    par = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)][:n]
    return np.asfortranarray(np.stack([H.create_spike_template(K, a, b, c) for a, b, c in par], 1))


def _check(O, H, y, sm, temps, sigma):
    x, ll = H.viterbi(y, sm, temps, sigma)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, sigma)
    assert np.array_equal(x, xo)
    assert abs(ll - llo) <= LL_RTOL * abs(llo)
    return x


def test_reference_viterbi_test_shape(O, H):
    # test/runtests.jl:17-34: two templates, K=60, overlaps on (3600 states), 20 000 samples
    temps = _templates(H, 60, 2)
    pp = [0.003, 0.001]
    sm = H.StateMatrix.create(2, 60, np.log(pp), True)
    y = H.create_signal(20000, 0.3, pp, temps, seed=11)
    y[5000:5060] += temps[:, 0]; y[5020:5080] += temps[:, 1]      # an overlapping pair
    x = _check(O, H, y, sm, temps, 0.3)
    assert H.get_option("last_escalations") == 0
    assert x.max() > 1 + 2 * 59                                      # pair states decoded
    # AUTO picks the blocked engine for overlap models of this length
    H.set_option("engine", H.ENGINE_AUTO)
    from hmmsort_amd import device
    p = device.Plan(len(y), sm, temps, 0.3)
    info = p.info()
    assert info["engine"] == H.ENGINE_BLOCKED and info["nchains"] > 1 and info["halo"] >= 256
    p.close()


def blocked_dispatch(H, plan):
    """the kernels a decode of this blocked plan launches, as the library names them (the undeclared test aid
    hmmsort_selftest_blocked_dispatch; csrc/generic_blocked.hip, blocked_pick)"""
    import ctypes as C
    fn = H._lib.lib().hmmsort_selftest_blocked_dispatch
    fn.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    fn.restype = C.c_int
    buf = C.create_string_buffer(256)
    assert fn(plan._h, buf, len(buf)) == 0
    return buf.value.decode()


# Every shape here has K <= 64 and two to five templates, so by default it runs a structured sweep (pair_vit_block for
# two templates, multi_vit_block for three and four) and the generic sweep only with HMMSORT_PAIR=0, which is what the
# host ladder drops to after a near-tie.  Both are decoded and each mode asserts the kernels the library says it runs:
# (3, 20) and (2, 33): two states per lane, wave-specialised; (4, 12): one state per lane; (3, 58), 9 919 states, and
# (4, 40), 9 283: one LDS column updated in place, ten states per thread; (4, 45): 11 793 states, twelve per thread;
# (4, 48): 13 443 states, columns in global memory with the constants in registers, 14 per thread; (4, 56): 18 371
# states, the same with 21 per thread.  All walk back by segments and sum ll from LDS.
OVERLAP_SHAPES = {   # (N, K): structured sweep, generic sweep
    (3, 20): ("multi<3>", "gen_vit_block<2,true,false,true>"),
    (2, 33): ("pair", "gen_vit_block<2,true,false,true>"),
    (4, 12): ("multi<4>", "gen_vit_block<1,true,false,true>"),
    (3, 58): ("multi<3>", "gen_vit_block1<10>"),
    (4, 40): ("multi<4>", "gen_vit_block1<10>"),
    (4, 45): ("multi<4>", "gen_vit_block1<12>"),
    (4, 48): ("multi<4>", "gen_vit_blockG<14>"),
    (4, 56): ("multi<4>", "gen_vit_blockG<21>")}


@pytest.mark.parametrize("N,K,T", [(3, 20, 30011), (2, 33, 4097), (4, 12, 25000), (3, 58, 9000),
                                   (4, 40, 6000), (4, 45, 5000), (4, 48, 5000), (4, 56, 3000 + 4096)])
def test_overlap_shapes(O, H, N, K, T, monkeypatch):
    import torch
    structured, generic = OVERLAP_SHAPES[N, K]
    temps = _templates(H, K, N)
    pp = [0.01, 0.006, 0.008, 0.005][:N]
    sm = H.StateMatrix.create(N, K, np.log(pp), True)
    y = H.create_signal(T, 0.3, pp, temps, seed=5 + N)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    # default: the host-buffer entry point, as before, on the structured sweep
    plan = H.Plan(T, sm, temps, 0.3)
    assert blocked_dispatch(H, plan) == "sweep=%s backtrace=seg ll=lds" % structured
    assert plan.overlap_sweep() == (N if N > 2 else 2)
    plan.close()
    x, ll = H.viterbi(y, sm, temps, 0.3)
    assert np.array_equal(x, xo)
    assert abs(ll - llo) <= LL_RTOL * abs(llo)
    assert H.get_option("last_escalations") == 0
    # the generic sweep on the same input (plan API: no ladder that could end on another engine)
    H.shutdown()
    monkeypatch.setenv("HMMSORT_PAIR", "0")
    st = torch.cuda.current_stream().cuda_stream
    plan = H.Plan(T, sm, temps, 0.3)
    assert blocked_dispatch(H, plan) == "sweep=%s backtrace=seg ll=lds" % generic
    assert plan.overlap_sweep() == 0
    dx = torch.zeros(T, dtype=torch.int16, device="cuda")
    dll = torch.full((1,), np.nan, dtype=torch.float64, device="cuda")
    plan.viterbi(torch.from_numpy(y).cuda(), dx, dll, st)
    d = plan.diagnostics(st)
    plan.close()
    monkeypatch.delenv("HMMSORT_PAIR", raising=False)
    assert d[0] == 0, d
    nbad = int(np.count_nonzero(dx.cpu().numpy() != xo))
    assert nbad == 0, "generic sweep: path differs at %d samples (diag %s)" % (nbad, d)
    assert abs(float(dll.cpu()[0]) - llo) <= LL_RTOL * abs(llo)


def test_ring_model_through_blocked_engine(O, H):
    temps = _templates(H, 40, 2)
    pp = [0.01, 0.005]
    sm = H.StateMatrix.create(2, temps.shape[0], np.log(pp), False)
    y = H.create_signal(50000, 0.3, pp, temps, seed=3)
    _check(O, H, y, sm, temps, 0.3)


def test_short_blocks_and_ragged_tail(O, H):
    temps = _templates(H, 16, 2)
    pp = [0.01, 0.01]
    sm = H.StateMatrix.create(2, 16, np.log(pp), True)
    y = H.create_signal(6000 + 37, 0.3, pp, temps, seed=9)
    H.set_option("block", 128)
    H.set_option("halo", 128)
    _check(O, H, y, sm, temps, 0.3)


def test_warmup_too_short_is_flagged_and_escalated(O, H):
    temps = _templates(H, 60, 2)
    pp = [0.02, 0.02]
    sm = H.StateMatrix.create(2, 60, np.log(pp), True)
    y = H.create_signal(20000, 0.3, pp, temps, seed=13)
    H.set_option("block", 256)
    H.set_option("halo", 64)          # shorter than one spike: the certificate must notice
    H.set_option("engine", H.ENGINE_AUTO)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    x, ll = H.viterbi(y, sm, temps, 0.3)
    assert H.get_option("last_escalations") >= 1
    assert np.array_equal(x, xo) and abs(ll - llo) <= LL_RTOL * abs(llo)
    from hmmsort_amd import device
    import torch
    p = device.Plan(len(y), sm, temps, 0.3)
    dy = torch.from_numpy(y).cuda()
    dx = torch.zeros(len(y), dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    p.viterbi(dy, dx, dll)
    torch.cuda.synchronize()
    d = p.diagnostics()
    assert d[0] > 0 and d[2] > 1e-6
    p.close()


def test_set_model_on_a_blocked_plan(O, H):
    import torch
    from hmmsort_amd import device
    temps = _templates(H, 30, 2)
    pp = [0.008, 0.004]
    sm = H.StateMatrix.create(2, 30, np.log(pp), True)
    y = H.create_signal(40000, 0.3, pp, temps, seed=21)
    p = device.Plan(len(y), sm, temps, 0.3)
    dy = torch.from_numpy(y).cuda()
    dx = torch.zeros(len(y), dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    p.viterbi(dy, dx, dll)
    x1 = dx.cpu().numpy().copy()
    # new model of the same shape: other firing rates, scaled templates, other sigma
    pp2 = [0.002, 0.012]
    sm2 = H.StateMatrix.create(2, 30, np.log(pp2), True)
    t2 = np.asfortranarray(temps * 0.8)
    p.set_model(sm2, t2, 0.35)
    p.viterbi(dy, dx, dll)
    torch.cuda.synchronize()
    x2, ll2 = dx.cpu().numpy(), float(dll.cpu()[0])
    xo1, _ = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    xo2, llo2 = O.viterbi(y, to_oracle_sm(O, sm2), t2, 0.35)
    assert np.array_equal(x1, xo1) and np.array_equal(x2, xo2)
    assert abs(ll2 - llo2) <= LL_RTOL * abs(llo2)
    assert p.diagnostics()[0] == 0
    p.close()


def test_arbitrary_lists(O, H):
    # the engines take the caller's list as it is (StateMatrix is a plain container, types.jl:1-9)
    rng = np.random.default_rng(4)
    # (a) a hub: every state reaches state 1 and state 1 reaches every state -> in-degree 320, which
    #     the blocked sweep refuses; AUTO must fall back to the op-for-op single sweep
    S, T = 320, 5000
    states = np.asfortranarray(np.arange(1, S + 1, dtype=np.int16)[None, :])
    tr = ([(1, j, np.log(1.0 / S)) for j in range(1, S + 1)] + [(j, 1, np.log(0.5)) for j in range(2, S + 1)]
          + [(j, j, np.log(0.5)) for j in range(2, S + 1)])
    tr.sort(key=lambda e: (e[0], e[1]))             # reference order: source-major, destination ascending
    sm = H.StateMatrix(states, np.array(tr, dtype=H._lib.TRANS_DTYPE), np.zeros(S), S, 1, S, False)
    mu = np.asfortranarray(rng.normal(0, 2, (S, 1)))
    y = rng.normal(0, 1, T) + mu[rng.integers(0, S, T) // 40 * 40, 0]
    H.set_option("engine", H.ENGINE_AUTO)
    _check(O, H, y, sm, mu, 0.8)
    from hmmsort_amd import device
    p = device.Plan(T, sm, mu, 0.8)
    assert p.info()["engine"] == H.ENGINE_STRICT
    p.close()
    # (b) a sparse random graph with in-degree <= 6 and some unreachable states: blocked sweep
    S = 700
    tr = []
    for j in range(1, S + 1):
        for d in sorted(set(rng.integers(1, S - 50 + 1, 3).tolist() + [min(j + 1, S)])):
            tr.append((j, int(d), float(np.log(rng.uniform(0.05, 0.5)))))
    tr.sort(key=lambda e: (e[0], e[1]))
    states = np.asfortranarray(np.arange(1, S + 1, dtype=np.int16)[None, :])
    sm = H.StateMatrix(states, np.array(tr, dtype=H._lib.TRANS_DTYPE), np.zeros(S), S, 1, S, False)
    mu = np.asfortranarray(rng.normal(0, 1.5, (S, 1)))
    y = rng.normal(0, 1, 9000)
    p = device.Plan(len(y), sm, mu, 0.7)
    assert p.info()["engine"] == H.ENGINE_BLOCKED
    p.close()
    _check(O, H, y, sm, mu, 0.7)


def test_golden_overlap_fixture_through_blocked_engine(H):
    # committed vectors (tests/golden/n2k16_ov.npz, made by make_golden.py from the oracle):
    # no oracle call here -- the decode is compared with the stored path and ll
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "n2k16_ov.npz"))
    N, K = int(g["N"]), int(g["K"])
    sm = H.StateMatrix.create(N, K, np.log(g["pp"]), True)
    assert np.array_equal(sm.transitions["src"], g["src"]) and np.array_equal(sm.transitions["lp"], g["val"])
    x, ll = H.viterbi(g["y"], sm, np.asfortranarray(g["temps"]), 0.3)
    assert H.get_option("last_escalations") == 0
    assert np.array_equal(x, g["x"]) and abs(ll - float(g["ll"])) <= LL_RTOL * abs(float(g["ll"]))


def test_duplicate_templates_near_ties_are_detected(O, H):
    # two pairs of identical templates with identical rates in an overlap model: whole families of
    # candidates differ by rounding only.  The blocks' additive frames can then separate what the
    # reference rounds to a tie (and resolves by list order): such blocks are counted in diag[7] and
    # the host-buffer entry point decodes with the strict engine (found by scripts/fuzz_gpu.py with
    # FUZZ_TIES=1: 902 samples differed on this kind of input before the check existed)
    K, N, T = 23, 4, 31_099
    base = _templates(H, K, 2)
    temps = np.asfortranarray(np.stack([base[:, 0], base[:, 0], base[:, 1], base[:, 1]], 1))
    pp = [0.004, 0.004, 0.003, 0.003]
    sm = H.StateMatrix.create(N, K, np.log(pp), True)
    for seed in (1, 2, 3):
        y = H.create_signal(T, 0.28, pp, temps, seed=seed)
        H.set_option("engine", H.ENGINE_AUTO)
        H.set_option("block", 512)
        H.set_option("halo", 256)
        x, ll = H.viterbi(y, sm, temps, 0.28)
        xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.28)
        assert np.array_equal(x, xo) and abs(ll - llo) <= LL_RTOL * abs(llo)


# ---- two-template overlap models: the sweep that treats pair runs as delays (csrc/pair_sweep.hip) ----------

def _pair_case(H, K, T, seed, silent_mean=(0.0, 0.0), amp=(3.0, 4.0)):
    t1 = H.create_spike_template(K, amp[0], 0.8, 0.2)
    t2 = H.create_spike_template(K, amp[1], 0.3, 0.2)
    temps = np.asfortranarray(np.stack([t1, t2], 1))
    pp = [0.003, 0.0015]
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    rng = np.random.default_rng(seed)
    L = K - 1
    for _ in range(max(4, T // 4000)):                      # overlapping pairs at random offsets, both orders
        t0 = int(rng.integers(L, T - 3 * L))
        d = int(rng.integers(0, L))
        a, b = (0, 1) if rng.random() < 0.5 else (1, 0)
        y[t0:t0 + L] += temps[1:, a]
        y[t0 + d:t0 + d + L] += temps[1:, b]
    mu = temps.copy(order="F")
    mu[0, :] = silent_mean
    sm = H.StateMatrix.create(2, K, np.log(pp), True)
    return y, sm, mu


@pytest.mark.parametrize("K,T,seed,silent_mean,sigma", [
    (60, 60_000, 1, (0.0, 0.0), 0.3),
    (60, 300_000, 2, (0.02, -0.01), 0.35),       # nonzero silent means: deviations from the silent state's mean
    (64, 40_000, 3, (0.0, 0.0), 0.25),           # longest ring the sweep takes (63 phases)
    (20, 30_000, 4, (0.0, 0.0), 0.3),
    (5, 8_000, 5, (0.0, 0.0), 0.3),
    (3, 5_000, 6, (0.0, 0.0), 0.3),              # two phases per ring
    (33, 4_099, 7, (0.0, 0.0), 0.3),             # barely above the blocked engine's minimum length
])
def test_pair_sweep_equals_oracle_and_generic_sweep(O, H, K, T, seed, silent_mean, sigma, monkeypatch):
    import torch
    y, sm, mu = _pair_case(H, K, T, seed, silent_mean)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), mu, sigma)
    assert np.count_nonzero(xo > 1 + 2 * (K - 1)) > 0                      # pair states on the path
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for mode in ("pair", "generic"):
        if mode == "generic":
            monkeypatch.setenv("HMMSORT_PAIR", "0")
        plan = H.Plan(T, sm, mu, sigma)
        assert plan.overlap_sweep() == (2 if mode == "pair" else 0)
        dy = torch.from_numpy(y).cuda()
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(dy, dx, dll, st)
        res[mode] = (dx.cpu().numpy(), float(dll.cpu()[0]), plan.diagnostics(st))
        plan.close()
    monkeypatch.delenv("HMMSORT_PAIR", raising=False)
    for mode, (x, ll, d) in res.items():
        assert d[0] == 0, (mode, d)                                         # every block boundary certified
        nbad = int(np.count_nonzero(x != xo))
        assert nbad == 0, "%s sweep: path differs at %d samples, first at %d (diag %s)" % (
            mode, nbad, int(np.argmax(x != xo)), d)
        assert abs(ll - llo) <= LL_RTOL * abs(llo)
    assert res["pair"][2][7] == 0, res["pair"][2]                           # no near-tie on the decoded path


def test_pair_sweep_duplicate_templates_fall_back(O, H):
    # twins: every spike is a tie that only the reference's operation order settles; the pair sweep flags the
    # decisions on the path, hmmsort_viterbi decodes again with the generic blocked sweep and then the strict engine
    K, T = 30, 30_000
    t1 = H.create_spike_template(K, 3.0, 0.8, 0.2)
    temps = np.asfortranarray(np.stack([t1, t1], 1))
    pp = [0.004, 0.004]
    sm = H.StateMatrix.create(2, K, np.log(pp), True)
    y = H.create_signal(T, 0.3, pp, temps, seed=9)
    H.set_option("engine", H.ENGINE_AUTO)
    x, ll = H.viterbi(y, sm, temps, 0.3)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    assert H.get_option("last_escalations") >= 1
    assert np.array_equal(x, xo) and abs(ll - llo) <= LL_RTOL * abs(llo)


# ---- three to five templates: tracks per neuron, pair runs as delays (csrc/multi_sweep.hip) ----
def _multi_case(H, N, K, T, seed, silent_mean=0.0):
    rng = np.random.default_rng(seed)
    shapes = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15), (2.0, 0.4, 0.3)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *shapes[i]) for i in range(N)], 1))
    pp = [0.004, 0.002, 0.003, 0.0025, 0.002][:N]
    pp = [p * min(1.0, 30.0 / K) for p in pp]
    y = H.create_signal(T, 0.3, pp, temps, seed=seed)
    L = K - 1
    for _ in range(max(6, T // 3000)):          # overlapping pairs at random offsets, a third spike as the first ends
        t0 = int(rng.integers(L, T - 4 * L))
        d = int(rng.integers(0, L))
        a, b = rng.choice(N, 2, replace=False)
        y[t0:t0 + L] += temps[1:, a]
        y[t0 + d:t0 + d + L] += temps[1:, b]
        if rng.random() < 0.5:
            c = int(rng.choice([q for q in range(N) if q != a]))
            y[t0 + L:t0 + 2 * L] += temps[1:, c]
    mu = temps.copy(order="F")
    mu[0, :] = silent_mean
    sm = H.StateMatrix.create(N, K, np.log(pp), True)
    return y, sm, mu


@pytest.mark.parametrize("N,K,T,seed,silent_mean,sigma", [
    (3, 12, 30_000, 1, 0.0, 0.3),
    (3, 25, 20_000, 2, 0.01, 0.35),              # nonzero silent means
    (4, 16, 24_000, 3, 0.0, 0.3),
    (4, 9, 12_000, 4, 0.0, 0.25),
    (5, 10, 12_000, 5, 0.0, 0.3),
    (3, 3, 6_000, 6, 0.0, 0.3),                  # two phases per ring
    (4, 20, 4_099, 7, 0.0, 0.2),                 # barely above the blocked engine's minimum length; sigma < 0.4: the
                                                 # path starts in a state whose deviation is ~0 (exact first decisions)
])
def test_multi_sweep_equals_oracle_and_generic_sweep(O, H, N, K, T, seed, silent_mean, sigma, monkeypatch):
    import torch
    y, sm, mu = _multi_case(H, N, K, T, seed, silent_mean)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), mu, sigma)
    assert np.count_nonzero(xo > 1 + N * (K - 1)) > 0                      # pair states on the path
    st = torch.cuda.current_stream().cuda_stream
    res = {}
    for mode in ("multi", "generic"):
        if mode == "generic":
            monkeypatch.setenv("HMMSORT_PAIR", "0")
        plan = H.Plan(T, sm, mu, sigma)
        assert plan.overlap_sweep() == (N if mode == "multi" else 0)         # the sweep under test is the one that runs
        dy = torch.from_numpy(y).cuda()
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(dy, dx, dll, st)
        res[mode] = (dx.cpu().numpy(), float(dll.cpu()[0]), plan.diagnostics(st))
        plan.close()
    monkeypatch.delenv("HMMSORT_PAIR", raising=False)
    for mode, (x, ll, d) in res.items():
        assert d[0] == 0, (mode, d)
        nbad = int(np.count_nonzero(x != xo))
        assert nbad == 0, "%s sweep: path differs at %d samples, first at %d (diag %s)" % (
            mode, nbad, int(np.argmax(x != xo)), d)
        assert abs(ll - llo) <= LL_RTOL * abs(llo)
    assert res["multi"][2][7] == 0, res["multi"][2]                         # no near-tie on the decoded path


def test_multi_sweep_cli_shape_equals_generic_sweep(H, monkeypatch):
    # the largest model the reference's CLI builds (hmmsort.jl:50-54): 4 templates, K = 60, 21 123 states; the CPU
    # oracle needs minutes here, the checker is the generic blocked sweep (itself oracle-checked above)
    import torch
    N, K, T = 4, 60, 400_000
    y, sm, mu = _multi_case(H, N, K, T, 11)
    assert sm.nstates == 21123
    st = torch.cuda.current_stream().cuda_stream
    dy = torch.from_numpy(y).cuda()
    res = {}
    for mode in ("multi", "generic"):
        if mode == "generic":
            monkeypatch.setenv("HMMSORT_PAIR", "0")
        plan = H.Plan(T, sm, mu, 0.3)
        assert plan.overlap_sweep() == (4 if mode == "multi" else 0)
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(dy, dx, dll, st)
        res[mode] = (dx.cpu().numpy(), float(dll.cpu()[0]), plan.diagnostics(st))
        plan.close()
    monkeypatch.delenv("HMMSORT_PAIR", raising=False)
    assert res["multi"][2][0] == 0 and res["multi"][2][7] == 0 and res["generic"][2][7] == 0, res
    assert np.array_equal(res["multi"][0], res["generic"][0])
    assert np.count_nonzero(res["multi"][0] > 1 + N * (K - 1)) > 0
    assert abs(res["multi"][1] - res["generic"][1]) <= LL_RTOL * abs(res["generic"][1])


def test_multi_sweep_duplicate_templates_fall_back(O, H):
    # twins among three templates: ties that only the reference's operation order settles are flagged on the path and
    # hmmsort_viterbi decodes again with the generic sweep / the strict engine
    K, T = 14, 20_000
    t1 = H.create_spike_template(K, 3.0, 0.8, 0.2)
    t2 = H.create_spike_template(K, 4.0, 0.3, 0.2)
    temps = np.asfortranarray(np.stack([t1, t2, t1], 1))
    pp = [0.004, 0.003, 0.004]
    sm = H.StateMatrix.create(3, K, np.log(pp), True)
    y = H.create_signal(T, 0.3, pp, temps, seed=9)
    H.set_option("engine", H.ENGINE_AUTO)
    x, ll = H.viterbi(y, sm, temps, 0.3)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    assert H.get_option("last_escalations") >= 1
    assert np.array_equal(x, xo) and abs(ll - llo) <= LL_RTOL * abs(llo)


def test_segment_backtrace_repairs_wrong_guesses(O, H, monkeypatch):
    # the backtrace by segments (k_seg_walk) guesses each segment's last state from a walk-in; with a walk-in of ONE
    # sample most guesses inside spikes are wrong and k_seg_fix has to re-walk those segments from the true state:
    # the path must still be the oracle's, with every boundary consistent (diag[0] == 0)
    import torch
    y, sm, mu = _multi_case(H, 3, 20, 40_000, 21)
    xo, llo = O.viterbi(y, to_oracle_sm(O, sm), mu, 0.3)
    st = torch.cuda.current_stream().cuda_stream
    monkeypatch.setenv("HMMSORT_SEG_WI", "1")
    plan = H.Plan(len(y), sm, mu, 0.3)
    dy = torch.from_numpy(y).cuda()
    dx = torch.zeros(len(y), dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    plan.viterbi(dy, dx, dll, st)
    d = plan.diagnostics(st)
    assert d[0] == 0, d
    assert np.array_equal(dx.cpu().numpy(), xo)
    # without fix passes the wrong guesses stay: they must be COUNTED (diag[0]), never silently returned ...
    monkeypatch.setenv("HMMSORT_SEG_PASSES", "0")
    plan.viterbi(dy, dx, dll, st)
    d0 = plan.diagnostics(st)
    plan.close()
    assert d0[0] > 0, d0
    # ... and the host-buffer entry point then falls back to an engine that needs no guess
    H.set_option("engine", H.ENGINE_AUTO)
    x, ll = H.viterbi(y, sm, mu, 0.3)
    assert np.array_equal(x, xo) and abs(ll - llo) <= LL_RTOL * abs(llo)
    assert H.get_option("last_escalations") >= 1


@pytest.mark.parametrize("N,first", [(3, 0), (4, 1), (4, 3), (2, 1)])
def test_overlap_sweeps_first_decisions(O, H, N, first):
    # a spike that starts at the SECOND sample of a recording: its first state is decided among Z, every A_l(L) and
    # every P(l:L, l':L) of the first column (emission only, viterbi.jl:55-63), candidates that tie to the last bit;
    # the structured sweeps take these decisions in the reference's own arithmetic (a fuzz case found lanes of the
    # junction reduction working on stale operands here: path wrong at sample 1, nothing flagged)
    import torch
    K, T, sigma = 24, 6_000, 0.36
    shapes = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *shapes[i]) for i in range(N)], 1))
    pp = [0.004, 0.006, 0.003, 0.005][:N]
    sm = H.StateMatrix.create(N, K, np.log(pp), True)
    st = torch.cuda.current_stream().cuda_stream
    for y0 in (0.18, 0.05, -0.3):
        y = H.create_signal(T, sigma, pp, temps, seed=77 + first)
        y[:K + 2] = 0.01
        y[0] = y0
        y[1:K] += temps[1:, first]
        xo, llo = O.viterbi(y, to_oracle_sm(O, sm), temps, sigma)
        plan = H.Plan(T, sm, temps, sigma)
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(torch.from_numpy(y).cuda(), dx, dll, st)
        d = plan.diagnostics(st)
        plan.close()
        x = dx.cpu().numpy()
        assert d[0] == 0
        assert d[7] > 0 or np.array_equal(x, xo), (y0, x[:4], xo[:4], d)
        assert np.array_equal(x[:3], xo[:3]) or d[7] > 0, (y0, x[:4], xo[:4])
