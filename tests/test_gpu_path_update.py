"""Viterbi training on the device (csrc/path_update.hip): hmmsort_plan_path_update on every engine, the host entry
hmmsort_viterbi_step, and the Python layers on top (viterbi_step, train_model(method="viterbi"),
sort_data(refine_steps=...)).  The reference is the numpy model of path_update_model.py evaluated with math.fsum;
test_path_update_cpu.py ties that model to update() of baumwelch.jl:205-309.

Tolerances, for any order of summing:
  |mu'[k,l] - model| <= c[k,l] 2^-52 max|y| + one ulp of the quotient
  sigma' within 4 T 2^-52 relative; lp' within 8 ulp of log T (two logs of <= 2 ulp each side, one subtraction)
  pp' and the three counts exact."""
import ctypes as C
import math

import numpy as np
import pytest

import path_update_model as PU
from conftest import to_oracle_sm

pytestmark = pytest.mark.gpu

OPTIONS = dict(engine=0, block=0, halo=0, escalate=1)


@pytest.fixture(autouse=True)
def default_options(H):
    H.shutdown()
    for k, v in OPTIONS.items():
        H.set_option(k, v)
    try:
        yield
    finally:
        for k, v in OPTIONS.items():
            H.set_option(k, v)
        H.shutdown()


def split(o, K, N, S):
    nlp = len(o) - K * N - 1 - S
    return dict(mu=np.asfortranarray(o[:K * N].reshape((K, N), order="F")), sigma=float(o[K * N]),
                lp=o[K * N + 1:K * N + 1 + nlp].copy(), pp=o[K * N + 1 + nlp:].copy())


def plan_update(H, y, sm, mu, sigma, engine, x=None):
    """path update on a plan of `engine`: of the plan's own decode, or of the path x.  Returns the split output with
    counts, x, ll, the plan's engine and the raw output vector."""
    import torch
    H.set_option("engine", engine)
    try:
        plan = H.Plan(len(y), sm, mu, sigma)
    finally:
        H.set_option("engine", H.ENGINE_AUTO)
    try:
        T = len(y)
        dy = torch.from_numpy(np.ascontiguousarray(y)).cuda()
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        if x is None:
            dx = torch.zeros(T, dtype=torch.int16, device="cuda")
            plan.viterbi(dy, dx, dll)
            dg = plan.diagnostics()
            assert dg[0] == 0 and dg[7] == 0, dg
        else:
            dx = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int16)).cuda()
        out = torch.full((plan.mstep_len(),), np.nan, dtype=torch.float64, device="cuda")
        cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        plan.path_update(dy, dx, out, cnt)
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        r = split(o, sm.K, sm.N, sm.nstates)
        r.update(counts=cnt.cpu().numpy().tolist(), x=dx.cpu().numpy(), ll=float(dll.cpu()[0]),
                 engine=plan.info()["engine"], raw=o)
        return r
    finally:
        plan.close()


def check(r, m, y):
    """the library's result r against the model m (evaluated with exact=True)"""
    T = len(y)
    ymax = float(np.abs(y).max())
    bound = m["c"] * 2.0 ** -52 * ymax + np.spacing(np.abs(m["mu"]))
    err = np.abs(r["mu"] - m["mu"])
    assert np.all(err <= bound), (err.max(), np.argwhere(err > bound)[:4])
    assert np.all(r["mu"][0] == 0.0)
    assert abs(r["sigma"] - m["sigma"]) <= 4 * T * 2.0 ** -52 * m["sigma"], (r["sigma"], m["sigma"])
    assert len(r["lp"]) == len(m["lp"])
    inf = np.isneginf(m["lp"])
    assert np.array_equal(np.isneginf(r["lp"]), inf)
    if (~inf).any():
        assert np.all(np.abs(r["lp"][~inf] - m["lp"][~inf]) <= 8 * np.spacing(math.log(max(T, 2)))), (r["lp"], m["lp"])
    assert np.array_equal(r["pp"], m["pp"])
    assert r["counts"] == m["counts"]


# ---- 1-3: the plan's own decode on three engines' shapes -----------------------------------------------------------
@pytest.mark.parametrize("name", ["3x20", "2x70"])
def test_ring_models_on_the_wave_engine(H, name):
    y, sm, temps, sigma = PU.shape(H, name)
    mu0 = np.asfortranarray(temps * 0.9)
    r = plan_update(H, y, sm, mu0, sigma, H.ENGINE_WAVE)
    assert r["engine"] == H.ENGINE_WAVE and len(r["lp"]) == sm.N
    m = PU.path_update(y, r["x"], sm.states, sm.transitions, mu0, by_template=True, exact=True)
    assert m["counts"] == [0, 0, 0] and m["c"][1:].min() > 0
    check(r, m, y)


def test_overlap_model_on_the_blocked_engine(H):
    y, sm, temps, sigma = PU.shape(H, "2x12o")
    assert sm.nstates == 144
    r = plan_update(H, y, sm, temps, sigma, H.ENGINE_BLOCKED)
    assert r["engine"] == H.ENGINE_BLOCKED
    m = PU.path_update(y, r["x"], sm.states, sm.transitions, temps, exact=True)
    tab = PU.single_table(sm.states)
    pairs = sum(1 for s in r["x"] if s > 1 and tab[s - 1] is None)
    assert pairs > 0 and m["c"][1:].sum() + pairs + int((r["x"] == 1).sum()) == len(y)   # absent from mu ...
    assert m["n"] == len(y)                                                                # ... present in sigma
    assert len(r["lp"]) == 3 and np.isneginf(r["lp"]).sum() == 1
    check(r, m, y)


# ---- 4: hand-built paths of prime length --------------------------------------------------------------------------
T_HAND, N_HAND, K_HAND = 10_007, 3, 20


def hand_path():
    """ring model 3 x 20 (rings of 19): x_0 inside a spike, an onset at every offset mod 64, (a,L) -> (b,1) back to
    back, a long silent stretch, a spike cut by the end of the data; template 2 never fires"""
    L, T = K_HAND - 1, T_HAND
    sid = lambda a, p: 1 + a * L + p                      # 1-based id of template a at phase p = 1..L  # noqa: E731
    x = np.ones(T, dtype=np.int16)
    x[:L - 4] = [sid(0, p) for p in range(5, L + 1)]      # phases 5..19: x_0 is not silent
    cur, a, offsets = L - 4, 1, set()
    for r in list(range(64)) * 4:
        t = cur + 1 + ((r - cur - 1) % 64)                # first sample >= cur + 1 with t % 64 == r
        if t + 2 * L > 8900:
            break
        x[t:t + L] = [sid(a, p) for p in range(1, L + 1)]
        offsets.add(t % 64)
        cur = t + L
        if r % 7 == 3:                                    # the other template follows with no silent sample between
            x[cur:cur + L] = [sid(1 - a, p) for p in range(1, L + 1)]
            offsets.add(cur % 64)
            cur += L
        a = 1 - a
    assert offsets == set(range(64))
    assert np.all(x[8900:T - 7] == 1)
    x[T - 7:] = [sid(1, p) for p in range(1, 8)]          # cut by the end
    return x, sid


@pytest.mark.parametrize("engine", ["wave", "strict"])
def test_hand_built_path(H, engine):
    temps = PU.templates(H, N_HAND, K_HAND)
    pp = [0.01, 0.01, 0.01]
    sm = H.StateMatrix.create(N_HAND, K_HAND, np.log(pp), False)
    y = np.random.default_rng(7).standard_normal(T_HAND) * 2.0
    x, sid = hand_path()
    eng = H.ENGINE_WAVE if engine == "wave" else H.ENGINE_STRICT
    r = plan_update(H, y, sm, temps, 0.3, eng, x=x)
    assert r["engine"] == eng
    m = PU.path_update(y, x, sm.states, sm.transitions, temps, by_template=engine == "wave", exact=True)
    assert m["counts"] == [0, 0, K_HAND - 1]
    check(r, m, y)
    assert np.array_equal(r["mu"][:, 2], temps[:, 2]) and r["lp"][2] == -np.inf and r["pp"][x[0] - 1] == 0.0
    # not a path of this model: three ids outside 1..S and one 1 -> (a,5)
    bad = x.copy()
    bad[9100], bad[9200], bad[9300], bad[9400] = 0, sm.nstates + 1, sm.nstates + 1, sid(0, 5)
    rb = plan_update(H, y, sm, temps, 0.3, eng, x=bad)
    assert rb["counts"][0] == 3 and rb["counts"][1] >= 1


# ---- 5: the shortest signals --------------------------------------------------------------------------------------
@pytest.mark.parametrize("x", [[1], [2], [1, 1], [1, 2], [2, 3]])
def test_one_and_two_samples(H, x):
    temps = PU.templates(H, 2, 12)
    sm = H.StateMatrix.create(2, 12, np.log([0.02, 0.015]), False)
    y = np.array([0.7, -1.3][:len(x)])
    r = plan_update(H, y, sm, temps, 0.3, H.ENGINE_STRICT, x=np.array(x, dtype=np.int16))
    m = PU.path_update(y, x, sm.states, sm.transitions, temps, exact=True)
    assert m["counts"][:2] == [0, 0]
    check(r, m, y)


# ---- 6: batched ----------------------------------------------------------------------------------------------------
def test_batched_wave_plan_equals_single_plans_bitwise(H):
    import torch
    nC, N, K, T = 3, 3, 20, 8000
    rng = np.random.default_rng(21)
    ms, ys = [], []
    for c in range(nC):
        temps = PU.templates(H, N, K) * rng.uniform(0.8, 1.2)
        pp = rng.uniform(0.005, 0.012, N)
        sg = float(rng.uniform(0.25, 0.4))
        ms.append((H.StateMatrix.create(N, K, np.log(pp), False), np.asfortranarray(temps), sg))
        ys.append(H.create_signal(T, sg, pp, temps, seed=60 + c))
    H.set_option("engine", H.ENGINE_WAVE)
    plan = H.Plan.batched(T, [m[0] for m in ms], [m[1] for m in ms], [m[2] for m in ms])
    try:
        dy = torch.from_numpy(np.stack(ys)).cuda()
        dx = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
        dll = torch.zeros(nC, dtype=torch.float64, device="cuda")
        out = torch.full((nC, plan.mstep_len()), np.nan, dtype=torch.float64, device="cuda")
        cnt = torch.full((nC, 3), -1, dtype=torch.int64, device="cuda")
        plan.viterbi(dy, dx, dll)
        plan.path_update(dy, dx, out, cnt)
        torch.cuda.synchronize()
        ob, xb, cb = out.cpu().numpy(), dx.cpu().numpy(), cnt.cpu().numpy()
    finally:
        plan.close()
    for c, (sm, temps, sg) in enumerate(ms):
        r = plan_update(H, ys[c], sm, temps, sg, H.ENGINE_WAVE)
        assert np.array_equal(xb[c], r["x"]), c
        assert ob[c].tobytes() == r["raw"].tobytes(), c
        assert cb[c].tolist() == r["counts"] == [0, 0, 0]


# ---- 7: the same bits every time -----------------------------------------------------------------------------------
def test_two_calls_and_another_stream_give_the_same_bits(H):
    import torch
    y, sm, temps, sigma = PU.shape(H, "2x70")
    H.set_option("engine", H.ENGINE_WAVE)
    plan = H.Plan(len(y), sm, temps, sigma)
    try:
        dy = torch.from_numpy(y).cuda()
        dx = torch.zeros(len(y), dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        outs = [torch.full((plan.mstep_len(),), np.nan, dtype=torch.float64, device="cuda") for _ in range(3)]
        plan.viterbi(dy, dx, dll)
        plan.path_update(dy, dx, outs[0])
        plan.path_update(dy, dx, outs[1])
        torch.cuda.synchronize()
        other = torch.cuda.Stream()
        plan.path_update(dy, dx, outs[2], None, other.cuda_stream)
        other.synchronize()
        a, b, c = (o.cpu().numpy().tobytes() for o in outs)
        assert a == b == c
    finally:
        plan.close()


# ---- 8: the host entry point ---------------------------------------------------------------------------------------
def host_step(H, y, sm, mu, sigma, want_x=True, lp_cap=None):
    from hmmsort_amd._lib import lib, ptr
    from hmmsort_amd.api import _model_args
    mu = np.array(mu, dtype=np.float64, order="F", copy=True)
    keep, margs = _model_args(sm, mu, sigma)
    st, tr, mu_f = keep
    assert mu_f is mu
    sig, nlp, ll = C.c_double(np.nan), C.c_int64(-1), C.c_double(np.nan)
    lp = np.full(len(tr) if lp_cap is None else max(lp_cap, 1), np.nan)
    pp = np.full(sm.nstates, np.nan)
    x = np.full(len(y), -9, dtype=np.int16) if want_x else None
    rc = lib().hmmsort_viterbi_step(ptr(y), len(y), ptr(st), sm.N, sm.K, sm.nstates, ptr(tr), len(tr), ptr(mu),
                                    float(sigma), C.cast(C.byref(sig), C.c_void_p), ptr(lp),
                                    len(tr) if lp_cap is None else lp_cap, C.byref(nlp), ptr(pp), ptr(x),
                                    C.cast(C.byref(ll), C.c_void_p) if want_x else None)
    return rc, dict(mu=mu, sigma=sig.value, lp=lp[:max(nlp.value, 0)], pp=pp, x=x, ll=ll.value)


@pytest.mark.parametrize("name", ["3x20", "2x12o"])
def test_host_entry_equals_plan_decode_plus_plan_update(H, name):
    y, sm, temps, sigma = PU.shape(H, name)
    mu0 = np.asfortranarray(temps * 0.9)
    r = plan_update(H, y, sm, mu0, sigma, H.ENGINE_AUTO)
    xv, llv = H.viterbi(y, sm, mu0, sigma)
    rc, h = host_step(H, y, sm, mu0, sigma)
    assert rc == 0 and H.get_option("last_escalations") == 0
    assert np.array_equal(h["x"], xv) and h["ll"] == llv and np.array_equal(h["x"], r["x"])
    assert not np.array_equal(h["mu"], mu0)                                     # rewritten in place
    for k in ("mu", "lp", "pp"):
        assert h[k].tobytes() == r[k].tobytes(), k
    assert h["sigma"] == r["sigma"]
    rc2, h2 = host_step(H, y, sm, mu0, sigma, want_x=False)                     # x_out = ll_out = NULL
    assert rc2 == 0 and h2["mu"].tobytes() == h["mu"].tobytes() and h2["sigma"] == h["sigma"]
    rc3, _ = host_step(H, y, sm, mu0, sigma, lp_cap=len(r["lp"]) - 1)
    assert rc3 == H._lib.EINVAL
    # the Python wrapper is the same call
    sm_n, mu_n, sig_n, xw, llw = H.viterbi_step(y, sm, mu0.copy(order="F"), sigma, return_path=True)
    assert mu_n.tobytes() == h["mu"].tobytes() and sig_n == h["sigma"] and np.array_equal(xw, xv) and llw == llv
    assert sm_n.nstates == sm.nstates


# ---- 9: the ladder -------------------------------------------------------------------------------------------------
def test_duplicate_templates_update_follows_the_ladders_path(O, H):
    K, T = 30, 30_000
    t1 = H.create_spike_template(K, 3.0, 0.8, 0.2)
    temps = np.asfortranarray(np.stack([t1, t1], 1))
    pp = [0.004, 0.004]
    sm = H.StateMatrix.create(2, K, np.log(pp), True)
    y = H.create_signal(T, 0.3, pp, temps, seed=9)
    H.set_option("engine", H.ENGINE_BLOCKED)
    rc, h = host_step(H, y, sm, temps, 0.3)
    assert rc == 0 and H.get_option("last_escalations") >= 1
    xo, _ = O.viterbi(y, to_oracle_sm(O, sm), temps, 0.3)
    assert np.array_equal(h["x"], xo)
    m = PU.path_update(y, xo, sm.states, sm.transitions, temps, exact=True)
    h["counts"] = m["counts"]                                                   # the host entry returns none
    check(h, m, y)


# ---- 10: shards ----------------------------------------------------------------------------------------------------
def test_a_time_shard_is_refused(H):
    import torch
    y, sm, temps, sigma = PU.shape(H, "3x20")
    H.set_option("engine", H.ENGINE_WAVE)
    plan = H.Plan(len(y), sm, temps, sigma)
    try:
        dy = torch.from_numpy(y).cuda()
        dx = torch.ones(len(y), dtype=torch.int16, device="cuda")
        out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
        plan.set_shard(1000, 5000, False, False)
        with pytest.raises(H.HmmsortError) as e:
            plan.path_update(dy, dx, out)
        assert e.value.code == H._lib.EINVAL and "shard" in str(e.value)
        plan.set_shard(0, len(y), True, True)                                   # the whole recording again
        plan.path_update(dy, dx, out)
        torch.cuda.synchronize()
    finally:
        plan.close()


# ---- 11: train_model ------------------------------------------------------------------------------------------------
def steps(H, y, sm, mu, sigma, n):
    mu = mu.copy(order="F")
    for _ in range(n):
        sm, mu, sigma = H.viterbi_step(y, sm, mu, sigma)
    return sm, mu, sigma


@pytest.mark.parametrize("name", ["3x20", "2x12o"])
def test_train_model_viterbi_is_a_loop_of_viterbi_steps(H, name):
    y, sm, temps, sigma = PU.shape(H, name)
    mu0 = np.asfortranarray(temps * 0.9)
    seen = []

    def capture(state_matrix, mu, sg):
        seen.append((state_matrix, mu.copy(order="F"), sg))
        return state_matrix, mu

    # the first round is nsteps steps: what the stage between the rounds is handed equals three viterbi_step calls
    H.train_model(y, sm, mu0, sigma, 3, postprocess=capture, method="viterbi")
    sm3, mu3, sig3 = steps(H, y, sm, mu0, sigma, 3)
    assert seen[0][1].tobytes() == mu3.tobytes() and seen[0][2] == sig3
    assert seen[0][0].transitions.tobytes() == sm3.transitions.tobytes()
    # the loop as a whole, stage skipped: the reference's second round adds nsteps // 2 = 1 step
    calls = []
    sm_t, mu_t, sig_t = H.train_model(y, sm, mu0, sigma, 3, lambda m: calls.append(m.copy()), postprocess=None,
                                      method="viterbi")
    sm4, mu4, sig4 = steps(H, y, sm3, mu3, sig3, 1)
    assert mu_t.tobytes() == mu4.tobytes() and sig_t == sig4
    assert sm_t.transitions.tobytes() == sm4.transitions.tobytes()
    assert len(calls) == 3 and calls[0].tobytes() == mu0.tobytes()
    assert np.array_equal(mu0, np.asfortranarray(temps * 0.9))                  # the caller's array is left alone
    one = H.train_model(y, sm, mu0.copy(order="F"), sigma, method="viterbi")  # the one-step form
    s1 = steps(H, y, sm, mu0, sigma, 1)
    assert one[1].tobytes() == s1[1].tobytes() and one[2] == s1[2]


def test_train_model_default_is_baum_welch(H):
    y, sm, temps, sigma = PU.shape(H, "3x20")
    mu0 = np.asfortranarray(temps * 0.9)
    a = H.train_model(y, sm, mu0, sigma, 2, postprocess=None)
    b = H.train_model(y, sm, mu0, sigma, 2, postprocess=None, method="baum-welch")
    assert a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    assert a[0].transitions.tobytes() == b[0].transitions.tobytes()
    with pytest.raises(ValueError, match="refine"):
        H.train_model(y, 3, 20, False, 4, method="viterbi")
    with pytest.raises(ValueError):
        H.train_model(y, sm, mu0, sigma, 2, method="hard")


# ---- 12: one hard step from the true model lands on the true model ---------------------------------------------------
@pytest.mark.parametrize("name", PU.SHAPES)
def test_one_step_from_the_truth_stays_at_the_truth(H, name):
    y, sm, temps, sigma = PU.shape(H, name)
    sm_n, mu_n, sig_n, x, _ = H.viterbi_step(y, sm, temps.copy(order="F"), sigma, return_path=True)
    c = PU.path_update(y, x, sm.states, sm.transitions, temps)["c"]
    seen = c > 0
    assert seen[1:].all()
    err = np.abs(mu_n - temps)
    assert np.all(err[seen] <= 8 * PU.SIGMA / np.sqrt(c[seen])), (err[seen] * np.sqrt(c[seen])).max()


# ---- 13: sort_data ---------------------------------------------------------------------------------------------------
def test_sort_data_refine_steps(H):
    K, N, T = 12, 2, 6000
    temps = PU.templates(H, N, K)
    p = np.array([0.02, 0.015])
    y = PU.overlap_signal(T, PU.SIGMA, p, temps, 31)
    spike_forms = np.zeros((K, 1, N))
    spike_forms[:, 0, :] = temps * 0.9
    cinv = [1.0 / PU.SIGMA ** 2]
    sm = H.StateMatrix.create(N, K, np.log(p), True)
    sigma = float(np.sqrt(1.0 / cinv[0]))
    mu0 = np.asfortranarray(spike_forms[:, 0, :])
    base = H.sort_data(spike_forms, cinv, p, y, dosave=False)
    zero = H.sort_data(spike_forms, cinv, p, y, dosave=False, refine_steps=0)
    assert sorted(base) == sorted(zero) == ["ll", "lp", "mlseq", "sigma", "waveforms"]
    assert np.array_equal(base["waveforms"], mu0) and base["sigma"] == sigma
    assert np.array_equal(base["lp"], H.get_lp(sm)[0])
    x0, ll0 = H.viterbi(y, sm, mu0, sigma)
    assert np.array_equal(base["mlseq"], H.unroll_mlseq(x0, sm)) and abs(base["ll"] - ll0) <= 1e-9 * abs(ll0)
    for k in base:
        assert np.array_equal(base[k], zero[k]), k
    two = H.sort_data(spike_forms, cinv, p, y, dosave=False, refine_steps=2)
    sm2, mu2, sig2 = steps(H, y, sm, mu0, sigma, 2)
    assert two["waveforms"].tobytes() == mu2.tobytes() and two["sigma"] == sig2
    assert np.array_equal(two["lp"], H.get_lp(sm2)[0])
    x2, _ = H.viterbi(y, sm2, mu2, sig2)
    assert np.array_equal(two["mlseq"], H.unroll_mlseq(x2, sm2))
    assert not np.array_equal(two["waveforms"], mu0)
