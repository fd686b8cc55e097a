"""Viterbi training from additive path statistics on the device (csrc/path_update.hip): hmmsort_plan_path_stats,
hmmsort_plan_path_finish, hmmsort_stats_sum on every engine, the host entry hmmsort_fit_step_channels and the Python
layers on top.  The reference is the numpy / math.fsum model of path_stats_model.py; test_path_stats_cpu.py ties it
to the two-pass model of path_update_model.py.

Tolerances, for any order of summing:
  integer slots of the vector, pp' and the three counts exact; mu', lp' as test_gpu_path_update.check
  s_e within c_e 2^-52 max|y|, sm_e within (samples in multi-active states) 2^-52 max|y|, sum y^2 within n 2^-52 of it
  sigma': each of the four sums of the identity carries at most T 2^-52 of its absolute sum, so
  |d tot| <= 4 T 2^-52 (sum y^2 + 2 sum_e |mu'_e| sum|y|_e + sum c mu'^2 + sum n_j M_j^2), computed from the MODEL;
  sigma' gets half of that relative error plus the 4 T 2^-52 of the two-pass form (path_stats_model.sigma_bound)."""
import ctypes as C
import math

import numpy as np
import pytest

import path_stats_model as PS
import path_update_model as PU
from test_gpu_path_update import K_HAND, N_HAND, T_HAND, hand_path, split

pytestmark = pytest.mark.gpu

OPTIONS = dict(engine=0, block=0, halo=0, escalate=1)
CUTS = (4099, 8209)


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


def make_plan(H, T, sm, mu, sigma, engine):
    H.set_option("engine", engine)
    try:
        return H.Plan(T, sm, mu, sigma)
    finally:
        H.set_option("engine", H.ENGINE_AUTO)


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def take_stats(plan, dy, dx, T, lo, hi, first, stream=0, nch=1):
    import torch
    st = torch.full((nch * plan.path_stats_len(),), np.nan, dtype=torch.float64, device="cuda")
    plan.path_stats(dy, dx, T, lo, hi, first, st, stream)
    return st


def finish(plan, dstats, sm, stream=0):
    import torch
    out = torch.full((plan.mstep_len(),), np.nan, dtype=torch.float64, device="cuda")
    cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    plan.path_finish(dstats, out, cnt, stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    r = split(o, sm.K, sm.N, sm.nstates)
    r.update(counts=cnt.cpu().numpy().tolist(), raw=o)
    return r


def check_vector(v, st, y, sm):
    """the library's vector v against the model's statistics st"""
    g = PS.split_vector(v, sm.N, sm.K, sm.nstates)
    for k in PS.INT_SLOTS:
        assert np.array_equal(np.asarray(g[k]), np.asarray(st[k], dtype=np.float64)), k
    ymax = float(np.abs(y).max())
    assert np.all(np.abs(g["s"] - st["s"]) <= st["c"] * 2.0 ** -52 * ymax)
    assert np.all(np.abs(g["sm"] - st["sm"]) <= int(st["nj"].sum()) * 2.0 ** -52 * ymax)
    assert abs(g["sum_y2"] - st["sum_y2"]) <= max(st["n"], 1) * 2.0 ** -52 * st["sum_y2"]


def check_step(r, f, y, T):
    """the library's finish r against the model's finish f of statistics over T samples of y in all"""
    ymax = float(np.abs(y).max())
    bound = f["c"] * 2.0 ** -52 * ymax + np.spacing(np.abs(f["mu"]))
    err = np.abs(r["mu"] - f["mu"])
    assert np.all(err <= bound), (err.max(), np.argwhere(err > bound)[:4])
    assert np.all(r["mu"][0] == 0.0)
    rel = abs(r["sigma"] - f["sigma"]) / f["sigma"]
    print("sigma' %.17g model %.17g rel %.3g bound %.3g" % (r["sigma"], f["sigma"], rel, PS.sigma_bound(f, T)))
    assert rel <= PS.sigma_bound(f, T), (r["sigma"], f["sigma"])
    assert len(r["lp"]) == len(f["lp"])
    inf = np.isneginf(f["lp"])
    assert np.array_equal(np.isneginf(r["lp"]), inf)
    if (~inf).any():
        assert np.all(np.abs(r["lp"][~inf] - f["lp"][~inf]) <= 8 * np.spacing(math.log(max(T, 2)))), (r["lp"], f["lp"])
    assert np.array_equal(r["pp"], f["pp"])
    assert r["counts"] == f["counts"]


def same_step_bits(a, b):
    for k in ("mu", "lp", "pp"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["counts"] == b["counts"]


# ---- 1: the whole recording on every engine --------------------------------------------------------------------------
@pytest.mark.parametrize("name,engine", [("3x20", "wave"), ("2x70", "wave"), ("2x12o", "blocked"), ("3x20", "strict")])
def test_whole_recording_matches_the_model_and_path_update(H, name, engine):
    import torch
    y, sm, temps, sigma = PU.shape(H, name)
    eng = dict(wave=H.ENGINE_WAVE, blocked=H.ENGINE_BLOCKED, strict=H.ENGINE_STRICT)[engine]
    mu0 = temps if engine == "blocked" else np.asfortranarray(temps * 0.9)
    T = len(y)
    plan = make_plan(H, T, sm, mu0, sigma, eng)
    try:
        assert plan.info()["engine"] == eng
        dy = dev(y)
        dx = torch.zeros(T, dtype=torch.int16, device="cuda")
        dll = torch.zeros(1, dtype=torch.float64, device="cuda")
        plan.viterbi(dy, dx, dll)
        dg = plan.diagnostics()
        assert dg[0] == 0 and dg[7] == 0, dg
        out = torch.full((plan.mstep_len(),), np.nan, dtype=torch.float64, device="cuda")
        cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        plan.path_update(dy, dx, out, cnt)
        ds = take_stats(plan, dy, dx, T, 0, T, True)
        r = finish(plan, ds, sm)
        two = split(out.cpu().numpy(), sm.K, sm.N, sm.nstates)
        two["counts"] = cnt.cpu().numpy().tolist()
        x, v = dx.cpu().numpy(), ds.cpu().numpy()
    finally:
        plan.close()
    assert len(v) == 3 * sm.N * (sm.K - 1) + sm.nstates + len(r["lp"]) + 6
    st = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, by_template=engine == "wave")
    if name == "2x12o":
        assert st["nj"].sum() > 0 and np.abs(st["sm"]).sum() > 0       # multi-active states on the decoded path
        g = PS.split_vector(v, sm.N, sm.K, sm.nstates)
        assert g["nj"].sum() > 0 and np.abs(g["sm"]).sum() > 0
    check_vector(v, st, y, sm)
    f = PS.finish(st, sm.states, mu0)
    assert f["counts"] == [0, 0, 0]
    check_step(r, f, y, T)
    same_step_bits(r, two)
    assert abs(r["sigma"] - two["sigma"]) <= (PS.sigma_bound(f, T) + 4 * T * 2.0 ** -52) * two["sigma"]


# ---- 2: ranges of the hand path, from the full arrays and from slices with halos ----------------------------------------
def hand_case(H):
    temps = PU.templates(H, N_HAND, K_HAND)
    sm = H.StateMatrix.create(N_HAND, K_HAND, np.log([0.01, 0.01, 0.01]), False)
    y = np.random.default_rng(7).standard_normal(T_HAND) * 2.0
    x, sid = hand_path()
    return y, x, sm, temps, sid


def onset_cut(x, lo, hi):
    for t in range(lo + 1, hi):
        if x[t - 1] == 1 and x[t] > 1 and (x[t] - 2) % (K_HAND - 1) == 0:
            return t
    raise AssertionError("no onset between the cuts")


def shard_vectors(plan, dy, dx, T, edges, sliced):
    """one vector per range, rows of one tensor: from the full arrays, or from slices with 64-sample halos"""
    import torch
    n = plan.path_stats_len()
    parts = torch.full((len(edges) - 1, n), np.nan, dtype=torch.float64, device="cuda")
    for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        a, b = (max(lo - 64, 0), min(hi + 64, T)) if sliced else (0, T)
        plan.path_stats(dy.data_ptr() + 8 * a, dx.data_ptr() + 2 * a, b - a, lo - a, hi - a, a == 0, parts[i])
    return parts


@pytest.mark.parametrize("engine", ["wave", "strict"])
def test_ranges_add_up_to_the_whole(H, engine):
    import torch
    y, x, sm, temps, sid = hand_case(H)
    T, wave = T_HAND, engine == "wave"
    c3 = onset_cut(x, *CUTS)
    edges = [0, CUTS[0], c3, CUTS[1], T]
    whole = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, wave)
    f = PS.finish(whole, sm.states, temps)
    ymax = float(np.abs(y).max())
    plan = make_plan(H, T, sm, temps, 0.3, H.ENGINE_WAVE if wave else H.ENGINE_STRICT)
    try:
        dy, dx = dev(y), dev(x, np.int16)
        n = plan.path_stats_len()
        v = take_stats(plan, dy, dx, T, 0, T, True).cpu().numpy()
        check_vector(v, whole, y, sm)
        g = PS.split_vector(v, sm.N, sm.K, sm.nstates)
        for sliced in (False, True):
            parts = shard_vectors(plan, dy, dx, T, edges, sliced)
            tot = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
            H.stats_sum(parts, len(edges) - 1, n, tot)
            torch.cuda.synchronize()
            hp, ht = parts.cpu().numpy(), tot.cpu().numpy()
            acc = hp[0].copy()
            for p in hp[1:]:
                acc += p
            assert ht.tobytes() == acc.tobytes()                         # ascending order, one add per part
            gt = PS.split_vector(ht, sm.N, sm.K, sm.nstates)
            for k in PS.INT_SLOTS:
                assert np.array_equal(np.asarray(gt[k]), np.asarray(g[k])), (sliced, k)
            assert np.all(np.abs(gt["s"] - g["s"]) <= whole["c"] * 2.0 ** -52 * ymax), sliced
            assert not gt["sm"].any() and abs(gt["sum_y2"] - g["sum_y2"]) <= T * 2.0 ** -52 * g["sum_y2"]
            for i, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
                m = PS.path_stats(y, x, sm.states, sm.transitions, sm.K, wave, lo, hi, first=lo == 0)
                check_vector(hp[i], m, y, sm)
            check_step(finish(plan, tot, sm), f, y, T)
        # the shard that ends on a silent sample owns the pair into the onset that follows
        alone = PS.split_vector(take_stats(plan, dy, dx, T, c3 - 1, c3, False).cpu().numpy(), sm.N, sm.K, sm.nstates)
        assert alone["b"] == 1 and alone["ent"].sum() == 1 and alone["n"] == 1
        assert not take_stats(plan, dy, dx, T, 500, 500, True).cpu().numpy().any()       # an empty range
        assert not take_stats(plan, dy, dx, T, T, T, False).cpu().numpy().any()
        for lo, hi in ((0, T + 1), (-1, 5), (6, 5)):
            with pytest.raises(H.HmmsortError) as e:
                take_stats(plan, dy, dx, T, lo, hi, True)
            assert e.value.code == H._lib.EINVAL
        # not a path of this model: the diagnostics land in the shard that owns them
        bad = x.copy()
        bad[9100], bad[9200], bad[9300], bad[9400] = 0, sm.nstates + 1, sm.nstates + 1, sid(0, 5)
        db = dev(bad, np.int16)
        bedges = [0, 9150, 9399, T]
        hb = shard_vectors(plan, dy, db, T, bedges, False).cpu().numpy()
        for i, (lo, hi) in enumerate(zip(bedges[:-1], bedges[1:])):
            m = PS.path_stats(y, bad, sm.states, sm.transitions, sm.K, wave, lo, hi, first=lo == 0)
            gb = PS.split_vector(hb[i], sm.N, sm.K, sm.nstates)
            assert (gb["bad0"], gb["bad1"], gb["n"]) == (m["bad0"], m["bad1"], m["n"]), i
        assert [PS.split_vector(h, sm.N, sm.K, sm.nstates)["bad0"] for h in hb] == [1, 2, 0]
        assert PS.split_vector(hb[2], sm.N, sm.K, sm.nstates)["bad1"] >= 1
    finally:
        plan.close()


# ---- 3: arrays longer than the plan --------------------------------------------------------------------------------------
def test_a_chunk_plan_takes_the_whole_recording(H):
    y, sm, temps, sigma = PU.shape(H, "2x12o")
    x, _ = H.viterbi(y, sm, temps, sigma)
    T = len(y)
    assert T == 6000
    dy, dx = dev(y), dev(x, np.int16)
    vs = []
    for n in (2000, T):
        plan = H.Plan(n, sm, temps, sigma)
        try:
            vs.append(take_stats(plan, dy, dx, T, 0, T, True).cpu().numpy())
            vs.append(finish(plan, dev(vs[-1]), sm)["raw"])
        finally:
            plan.close()
    assert vs[0].tobytes() == vs[2].tobytes() and vs[1].tobytes() == vs[3].tobytes()
    check_vector(vs[0], PS.path_stats(y, x, sm.states, sm.transitions, sm.K), y, sm)


# ---- 4: batched --------------------------------------------------------------------------------------------------------
def test_batched_wave_plan_channels_and_their_sum(H):
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
        n = plan.path_stats_len()
        dy = dev(np.stack(ys))
        dx = torch.zeros((nC, T), dtype=torch.int16, device="cuda")
        dll = torch.zeros(nC, dtype=torch.float64, device="cuda")
        plan.viterbi(dy, dx, dll)
        ds = take_stats(plan, dy, dx, T, 0, T, True, nch=nC)
        out = torch.full((nC, plan.mstep_len()), np.nan, dtype=torch.float64, device="cuda")
        cnt = torch.full((nC, 3), -1, dtype=torch.int64, device="cuda")
        plan.path_finish(ds, out, cnt)
        tot = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
        H.stats_sum(ds, nC, n, tot)
        torch.cuda.synchronize()
        with pytest.raises(H.HmmsortError) as e:                                 # a foreign T
            plan.path_stats(dy, dx, T - 1, 0, T - 1, True, ds)
        assert e.value.code == H._lib.EINVAL
        vb, ob, cb, xb = ds.cpu().numpy().reshape(nC, n), out.cpu().numpy(), cnt.cpu().numpy(), dx.cpu().numpy()
    finally:
        plan.close()
    for c, (sm, temps, sg) in enumerate(ms):
        single = make_plan(H, T, sm, temps, sg, H.ENGINE_WAVE)
        try:
            d1 = take_stats(single, dev(ys[c]), dev(xb[c]), T, 0, T, True)
            r1 = finish(single, d1, sm)
            assert d1.cpu().numpy().tobytes() == vb[c].tobytes(), c
            assert r1["raw"].tobytes() == ob[c].tobytes() and r1["counts"] == cb[c].tolist() == [0, 0, 0], c
            if c == 0:
                rp = finish(single, tot, sm)
        finally:
            single.close()
    sm0, mu0, _ = ms[0]
    f, _st = PS.pooled([(ys[c], xb[c]) for c in range(nC)], sm0.states, sm0.transitions, mu0, True)
    check_step(rp, f, np.concatenate(ys), nC * T)


# ---- 5: more entries than one pass over the tile holds ------------------------------------------------------------------
def test_group_passes_of_a_long_ring(H):
    N, K, T = 2, 2100, 9000
    L = K - 1
    rng = np.random.default_rng(3)
    mu = np.asfortranarray(rng.standard_normal((K, N)))
    mu[0] = 0.0
    sm = H.StateMatrix.create(N, K, np.log([0.001, 0.001]), False)
    assert N * L > 4096
    x = np.ones(T, dtype=np.int16)
    for a, t in ((0, 100), (1, 2500), (0, 4700), (1, 6901)):
        x[t:t + L] = 2 + a * L + np.arange(L)
    assert x[-1] > 1 and x[6900] == 1                                    # the last ring ends with the data
    y = rng.standard_normal(T)
    plan = make_plan(H, T, sm, mu, 1.0, H.ENGINE_STRICT)
    try:
        import torch
        dy, dx = dev(y), dev(x)
        out = torch.full((plan.mstep_len(),), np.nan, dtype=torch.float64, device="cuda")
        cnt = torch.full((3,), -1, dtype=torch.int64, device="cuda")
        plan.path_update(dy, dx, out, cnt)
        ds = take_stats(plan, dy, dx, T, 0, T, True)
        r = finish(plan, ds, sm)
        two = split(out.cpu().numpy(), K, N, sm.nstates)
        two["counts"] = cnt.cpu().numpy().tolist()
        v = ds.cpu().numpy()
    finally:
        plan.close()
    st = PS.path_stats(y, x, sm.states, sm.transitions, K)
    check_vector(v, st, y, sm)
    check_step(r, PS.finish(st, sm.states, mu), y, T)
    same_step_bits(r, two)


# ---- 6: the same bits every time ------------------------------------------------------------------------------------------
def test_two_calls_and_another_stream_give_the_same_bits(H):
    import torch
    y, sm, temps, sigma = PU.shape(H, "2x12o")
    x, _ = H.viterbi(y, sm, temps, sigma)
    T = len(y)
    plan = H.Plan(T, sm, temps, sigma)
    try:
        dy, dx = dev(y), dev(x, np.int16)
        a = take_stats(plan, dy, dx, T, 0, T, True)
        b = take_stats(plan, dy, dx, T, 0, T, True)
        ra = finish(plan, a, sm)
        other = torch.cuda.Stream()
        c = take_stats(plan, dy, dx, T, 0, T, True, other.cuda_stream)
        rc = finish(plan, c, sm, other.cuda_stream)
        other.synchronize()
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
        assert ra["raw"].tobytes() == rc["raw"].tobytes() and not np.isnan(a.cpu().numpy()).any()
    finally:
        plan.close()


# ---- 7: the host entry -----------------------------------------------------------------------------------------------------
def channels_case(H):
    temps = PU.templates(H, 2, 12)
    pp = [0.02, 0.015]
    sm = H.StateMatrix.create(2, 12, np.log(pp), True)
    tms = [H.HMMSpikeTemplateModel(sm, np.asfortranarray(temps * s), PU.SIGMA) for s in (1.0, 0.95, 1.05)]
    # seeds whose chunk loop ends well: the last chunk is a few samples long, and a chunk that short decodes as the
    # tail of a spike on most noise (no entry cost at its first sample), where fit.jl:26 dies; noise alone at the end
    seeds = (41, 42, 51)
    ys = [PU.overlap_signal(6000, PU.SIGMA, pp, temps, s) for s in seeds]
    for s, y in zip(seeds, ys):
        y[-100:] = PU.SIGMA * np.random.default_rng(s + 10).standard_normal(100)
    return sm, tms, ys


def host_models(H, tms):
    from hmmsort_amd.api import _model_args
    keep, models = [], (H._lib.Model * len(tms))()
    for c, tm in enumerate(tms):
        k, m = _model_args(tm.state_matrix, tm.mu, tm.sigma)
        keep.append(k)
        models[c] = H._lib.Model(*m)
    return keep, models


def host_step(H, tms, ys, chunksize, devices, pooled, lp_cap=None, want_ml=True):
    """hmmsort_fit_step_channels through ctypes: rc, paths, lls and the list of per-record dicts"""
    from hmmsort_amd._lib import lib, ptr
    nch, T = len(ys), len(ys[0])
    keep, models = host_models(H, tms)
    ml = [np.full(T, -9, dtype=np.int16) for _ in range(nch)]
    ll = np.full(nch, np.nan)
    yp = (C.c_void_p * nch)(*[y.ctypes.data for y in ys])
    mp = (C.c_void_p * nch)(*[m.ctypes.data for m in ml]) if want_ml else None
    dv = (C.c_int * len(devices))(*devices) if devices else None
    nout = 1 if pooled else nch
    recs, bufs = (H._lib.StepOut * nout)(), []
    for c in range(nout):
        sm = tms[c].state_matrix
        b = dict(mu=np.full((sm.K, sm.N), np.nan, order="F"), sigma=np.full(1, np.nan),
                 lp=np.full(max(len(sm.transitions) if lp_cap is None else lp_cap, 1), np.nan),
                 nlp=np.full(1, -1, dtype=np.int64), pp=np.full(sm.nstates, np.nan), counts=np.full(3, -1, dtype=np.int64))
        bufs.append(b)
        recs[c] = H._lib.StepOut(b["mu"].ctypes.data, b["sigma"].ctypes.data, b["lp"].ctypes.data,
                                 len(sm.transitions) if lp_cap is None else lp_cap, b["nlp"].ctypes.data,
                                 b["pp"].ctypes.data, b["counts"].ctypes.data)
    status = (C.c_int * nch)()
    rc = lib().hmmsort_fit_step_channels(nch, yp, H._lib.SAMPLES_F64, T, chunksize, models, dv,
                                         len(devices) if devices else 0, int(pooled), mp, ptr(ll), recs, status)
    outs = [dict(mu=b["mu"], sigma=float(b["sigma"][0]), lp=b["lp"][:max(int(b["nlp"][0]), 0)], pp=b["pp"],
                 counts=b["counts"].tolist()) for b in bufs]
    return rc, ml, ll, outs


def plan_level(H, tm, y, x, summed=None):
    """plan-level statistics of (y, x) under tm, and the finish of them (or of `summed`) with tm"""
    sm = tm.state_matrix
    plan = H.Plan(2000, sm, tm.mu, tm.sigma)
    try:
        v = take_stats(plan, dev(y), dev(x, np.int16), len(y), 0, len(y), True)
        r = finish(plan, v if summed is None else dev(summed), sm)
        return v.cpu().numpy(), r
    finally:
        plan.close()


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_host_entry(H, devices):
    sm, tms, ys = channels_case(H)
    ref = H.fit_channels(tms, ys, 2000, devices)
    assert all(m.ml_seq.max() > 1 for m in ref)
    rc, ml, ll, outs = host_step(H, tms, ys, 2000, devices, False)
    assert rc == 0, H._lib.last_error()
    vs = []
    for c in range(3):
        assert np.array_equal(ml[c], ref[c].ml_seq) and ll[c] == ref[c].ll, c
        v, r = plan_level(H, tms[c], ys[c], ml[c])
        vs.append(v)
        same_step_bits(outs[c], r)
        assert outs[c]["sigma"] == r["sigma"], c
        assert not np.array_equal(outs[c]["mu"], tms[c].mu)
    # pooled, and paths nobody asked for
    rc, _ml, llp, pooled = host_step(H, tms, ys, 2000, devices, True, want_ml=False)
    assert rc == 0, H._lib.last_error()
    assert np.array_equal(llp, ll)
    acc = vs[0].copy()
    for v in vs[1:]:
        acc += v
    _v, r = plan_level(H, tms[0], ys[0], ml[0], summed=acc)
    same_step_bits(pooled[0], r)
    assert pooled[0]["sigma"] == r["sigma"]
    f, _st = PS.pooled([(ys[c], ml[c]) for c in range(3)], sm.states, sm.transitions, tms[0].mu)
    check_step(pooled[0], f, np.concatenate(ys), 3 * len(ys[0]))
    if devices is None:
        # one whole-recording decode per channel takes the same step
        rc, mlw, _llw, outw = host_step(H, tms[:1], ys[:1], 0, None, False)
        assert rc == 0, H._lib.last_error()
        _v, rw = plan_level(H, tms[0], ys[0], mlw[0])
        same_step_bits(outw[0], rw)
        assert outw[0]["sigma"] == rw["sigma"]
        # refusals
        other = H.HMMSpikeTemplateModel(H.StateMatrix.create(2, 13, np.log([0.02, 0.015]), True),
                                        PU.templates(H, 2, 13), PU.SIGMA)
        rc, *_ = host_step(H, [tms[0], other, tms[2]], ys, 2000, None, True)
        assert rc == H._lib.EINVAL and "pooled" in H._lib.last_error()
        rc, *_ = host_step(H, tms, ys, 2000, None, False, lp_cap=len(outs[0]["lp"]) - 1)
        assert rc == H._lib.EINVAL


# ---- 8: the Python layers --------------------------------------------------------------------------------------------------
def test_api_fit_step_channels(H):
    sm, tms, ys = channels_case(H)
    rc, ml, ll, outs = host_step(H, tms, ys, 2000, None, False)
    assert rc == 0
    models, steps = H.fit_step_channels(tms, ys, 2000)
    assert len(models) == len(steps) == 3
    for c, (sm_n, mu_n, sig_n, counts) in enumerate(steps):
        assert np.array_equal(models[c].ml_seq, ml[c]) and models[c].ll == ll[c]
        assert mu_n.tobytes() == outs[c]["mu"].tobytes() and sig_n == outs[c]["sigma"] and counts == outs[c]["counts"]
        assert sm_n.nstates == sm.nstates
    rc, _ml, _ll, pooled = host_step(H, tms, ys, 2000, None, True)
    _models, one = H.fit_step_channels(tms, np.stack(ys), 2000, pooled=True)
    assert len(one) == 1 and one[0][1].tobytes() == pooled[0]["mu"].tobytes() and one[0][2] == pooled[0]["sigma"]
