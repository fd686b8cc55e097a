"""The interior form of the forward and Viterbi sweeps (kw_fwd MODE 3 / 4, vit_chain STORE = 2 / 3; DESIGN §3.3, §5
Round 11): the full owned super-steps of a chain run without the bookkeeping of partial steps, rings of at most 64
states take the delay line's values from the lane's registers (W == L), and the Viterbi sweep divides by the chain's
invariant through one reciprocal.  None of this may change a bit of any output, so every case runs the three calls
(viterbi, estep, decode_estep) and the M-step with option "interior" = 0 -- the general super-steps everywhere, in
kw_bwd too -- and = 1, compares x, ll, the statistics, the M-step output, diag and the tie counters bit for bit, and
holds the result to the oracle at the tolerances of tests/test_gpu_bwd_interior.py and
tests/test_gpu_decode_under_bwd.py (path equal, ll to 1e-9, the EM step to 1e-8).

Chains of 1024 samples with a warm-up of 256: a chain of L = 59 has 17 full owned super-steps.  A chain has an
interior range as soon as it owns one full super-step, and the wave engine takes no recording shorter than 512
samples, so no recording is without one; the shortest the engine takes (one chain, no warm-up, eight full steps)
stands in the list for it.
"""
import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm

pytestmark = pytest.mark.gpu

BLOCK, HALO = 1024, 256


@pytest.fixture(autouse=True)
def options(H):
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", BLOCK)
    H.set_option("halo", HALO)
    yield
    for k, v in (("engine", H.ENGINE_AUTO), ("block", 0), ("halo", 0), ("tie_scale", 1), ("interior", 1)):
        H.set_option(k, v)


def model(H, N, K):
    """bench.py's family of templates and rates (the headline rates at N = 4, K = 60), and a start model for the E-step"""
    base = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    amps = [(base[i % 4][0] * (1 + 0.13 * (i // 4)), base[i % 4][1] + 0.03 * (i // 4), base[i % 4][2])
            for i in range(N)]
    pp = [[0.003, 0.001, 0.002, 0.0015][i % 4] * (60.0 / K) for i in range(N)]
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, *a) for a in amps], 1))
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    return temps, pp, H.StateMatrix.create(N, K, np.log(pp), False), mu


def hexed(d):
    return [v.hex() if isinstance(v, float) else int(v) for v in d]


def all_calls(H, ys, sms, mus, sigmas):
    """viterbi, estep, decode_estep and the M-step of one plan; every output as bytes or exact values"""
    import torch
    C, T = len(ys), len(ys[0])
    st = torch.cuda.current_stream().cuda_stream
    plan = H.Plan(T, sms[0], mus[0], sigmas[0]) if C == 1 else H.Plan.batched(T, sms, mus, sigmas)
    try:
        assert plan.info()["engine"] == H.ENGINE_WAVE, plan.info()
        dy = torch.from_numpy(np.ascontiguousarray(np.stack(ys))).cuda()
        dx = torch.full((C, T), -1, dtype=torch.int16, device="cuda")
        dll = torch.zeros(C, dtype=torch.float64, device="cuda")
        stats = torch.zeros((C, plan.stats_len()), dtype=torch.float64, device="cuda")
        out = torch.zeros((C, plan.mstep_len()), dtype=torch.float64, device="cuda")
        r = {"info": plan.info()}
        plan.viterbi(dy, dx, dll, st)
        r["x"], r["ll"] = dx.cpu().numpy().copy(), dll.cpu().numpy().copy()
        r["diag_v"], r["ties_v"] = hexed(plan.diagnostics(st)), plan.tie_stats(st)
        plan.estep(dy, stats, st)
        r["stats"], r["diag_e"] = stats.cpu().numpy().copy(), hexed(plan.diagnostics(st))
        plan.mstep(stats, out, st)
        r["mstep"] = out.cpu().numpy().copy()
        dx.fill_(-1)
        stats.fill_(0)
        plan.decode_estep(dy, dx, dll, stats, st)
        r["xf"], r["llf"], r["statsf"] = dx.cpu().numpy().copy(), dll.cpu().numpy().copy(), stats.cpu().numpy().copy()
        r["diag_f"], r["ties_f"] = hexed(plan.diagnostics(st)), plan.tie_stats(st)
        out.fill_(0)
        plan.mstep(stats, out, st)
        r["mstepf"] = out.cpu().numpy().copy()
        return r
    finally:
        plan.close()


def both_forms(H, ys, sms, mus, sigmas):
    """the calls with "interior" = 0 and 1 (read when the plan is created), every output bit for bit"""
    got = {}
    try:
        for it in (0, 1):
            H.set_option("interior", it)
            got[it] = all_calls(H, ys, sms, mus, sigmas)
    finally:
        H.set_option("interior", 1)
    a, b = got[0], got[1]
    print("interior 0: diag %s %s %s ties %s" % (a["diag_v"], a["diag_e"], a["diag_f"], a["ties_v"]))
    print("interior 1: diag %s %s %s ties %s" % (b["diag_v"], b["diag_e"], b["diag_f"], b["ties_v"]))
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), "%s differs between interior 0 and 1 (%d entries)" % (
                k, int(np.count_nonzero(a[k] != b[k])))
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    return b


_oracle_cache = {}


def oracle(O, key, y, sm, mu, sigma):
    """oracle.viterbi and oracle.train_step of a case, computed once"""
    if key not in _oracle_cache:
        osm = to_oracle_sm(O, sm)
        xo, llo = O.viterbi(y, osm, mu, sigma)
        _, omu, osig, olp, _ = O.train_step(y, osm, mu.copy(order="F"), sigma)
        _oracle_cache[key] = (xo, llo, omu, osig, olp)
    return _oracle_cache[key]


def against_oracle(O, key, r, ys, sms, mus, sigmas, estep=True):
    for c, (y, sm, mu, sigma) in enumerate(zip(ys, sms, mus, sigmas)):
        xo, llo, omu, osig, olp = oracle(O, (key, c), y, sm, mu, sigma)
        K, N = sm.K, sm.N
        for x, ll in ((r["x"], r["ll"]), (r["xf"], r["llf"])):
            nbad = int(np.count_nonzero(x[c] != xo))
            assert nbad == 0, "channel %d: path differs from the oracle at %d samples, first at %d" % (
                c, nbad, int(np.argmax(x[c] != xo)))
            assert abs(ll[c] - llo) <= 1e-9 * abs(llo), (ll[c], llo)
        if not estep:
            continue
        for o in (r["mstep"][c], r["mstepf"][c]):
            m = o[:K * N].reshape((K, N), order="F")
            print("channel %d: max |mu - oracle| %.3e, sigma %.12g (oracle %.12g)" % (c, np.abs(m - omu).max(), o[K * N], osig))
            assert np.allclose(m, omu, rtol=1e-8, atol=1e-11), np.abs(m - omu).max()
            assert abs(o[K * N] - osig) <= 1e-8 * osig
            assert np.allclose(o[K * N + 1:K * N + 1 + N], olp, rtol=1e-8, atol=1e-12)


def clean(r, open_ties=0):
    """no failed certificate, nothing (open_ties decisions) left open by the resolver"""
    for d in (r["diag_v"], r["diag_f"]):
        assert d[0] == 0 and d[7] == open_ties, d
    for d in (r["diag_e"], r["diag_f"]):
        assert d[3] == 0 and d[5] == 0, d


# ---------------------------------------------------------------- ring lengths and ring counts
# L = 59, 8: W == L (register carry; 8: many short steps); 63: one idle lane; 64: none; 65, 127: W = 64 != L (no
# carry).  kw_vit carries with up to 8 rings, kw_fwd with 1, 3, 4, 7 and 8 (fwd_carry, wave_estep.hip): N = 1, 4, 8 have
# both, 2 and 5 the Viterbi sweep's only, 12 rings (one delay line per ring in log form in kw_fwd) only the interior
# form.  T = 4 * 1024 + 100: the last chain has one full step and a partial one.
GEOMETRY = [(4, 60), (1, 9), (5, 9), (2, 64), (8, 65), (5, 66), (1, 66), (4, 128), (8, 128), (2, 60), (8, 60),
            (12, 60), (12, 66)]


@pytest.mark.parametrize("N,K", GEOMETRY)
def test_ring_lengths_and_counts(O, H, N, K):
    T = 4 * BLOCK + 100
    temps, pp, sm, mu = model(H, N, K)
    y = H.create_signal(T, 0.3, pp, temps, seed=100 * N + K)
    r = both_forms(H, [y], [sm], [mu], [0.35])
    assert r["info"]["nchains"] >= 4, r["info"]      # (the plan rounds the chain length: 1024 or 1088 samples)
    clean(r)
    against_oracle(O, ("geom", N, K), r, [y], [sm], [mu], [0.35])


# ---------------------------------------------------------------- recording lengths (L = 59)
# 4 * 1024 + 60: the last chain is at its minimum length of L + 1 samples (one full step, one step of one sample);
# 519 and 1023: one chain without a warm-up, eight and seventeen full steps; 2 * 1024 + 1: one sample past the
# second chain, whatever the geometry makes of it; 3 * 1024: whole chains only
@pytest.mark.parametrize("T", [4 * BLOCK + 60, 519, 1023, 2 * BLOCK + 1, 3 * BLOCK])
def test_recording_lengths(O, H, T):
    N, K = 4, 60
    temps, pp, sm, mu = model(H, N, K)
    y = H.create_signal(T, 0.3, pp, temps, seed=T)
    r = both_forms(H, [y], [sm], [mu], [0.35])
    clean(r)
    against_oracle(O, ("len", T), r, [y], [sm], [mu], [0.35])


def test_shortest_recording_of_long_rings(O, H):
    N, K, T = 4, 128, 519
    temps, pp, sm, mu = model(H, N, K)
    y = H.create_signal(T, 0.3, pp, temps, seed=5)
    r = both_forms(H, [y], [sm], [mu], [0.35])
    clean(r)
    against_oracle(O, ("short", K), r, [y], [sm], [mu], [0.35])


def test_two_channels_of_odd_length(O, H):
    """a batched plan: the second channel's planes start off 16 bytes, and its model differs"""
    N, K, T = 4, 60, 3 * BLOCK + 77
    temps, pp, sm, mu = model(H, N, K)
    t2 = np.asfortranarray(temps * 1.2)
    mu2 = np.asfortranarray(mu * 1.15)
    ys = [H.create_signal(T, 0.3, pp, temps, seed=811), H.create_signal(T, 0.35, pp, t2, seed=812)]
    r = both_forms(H, ys, [sm, sm], [mu, mu2], [0.35, 0.4])
    clean(r)
    against_oracle(O, "two", r, ys, [sm, sm], [mu, mu2], [0.35, 0.4])


# ---------------------------------------------------------------- recordings
def test_recording_begins_and_ends_inside_a_spike(O, H):
    N, K, T = 4, 60, 4 * BLOCK + 100
    temps, pp, sm, mu = model(H, N, K)
    y = H.create_signal(T, 0.3, pp, temps, seed=61)
    y[:25] += temps[K - 25:, 0]          # the last 25 states of ring 0 at the start
    y[T - 11:] += temps[1:12, 1]         # the first 11 of ring 1 at the end
    r = both_forms(H, [y], [sm], [mu], [0.35])
    clean(r)
    against_oracle(O, "cut", r, [y], [sm], [mu], [0.35])
    assert r["x"][0][0] > 1 and r["x"][0][-1] > 1, "the decode should begin and end inside a spike"


def test_pure_noise(O, H):
    N, K, T = 4, 60, 4 * BLOCK + 100
    temps, pp, sm, mu = model(H, N, K)
    y = 0.3 * np.random.default_rng(7).standard_normal(T)
    r = both_forms(H, [y], [sm], [mu], [0.35])
    clean(r)
    against_oracle(O, "noise", r, [y], [sm], [mu], [0.35])


def test_flagged_decisions_are_counted(O, H):
    """tie_scale = 1e10 on a noisy recording: the decisions the sweep stores carry their flags by the hundred, and
    the backtrace and the resolver count the flags the interior steps stored"""
    N, K, T = 4, 60, 4 * BLOCK + 100
    temps, pp, sm, mu = model(H, N, K)
    y = H.create_signal(T, 0.6, pp, temps, seed=33)
    H.set_option("tie_scale", 10 ** 10)
    r = both_forms(H, [y], [sm], [mu], [0.6])
    assert r["ties_v"]["flagged"] > 50 and r["ties_v"]["decided"] > 50, r["ties_v"]   # (a handful at tie_scale = 1)
    assert r["ties_v"] == r["ties_f"], (r["ties_v"], r["ties_f"])
    # at this scale the final arg-max is flagged too and the resolver leaves it as the sweep found it ("tail"), in
    # the general form as in the interior form; the path is the oracle's all the same
    clean(r, open_ties=r["ties_v"]["tail"])
    against_oracle(O, "ties", r, [y], [sm], [mu], [0.6])


def test_failed_certificates_sweep_chains_again(O, H):
    """the busy signal and the short warm-up of tests/test_gpu_decode_under_bwd.py::test_failed_certificates_run_every_round
    (seed 22: seven chains are swept again by kw_vit_redo)"""
    K, N, T = 60, 4, 20_000
    temps = four_templates(H, K)
    pp = [0.03, 0.02, 0.025, 0.02]
    y = H.create_signal(T, 0.3, pp, temps, seed=22)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    H.set_option("block", 128)
    H.set_option("halo", 128)
    r = both_forms(H, [y], [sm], [temps], [0.3])
    assert r["diag_v"][0] == 0 and r["diag_v"][1] == 7, r["diag_v"]
    assert r["diag_f"][0] == 0 and r["diag_f"][1] == 7, r["diag_f"]
    # the E-step's own certificates fail on this signal at this warm-up (tests/test_gpu_wave_estep.py: the host call
    # escalates), so only the decode is held to the oracle here
    against_oracle(O, "redo", r, [y], [sm], [temps], [0.3], estep=False)


def test_two_time_shards(O, H):
    """the statistics of two time shards (dist.time_shard_plan) add up to the whole recording's, and each shard's
    are the same bits with and without the interior ranges (kw_bwd's ends at the shard edge)"""
    import torch
    N, K, T = 4, 60, 12_000
    temps, pp, sm, mu = model(H, N, K)
    y = H.create_signal(T, 0.3, pp, temps, seed=17)
    st = torch.cuda.current_stream().cuda_stream
    got = {}
    try:
        for it in (0, 1):
            H.set_option("interior", it)
            whole = H.Plan(T, sm, mu, 0.35)
            ref = torch.zeros(whole.stats_len(), dtype=torch.float64, device="cuda")
            whole.estep(torch.from_numpy(y).cuda(), ref, st)
            parts = []
            for rank in range(2):
                plan, ys, own = H.dist.time_shard_plan(y, rank, 2, sm, mu, 0.35, halo=256)
                part = torch.zeros_like(ref)
                plan.estep(torch.from_numpy(ys).cuda(), part, st)
                d = plan.diagnostics(st)
                assert d[3] == 0 and d[5] == 0 and max(d[4], d[6]) < 1e-9, d
                parts.append(part.cpu().numpy().copy())
                plan.close()
            out = torch.zeros(whole.mstep_len(), dtype=torch.float64, device="cuda")
            total = torch.from_numpy(parts[0] + parts[1]).cuda()
            whole.mstep(total, out, st)
            got[it] = (ref.cpu().numpy().copy(), parts[0], parts[1], out.cpu().numpy().copy())
            whole.close()
    finally:
        H.set_option("interior", 1)
    for a, b in zip(got[0], got[1]):
        assert a.tobytes() == b.tobytes(), int(np.count_nonzero(a != b))
    ref, p0, p1, o = got[1]
    assert np.allclose(p0 + p1, ref, rtol=1e-9, atol=1e-12), np.abs(p0 + p1 - ref).max()
    _, omu, osig, olp, _ = O.train_step(y, to_oracle_sm(O, sm), mu.copy(order="F"), 0.35)
    assert np.allclose(o[:K * N].reshape((K, N), order="F"), omu, rtol=1e-8, atol=1e-11)
    assert abs(o[K * N] - osig) <= 1e-8 * osig and np.allclose(o[K * N + 1:K * N + 1 + N], olp, rtol=1e-8)
