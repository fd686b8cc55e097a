"""The interior form of the backward sweep's owned super-steps (kw_bwd MODE 4) and
the mirrored rings of its statistics feed.  Chains of 1024 samples with a warm-up of 256 have about eleven
interior super-steps: the y ring of 256 entries wraps twice in them and the rho ring of 128 rows five times.
Every check here is one the general form passes as well: fused statistics against the separate kernel, the
oracle's train_step, additivity over time shards whose edges sit on and next to the interior range, and
recordings that have no interior range at all."""
import numpy as np
import pytest

from conftest import to_oracle_sm

pytestmark = pytest.mark.gpu

BLOCK, HALO = 1024, 256
# W = 59: the product's alignment runs through all four phases; W = 16: always aligned; W = 64; FT = 2; FT = 4
SHAPES = [(4, 60), (3, 17), (4, 65), (5, 50), (7, 129)]


@pytest.fixture(autouse=True)
def short_chains(H):
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", BLOCK)
    H.set_option("halo", HALO)
    yield
    H.set_option("engine", H.ENGINE_AUTO)
    H.set_option("block", 0)
    H.set_option("halo", 0)


def _model(H, N, K, T, seed=None):
    temps = np.asfortranarray(np.stack([H.create_spike_template(K, 2.5 + 0.3 * i, 0.3 + 0.08 * i, 0.2) for i in range(N)], 1))
    pp = ([0.003, 0.001, 0.002, 0.0015] * 2)[:N]
    pp = [p * min(1.0, 60.0 / K) for p in pp]
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    y = H.create_signal(T, 0.3, pp, temps, seed=N * K if seed is None else seed)
    mu0 = np.asfortranarray(temps * 0.9)
    mu0[0, :] = 0
    return y, sm, mu0


def _fused_vs_separate(H, N, K, T, monkeypatch):
    y, sm, mu0 = _model(H, N, K, T)
    H.set_option("plan_cache", 0)
    try:
        fused = H.train_step(y, sm, mu0.copy(order="F"), 0.35)
        monkeypatch.setenv("HMMSORT_GSUM_SEPARATE", "1")
        separate = H.train_step(y, sm, mu0.copy(order="F"), 0.35)
    finally:
        monkeypatch.delenv("HMMSORT_GSUM_SEPARATE", raising=False)
        H.set_option("plan_cache", 4)
    assert np.allclose(fused[1], separate[1], rtol=1e-11, atol=1e-13), np.abs(fused[1] - separate[1]).max()
    assert abs(fused[2] - separate[2]) <= 1e-12 * separate[2]
    assert np.allclose(fused[0].transitions["lp"], separate[0].transitions["lp"], rtol=1e-12, atol=1e-14)


# 5 * 1024 + 37: the recording ends 37 samples into a sixth block; 4 * 1024 + 1: one sample
@pytest.mark.parametrize("T", [5 * 1024 + 37, 4 * 1024 + 1])
@pytest.mark.parametrize("N,K", SHAPES)
def test_fused_statistics_equal_the_separate_kernel_short_chains(H, N, K, T, monkeypatch):
    _fused_vs_separate(H, N, K, T, monkeypatch)


# one chain (T < block): no interior range; a last chain of exactly L = K - 1 samples: all its onsets but the first lie
# within L samples of the end of the recording (a chain owns at least L samples), so it has no interior range either
@pytest.mark.parametrize("N,K,T", [(4, 60, 900), (3, 17, 700), (4, 60, 4 * 1024 + 59), (4, 65, 3 * 1024 + 64),
                                   (3, 17, 2 * 1024 + 16)])
def test_recordings_without_an_interior_range(O, H, N, K, T, monkeypatch):
    _fused_vs_separate(H, N, K, T, monkeypatch)
    y, sm, mu0 = _model(H, N, K, T)
    _compare_step(O, H, y, sm, mu0, 0.35)


def _compare_step(O, H, y, sm, mu, sigma, rtol=1e-8):
    sm_n, mu_n, sig_n = H.train_step(y, sm, mu.copy(order="F"), sigma)
    osm_n, omu, osig, olp, opp = O.train_step(y, to_oracle_sm(O, sm), mu.copy(order="F"), sigma)
    assert np.allclose(mu_n, omu, rtol=rtol, atol=1e-11), np.abs(mu_n - omu).max()
    assert abs(sig_n - osig) <= rtol * osig
    assert np.allclose(sm_n.transitions["lp"], osm_n.val, rtol=rtol, atol=1e-12)
    assert np.allclose(sm_n.pi, opp, rtol=1e-8, atol=1e-8), np.abs(sm_n.pi - opp).max()


@pytest.mark.parametrize("N,K", SHAPES)
def test_em_step_matches_oracle_short_chains(O, H, N, K):
    y, sm, mu0 = _model(H, N, K, 6_000 + N)
    _compare_step(O, H, y, sm, mu0, 0.35)


def _interior_edges(T, B, He, L, c):
    """Chain c of a T-sample slice with chains of B samples: (t_hi, t_lo), the highest sample of its first interior
    super-step and the lowest of its last one -- the schedule of kw_bwd restated.  To be kept in step with the
    library: W, He and the rounding of the warm-up to super-steps (wave_engine.hip, wave geometry) and start, w0,
    kwarm, nsteps, rk, km, ko1 and the interior condition of kw_bwd (wave_estep.hip).  The chain length B and the
    warm-up He are the plan's own (info()); if the schedule itself changes, the edges below no longer sit on the
    interior range's ends (the sums still have to add up, so the test keeps passing but checks less)."""
    W = min(L, 64)
    assert He % W == 0 and He == -(-max(HALO, L + 8) // W) * W, He
    tc = c * B
    tend = min(tc + B, T)
    te = min(tend + He, T)
    n_warm, n_total = te - tend, te - tc
    w0 = n_warm % W or W
    start = lambda k: 0 if k == 0 else w0 + (k - 1) * W
    kwarm = 0 if n_warm == 0 else 1 + (n_warm - w0) // W
    nsteps = 1 + -(-(n_total - w0) // W)
    rk = -(-L // W) + 1
    ko1 = max(nsteps - rk, kwarm)
    km = min(kwarm + rk, ko1)
    inner = [k for k in range(km, ko1) if start(k) + W <= n_total - 1]
    assert len(inner) >= 8, (km, ko1, inner)
    return te - 2 - start(inner[0]), te - 2 - start(inner[-1]) - (W - 1)


@pytest.mark.parametrize("N,K", [(4, 60), (3, 17), (4, 65)])
def test_shard_edges_around_the_interior_range(H, N, K):
    # two time shards of one recording, cut at p: the first is the whole slice owning [0, p), the second the slice
    # from sample 1024 on owning the rest.  p lies in chain 2 of the first and, 1024 lower, in chain 1 of the second,
    # at the same place of the chain's schedule: inside the interior range, and one sample either side of the first
    # and of the last interior super-step (as the end of one owned range and as the start of the other).
    import torch
    T = 6 * 1024 + 100
    y, sm, mu0 = _model(H, N, K, T)
    st = torch.cuda.current_stream().cuda_stream
    whole = H.Plan(T, sm, mu0, 0.35)
    rest = H.Plan(T - 1024, sm, mu0, 0.35)
    assert whole.info()["block"] == BLOCK and rest.info()["block"] == BLOCK
    He = whole.info()["halo"]
    assert rest.info()["halo"] == He and whole.info()["nchains"] == 7 and rest.info()["nchains"] == 6
    dy = torch.from_numpy(y).cuda()
    dr = torch.from_numpy(np.ascontiguousarray(y[1024:])).cuda()
    ref = torch.zeros(whole.stats_len(), dtype=torch.float64, device="cuda")
    whole.estep(dy, ref, st)
    torch.cuda.synchronize()
    r = ref.cpu().numpy()
    t_hi, t_lo = _interior_edges(T, BLOCK, He, K - 1, 2)
    assert _interior_edges(T - 1024, BLOCK, He, K - 1, 1) == (t_hi - 1024, t_lo - 1024)
    assert 2048 < t_lo < t_hi < 3072
    for p in [(t_hi + t_lo) // 2, t_hi, t_hi + 1, t_hi + 2, t_lo - 1, t_lo, t_lo + 1]:
        a, b = torch.zeros_like(ref), torch.zeros_like(ref)
        whole.set_shard(0, p, True, False)
        whole.estep(dy, a, st)
        rest.set_shard(p - 1024, T - 1024, False, True)
        rest.estep(dr, b, st)
        for plan in (whole, rest):
            d = plan.diagnostics(st)
            assert d[3] == 0 and d[5] == 0 and max(d[4], d[6]) < 1e-9, (p, d)
        torch.cuda.synchronize()
        t = (a + b).cpu().numpy()
        assert np.allclose(t, r, rtol=1e-9, atol=1e-12), (p, np.abs(t - r).max())
    whole.close()
    rest.close()
