"""Pre-pass tiling of the wave engine: recordings whose length sits on, just before and just after a multiple of
the pre-pass tile (256 threads x 8 onsets = 2 048 samples up to 4 rings, x 4 = 1 024 above), where the tile's
tail of L samples, the truncated rings of the last onsets (kmax < L) and the `interior` switch of a tile change
sides; spikes across a tile edge, before the first and past the last sample (the virtual onsets are computed by
the first workgroup of the pre-pass grid); a batched plan with two models.  Everything against the CPU oracle,
as in test_gpu_wave_edges.py: exact path, log-likelihood to 1e-9, the EM step to 1e-8."""
import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def wave_engine(H):
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", 0)
    H.set_option("halo", 0)
    yield
    H.set_option("engine", H.ENGINE_AUTO)
    H.set_option("block", 0)
    H.set_option("halo", 0)


def _templates(H, N, K):
    if N == 4:
        return four_templates(H, K)
    base = [(3.0, 0.8, 0.2), (4.0, 0.3, 0.2), (2.5, 0.6, 0.25), (3.5, 0.5, 0.15)]
    return np.asfortranarray(np.stack([H.create_spike_template(K, base[i % 4][0] * (1 + 0.15 * (i // 4)),
                                                                 base[i % 4][1] + 0.04 * (i // 4), base[i % 4][2])
                                        for i in range(N)], 1))


def _rates(N):
    return (np.array([0.006, 0.004, 0.005, 0.003, 0.004, 0.005, 0.003, 0.004])[:N] * min(1.0, 4.0 / N)).tolist()


def _check(O, H, y, sm, temps, sigma=0.3):
    osm = to_oracle_sm(O, sm)
    x, ll = H.viterbi(y, sm, temps, sigma)
    xo, llo = O.viterbi(y, osm, temps, sigma)
    assert np.array_equal(x, xo), int(np.count_nonzero(x != xo))
    assert abs(ll - llo) <= 1e-9 * abs(llo)
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    smn, mun, sgn = H.train_step(y, sm, mu.copy(order="F"), sigma + 0.1)
    osmn, omu, osig, olp, opp = O.train_step(y, osm, mu.copy(order="F"), sigma + 0.1)
    assert H.get_option("last_escalations") == 0
    assert np.allclose(mun, omu, rtol=1e-8, atol=1e-11), np.abs(mun - omu).max()
    assert abs(sgn - osig) <= 1e-8 * osig
    assert np.allclose(smn.transitions["lp"], osmn.val, rtol=1e-8)
    assert np.allclose(smn.pi, opp, rtol=1e-8, atol=1e-8)
    return xo


def _lengths(tile, L):
    # T = tile * m + r; with m = 1 and r = L - 1, L, L + 1 the first tile stops / starts being `interior`
    out = [512]    # the shortest recording a plan takes (512 samples, at least four ring lengths)
    for m in (1, 2, 3):
        for r in (0, 1, L - 1, L, L + 1, tile - 1):
            out.append(tile * m + r)
    return out


CASES = [(4, 60, T) for T in _lengths(2048, 59)] + [(8, 24, T) for T in _lengths(1024, 23)]


@pytest.mark.parametrize("N,K,T", CASES)
def test_lengths_around_the_prepass_tile(O, H, N, K, T):
    temps = _templates(H, N, K)
    pp = _rates(N)
    y = H.create_signal(T, 0.3, pp, temps, seed=T + N)
    L = K - 1
    y[T - L - 3:T - 3] += 1.2 * temps[1:, 0]      # a whole spike among the last onsets with full rings
    y[T - L // 2:] += 1.2 * temps[1:1 + L // 2, 1]   # and one the recording cuts in half (kmax < L)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    _check(O, H, y, sm, temps)


@pytest.mark.parametrize("N,K,edge", [(4, 60, 2048), (8, 24, 1024)])
def test_spikes_across_a_tile_edge_and_both_ends(O, H, N, K, edge):
    temps = _templates(H, N, K)
    pp = _rates(N)
    L = K - 1
    T = edge + 300
    y = H.create_signal(T, 0.3, pp, temps, seed=edge)
    half = L // 2
    y[edge - half - 40:edge + half + 40] = 0.3 * np.random.default_rng(edge).standard_normal(2 * half + 80)
    y[edge - half:edge - half + L] += 1.5 * temps[1:, 2]   # onset in one tile, end in the next
    y[:L - half] += 1.5 * temps[1 + half:, 0]              # tail of a spike that began before the recording
    y[T - half:] += 1.5 * temps[1:1 + half, 1]             # head of a spike that runs past the end
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    xo = _check(O, H, y, sm, temps)
    # the decode really starts and ends inside rings, and a ring is running at the tile edge
    assert xo[0] > 1 and xo[-1] > 1 and xo[edge - 1] > 1 and xo[edge] > 1


def test_two_channel_plan_with_two_models(O, H):
    import torch
    N, K, T = 4, 60, 2048 * 2 + 61
    temps = [_templates(H, N, K), np.asfortranarray(_templates(H, N, K)[:, ::-1] * 1.1)]
    pps = [_rates(N), [0.003, 0.006, 0.004, 0.005]]
    sigmas = [0.3, 0.35]
    sms = [H.StateMatrix.create(N, K, np.log(pp), False) for pp in pps]
    ys = np.stack([H.create_signal(T, 0.3, pps[c], temps[c], seed=70 + c) for c in range(2)])
    for c in range(2):
        ys[c, T - 25:] += temps[c][1:26, c]
        ys[c, :30] += temps[c][K - 30:, c + 1]
    mus = [np.asfortranarray(t * 0.9) for t in temps]
    for m in mus:
        m[0, :] = 0
    st = torch.cuda.current_stream().cuda_stream
    dy = torch.from_numpy(ys).cuda()
    # the decode with the templates, the EM step from the perturbed means (two plans, as the host calls do it)
    plan = H.Plan.batched(T, sms, temps, sigmas)
    dx = torch.zeros((2, T), dtype=torch.int16, device="cuda")
    dll = torch.zeros(2, dtype=torch.float64, device="cuda")
    plan.viterbi(dy, dx, dll, st)
    dg = plan.diagnostics(st)
    plan.close()
    assert dg[0] == 0 and dg[7] == 0, dg
    plan = H.Plan.batched(T, sms, mus, [s + 0.1 for s in sigmas])
    stats = torch.zeros(2 * plan.stats_len(), dtype=torch.float64, device="cuda")
    out = torch.zeros(2 * plan.mstep_len(), dtype=torch.float64, device="cuda")
    dx2 = torch.zeros((2, T), dtype=torch.int16, device="cuda")
    dll2 = torch.zeros(2, dtype=torch.float64, device="cuda")
    plan.decode_estep(dy, dx2, dll2, stats, st)
    plan.mstep(stats, out, st)
    dg = plan.diagnostics(st)
    plan.close()
    assert dg[0] == 0 and dg[3] == 0 and dg[5] == 0 and dg[7] == 0, dg
    x, ll, o = dx.cpu().numpy(), dll.cpu().numpy(), out.cpu().numpy().reshape(2, -1)
    for c in range(2):
        osm = to_oracle_sm(O, sms[c])
        xo, llo = O.viterbi(ys[c], osm, temps[c], sigmas[c])
        assert np.array_equal(x[c], xo), (c, int(np.count_nonzero(x[c] != xo)))
        assert abs(ll[c] - llo) <= 1e-9 * abs(llo)
        osmn, omu, osig, olp, opp = O.train_step(ys[c], osm, mus[c].copy(order="F"), sigmas[c] + 0.1)
        mun = o[c, :K * N].reshape((K, N), order="F")
        assert np.allclose(mun, omu, rtol=1e-8, atol=1e-11), (c, np.abs(mun - omu).max())
        assert abs(o[c, K * N] - osig) <= 1e-8 * osig
