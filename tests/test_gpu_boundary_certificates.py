"""The boundary certificates of the wave engine still bite: the forward/backward certificate (kw_fb_check,
diag[3..6]) and the Viterbi certificate (kw_vit_check, diag[0..2]) on the
busy signal of test_busy_signal_certificate_and_escalation with warm-ups that are too short, with the default
geometry, and on a plan of exactly two chains (chain 0, which has no boundary, and one boundary)."""
import numpy as np
import pytest

from conftest import four_templates, to_oracle_sm

pytestmark = pytest.mark.gpu

COUNTERS = (0, 1, 3, 5, 7)   # diag entries that count events; 2, 4, 6 are the largest errors seen


@pytest.fixture(autouse=True)
def wave_engine(H):
    H.set_option("engine", H.ENGINE_WAVE)
    H.set_option("block", 0)
    H.set_option("halo", 0)
    yield
    H.set_option("engine", H.ENGINE_AUTO)
    H.set_option("block", 0)
    H.set_option("halo", 0)


@pytest.fixture(scope="module")
def busy(H):
    K, N, T = 60, 4, 40_000
    temps = four_templates(H, K)
    pp = [0.03, 0.02, 0.025, 0.02]
    y = H.create_signal(T, 0.3, pp, temps, seed=21)
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    return y, sm, temps, mu


def _estep_twice(H, y, sm, mu, sigma):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    plan = H.Plan(len(y), sm, mu, sigma)
    dy = torch.from_numpy(y).cuda()
    s1 = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
    s2 = torch.zeros_like(s1)
    plan.estep(dy, s1, st)
    diag = plan.diagnostics(st)
    plan.estep(dy, s2, st)
    info = plan.info()
    plan.close()
    return s1.cpu().numpy(), s2.cpu().numpy(), diag, info


def test_short_warmup_on_a_busy_signal_is_flagged(H, busy):
    y, sm, temps, mu = busy
    H.set_option("block", 128)
    H.set_option("halo", 128)
    s1, s2, diag, info = _estep_twice(H, y, sm, mu, 0.35)
    print("block 128, halo 128:", info, diag)
    assert info["nchains"] > 100
    # a certificate fails exactly when its posterior-weighted error (an L1 distance of two distributions, so at
    # most 2) exceeds 1e-9
    assert (diag[3] + diag[5] > 0) == (max(diag[4], diag[6]) > 1e-9), diag
    assert 0.0 <= max(diag[4], diag[6]) <= 2.0, diag
    # warm-ups of two ring lengths from a flat start do not reproduce the neighbour's state on this signal to the
    # last bit: both directions of the certificate see a mismatch (a check that computed 0 everywhere fails here)
    assert diag[4] > 0.0 and diag[6] > 0.0, diag
    assert np.array_equal(s1, s2)


def test_default_geometry_on_a_busy_signal_is_clean(H, busy):
    y, sm, temps, mu = busy
    s1, s2, diag, info = _estep_twice(H, y, sm, mu, 0.35)
    print("default geometry:", info, diag)
    assert all(diag[i] == 0 for i in COUNTERS), diag
    assert 0.0 <= max(diag[4], diag[6]) <= 1e-9, diag
    assert np.array_equal(s1, s2)


def test_short_viterbi_warmup_is_counted_without_escalation(H, busy):
    import torch
    y, sm, temps, mu = busy
    H.set_option("block", 128)
    H.set_option("halo", 64)
    st = torch.cuda.current_stream().cuda_stream
    plan = H.Plan(len(y), sm, temps, 0.3)     # plan API: flags only, no retry with a longer warm-up
    dy = torch.from_numpy(y).cuda()
    dx = torch.zeros(len(y), dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    plan.viterbi(dy, dx, dll, st)
    diag = plan.diagnostics(st)
    plan.close()
    print("block 128, halo 64:", diag)
    assert diag[0] > 0, diag


def test_two_chains_one_boundary(O, H):
    import torch
    K, N = 60, 4
    temps = four_templates(H, K)
    pp = [0.006, 0.004, 0.005, 0.003]
    sm = H.StateMatrix.create(N, K, np.log(pp), False)
    probe = H.Plan(4096, sm, temps, 0.3)
    B = probe.info()["block"]
    probe.close()
    T = B + 100                                # just above one chain
    y = H.create_signal(T, 0.3, pp, temps, seed=9)
    y[B - 30:B + 29] += 1.5 * temps[1:, 1]     # a ring running across the boundary
    mu = np.asfortranarray(temps * 0.9)
    mu[0, :] = 0
    st = torch.cuda.current_stream().cuda_stream
    dy = torch.from_numpy(y).cuda()
    dx = torch.zeros(T, dtype=torch.int16, device="cuda")
    dll = torch.zeros(1, dtype=torch.float64, device="cuda")
    plan = H.Plan(T, sm, temps, 0.3)
    assert plan.info()["nchains"] == 2 and plan.info()["block"] == B
    plan.viterbi(dy, dx, dll, st)
    dv = plan.diagnostics(st)
    plan.close()
    plan = H.Plan(T, sm, mu, 0.4)
    stats = torch.zeros(plan.stats_len(), dtype=torch.float64, device="cuda")
    out = torch.zeros(plan.mstep_len(), dtype=torch.float64, device="cuda")
    plan.estep(dy, stats, st)
    plan.mstep(stats, out, st)
    de = plan.diagnostics(st)
    plan.close()
    assert all(dv[i] == 0 for i in COUNTERS) and all(de[i] == 0 for i in COUNTERS), (dv, de)
    assert 0.0 <= max(de[4], de[6]) <= 1e-9, de
    osm = to_oracle_sm(O, sm)
    xo, llo = O.viterbi(y, osm, temps, 0.3)
    x, ll = dx.cpu().numpy(), float(dll.cpu()[0])
    assert np.array_equal(x, xo) and abs(ll - llo) <= 1e-9 * abs(llo)
    assert xo[B - 1] > 1 and xo[B] > 1
    osmn, omu, osig, olp, opp = O.train_step(y, osm, mu.copy(order="F"), 0.4)
    o = out.cpu().numpy()
    mun = o[:K * N].reshape((K, N), order="F")
    assert np.allclose(mun, omu, rtol=1e-8, atol=1e-11), np.abs(mun - omu).max()
    assert abs(o[K * N] - osig) <= 1e-8 * osig
