"""The template seed on the device (csrc/seed_templates.hip) against the numpy model of seed_model.py: the exact
median, detection with ties and plateaux across every tile edge, the window-edge rule, both sample types, bit-for-bit
repeatability, the realistic recordings of the DESIGN table, and the layers on top -- train_model(init="detect") with
both methods and sortdata.learn_templates -> sort_data.

What is compared how: event times, sigma, n_events, iterations, labels and counts are equal to the model's exactly
(on float signals that is fair because test_seed_cpu.py shows every assignment is decided by a margin >= 1e-9; on
the integer signals sums are exact in any order, so even ties fall the same way).  mu is within 1e-12 max|mu| (the
centre sums are ordered differently); lp within 4 ulp (one division, one log).

End-to-end figures measured on the MI355X are recorded in DESIGN.md "Template seed"."""
import numpy as np
import pytest

import seed_cases as SC
import seed_model as SM

pytestmark = pytest.mark.gpu


def run(H, y, N, K, **opts):
    """the C ABI's outputs for all N clusters, through api.seed_templates"""
    sm, mu, sigma, info = H.seed_templates(y, N, K, **opts)
    raw = info["raw"]
    return dict(mu=raw["mu"], lp=raw["lp"], counts=raw["counts"], sigma=sigma, times=info["times"],
                labels=info["raw_labels"], n_events=info["n_events"], iters=info["iters"], sm=sm, kept_mu=mu,
                info=info)


def same(g, r, what=""):
    assert g["n_events"] == r["n_events"], what
    assert g["sigma"] == r["sigma"], what
    assert np.array_equal(g["times"], r["times"]), what
    assert g["iters"] == r["iters"], what
    assert np.array_equal(g["labels"], r["labels"]), what
    assert np.array_equal(g["counts"], r["counts"]), what
    assert g["mu"].shape == r["mu"].shape and np.all(g["mu"][0] == 0), what
    scale = np.abs(r["mu"]).max()
    assert np.abs(g["mu"] - r["mu"]).max() <= 1e-12 * scale, what
    fin = np.isfinite(r["lp"])
    assert np.array_equal(np.isneginf(g["lp"]), ~fin), what
    assert np.all(np.abs(g["lp"][fin] - r["lp"][fin]) <= 4 * np.spacing(np.abs(r["lp"][fin]))), what


@pytest.mark.parametrize("K", SC.ADV_K)
def test_adversarial_integer_signals(H, K):
    D, N = K - 1, 3
    parities = set()
    for T in SC.adversarial_T(K):
        y = SC.adversarial(K, T)
        parities.add(T % 2)
        for polarity in (-1, 0, 1):
            for align in sorted({0, D // 3, D - 1}):
                g = run(H, y, N, K, threshold=1.0, polarity=polarity, align=align)
                r = SM.seed_model(y, N, K, threshold=1.0, polarity=polarity, align=align)
                same(g, r, (K, T, polarity, align))
        # the default refractory leaves few events in such a signal; a short one gives hundreds, closer together
        # than a snippet is long, and many equal distances
        for R in (1, 2):
            g = run(H, y, N, K, threshold=1.0, refractory=R)
            r = SM.seed_model(y, N, K, threshold=1.0, refractory=R)
            same(g, r, (K, T, "refractory", R))
            assert T < 1000 or r["n_events"] > T // 100
    assert parities == {0, 1}
    # fewer events than clusters: duplicate starting centres, empty clusters that keep theirs
    y = np.zeros(4 * K + 10, dtype=np.int16)
    y[2 * K] = 7
    g, r = run(H, y, N, K, sigma=1.0), SM.seed_model(y, N, K, sigma=1.0)
    assert r["n_events"] == 1 and r["counts"].tolist() == [1, 0, 0]
    same(g, r, "one event")
    assert g["sm"].N == 1 and g["kept_mu"].shape == (K, 1)


def test_no_event(H):
    for y in (np.zeros(5000, dtype=np.int16), np.zeros(4097)):
        g = run(H, y, 3, 20)
        same(g, SM.seed_model(y, 3, 20), "zeros")
        assert g["n_events"] == 0 and g["sigma"] == 0.0 and np.all(g["mu"] == 0) and np.all(g["counts"] == 0)
        assert np.all(np.isneginf(g["lp"])) and g["iters"] == 0
        assert g["sm"].N == 0 and g["sm"].nstates == 1 and g["kept_mu"].shape == (20, 0)


@pytest.mark.parametrize("K,align", [(20, 6), (60, 0), (257, 255)])
def test_window_edges(H, K, align):
    """a snippet must lie inside the recording: t - align >= 0 and t - align + D - 1 <= T - 1, so the accepted
    event samples are exactly align .. T - D + align"""
    D, T = K - 1, 3000
    for t, ok in ((align - 1, False), (align, True), (T - D + align - 1, True), (T - D + align, True),
                  (T - D + align + 1, False)):
        if t < 0 or t >= T:
            continue
        y = np.zeros(T)
        y[t] = 9.0
        g = run(H, y, 1, K, sigma=1.0, align=align, polarity=1)
        same(g, SM.seed_model(y, 1, K, sigma=1.0, align=align, polarity=1), (K, t))
        assert g["n_events"] == int(ok), (K, align, t)
        if ok:
            assert g["times"].tolist() == [t + 1] and g["mu"][1 + align, 0] == 9.0


def test_f64_against_i16_and_determinism(H):
    y16 = SC.adversarial(60, 20011)
    a = run(H, y16, 4, 60, threshold=1.0, refractory=2)
    b = run(H, y16.astype(np.float64), 4, 60, threshold=1.0, refractory=2)
    for k in ("mu", "lp", "counts", "times", "labels"):
        assert np.array_equal(a[k], b[k]), k
    assert a["sigma"] == b["sigma"] and a["iters"] == b["iters"] and a["n_events"] == b["n_events"] > 4
    y, _, _ = SC.realistic("k60")
    c, d = run(H, y, 7, 60), run(H, y, 7, 60)
    assert c["mu"].tobytes() == d["mu"].tobytes() and c["lp"].tobytes() == d["lp"].tobytes()


@pytest.mark.parametrize("N", SC.GPU_N)
@pytest.mark.parametrize("name", SC.GPU_REALISTIC)
def test_realistic_equals_model(H, name, N):
    import torch
    y, _, _ = SC.realistic(name)
    K = SC.REALISTIC[name][0]
    r = SC.realistic_model(name, N)
    assert r["margin"] >= 1e-9
    g = run(H, y, N, K)
    same(g, r, (name, N))
    dy = torch.from_numpy(np.array(y)).cuda()
    sm, mu, sigma, info = H.device.seed_templates(dy, N, K)
    assert mu.tobytes() == g["kept_mu"].tobytes() and sigma == g["sigma"]
    assert info["raw"]["mu"].tobytes() == g["mu"].tobytes() and np.array_equal(info["raw"]["lp"], g["lp"])
    assert np.array_equal(info["times"], g["times"]) and np.array_equal(info["raw_labels"], g["labels"])
    assert np.array_equal(info["counts"], g["info"]["counts"]) and sm.N == g["sm"].N
    assert np.array_equal(sm.transitions, g["sm"].transitions)
    # the kept clusters, their labels and the state matrix built from their entry log-probabilities
    kept = info["kept"]
    assert np.array_equal(kept, np.nonzero(r["counts"] > 0)[0]) and sm.K == K and not sm.resolve_overlaps
    assert np.array_equal(np.bincount(info["labels"], minlength=len(kept)), r["counts"][kept])


def onset_counts(H, y, sm, mu, sigma):
    model = H.fit(H.HMMSpikeTemplateModel(sm, mu, sigma), np.asarray(y))
    return np.array([len(t) for t in H.extract_spiketimes(model)])


@pytest.mark.parametrize("overlaps", (False, True))
@pytest.mark.parametrize("name", SC.GPU_REALISTIC)
def test_viterbi_training_from_the_seed(H, name, overlaps):
    """Measured on the MI355X (generating counts 145 / 43 at K = 60, 93 / 30 at K = 20): see DESIGN.md."""
    y, temps, true = SC.realistic(name)
    K = SC.REALISTIC[name][0]
    seed_err, _ = SM.match_errors(SC.realistic_model(name, 2)["mu"], temps)
    sm, mu, sigma = H.train_model(np.array(y), 2, K, overlaps, 4, method="viterbi", init="detect", postprocess=None)
    assert sm.N == 2 and mu.shape == (K, 2) and np.all(np.isfinite(mu)) and np.isfinite(sigma)
    err, col = SM.match_errors(mu, temps)
    counts = onset_counts(H, y, sm, mu, sigma)[col]
    print(name, "overlaps" if overlaps else "ring", "counts", counts, "generating", true, "errors", err,
          "seed errors", seed_err, "sigma", sigma)
    assert sorted(col) == [0, 1]                                    # no template lost, none doubled
    assert np.all(np.abs(counts - true) <= 0.05 * true)
    assert np.all(err <= seed_err + 0.02)


def test_random_start_is_unchanged(H):
    y, _, _ = SC.realistic("k20")
    with pytest.raises(ValueError, match="needs a model to refine"):
        H.train_model(np.array(y), 2, 20, False, 4, method="viterbi")


def test_soft_training_from_the_seed(H):
    y, temps, _ = SC.realistic("k20")
    sm, mu, sigma = H.train_model(np.array(y), 2, 20, False, 2, init="detect")
    print("soft: N", sm.N, "sigma", sigma, "errors", SM.match_errors(mu, temps) if sm.N else None)
    assert sm.N == 2 and mu.shape == (20, 2) and np.all(np.isfinite(mu)) and np.isfinite(sigma) and sigma > 0


def test_learn_then_sort(H):
    y, temps, true = SC.realistic("k20")
    d = H.learn_templates(np.array(y), 2, 20, nsteps=4, method="viterbi", resolve_overlaps=True)
    assert d["spikeForms"].shape == (20, 1, 2) and d["cinv"].shape == (1,) and d["p"].shape == (2,)
    assert np.all(d["p"] > 0) and np.all(d["p"] < 1) and d["cinv"][0] > 0
    out = H.sort_data(d["spikeForms"], d["cinv"], d["p"], np.array(y), dosave=False)
    assert set(out) == {"mlseq", "ll", "waveforms", "lp", "sigma"}
    assert out["mlseq"].shape == (2, len(y))
    _, col = SM.match_errors(d["spikeForms"][:, 0, :], temps)
    counts = np.array([np.count_nonzero(out["mlseq"][a] == 2) for a in range(2)])[col]
    print("learn -> sort: counts", counts, "generating", true)
    assert sorted(col) == [0, 1] and np.all(np.abs(counts - true) <= 0.05 * true)
