"""The per-spike fit on the CPU (tests/spike_fit_model.py): its window and overlap rules on hand-made paths, the
two-level summary fold, the drift figures the amplitude gives on the recording D(seed, 0.4) of the drift-tracking
tests, and api.get_energy.  No GPU: the state space helpers of the library run on the host."""
import numpy as np
import pytest

import fit_adaptive_model as FA
import spike_fit_model as SF

# 2 x 5: template 0 has its trough at row 3 (qv = 3), template 1 at row 4 (qv = 4).  0.7 * MU[:, 0] is exact.
MU = np.asfortranarray(np.array([[0.0, -10.0, -30.0, -20.0, 10.0], [0.0, 1.0, -4.0, -8.0, 2.0]]).T)


@pytest.fixture(scope="module")
def table(H):
    """(states 2 x S with overlaps, sid: (phase of template 0, phase of template 1) -> 1-based state id)"""
    st = np.asarray(H.StateMatrix.create(2, 5, np.log([0.01, 0.01]), True).states)
    sid = {(int(st[0, j]), int(st[1, j])): j + 1 for j in range(st.shape[1])}
    assert len(sid) == st.shape[1] == 25 and sid[(1, 1)] == 1
    return st, sid


def used(R, e):
    return [j + 2 for j in range(len(R)) if R[j][e] is not None]


def test_events_cut_by_the_ends_of_the_array(table):
    st, sid = table
    x = np.array([sid[(3, 1)], sid[(4, 1)], sid[(5, 1)], 1, 1, 1, sid[(2, 1)], sid[(3, 1)]], dtype=np.int16)
    y = np.arange(8, dtype=np.float64)
    f = SF.fit_template(y, x, st, MU, 0)
    assert f["times"].tolist() == [1, 8] and f["nused"].tolist() == [3, 2]
    assert used(f["R"], 0) == [3, 4, 5] and used(f["R"], 1) == [2, 3]
    # the first event by hand: r = y (template 1 silent: oth = 0.0 + MU[0, 1]), m = rows 3..5
    m, r = MU[2:5, 0], y[0:3]
    assert f["amp"][0] == np.sum(r * m) / np.sum(m * m) and f["energy"][0] == 0.0 + 1.0 + 4.0
    s = f["summary"]
    assert s[:2].tolist() == [2.0, 0.0] and s[2:6].tolist() == [0.0] * 4 and s[6] == 5.0 and s[7] == 1500.0
    assert s[8 + 2 * 4:].tolist() == [1.0, 2.0, 1.0, 1.0] and s[8:12].tolist() == [6.0, 0.0 + 7.0, 1.0, 2.0]


def test_path_that_jumps_mid_spike(table):
    st, sid = table
    x = np.array([1, sid[(2, 1)], sid[(3, 1)], 1, 1, 1], dtype=np.int16)
    f = SF.fit_template(np.ones(6), x, st, MU, 0)
    assert f["times"].tolist() == [3] and f["nused"].tolist() == [2] and used(f["R"], 0) == [2, 3]


@pytest.mark.parametrize("bad", [0, 26, -3])
def test_ids_outside_the_table_inside_a_window(table, bad):
    st, sid = table
    x = np.array([1, sid[(2, 1)], sid[(3, 1)], bad, sid[(5, 1)], 1], dtype=np.int16)
    f = SF.fit_template(np.ones(6), x, st, MU, 0)
    assert f["times"].tolist() == [3] and f["nused"].tolist() == [3] and used(f["R"], 0) == [2, 3, 5]
    assert SF.fit_template(np.ones(6), x, st, MU, 1)["summary"][0] == 0.0


def test_overlap_is_taken_out_exactly(table):
    st, sid = table
    pa = [1, 1, 1, 2, 3, 4, 5, 1, 1, 1, 1]       # template 0 at samples 3..6
    pb = [1, 1, 1, 1, 1, 2, 3, 4, 5, 1, 1]       # template 1 at samples 5..8
    x = np.array([sid[(a, b)] for a, b in zip(pa, pb)], dtype=np.int16)
    ya = 0.7 * MU[np.array(pa) - 1, 0]
    assert np.all(ya == np.round(ya))            # exact: every 0.7 * m is an integer
    y = ya + MU[np.array(pb) - 1, 1]
    fa, fb = SF.spike_fit(y, x, st, MU)
    assert fa["nused"].tolist() == [4] and fb["nused"].tolist() == [4]
    smm = fa["summary"][7]
    assert abs(fa["amp"][0] - 0.7) <= 4 * np.spacing(0.7)
    assert abs(fa["rss"][0] - 0.09 * smm) <= 4 * np.spacing(0.09 * smm)
    # for template 1 the other template is taken out at the model's amplitude, 1, not at the fitted 0.7
    r_b = y[5:9] - MU[np.array(pa[5:9]) - 1, 0]
    m_b = MU[1:5, 1]
    assert fb["amp"][0] == np.sum(r_b * m_b) / np.sum(m_b * m_b)


def test_silent_trough_is_refused(table):
    st, _ = table
    mu = MU.copy()
    mu[:, 1] = np.abs(mu[:, 1])                  # minimum in row 1, the silent row
    with pytest.raises(ValueError):
        SF.fit_template(np.zeros(4), np.ones(4, dtype=np.int16), st, mu, 1)


def test_event_before_the_track_is_nan_and_counted(table):
    st, sid = table
    one = [sid[(2, 1)], sid[(3, 1)], sid[(4, 1)], sid[(5, 1)], 1]
    x = np.array([1] + one + one, dtype=np.int16)
    y = np.linspace(-1.0, 1.0, len(x))
    track = (np.array([6, 9]), np.stack([2.0 * MU, 3.0 * MU]))       # 1-based chunk starts
    f = SF.fit_template(y, x, st, MU, 0, track)
    assert f["times"].tolist() == [3, 8] and np.isnan(f["amp"][0]) and np.isnan(f["rss"][0]) and f["nused"].tolist() == [0, 4]
    # the second trough (0-based 7, sample 8) lies in chunk 0 = [6, 9): its templates serve the whole window
    g = SF.fit_template(y, x, st, 2.0 * MU, 0)
    assert f["amp"][1] == g["amp"][1] and f["summary"][0] == 2.0 and f["summary"][1] == 1.0
    assert f["summary"][7] == 1500.0             # of the base templates


def test_two_level_fold():
    rng = np.random.default_rng(7)
    st = np.array([[1, 2, 3, 4, 5]], dtype=np.int16)          # one template, ring of 4
    mu = np.asfortranarray(MU[:, :1])
    x = np.tile(np.array([2, 3, 4, 5, 1, 1], dtype=np.int16), 1000)
    y = np.tile(np.concatenate([MU[1:, 0], [0.0, 0.0]]), 1000) * np.repeat(rng.uniform(0.5, 1.5, 1000), 6)
    y = y + rng.standard_normal(len(y))
    f = SF.fit_template(y, x, st, mu, 0)
    assert len(f["amp"]) == 1000 and np.all(f["nused"] == 4)

    def stated(v):   # blocks of 256, serial inside (cumsum is a serial left fold), serial over the partials
        parts = [np.cumsum(v[b:b + 256])[-1] for b in range(0, len(v), 256)]
        return np.cumsum(np.array([0.0] + parts))[-1]

    def flat(v):
        return np.cumsum(v)[-1]

    cols = [f["amp"], f["amp"] * f["amp"], f["rss"], f["energy"]]
    assert [stated(c) for c in cols] == f["summary"][2:6].tolist()
    assert any(flat(c) != stated(c) for c in cols)
    rr = np.array(f["R"][1])
    assert f["summary"][8 + 1] == stated(rr) and f["summary"][8 + 4 + 1] == stated(rr * rr)
    assert f["summary"][[0, 1, 6]].tolist() == [1000.0, 1000.0, 4000.0] and np.all(f["summary"][16:] == 1000.0)


@pytest.fixture(scope="module")
def drift(O, H):
    out = {}
    sm = O.state_matrix(2, FA.K_D, np.log(FA.PP_D), False)
    for seed in (1, 2, 3):
        y, onsets, temps = FA.drifting(H, seed, 0.4)
        x, _ll = O.viterbi(y, sm, temps, FA.SIGMA_D)
        out[seed] = (y, temps, SF.spike_fit(y, x, np.asarray(sm.states), temps))
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_amplitude_follows_the_drift(drift, seed):
    y, temps, fits = drift[seed]
    gain = np.linspace(1.0, 0.4, len(y))
    for a, f in enumerate(fits):
        assert len(f["amp"]) > 100 and np.all(f["nused"] == FA.K_D - 1)
        onset = f["times"] - 1 - (SF.trough_value(temps, a) - 1)
        z = (f["amp"] - gain[onset]) / (FA.SIGMA_D / np.sqrt(f["summary"][7]))
        late = f["amp"][f["times"] - 1 >= 32_000]
        print("seed %d template %d: %d events, rms z %.3f, max |z| %.3f, late median amp %.3f"
              % (seed, a, len(z), np.sqrt(np.mean(z * z)), np.abs(z).max(), np.median(late)))
        assert 0.85 <= np.sqrt(np.mean(z * z)) <= 1.15 and np.abs(z).max() <= 4.0
        assert np.median(late) < 0.7


def test_get_energy_against_a_literal_loop(H):
    rng = np.random.default_rng(3)
    W = rng.standard_normal((60, 5)) * 40.0
    ee = H.get_energy(W, 0.0123)
    assert ee.shape == (5,) and np.array_equal(ee, SF.get_energy(W, 0.0123))
    assert np.array_equal(H.get_energy(np.asfortranarray(W), 0.0123), ee)


def test_quality_from_summary(H):
    K, P = 5, 4
    s = np.concatenate([[10, 8, 7.2, 6.6, 40.0, 90.0, 38, 2.0], np.full(P, 9.0), np.full(P, 9.9), np.full(P, 9.0)])
    q = H.quality_from_summary(s, K, 0.5)
    assert (q.n, q.n_full) == (10, 8) and q.mean_amp == 7.2 / 8 and q.sd_expected == 0.5 / np.sqrt(2.0)
    assert abs(q.sd_amp - np.sqrt(6.6 / 8 - 0.81)) < 1e-12 and q.chi2 == 40.0 / (0.25 * 4 * 8) and q.energy == 8.0
    assert np.allclose(q.waveform, 1.0) and np.allclose(q.waveform_sd, np.sqrt(0.1))
