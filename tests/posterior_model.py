"""Numpy restatement of the posterior outputs (INTEGRATION.md "Posteriors") from the CPU oracle's
forward/backward (reference baumwelch.jl:25-51, :73-98).  The GPU tests compare against these; the
definitions, not the kernels, are the contract.  Checked on the oracle alone in test_posteriors_cpu.py."""
import numpy as np


def gamma(O, y, osm, mu, sigma):
    """(gamma S x T, z): gamma_t(s) = exp(alpha_t(s) + beta_t(s) - z), z = logsumexp_s alpha_{T-1}(s)"""
    al = O.forward(y, osm, mu, sigma)
    be = O.backward(y, osm, mu, sigma)
    m = al[:, -1].max()
    z = m + np.log(np.exp(al[:, -1] - m).sum())
    return np.exp(al + be - z), float(z)


def oracle_defect(g):
    """the oracle's own self-consistency: max_t |sum_s gamma_t(s) - 1|"""
    return float(np.abs(g.sum(0) - 1.0).max())


def tolerance(g):
    """absolute tolerance on probabilities: the project's E-step bar, or ten times the oracle's own rounding when
    that is larger; above the north-star bar the comparison fails whatever the oracle's defect"""
    tol = max(1e-8, 10.0 * oracle_defect(g))
    assert tol <= 1e-6, "oracle gamma self-consistent to %.3g only: no yardstick below the 1e-6 bar" % (tol / 10)
    return tol


def marginals(g, states):
    """onset (N x T), occ (N x T), silent (T) from gamma; states: N x S, 1-based phases"""
    N = states.shape[0]
    onset = np.stack([g[states[a] == 2].sum(0) for a in range(N)])
    occ = np.stack([g[states[a] > 1].sum(0) for a in range(N)])
    return onset, occ, g[0].copy()


def decode(g):
    """arg max_s gamma_t(s), 1-based, ties to the lower state number"""
    return (np.argmax(g, axis=0) + 1).astype(np.int16)


def trough_values(mu):
    """state value of each template's trough: indmin(mu[:, a]) (first minimum, extraction.jl:18), 1-based"""
    return [int(np.argmin(mu[:, a])) + 1 for a in range(mu.shape[1])]


def spike_times(x, states, mu):
    """extract_spiketimes restated: 1-based samples at which the path is in a trough state of template a"""
    x = np.asarray(x, dtype=np.int64)
    return [np.nonzero(states[a, x - 1] == q)[0] + 1 for a, q in enumerate(trough_values(mu))]


def confidence(g, states, mu, x, J):
    """per template (times, conf): conf = min(1, sum_{|d| <= J} sum_{s: states[a,s] == q_a} gamma_{t+d}(s))"""
    T = g.shape[1]
    out = []
    for a, (q, times) in enumerate(zip(trough_values(mu), spike_times(x, states, mu))):
        tq = g[states[a] == q].sum(0)
        c = np.array([min(1.0, tq[max(t - 1 - J, 0):min(t - 1 + J, T - 1) + 1].sum()) for t in times])
        out.append((times, c))
    return out
