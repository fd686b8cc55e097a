"""The acceptance rule of a decode against the extended-precision MAP reference (oracle/hp_viterbi.c), shared by
tests/test_hp_viterbi_cpu.py (the fp64 oracle in the device's place) and tests/test_gpu_viterbi_at_size.py.
The rule and its derivation: oracle/hp.py, compare_paths.  Nothing here is measured on the code under test.

A decode x with its ll passes against the reference path x* when
  1. x is a valid path of the transition list;
  2. on every maximal run on which they differ  -eps <= Delta <= tau  (Delta < -eps: the reference was beaten,
     reported apart, because then the reference is what is wrong);
  4. unless the case has duplicate templates, the samples inside differing runs are at most 1e-5 of T;
  5. |ll - ll*| <= 1e-9 |ll*|   (LL_RTOL of the device tests).
(3 is the definition of tau.)
"""
import numpy as np

from oracle import hp

LL_RTOL = 1e-9
CAP = 1e-5


class Ref:
    """a reference path with what the rule needs of it"""

    def __init__(self, x, ll, idx=(), cum=(), dmax=0.0, score=None):
        self.x, self.ll, self.idx, self.cum, self.dmax, self.score = np.asarray(x), ll, idx, cum, dmax, score

    @classmethod
    def live(cls, y, sm, mu, sigma, threads=1, block=1024):
        M = hp.viterbi(y, sm, mu, sigma, block=block, threads=threads, idx=np.arange(0, len(y), 64))
        return cls(M.x, M.ll, M.idx, M.cum, M.dmax, M.score)


def accept(tag, y, sm, mu, sigma, ref, x, ll, duplicates=False, model=None):
    """prints the figures, then asserts rules 1, 2, 4, 5; returns (differing samples, largest Delta/tau, ll error)"""
    model = model or hp._Model(sm, mu, sigma)
    x = np.asarray(x)
    assert x.shape == ref.x.shape
    assert hp.path_is_valid(model, x), "%s: the decode is not a valid path of the transition list" % tag
    runs = hp.compare_paths(y, model, None, None, ref.x, x, ref.idx, ref.cum, ref.dmax)
    n, worst, over, beaten = hp.judge(runs)
    ell = abs(float(hp.LD(ll) - ref.ll)) / abs(float(ref.ll))
    print("%-34s T=%-8d differing samples %d in %d runs   largest Delta/tau %.3g   ll error %.3g" % (
        tag, len(y), n, len(runs), worst, ell), flush=True)
    for r in (over + beaten)[:5]:
        print("    run [%d, %d]: Delta %.6g  tau %.3g  eps %.3g  J %d  V %.6g   ref %s  got %s" % (
            r.s, r.e, r.delta, r.tau, r.eps, r.J, r.V, ref.x[r.s:r.s + 4], x[r.s:r.s + 4]), flush=True)
    assert not beaten, "%s: THE REFERENCE WAS BEATEN on %d runs (first [%d, %d], Delta %.3g < -eps %.3g): the " \
        "reference path is not the maximum" % (tag, len(beaten), beaten[0].s, beaten[0].e, beaten[0].delta, beaten[0].eps)
    assert not over, "%s: %d runs score worse than fp64 rounding allows (first [%d, %d], Delta %.3g > tau %.3g)" % (
        tag, len(over), over[0].s, over[0].e, over[0].delta, over[0].tau)
    if not duplicates:
        assert n <= CAP * len(y), "%s: %d differing samples exceed the cap of %g T" % (tag, n, CAP)
    assert ell <= LL_RTOL, "%s: ll %r against %r" % (tag, ll, float(ref.ll))
    return n, worst, ell
