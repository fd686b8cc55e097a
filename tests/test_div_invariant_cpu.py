"""div_invariant (csrc/fastmath.h): the Viterbi sweep divides (y - mean0)^2 by the chain's invariant 2 sigma^2 with
one reciprocal per chain and a product and two fused multiply-adds per sample.  The quotient must have the bits of
the IEEE division, or the decoded path could change.  The function is __host__ __device__, so a plain host program
(tests/div_invariant_check.cpp) runs the very code of the kernel:

* divisors: 2 * 0.3^2 (the headline sigma), its two neighbours in the last place, 64 random ones in [1e-3, 1e3]
  and two outside the range div_invariant_of accepts (which must fall back to the division);
* numerators: 10^7 per divisor -- bit patterns below 2^-20 down to subnormals and zero, log-uniform up to 30,
  uniform in [0, 30], up to 1e6, squares of single-precision differences, and the specials (the range limits of
  the fast path, the largest double, infinity, NaN);
* the same program once more under AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone host program,
  nothing preloaded), with fewer numerators.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "hmmspikesorter.jl_amd", "csrc")
SRC = os.path.join(HERE, "div_invariant_check.cpp")
N_FULL = 10_000_000
N_SAN = 200_000
N_DIVISORS = 3 + 64 + 2


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    return " fma " in line + " "
    except OSError:
        pass
    return False


def _build(tmp_path, name, extra):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the host check"
    exe = str(tmp_path / name)
    # -ffp-contract=off as the library's own build: only the fma calls that are written out may fuse
    cmd = [cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, SRC, "-o", exe] + extra
    if _cpu_has_fma():
        cmd.append("-mfma")        # __builtin_fma as one instruction (otherwise libm's fma: same result, slower)
    subprocess.check_call(cmd)
    return exe


def _run(exe, n):
    p = subprocess.run([exe, str(n)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:]
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "checked" and int(last[1]) == n * N_DIVISORS and int(last[5]) == 0, last
    # most numerators must have gone through the fast path, or the check says nothing about it
    assert int(last[3]) > 0.7 * n * (N_DIVISORS - 2), last


def test_quotients_have_the_bits_of_the_division(tmp_path):
    _run(_build(tmp_path, "div_invariant_check", ["-fopenmp"]), N_FULL)


def test_the_host_check_is_clean_under_sanitizers(tmp_path):
    exe = _build(tmp_path, "div_invariant_check_san",
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _run(exe, N_SAN)
