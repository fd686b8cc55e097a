// Host check of div_invariant (csrc/fastmath.h): the quotient by a divisor whose reciprocal was taken once must
// have the bits of the IEEE division.  Built and run by tests/test_div_invariant_cpu.py; the function is the one
// the Viterbi sweep calls on the device.
//   usage: div_invariant_check <numerators per divisor> [den ...]     (divisors as hex floats; none: the built-in set)
// Prints one line "checked <n> mismatches <m>" and up to ten mismatching cases; exit status 1 on a mismatch.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fastmath.h"

static inline uint64_t splitmix(uint64_t &s)
{
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static inline double unit(uint64_t &s) { return (double)(splitmix(s) >> 11) * 0x1p-53; }   // [0, 1)
static inline uint64_t bits(double v) { uint64_t b; memcpy(&b, &v, sizeof b); return b; }

// numerator i of n: a tenth each of random bit patterns below 2^-20 (subnormals and zero included: dense near 0),
// log-uniform in [2^-60, 30] and log-uniform in [30, 1e6]; half uniform in [0, 30], where (y - mean)^2 of a
// recording lies; a tenth uniform in [0, 1e6]; a tenth squares of single-precision differences; and a few specials
static double numerator(int64_t i, int64_t n, uint64_t &s)
{
    static const double special[] = {0.0, 0x1p-1074, 0x1p-1022, 0x0.fffffffffffffp-1022, 0x1p-800, 0x1.fffffffffffffp-801,
                                     0x1p800, 0x1.0000000000001p800, 0x1.fffffffffffffp1023, INFINITY, NAN, 1.0, 30.0, 1e6};
    const int ns = (int)(sizeof(special) / sizeof(special[0]));
    if (i < ns) return special[i];
    const int64_t k = (i * 10) / n;
    double v;
    switch (k) {
    case 0: { uint64_t b = splitmix(s) % bits(0x1p-20); memcpy(&v, &b, sizeof v); return v; }
    case 1: return exp2(-60.0 + unit(s) * (60.0 + log2(30.0)));
    case 2: return exp2(log2(30.0) + unit(s) * (log2(1e6) - log2(30.0)));
    case 3: return unit(s) * 1e6;
    case 4: { const float a = (float)(unit(s) * 8.0 - 4.0), b = (float)(unit(s) * 0.5); const double d = (double)a - (double)b; return d * d; }
    default: return unit(s) * 30.0;
    }
}

int main(int argc, char **argv)
{
    const int64_t n = argc > 1 ? atoll(argv[1]) : 10000000;
    std::vector<double> dens;
    for (int i = 2; i < argc; i++) dens.push_back(strtod(argv[i], nullptr));
    if (dens.empty()) {
        const double d0 = 2.0 * 0.3 * 0.3;
        dens = {d0, nextafter(d0, 0.0), nextafter(d0, 1.0)};
        uint64_t s = 12345;
        for (int i = 0; i < 64; i++) dens.push_back(exp2(log2(1e-3) + unit(s) * (log2(1e3) - log2(1e-3))));
        dens.push_back(0x1p-300);   // outside div_invariant_of's range: every quotient takes the division
        dens.push_back(0x1p+300);
    }
    int64_t bad = 0, fast = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : bad, fast)
    for (size_t j = 0; j < dens.size(); j++) {
        const hmmsort::DivInv dv = hmmsort::div_invariant_of(dens[j]);
        uint64_t s = 0x1234567ull * (j + 1);
        for (int64_t i = 0; i < n; i++) {
            const double x = numerator(i, n, s);
            volatile double den = dens[j];          // a division the compiler cannot turn into anything else
            const double want = x / den, got = hmmsort::div_invariant(x, dv);
            fast += (x >= dv.nlo && x <= 0x1p800) ? 1 : 0;
            if (bits(want) != bits(got)) {
#pragma omp critical
                if (bad++ < 10) printf("mismatch: %a / %a = %a, div_invariant %a\n", x, dens[j], want, got);
            }
        }
    }
    printf("checked %" PRId64 " fast %" PRId64 " mismatches %" PRId64 "\n", n * (int64_t)dens.size(), fast, bad);
    return bad ? 1 : 0;
}
