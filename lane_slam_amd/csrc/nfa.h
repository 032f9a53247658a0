// The number of false alarms of a rectangle with n pixels of which k are aligned: the binomial tail both line detectors validate
// with -- LSD (lsd_grow.h: OpenCV lsd.cpp nfa, restated in oracle/lf_oracle_lsd.c) and EDLines (k_edlines.hip: the reference's
// line_descriptor/descriptor_custom.hpp:630-813, restated in oracle/lf_oracle_edlines.c).  Every transcendental goes through
// detmath.h, so host and device give the same bits.  Host and device, like detmath.h: no HIP header when g++ compiles it
// (tests/hostsim builds lsd_grow.h, tests/hostsim/nfa_host.cpp this file).
#pragma once
#include "detmath.h"

namespace lf {

LF_HD double dabs(double v) { return v < 0 ? -v : v; }

// equal up to 100 units of relative rounding error
LF_HD bool double_equal(double a, double b)
{
    if (a == b) return true;
    const double abs_diff = dabs(a - b), aa = dabs(a), bb = dabs(b);
    double abs_max = aa > bb ? aa : bb;
    const double DBL_MIN_ = 2.2250738585072014e-308, DBL_EPS_ = 2.2204460492503131e-16;
    if (abs_max < DBL_MIN_) abs_max = DBL_MIN_;
    return (abs_diff / abs_max) <= (100.0 * DBL_EPS_);
}

LF_HD double log_gamma_lanczos(double x)
{
    const double q[7] = { 75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424, 2.50662827511 };
    double a = (x + 0.5) * dm::dlog(x + 5.5) - (x + 5.5);
    double b = 0;
    for (int n = 0; n < 7; ++n) {
        a -= dm::dlog(x + (double)n);
        b += q[n] * dm::dpow(x, (double)n);
    }
    return a + dm::dlog(b);
}
LF_HD double log_gamma_windschitl(double x)
{
    return 0.918938533204673 + (x - 0.5) * dm::dlog(x) - x + 0.5 * x * dm::dlog(x * dm::dsinh_small(1 / x) + 1 / (810.0 * dm::dpow(x, 6.0)));
}
LF_HD double log_gamma(double x) { return x > 15.0 ? log_gamma_windschitl(x) : log_gamma_lanczos(x); }

// -log10(NT * B(n, k, p)): B the tail of the binomial distribution, log_nt = log10 of the number of tests.
//
// kPlainFirstTerm: the first term of log(n choose k).
//   false  log_gamma(n + 1), the logarithm of n!.  EDLines (ed_nfa, k_edlines.hip): descriptor_custom.hpp:774 has it, and so has
//          oracle/lf_oracle_edlines.c.
//   true   n + 1 itself.  LSD (nfa_eval, lsd_grow.h), as oracle/lf_oracle_lsd.c states it.
// Each detector is held to its own oracle bit for bit (tests/test_nfa_cpu.py, the detectors' GPU tests): the difference is
// intended.  Do NOT unify the two forms -- making one "match" the other changes which lines that detector accepts.
//
// kLogGamma: log_gamma above, or a caller's out-of-line wrapper of it (ed_log_gamma: three calls inlined would double the code
// k_ed_detect's fitting loop reaches; nfa_eval has two and is out of line itself).
template <bool kPlainFirstTerm, double (*kLogGamma)(double) = log_gamma>
LF_HD double nfa_tail(int n, int k, double p, double log_nt)
{
    if (n == 0 || k == 0) return -log_nt;
    if (n == k) return -log_nt - (double)n * dm::dlog10(p);
    const double p_term = p / (1.0 - p);
    const double first = kPlainFirstTerm ? (double)n + 1.0 : kLogGamma((double)n + 1.0);
    const double log1term = first - kLogGamma((double)k + 1.0) - kLogGamma((double)(n - k) + 1.0)
                          + (double)k * dm::dlog(p) + (double)(n - k) * dm::dlog(1.0 - p);
    double term = dm::dexp(log1term);
    if (double_equal(term, 0.0)) {
        if ((double)k > (double)n * p) return -log1term / 2.30258509299404568402 - log_nt;
        else return -log_nt;
    }
    double bin_tail = term;
    const double tolerance = 0.1;
    for (int i = k + 1; i <= n; ++i) {
        const double bin_term = (double)(n - i + 1) / (double)i;
        const double mult_term = bin_term * p_term;
        term *= mult_term;
        bin_tail += term;
        if (bin_term < 1.0) {
            const double err = term * ((1.0 - dm::dpow(mult_term, (double)(n - i + 1))) / (1.0 - mult_term) - 1.0);
            if (err < tolerance * dabs(-dm::dlog10(bin_tail) - log_nt) * bin_tail) break;
        }
    }
    return -dm::dlog10(bin_tail) - log_nt;
}

}  // namespace lf
