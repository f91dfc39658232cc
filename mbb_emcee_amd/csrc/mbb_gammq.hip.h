// mbb_gammq.hip.h -- the chi-square tail probability Q(nb/2, chisq/2) in fp64, for the device and the host.
//
// Q(a, x) is the regularised upper incomplete gamma function.  For the half-integer orders a = nb/2 of a chi-square
// with nb degrees of freedom it has finite closed forms (Abramowitz & Stegun 6.5.13 and 26.4.4-5), with x = chisq/2:
//   nb even, a = n:        e^-x sum_{j<n} x^j / j!
//   nb odd,  a = n + 1/2:  erfc(sqrt x) + e^-x sqrt(x) (2/sqrt pi) sum_{j<n} x^j / ((3/2)(5/2)...(j + 1/2))
// Every term is positive: there is no cancellation.  The sums are taken in Horner form from the last term down, so
// that no power of x is formed, and e^-x is applied as e^(-x/2) twice, the sum between: the product neither overflows
// while e^-x has underflowed nor goes through a subnormal e^-x while the result is still a normal number.  sqrt(x) is
// rounded, and erfc at s is sensitive to 2 s^2 times a relative change of s -- 1400 half-ulps at x = 700 --: the
// remainder x - s^2 (exact, one fma) is put back through erfc's derivative, -(2/sqrt pi) e^(-s^2).
//
// Edge values: chisq <= 0 gives 1, +inf 0, NaN NaN.  From x = 1500 on the result is 0: for nb <= kGammqMaxNb the true
// value is below e^-1060 there, far under the smallest subnormal.
//
// Compiles for the host too (MBB_MATH_HOST, as mbb_math.hip.h): tests/test_goodness_cpu.py holds that build to mpmath.
#pragma once
#include "mbb_math.hip.h"

namespace mbbm {

constexpr int kGammqMaxNb = 256;     // degrees of freedom the closed forms are used for (terms up to 1600^127 / 127!)

MBB_HD double m_gammq_half(int nb, double chisq)
{
    if (chisq != chisq) return chisq;
    if (!(chisq > 0.0)) return 1.0;
    const double x = 0.5 * chisq;
    if (x == 0.0) return 1.0;                              // the smallest subnormal halves to 0: no 0 / sqrt(0) below
    if (x >= 1500.0) return 0.0;
    const double t = m_exp(-0.5 * x);                      // e^-x = t t
    double q;
    if ((nb & 1) == 0) {
        const int n = nb >> 1;
        double h = 1.0;                                    // sum_{j<n} x^j / j! = 1 + x/1 (1 + x/2 (1 + ... x/(n-1)))
        for (int j = n - 1; j >= 1; --j) h = fma(h, x / (double)j, 1.0);
        q = (h * t) * t;
    } else {
        const int n = nb >> 1;
        const double rsqrtpi = 0.56418958354775628695;     // 1 / sqrt(pi)
        const double s = sqrt(x), rem = fma(-s, s, x);     // x = s^2 + rem exactly
        q = erfc(s) - ((rem / s) * rsqrtpi * t) * t;       // erfc(sqrt x) to first order in rem
        if (n >= 1) {
            double h = 1.0;                                // 1 + x/(3/2) (1 + x/(5/2) (1 + ... x/(n - 1/2)))
            for (int j = n; j >= 2; --j) h = fma(h, x / ((double)j - 0.5), 1.0);
            q += ((2.0 * rsqrtpi * s * h) * t) * t;
        }
    }
    return q > 1.0 ? 1.0 : q;                              // (not fmin: a NaN made above must come out as one)
}

}   // namespace mbbm
