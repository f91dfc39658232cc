// mbb_bridge.hip.h -- the step logic of a bridge-sampling estimate of a marginal likelihood, for the device and the host.
//
// Z = integral of P(theta) over the free parameters, from N1 posterior samples and N2 draws of a Gaussian proposal q
// fitted to another part of the chain (Meng & Wong 1996, the optimal bridge; the recipe of Gronau et al. 2017).  With
// l1_j = P(theta*_j) / q(theta*_j) at the posterior samples and l2_i = P(theta~_i) / q(theta~_i) at the proposal draws,
//   rho <- [ mean_i l2_i / (s1 l2_i + s2 rho) ] / [ mean_j 1 / (s1 l1_j + s2 rho) ],   s1 = n1e / (n1e + N2), s2 = 1 - s1,
// converges to Z.  Everything works on a = ln l1 - l* and b = ln l2 - l* with a common shift l*, so rho is Z e^(-l*).
// Small functions on plain pointers so that the kernels (mbb_evidence.hip.h) and tests/_evidence_host.cpp run the same text:
//   br_centered     53 random bits k -> u - 1/2 with u = (k + 1/2) 2^-53, exactly (u itself needs 54 bits)
//   br_ppnd         the inverse normal CDF at u, given u - 1/2: Wichura's AS 241 PPND16 (Appl. Statist. 37, 1988)
//   br_free_mask    which parameters are integrated over: not the caller's fixed ones, not lambda0 of a thin model, not
//                   alpha of a model without one (lm_fixed_mask), and none that the chain itself holds constant
//   br_chol         L of the covariance over the free set and sum ln L_ii; a pivot that is not positive, not finite or
//                   lost to rounding is reported (0), never divided by
//   br_lnq          ln q(theta) = -d/2 ln 2 pi - sum ln L_ii - |L^-1 (theta - mu)|^2 / 2
//   br_draw         theta = mu + L z over the free set; a held parameter takes its held value bit for bit
//   br_term_num, br_term_den   one term of either bridge sum, in the form whose exponential has a non-positive argument
//   br_converged    |rho_new - rho| <= tol rho_new
//   br_relerr2      the relative mean-square error of the estimate (Fruehwirth-Schnatter 2004)
// Every fused multiply-add is written as one: the device units are built with -ffp-contract=off.
#pragma once
#include "mbb_math.hip.h"
#include "mbb_lm.hip.h"

namespace mbbbr {

constexpr int kNP = 5;
constexpr double kLn2Pi = 1.8378770664093454836;     // ln(2 pi)
constexpr double kPivotRel = 1e-12;                  // a squared pivot below this times its diagonal element is rounding
constexpr double kTolDefault = 1e-10;
constexpr int kMaxIterDefault = 1000;
constexpr double kDblMax = 1.7976931348623157e308;

MBB_HD bool br_finite(double v) { return fabs(v) <= kDblMax; }      // (false for a NaN)

// u - 1/2 for u = (k + 1/2) 2^-53, k < 2^53: (2 (k - 2^52) + 1) 2^-54, an odd integer below 2^53 in magnitude -- exact
MBB_HD double br_centered(unsigned long long k)
{
    const long long kk = (long long)k - (1ll << 52);
    return (double)(2 * kk + 1) * (1.0 / 18014398509481984.0);
}

// ... and k from two Philox words, as the stretch move takes its 53 bits
MBB_HD unsigned long long br_bits53(unsigned int w0, unsigned int w1)
{
    return ((unsigned long long)(w0 >> 5) << 26) | (unsigned long long)(w1 >> 6);
}

// The normal deviate of lower tail area u = q + 1/2, 0 < u < 1.  q is taken (not u) because near 1 a double cannot
// tell u from 1: min(u, 1 - u) = 1/2 - |q| is exact from |q| = 0.425 on.
MBB_HD double br_ppnd(double q)
{
    if (fabs(q) <= 0.425) {
        const double r = fma(-q, q, 0.180625);
        double n = 2.5090809287301226727e3;
        n = fma(n, r, 3.3430575583588128105e4);
        n = fma(n, r, 6.7265770927008700853e4);
        n = fma(n, r, 4.5921953931549871457e4);
        n = fma(n, r, 1.3731693765509461125e4);
        n = fma(n, r, 1.9715909503065514427e3);
        n = fma(n, r, 1.3314166789178437745e2);
        n = fma(n, r, 3.3871328727963666080);
        double d = 5.2264952788528545610e3;
        d = fma(d, r, 2.8729085735721942674e4);
        d = fma(d, r, 3.9307895800092710610e4);
        d = fma(d, r, 2.1213794301586595867e4);
        d = fma(d, r, 5.3941960214247511077e3);
        d = fma(d, r, 6.8718700749205790830e2);
        d = fma(d, r, 4.2313330701600911252e1);
        d = fma(d, r, 1.0);
        return q * n / d;
    }
    const double tail = 0.5 - fabs(q);                   // min(u, 1 - u), exact
    double r = sqrt(-mbbm::m_log(tail));
    double n, d;
    if (r <= 5.0) {
        r -= 1.6;
        n = 7.74545014278341407640e-4;
        n = fma(n, r, 2.27238449892691845833e-2);
        n = fma(n, r, 2.41780725177450611770e-1);
        n = fma(n, r, 1.27045825245236838258);
        n = fma(n, r, 3.64784832476320460504);
        n = fma(n, r, 5.76949722146069140550);
        n = fma(n, r, 4.63033784615654529590);
        n = fma(n, r, 1.42343711074968357734);
        d = 1.05075007164441684324e-9;
        d = fma(d, r, 5.47593808499534494600e-4);
        d = fma(d, r, 1.51986665636164571966e-2);
        d = fma(d, r, 1.48103976427480074590e-1);
        d = fma(d, r, 6.89767334985100004550e-1);
        d = fma(d, r, 1.67638483018380384940);
        d = fma(d, r, 2.05319162663775882187);
        d = fma(d, r, 1.0);
    } else {
        r -= 5.0;
        n = 2.01033439929228813265e-7;
        n = fma(n, r, 2.71155556874348757815e-5);
        n = fma(n, r, 1.24266094738807843860e-3);
        n = fma(n, r, 2.65321895265761230930e-2);
        n = fma(n, r, 2.96560571828504891230e-1);
        n = fma(n, r, 1.78482653991729133580);
        n = fma(n, r, 5.46378491116411436990);
        n = fma(n, r, 6.65790464350110377720);
        d = 2.04426310338993978564e-15;
        d = fma(d, r, 1.42151175831644588870e-7);
        d = fma(d, r, 1.84631831751005468180e-5);
        d = fma(d, r, 7.86869131145613259100e-4);
        d = fma(d, r, 1.48753612908506148525e-2);
        d = fma(d, r, 1.36929880922735805310e-1);
        d = fma(d, r, 5.99832206555887937690e-1);
        d = fma(d, r, 1.0);
    }
    const double v = n / d;
    return q < 0.0 ? -v : v;
}

// bit i set: parameter i is integrated over.  `fixed` is mbblm::lm_fixed_mask (the caller's, lambda0 of a thin model,
// alpha of a model without one), `held` the parameters the chain itself holds constant (bit i).
MBB_HD unsigned br_free_mask(unsigned fixed, unsigned held) { return ~(fixed | held) & 31u; }

MBB_HD int br_count(unsigned mask)
{
    int d = 0;
    for (int i = 0; i < kNP; ++i) d += (int)((mask >> i) & 1u);
    return d;
}

// L (lower triangle, 5 x 5, unit rows and columns outside the free set) with L L^T = cov over the free set, and
// sum ln L_ii.  Returns 1, or 0 when a pivot was not positive, not finite or below kPivotRel of its diagonal element:
// L is then the zero matrix and the sum NaN.
MBB_HD int br_chol(const double *cov, unsigned free_, double *L, double *sumlog)
{
    for (int i = 0; i < kNP; ++i)
        for (int j = 0; j < kNP; ++j) {
            const bool in = ((free_ >> i) & 1u) && ((free_ >> j) & 1u);
            L[i * kNP + j] = in ? cov[i * kNP + j] : (i == j ? 1.0 : 0.0);
        }
    int ok = 1;
    for (int j = 0; j < kNP && ok; ++j) {
        const double ajj = L[j * kNP + j];
        double s = ajj;
        for (int k = 0; k < j; ++k) s = fma(-L[j * kNP + k], L[j * kNP + k], s);
        if (!(s > 0.0) || !br_finite(s) || !(s > kPivotRel * ajj)) { ok = 0; break; }
        const double l = sqrt(s);
        L[j * kNP + j] = l;
        for (int i = j + 1; i < kNP; ++i) {
            double t = L[i * kNP + j];
            for (int k = 0; k < j; ++k) t = fma(-L[i * kNP + k], L[j * kNP + k], t);
            L[i * kNP + j] = t / l;
        }
    }
    if (!ok) {
        for (int i = 0; i < kNP * kNP; ++i) L[i] = 0.0;
        *sumlog = __builtin_nan("");
        return 0;
    }
    double sl = 0.0;
    for (int i = 0; i < kNP; ++i) {
        for (int j = i + 1; j < kNP; ++j) L[i * kNP + j] = 0.0;
        if ((free_ >> i) & 1u) sl += mbbm::m_log(L[i * kNP + i]);
    }
    *sumlog = sl;
    return 1;
}

// ln q(theta) of the Gaussian N(mu, L L^T) over the free set (d = its size)
MBB_HD double br_lnq(const double *theta, const double *mu, const double *L, unsigned free_, double sumlog)
{
    double y[kNP];
    double ss = 0.0;
    for (int i = 0; i < kNP; ++i) {
        double t = ((free_ >> i) & 1u) ? theta[i] - mu[i] : 0.0;
        for (int k = 0; k < i; ++k) t = fma(-L[i * kNP + k], y[k], t);
        y[i] = t / L[i * kNP + i];
        ss = fma(y[i], y[i], ss);
    }
    return fma(-0.5, ss, fma(-0.5 * (double)br_count(free_), kLn2Pi, -sumlog));
}

// theta = mu + L z over the free set; the others take held[i] bit for bit
MBB_HD void br_draw(const double *mu, const double *L, const double *z, unsigned free_, const double *held, double *theta)
{
    for (int i = 0; i < kNP; ++i) {
        if (!((free_ >> i) & 1u)) { theta[i] = held[i]; continue; }
        double t = mu[i];
        for (int k = 0; k <= i; ++k)
            if ((free_ >> k) & 1u) t = fma(L[i * kNP + k], z[k], t);
        theta[i] = t;
    }
}

// l2 / (s1 l2 + s2 rho) with l2 = e^b; b = -inf (a draw where P is 0) and a NaN give 0
MBB_HD double br_term_num(double b, double rho, double s1, double s2)
{
    if (!(b > -kDblMax)) return 0.0;
    if (b > 0.0) return 1.0 / fma(s2 * rho, mbbm::m_exp(-b), s1);
    const double e = mbbm::m_exp(b);
    return e / fma(s1, e, s2 * rho);
}

// 1 / (s1 l1 + s2 rho) with l1 = e^a, a finite
MBB_HD double br_term_den(double a, double rho, double s1, double s2)
{
    if (a > 0.0) {
        const double e = mbbm::m_exp(-a);
        return e / fma(s2 * rho, e, s1);
    }
    return 1.0 / fma(s1, mbbm::m_exp(a), s2 * rho);
}

MBB_HD bool br_converged(double rho_new, double rho, double tol) { return fabs(rho_new - rho) <= tol * rho_new; }

// RE^2 = Var(f1) / (N2 mean(f1)^2) + Var(f2) / (n1e mean(f2)^2), f1 = p / (s1 p + s2) over the proposal draws and
// f2 = 1 / (s1 p + s2) over the posterior samples, p = l / z.  f1 is br_term_num at the final rho and f2 is rho times
// br_term_den: the ratios Var / mean^2 do not see the factor, so the terms' own moments are what is handed in.
// Dividing the second by the effective sample count n1e stands in for the spectral density at frequency zero of the
// original formula.
MBB_HD double br_relerr2(double mean1, double var1, double n2, double mean2, double var2, double n1e)
{
    return var1 / (n2 * mean1 * mean1) + var2 / (n1e * mean2 * mean2);
}

}   // namespace mbbbr
