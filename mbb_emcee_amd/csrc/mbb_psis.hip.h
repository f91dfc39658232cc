// mbb_psis.hip.h -- the step logic of Pareto-smoothed importance sampling, for the device and the host.
//
// Leave-one-band-out cross-validation of a chain (include/mbb_hip.h: "out-of-sample fit") turns the pointwise term
// ll_b(theta) of every window entry into importance weights lw = -ll - max(-ll), replaces the M largest of them by the
// quantiles of a generalised Pareto distribution fitted to them (Vehtari, Simpson, Gelman, Yao & Gabry; `loo` 2.x
// psislw) and sums.  Small functions on plain pointers so that the kernels (mbb_pointwise.hip.h) and
// tests/_loo_host.cpp run the same text:
//   ps_finite        |v| <= DBL_MAX (false for a NaN)
//   ps_tail_len      M = ceil(min(S / 5, 3 sqrt(S))), in integers
//   ps_theta         theta_j of Zhang & Stephens' (2009) grid
//   ps_profile       k_j = mean log1p(-theta_j x) over the ascending tail, and l_j = M (ln(-theta_j / k_j) - k_j - 1)
//   ps_combine       softmax of l (maximum subtracted), theta-hat, k, sigma, the prior on k, and the fallback decision
//   ps_gpd_fit       the three above in a row, as one thread would do them: the kernel spreads ps_profile over its
//                    threads, a theta_j each, and gets the same bits because each sum is one thread's in either form
//   ps_gpd_quantile  sigma expm1(-k log1p(-p)) / k
//   ps_norm_cdf      Phi(z) through erfc
//   ps_lse_merge     a (max, sum of exp(. - max)) pair merged with another; ps_lse_add: with one value
// Every sum runs in a fixed order: the tail ascending, the grid from j = 1.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(MBB_MATH_HOST) || !defined(__HIPCC__)
#define PS_HD inline
#else
#include <hip/hip_runtime.h>
#define PS_HD __host__ __device__ __forceinline__
#endif

namespace mbbps {

constexpr int kTailMax = 4096;        // the longest tail one workgroup sorts in LDS: S <= 1 864 135 entries per source
constexpr int kGridMax = 30 + 64;     // m = 30 + floor(sqrt(M)) at M = kTailMax
constexpr double kDblMax = 1.7976931348623157e308;
constexpr double kLn2Pi = 1.8378770664093454836;     // ln(2 pi)
constexpr double kInv2PiHi = 0x1.45f306dc9c883p-3, kInv2PiLo = -0x1.6b01ec5417056p-57;     // 1 / (2 pi) = hi + lo
constexpr double kSqrtHalf = 0.70710678118654752440;

// why a call did without the Pareto fit (ps_combine's return; 0: it did not)
constexpr int kFitOk = 0, kFitShort = 1, kFitFlat = 2;

PS_HD bool ps_finite(double v) { return fabs(v) <= kDblMax; }

// M = ceil(min(0.2 S, 3 sqrt(S))): 0.2 S is the smaller up to S = 225; beyond, ceil(sqrt(9 S)) by an integer root
PS_HD long long ps_tail_len(long long S)
{
    if (S <= 0) return 0;
    if (S <= 225) return (S + 4) / 5;
    const long long v = 9 * S;
    long long r = (long long)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r * r == v ? r : r + 1;
}

PS_HD int ps_grid_len(int M) { return 30 + (int)sqrt((double)M); }

// x* = x[floor(M / 4 + 1/2)], 1-based
PS_HD double ps_xstar(const double *x, int M) { return x[(int)floor(0.25 * (double)M + 0.5) - 1]; }

// theta_j, j = 1 .. m
PS_HD double ps_theta(int j, int m, double xM, double xstar)
{
    return 1.0 / xM + (1.0 - sqrt((double)m / ((double)j - 0.5))) / (3.0 * xstar);
}

// k(theta) = mean log1p(-theta x), the tail ascending
PS_HD double ps_kmean(double theta, const double *x, int M)
{
    double acc = 0.0;
    for (int i = 0; i < M; ++i) acc += log1p(-theta * x[i]);
    return acc / (double)M;
}

// the profile log-likelihood l_j at theta_j
PS_HD double ps_profile(double theta, const double *x, int M)
{
    const double k = ps_kmean(theta, x, M);
    return (double)M * (log(-theta / k) - k - 1.0);
}

// From the grid and its profile: theta-hat = sum theta_j w_j with w the softmax of l, k and sigma at theta-hat, then
// k-hat = (k M + 5) / (M + 10).  Returns kFitOk, or kFitFlat when any of k, sigma, k-hat is not finite.
PS_HD int ps_combine(const double *theta, const double *l, int m, const double *x, int M, double *k, double *sigma,
                     double *khat)
{
    double lmax = -INFINITY;
    for (int j = 0; j < m; ++j) if (l[j] > lmax) lmax = l[j];      // (a NaN never becomes the maximum; it poisons the sum)
    double sw = 0.0;
    for (int j = 0; j < m; ++j) sw += exp(l[j] - lmax);
    double th = 0.0;
    for (int j = 0; j < m; ++j) th += theta[j] * (exp(l[j] - lmax) / sw);
    const double kk = ps_kmean(th, x, M);
    const double sg = -kk / th;
    const double kh = (kk * (double)M + 5.0) / ((double)M + 10.0);
    *k = kk; *sigma = sg; *khat = kh;
    return ps_finite(kk) && ps_finite(sg) && ps_finite(kh) ? kFitOk : kFitFlat;
}

// The whole fit of an ascending tail x[0 .. M-1] (x_i = exp(lw_i) - exp(c) >= 0), M <= kTailMax; theta and l are work
// arrays of kGridMax.  On a fallback k-hat is +inf and k, sigma are NaN.
PS_HD int ps_gpd_fit(const double *x, int M, double *theta, double *l, double *k, double *sigma, double *khat)
{
    int why = kFitOk;
    if (M < 5) why = kFitShort;
    else if (!(x[M - 1] > x[0]) || !(ps_xstar(x, M) > 0.0)) why = kFitFlat;
    if (why == kFitOk) {
        const int m = ps_grid_len(M);
        const double xs = ps_xstar(x, M);
        for (int j = 0; j < m; ++j) {
            theta[j] = ps_theta(j + 1, m, x[M - 1], xs);
            l[j] = ps_profile(theta[j], x, M);
        }
        why = ps_combine(theta, l, m, x, M, k, sigma, khat);
    }
    if (why != kFitOk) { *k = *sigma = NAN; *khat = INFINITY; }
    return why;
}

// the quantile of the fitted distribution at probability p
PS_HD double ps_gpd_quantile(double p, double khat, double sigma)
{
    if (khat == 0.0) return -sigma * log1p(-p);
    return sigma * expm1(-khat * log1p(-p)) / khat;
}

// the smoothed log weight of the tail entry of ascending rank i (0-based) of M, capped at 0
PS_HD double ps_smoothed(int i, int M, double khat, double sigma, double expc)
{
    const double p = ((double)i + 0.5) / (double)M;
    return fmin(log(ps_gpd_quantile(p, khat, sigma) + expc), 0.0);
}

PS_HD double ps_norm_cdf(double z) { return 0.5 * erfc(-z * kSqrtHalf); }

// (m, s): max of the values seen and the sum of exp(value - m); nothing seen is (-inf, 0)
PS_HD void ps_lse_merge(double &m, double &s, double m2, double s2)
{
    if (s2 == 0.0) return;
    if (s == 0.0) { m = m2; s = s2; return; }
    if (m2 <= m) s += s2 * exp(m2 - m);
    else { s = s * exp(m - m2) + s2; m = m2; }
}
PS_HD void ps_lse_add(double &m, double &s, double v) { ps_lse_merge(m, s, v, 1.0); }
PS_HD double ps_lse_value(double m, double s) { return s == 0.0 ? -INFINITY : m + log(s); }

// the pointwise term from g_b = (Lambda r)_b and Lambda_bb.  Its constant is log(lam / 2 pi) / 2 with the quotient kept to
// twice the working precision (p + e), not log(lam) - log(2 pi): where Lambda_bb is next to 2 pi -- an uncertainty of 0.4 --
// that difference cancels and keeps the absolute error of log(lam), hundreds of ulps of what is left.
PS_HD double ps_ll(double g, double lam)
{
    const double p = lam * kInv2PiHi, e = fma(lam, kInv2PiHi, -p) + lam * kInv2PiLo;
    return 0.5 * (log(p) + e / p) - 0.5 * (g * g) / lam;
}

}   // namespace mbbps
