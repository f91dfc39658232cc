// mbb_popsteps.hip.h -- the step logic of the population hyper-likelihood, for the device and the host
// (include/mbb_hip.h: "the population of a catalogue").  Small functions on plain values so that the kernels
// (mbb_population.hip.h) and tests/_population_host.cpp run the same text:
//   pop_prior_factor  the likelihood's separable prior factor of one parameter, unnormalised: 0 up to the upper limit,
//                     the half-Gaussian of width 0.02 (uplim - lowlim) beyond it, plus the Gaussian prior
//   pop_transform     x = g(theta) and the Jacobian term ln |d theta / dx|: 0 for the identity, ln(theta ln 10) for log10
//   pop_entry         x[d] and b = -ln pi0(x) of one chain row, or b = -inf for a row that is left out
//   pop_prepare       a candidate (mu, L row by row) as the evaluation reads it: mu, the strict lower triangle, 1 / L_ii
//                     and c0 = -sum ln L_ii - (d / 2) ln 2 pi; false for a bad candidate
//   pop_logdens       a_j = -1/2 |L^-1 (x - mu)|^2 + c0 + b by forward substitution
//   pop_merge         a record (m, s, s2[, mean, M2]) merged with another: m the maximum of a seen, s = sum e^(a - m),
//                     s2 = sum e^(2 (a - m)), mean the weighted mean of x and M2 = sum e^(a - m) (x - mean)(x - mean)^T
//                     (Chan, Golub & LeVeque's pairwise update with weights).  Nothing seen is (-inf, 0, 0, 0, 0): it
//                     merges as the identity.  pop_add merges one entry, the record (a, 1, 1, x, 0).
// The (m, s) part of pop_merge is ps_lse_merge of mbb_psis.hip.h, bit for bit.  Every function treats a candidate
// and an entry by itself: nothing depends on what else shares a call.
#pragma once
#include "mbb_math.hip.h"
#include "mbb_psis.hip.h"

#if defined(MBB_MATH_HOST) || !defined(__HIPCC__)
#define POP_HD inline
#else
#define POP_HD __device__ __forceinline__       // (m_exp and m_log are device functions in this build)
#endif

namespace mbbpops {

constexpr int kMaxD = 5;
constexpr int kIdentity = 0, kLog10 = 1;
constexpr double kLn10 = 2.30258509299404568402;
constexpr double kInvLn10 = 0.43429448190325182765;
constexpr double kWallRelWidth = 0.02;       // the soft upper wall's width over (uplim - lowlim)
constexpr double kUnderflow = -745.0;        // e^a is below the smallest float64 for a < this

constexpr int pop_tri(int d) { return d * (d + 1) / 2; }
constexpr int pop_hyper_len(int d) { return d + pop_tri(d); }
constexpr int pop_prep_len(int d) { return d + d * (d - 1) / 2 + d + 1; }     // mu, strict lower triangle, 1 / L_ii, c0

// What the prior factors of the five parameters are made of (the spec's copy of the likelihood's limits and priors)
struct PopPrior {
    int has_uplim[kMaxD], has_gprior[kMaxD];
    double lowlim[kMaxD], uplim[kMaxD], gmean[kMaxD], givar[kMaxD];
};

POP_HD double pop_prior_factor(double theta, int has_uplim, double uplim, double lowlim, int has_gprior, double gmean,
                              double givar)
{
    double lp = 0.0;
    if (has_uplim && theta > uplim) {
        const double lw = kWallRelWidth * (uplim - lowlim), d = theta - uplim;
        lp -= 0.5 * d * d / (lw * lw);
    }
    if (has_gprior) {
        const double d = theta - gmean;
        lp += -0.5 * givar * d * d;
    }
    return lp;
}

// x = g(theta) and ln |d theta / dx|; theta > 0 finite for log10 (the caller's check)
POP_HD double pop_transform(double theta, int transform, double *lnjac)
{
    if (transform == kLog10) {
        *lnjac = mbbm::m_log(theta * kLn10);
        return mbbm::m_log(theta) * kInvLn10;
    }
    *lnjac = 0.0;
    return theta;
}

// One chain row: x[0 .. d-1] and b = -ln pi0(x).  A row that is left out has b = -inf and x = 0.
POP_HD double pop_entry(const double *theta5, int d, const int *col, const int *transform, const PopPrior &p, double *x)
{
    double lnpi = 0.0;
    bool ok = true;
    for (int i = 0; i < d; ++i) {
        const int k = col[i];
        const double th = theta5[k];
        if (!mbbps::ps_finite(th) || (transform[i] == kLog10 && !(th > 0.0))) { ok = false; break; }
        double lnjac;
        x[i] = pop_transform(th, transform[i], &lnjac);
        lnpi += pop_prior_factor(th, p.has_uplim[k], p.uplim[k], p.lowlim[k], p.has_gprior[k], p.gmean[k], p.givar[k]);
        lnpi += lnjac;
    }
    if (ok && mbbps::ps_finite(lnpi)) return -lnpi;
    for (int i = 0; i < d; ++i) x[i] = 0.0;
    return -INFINITY;
}

// A candidate h = (mu[d], L row by row) into prep[pop_prep_len(d)]; false (prep untouched) when a value is not finite
// or an L_ii is not positive.
POP_HD bool pop_prepare(const double *h, int d, double *prep)
{
    for (int i = 0; i < pop_hyper_len(d); ++i) if (!mbbps::ps_finite(h[i])) return false;
    const double *L = h + d;
    for (int i = 0; i < d; ++i) if (!(L[pop_tri(i) + i] > 0.0)) return false;
    double *mu = prep, *off = prep + d, *rdiag = off + d * (d - 1) / 2;
    double sumln = 0.0;
    int o = 0;
    for (int i = 0; i < d; ++i) {
        mu[i] = h[i];
        for (int k = 0; k < i; ++k) off[o++] = L[pop_tri(i) + k];
        rdiag[i] = 1.0 / L[pop_tri(i) + i];
        sumln += mbbm::m_log(L[pop_tri(i) + i]);
    }
    rdiag[d] = -sumln - 0.5 * (double)d * mbbps::kLn2Pi;
    return true;
}

// a = -1/2 |z|^2 + c0 + b,  L z = x - mu
template <int D> POP_HD double pop_logdens(const double *prep, const double *x, double b)
{
    const double *mu = prep, *off = prep + D, *rdiag = off + D * (D - 1) / 2;
    double z[D], q = 0.0;
    int o = 0;
    for (int i = 0; i < D; ++i) {
        double y = x[i] - mu[i];
        for (int k = 0; k < i; ++k) y -= off[o++] * z[k];
        z[i] = y * rdiag[i];
        q += z[i] * z[i];
    }
    return -0.5 * q + rdiag[D] + b;
}

template <int D, bool MOM> struct PopRec {
    static constexpr int kMean = MOM ? D : 0, kM2 = MOM ? pop_tri(D) : 0, kWords = 3 + kMean + kM2;
    double m, s, s2;
    double mean[MOM ? D : 1], M2[MOM ? pop_tri(D) : 1];
};

template <int D, bool MOM> POP_HD void pop_clear(PopRec<D, MOM> &r)
{
    r.m = -INFINITY; r.s = r.s2 = 0.0;
    for (int i = 0; i < r.kMean; ++i) r.mean[i] = 0.0;
    for (int i = 0; i < r.kM2; ++i) r.M2[i] = 0.0;
}

// A <- A merged with B.  One exponential: of -|A.m - B.m|.
template <int D, bool MOM> POP_HD void pop_merge(PopRec<D, MOM> &A, const PopRec<D, MOM> &B)
{
    if (B.s == 0.0) return;
    const bool up = B.m > A.m;
    const double e = mbbm::m_exp(up ? A.m - B.m : B.m - A.m);
    const double ra = up ? e : 1.0, rb = up ? 1.0 : e;
    const double sa = A.s * ra, sb = B.s * rb, st = sa + sb;
    A.s2 = A.s2 * ra * ra + B.s2 * rb * rb;
    if (MOM) {
        const double f = sb / st, g = sa * f;
        double del[MOM ? D : 1];
        for (int i = 0; i < A.kMean; ++i) del[i] = B.mean[i] - A.mean[i];
        int o = 0;
        for (int i = 0; i < A.kMean; ++i)
            for (int k = 0; k <= i; ++k, ++o) A.M2[o] = A.M2[o] * ra + B.M2[o] * rb + g * del[i] * del[k];
        for (int i = 0; i < A.kMean; ++i) A.mean[i] += f * del[i];
    }
    A.s = st;
    if (up) A.m = B.m;
}

// ... with one entry of log density a at x: the record (a, 1, 1, x, 0).  An a that is not above -inf adds nothing.
template <int D, bool MOM> POP_HD void pop_add(PopRec<D, MOM> &A, double a, const double *x)
{
    if (!(a > -INFINITY)) return;
    PopRec<D, MOM> B;
    B.m = a; B.s = B.s2 = 1.0;
    for (int i = 0; i < B.kMean; ++i) B.mean[i] = x[i];
    for (int i = 0; i < B.kM2; ++i) B.M2[i] = 0.0;
    pop_merge(A, B);
}

template <int D, bool MOM> POP_HD void pop_store(const PopRec<D, MOM> &r, double *w)
{
    w[0] = r.m; w[1] = r.s; w[2] = r.s2;
    for (int i = 0; i < r.kMean; ++i) w[3 + i] = r.mean[i];
    for (int i = 0; i < r.kM2; ++i) w[3 + r.kMean + i] = r.M2[i];
}

template <int D, bool MOM> POP_HD void pop_load(PopRec<D, MOM> &r, const double *w)
{
    r.m = w[0]; r.s = w[1]; r.s2 = w[2];
    for (int i = 0; i < r.kMean; ++i) r.mean[i] = w[3 + i];
    for (int i = 0; i < r.kM2; ++i) r.M2[i] = w[3 + r.kMean + i];
}

}   // namespace mbbpops
