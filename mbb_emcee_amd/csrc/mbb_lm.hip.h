// mbb_lm.hip.h -- the step logic of a Levenberg-Marquardt search over up to five parameters, for the device and the host.
//
// The objective is a sum of squares F(p) = r(p)^T r(p) (for this library: -2 ln P).  The caller brings the normal
// equations at the current point, A = J^T J and g = -J^T r (so that A d = g is the Gauss-Newton step), and evaluates F
// at the trial points; everything between is here, as small functions on plain pointers (LDS on the device, the stack
// on the host) so that the kernel (mbb_map.hip.h) and tests/_map_host.cpp run the same text:
//   lm_fixed_mask   which parameters never move: the caller's, lambda0 of an optically thin model, alpha without one
//   lm_active       the active set of an iteration: not fixed, and not sitting on a lower limit with g pointing outward
//   lm_solve        (A + lam diag(A)) d = g over the active set by Cholesky; diag(A) floored; a non-positive pivot
//                   is reported (0), never divided by
//   lm_project      the trial point p + d, put back onto p_i >= lowlim_i; lm_clipped  whether that moved it
//   lm_predicted    the reduction of F the quadratic model expects of a step s: 2 g^T s - s^T A s
//   lm_accept       a step is taken iff F went down; a trial that is not finite (NaN, +inf) is a rejected step
//   lm_gain         actual over predicted reduction
//   lm_candidates   the damping values tried at once; lm_lambda_accept / lm_lambda_reject  how lam follows
//   lm_pick         of several trials the one of smallest F that lm_accept admits, ties to the lowest index
//   lm_converged_f, lm_converged_x, lm_scaled_step   the stopping tests.  The caller hands lm_converged_f the largest
//                   predicted reduction among the candidates that were solved and NOT clipped; when there is none (all
//                   clipped onto a limit, or none solved) the try is a rejection and no convergence is declared from it
//   lm_laplace      A^-1 over the parameters that are free and off their limit, NaN elsewhere
// The damping rule is Nielsen's (H. B. Nielsen 1999, "Damping parameter in Marquardt's method", IMM-REP-1999-05):
// after an accepted step of gain rho, lam <- lam max(1/3, 1 - (2 rho - 1)^3) and nu <- 2; after a rejected one,
// lam <- lam nu and nu <- 2 nu.  The candidates tried at once are one bolder value and then the values that rule
// would try one after the other if each were rejected: lam/3, lam, lam nu, lam nu (2 nu).  When one is accepted the
// rule's first half is applied to ITS lam; when none is, lam and nu are where four rejections in a row leave them.
// Every fused multiply-add is written as one: the device units are built with -ffp-contract=off.
#pragma once
#include "mbb_math.hip.h"

namespace mbblm {

constexpr int kNP = 5;               // parameters
constexpr int kCand = 4;             // damping values tried at once
constexpr int kTries = 3;            // ... sets of them per iteration before the iteration is given up
constexpr double kLamStart = 1e-3;   // Marquardt's customary first damping, relative to diag(A)
constexpr double kLamMin = 1e-15, kLamMax = 1e15;
constexpr double kDiagRel = 1e-30;   // diag(A)_i is floored at this times the largest diagonal element, and at kDiagAbs
constexpr double kDiagAbs = 1e-300;
// Defaults of the stopping tests.
// ftol: F is evaluated to about nb eps ~ 1e-15 of itself; a predicted reduction below 1e-13 max(1, F) is within a
//       hundred roundings of F and a thousand times under the 2e-10 max(1, F) the tests allow between two optima.
constexpr double kFtolDefault = 1e-13;
// xtol: a step of 1e-9 of a parameter, with sigma / theta <= 1, moves F by (1e-9)^2 / 2: nothing F can show.
constexpr double kXtolDefault = 1e-9;
// maxiter: the CPU study needed 36-102 function evaluations, under 20 iterations; ten times that.
constexpr int kMaxIterDefault = 200;
constexpr double kXFloor = 1e-8;     // |p_i| is taken to be at least this when a step is scaled or a difference step made

MBB_HD unsigned lm_fixed_mask(const int *fixed, int opthin, int noalpha)
{
    unsigned m = 0;
    for (int i = 0; i < kNP; ++i) if (fixed[i]) m |= 1u << i;
    if (opthin) m |= 1u << 2;
    if (noalpha) m |= 1u << 3;
    return m;
}

// bit i set: parameter i takes part in this iteration's step
MBB_HD unsigned lm_active(const double *p, const double *lowlim, const double *g, unsigned fixed)
{
    unsigned a = 0;
    for (int i = 0; i < kNP; ++i) {
        if ((fixed >> i) & 1u) continue;
        if (p[i] <= lowlim[i] && g[i] < 0.0) continue;     // on its limit, and the step would leave the allowed side
        a |= 1u << i;
    }
    return a;
}

// (A + lam D) d = g over the active set, D = diag(A) floored; work[25] is the caller's.  Parameters outside the set get
// d_i = 0: their row and column are replaced by the unit matrix's.  Returns 1, or 0 when a pivot was not positive
// (d is then all zero).
MBB_HD int lm_solve(const double *A, const double *g, double lam, unsigned active, double *work, double *d)
{
    double dmax = 0.0;
    for (int i = 0; i < kNP; ++i) if (((active >> i) & 1u) && A[i * kNP + i] > dmax) dmax = A[i * kNP + i];
    const double floor_ = fmax(kDiagRel * dmax, kDiagAbs);
    for (int i = 0; i < kNP; ++i)
        for (int j = 0; j < kNP; ++j) {
            const bool in = ((active >> i) & 1u) && ((active >> j) & 1u);
            double v = in ? A[i * kNP + j] : (i == j ? 1.0 : 0.0);
            if (in && i == j) v = fma(lam, fmax(v, floor_), v);
            work[i * kNP + j] = v;
        }
    for (int i = 0; i < kNP; ++i) d[i] = 0.0;
    // Cholesky, L in the lower triangle of work
    for (int j = 0; j < kNP; ++j) {
        double s = work[j * kNP + j];
        for (int k = 0; k < j; ++k) s = fma(-work[j * kNP + k], work[j * kNP + k], s);
        if (!(s > 0.0) || !(s <= 1.7976931348623157e308)) return 0;
        const double l = sqrt(s);
        work[j * kNP + j] = l;
        for (int i = j + 1; i < kNP; ++i) {
            double t = work[i * kNP + j];
            for (int k = 0; k < j; ++k) t = fma(-work[i * kNP + k], work[j * kNP + k], t);
            work[i * kNP + j] = t / l;
        }
    }
    // L y = g, L^T d = y
    for (int i = 0; i < kNP; ++i) {
        double t = ((active >> i) & 1u) ? g[i] : 0.0;
        for (int k = 0; k < i; ++k) t = fma(-work[i * kNP + k], d[k], t);
        d[i] = t / work[i * kNP + i];
    }
    for (int i = kNP - 1; i >= 0; --i) {
        double t = d[i];
        for (int k = i + 1; k < kNP; ++k) t = fma(-work[k * kNP + i], d[k], t);
        d[i] = t / work[i * kNP + i];
    }
    return 1;
}

// trial = p + d on the allowed side of the lower limits; parameters outside the active set keep their value bit for bit
MBB_HD void lm_project(const double *p, const double *d, const double *lowlim, unsigned active, double *trial)
{
    for (int i = 0; i < kNP; ++i) {
        double t = p[i];
        if ((active >> i) & 1u) {
            t = p[i] + d[i];
            if (t < lowlim[i]) t = lowlim[i];
        }
        trial[i] = t;
    }
}

// whether lm_project had to move p + d: a clipped step is not the damped model's minimiser, and lm_predicted of it says
// nothing about how close the search is
MBB_HD bool lm_clipped(const double *p, const double *d, const double *lowlim, unsigned active)
{
    for (int i = 0; i < kNP; ++i)
        if (((active >> i) & 1u) && p[i] + d[i] < lowlim[i]) return true;
    return false;
}

// what the quadratic model F(p + s) ~ F - 2 g^T s + s^T A s expects F to go down by
MBB_HD double lm_predicted(const double *A, const double *g, const double *p, const double *trial)
{
    double lin = 0.0, quad = 0.0;
    for (int i = 0; i < kNP; ++i) {
        const double si = trial[i] - p[i];
        double t = 0.0;
        for (int j = 0; j < kNP; ++j) t = fma(A[i * kNP + j], trial[j] - p[j], t);
        lin = fma(g[i], si, lin);
        quad = fma(si, t, quad);
    }
    return fma(2.0, lin, -quad);
}

MBB_HD bool lm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (false for a NaN)

MBB_HD bool lm_accept(double f, double ftrial) { return lm_finite(ftrial) && ftrial < f; }

MBB_HD double lm_gain(double f, double ftrial, double predicted)
{
    return predicted > 0.0 ? (f - ftrial) / predicted : 0.0;
}

MBB_HD double lm_clamp(double lam) { return fmin(fmax(lam, kLamMin), kLamMax); }

MBB_HD void lm_candidates(double lam, double nu, double *cand)
{
    cand[0] = lm_clamp(lam / 3.0);
    cand[1] = lm_clamp(lam);
    cand[2] = lm_clamp(lam * nu);
    cand[3] = lm_clamp(lam * nu * (2.0 * nu));
}

MBB_HD void lm_lambda_accept(double lam_taken, double rho, double *lam, double *nu)
{
    const double t = fma(2.0, rho, -1.0);
    *lam = lm_clamp(lam_taken * fmax(1.0 / 3.0, 1.0 - t * t * t));
    *nu = 2.0;
}

// all kCand candidates of lm_candidates(lam, nu) were rejected: one more step of the rejection rule from the last
MBB_HD void lm_lambda_reject(double *lam, double *nu)
{
    *lam = lm_clamp(*lam * *nu * (2.0 * *nu) * (4.0 * *nu));
    *nu = fmin(8.0 * *nu, 1e6);
}

// of n trials the index of the smallest F that lm_accept admits (ties: the lowest index), -1 when none
MBB_HD int lm_pick(double f, const double *ftrial, int n)
{
    int best = -1;
    for (int i = 0; i < n; ++i)
        if (lm_accept(f, ftrial[i]) && (best < 0 || ftrial[i] < ftrial[best])) best = i;
    return best;
}

MBB_HD bool lm_converged_f(double predicted, double f, double ftol) { return predicted <= ftol * fmax(1.0, f); }

MBB_HD double lm_scaled_step(const double *p, const double *trial)
{
    double m = 0.0;
    for (int i = 0; i < kNP; ++i) m = fmax(m, fabs(trial[i] - p[i]) / fmax(fabs(p[i]), kXFloor));
    return m;
}

MBB_HD bool lm_converged_x(double scaled_step, double xtol) { return scaled_step <= xtol; }

// cov = A^-1 over the parameters of `free` (bit i: parameter i is free and off its limit), NaN in the rows and columns
// of the others; work[25] is the caller's.  Returns 1, or 0 when A over that set is not positive definite or the set
// is empty: the whole matrix is then NaN.
MBB_HD int lm_laplace(const double *A, unsigned free_, double *work, double *cov)
{
    const double qnan = __builtin_nan("");
    int ok = free_ != 0;
    for (int i = 0; i < kNP; ++i)
        for (int j = 0; j < kNP; ++j) {
            const bool in = ((free_ >> i) & 1u) && ((free_ >> j) & 1u);
            work[i * kNP + j] = in ? A[i * kNP + j] : (i == j ? 1.0 : 0.0);
        }
    for (int j = 0; j < kNP && ok; ++j) {
        double s = work[j * kNP + j];
        for (int k = 0; k < j; ++k) s = fma(-work[j * kNP + k], work[j * kNP + k], s);
        if (!(s > 0.0) || !lm_finite(s)) { ok = 0; break; }
        const double l = sqrt(s);
        work[j * kNP + j] = l;
        for (int i = j + 1; i < kNP; ++i) {
            double t = work[i * kNP + j];
            for (int k = 0; k < j; ++k) t = fma(-work[i * kNP + k], work[j * kNP + k], t);
            work[i * kNP + j] = t / l;
        }
    }
    // a pivot that is positive but lost to rounding: the smallest squared pivot against the diagonal it came from
    if (ok)
        for (int j = 0; j < kNP; ++j)
            if (((free_ >> j) & 1u) && !(work[j * kNP + j] * work[j * kNP + j] > 1e-14 * A[j * kNP + j])) ok = 0;
    if (!ok) {
        for (int i = 0; i < kNP * kNP; ++i) cov[i] = qnan;
        return 0;
    }
    // column c of the inverse: L y = e_c, L^T x = y
    for (int c = 0; c < kNP; ++c) {
        for (int i = 0; i < kNP; ++i) {
            double t = i == c ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) t = fma(-work[i * kNP + k], cov[k * kNP + c], t);
            cov[i * kNP + c] = t / work[i * kNP + i];
        }
        for (int i = kNP - 1; i >= 0; --i) {
            double t = cov[i * kNP + c];
            for (int k = i + 1; k < kNP; ++k) t = fma(-work[k * kNP + i], cov[k * kNP + c], t);
            cov[i * kNP + c] = t / work[i * kNP + i];
        }
    }
    // (the columns were solved for one by one: the upper triangle is the answer, the lower its mirror, bit for bit)
    for (int i = 0; i < kNP; ++i)
        for (int j = 0; j < i; ++j) cov[i * kNP + j] = cov[j * kNP + i];
    for (int i = 0; i < kNP; ++i)
        for (int j = 0; j < kNP; ++j)
            if (!((free_ >> i) & 1u) || !((free_ >> j) & 1u)) cov[i * kNP + j] = qnan;
    return 1;
}

}   // namespace mbblm
