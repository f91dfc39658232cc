// The host build of csrc/mbb_lm.hip.h for tests/test_map_cpu.py: every step function behind a C entry point.
#define MBB_MATH_HOST
#include "../mbb_emcee_amd/csrc/mbb_lm.hip.h"

using namespace mbblm;

extern "C" {
void lm_constants(double *out)
{
    out[0] = kCand; out[1] = kTries; out[2] = kLamStart; out[3] = kFtolDefault; out[4] = kXtolDefault;
    out[5] = kMaxIterDefault; out[6] = kXFloor; out[7] = kLamMin; out[8] = kLamMax;
}
unsigned lm_host_fixed_mask(const int *fixed, int opthin, int noalpha) { return lm_fixed_mask(fixed, opthin, noalpha); }
unsigned lm_host_active(const double *p, const double *lowlim, const double *g, unsigned fixed)
{
    return lm_active(p, lowlim, g, fixed);
}
int lm_host_solve(const double *A, const double *g, double lam, unsigned active, double *d)
{
    double work[25];
    return lm_solve(A, g, lam, active, work, d);
}
void lm_host_project(const double *p, const double *d, const double *lowlim, unsigned active, double *trial)
{
    lm_project(p, d, lowlim, active, trial);
}
int lm_host_clipped(const double *p, const double *d, const double *lowlim, unsigned active)
{
    return lm_clipped(p, d, lowlim, active);
}
double lm_host_predicted(const double *A, const double *g, const double *p, const double *trial)
{
    return lm_predicted(A, g, p, trial);
}
int lm_host_accept(double f, double ftrial) { return lm_accept(f, ftrial); }
double lm_host_gain(double f, double ftrial, double predicted) { return lm_gain(f, ftrial, predicted); }
void lm_host_candidates(double lam, double nu, double *cand) { lm_candidates(lam, nu, cand); }
void lm_host_lambda_accept(double lam_taken, double rho, double *lam, double *nu) { lm_lambda_accept(lam_taken, rho, lam, nu); }
void lm_host_lambda_reject(double *lam, double *nu) { lm_lambda_reject(lam, nu); }
int lm_host_pick(double f, const double *ftrial, int n) { return lm_pick(f, ftrial, n); }
int lm_host_converged_f(double predicted, double f, double ftol) { return lm_converged_f(predicted, f, ftol); }
double lm_host_scaled_step(const double *p, const double *trial) { return lm_scaled_step(p, trial); }
int lm_host_converged_x(double step, double xtol) { return lm_converged_x(step, xtol); }
int lm_host_laplace(const double *A, unsigned free_, double *cov)
{
    double work[25];
    return lm_laplace(A, free_, work, cov);
}
}
