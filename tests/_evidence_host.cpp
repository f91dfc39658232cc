// The host build of csrc/mbb_bridge.hip.h for tests/test_evidence_cpu.py: every step function behind a C entry point,
// and the two bridge sums over arrays (terms added in order) so that the fixed-point loop can be driven from Python.
#define MBB_MATH_HOST
#include "../mbb_emcee_amd/csrc/mbb_bridge.hip.h"

using namespace mbbbr;

extern "C" {
void br_constants(double *out) { out[0] = kTolDefault; out[1] = kMaxIterDefault; out[2] = kPivotRel; out[3] = kLn2Pi; }
double br_host_centered(unsigned long long k) { return br_centered(k); }
unsigned long long br_host_bits53(unsigned int w0, unsigned int w1) { return br_bits53(w0, w1); }
double br_host_ppnd(double q) { return br_ppnd(q); }
void br_host_ppnd_k(const unsigned long long *k, int n, double *z)
{
    for (int i = 0; i < n; ++i) z[i] = br_ppnd(br_centered(k[i]));
}
double br_host_log(double x) { return mbbm::m_log(x); }
unsigned br_host_free_mask(const int *fixed, int opthin, int noalpha, unsigned held)
{
    return br_free_mask(mbblm::lm_fixed_mask(fixed, opthin, noalpha), held);
}
int br_host_chol(const double *cov, unsigned free_, double *L, double *sumlog) { return br_chol(cov, free_, L, sumlog); }
double br_host_lnq(const double *theta, const double *mu, const double *L, unsigned free_, double sumlog)
{
    return br_lnq(theta, mu, L, free_, sumlog);
}
void br_host_draw(const double *mu, const double *L, const double *z, unsigned free_, const double *held, double *theta)
{
    br_draw(mu, L, z, free_, held, theta);
}
double br_host_term_num(double b, double rho, double s1, double s2) { return br_term_num(b, rho, s1, s2); }
double br_host_term_den(double a, double rho, double s1, double s2) { return br_term_den(a, rho, s1, s2); }
int br_host_converged(double rho_new, double rho, double tol) { return br_converged(rho_new, rho, tol); }
double br_host_relerr2(double m1, double v1, double n2, double m2, double v2, double n1e)
{
    return br_relerr2(m1, v1, n2, m2, v2, n1e);
}
// out: sum of the numerator terms over b[n2], of the denominator terms over a[n1]
void br_host_sums(const double *a, int n1, const double *b, int n2, double rho, double s1, double s2, double *out)
{
    double sn = 0.0, sd = 0.0;
    for (int i = 0; i < n2; ++i) sn += br_term_num(b[i], rho, s1, s2);
    for (int j = 0; j < n1; ++j) sd += br_term_den(a[j], rho, s1, s2);
    out[0] = sn; out[1] = sd;
}
// out: mean and variance (ddof = 1) of the numerator terms, then of the denominator terms
void br_host_moments(const double *a, int n1, const double *b, int n2, double rho, double s1, double s2, double *out)
{
    double s[2];
    br_host_sums(a, n1, b, n2, rho, s1, s2, s);
    const double m1 = s[0] / n2, m2 = s[1] / n1;
    double v1 = 0.0, v2 = 0.0;
    for (int i = 0; i < n2; ++i) { const double d = br_term_num(b[i], rho, s1, s2) - m1; v1 = fma(d, d, v1); }
    for (int j = 0; j < n1; ++j) { const double d = br_term_den(a[j], rho, s1, s2) - m2; v2 = fma(d, d, v2); }
    out[0] = m1; out[1] = v1 / (n2 - 1.0); out[2] = m2; out[3] = v2 / (n1 - 1.0);
}
}
