// The HOST build of csrc/mbb_psis.hip.h for tests/test_loo_cpu.py: the text the kernels of csrc/mbb_pointwise.hip.h run.
#define MBB_MATH_HOST 1
#include "../mbb_emcee_amd/csrc/mbb_psis.hip.h"

using namespace mbbps;

extern "C" {
void ps_constants(double *c) { c[0] = kTailMax; c[1] = kGridMax; c[2] = kLn2Pi; }
long long ps_host_tail_len(long long S) { return ps_tail_len(S); }
int ps_host_grid_len(int M) { return ps_grid_len(M); }
// out: k, sigma, khat; l [kGridMax] the profile (NaN where the grid was not walked)
int ps_host_gpd_fit(const double *x, int M, double *out, double *theta, double *l)
{
    for (int j = 0; j < kGridMax; ++j) theta[j] = l[j] = NAN;
    return ps_gpd_fit(x, M, theta, l, &out[0], &out[1], &out[2]);
}
double ps_host_gpd_quantile(double p, double khat, double sigma) { return ps_gpd_quantile(p, khat, sigma); }
double ps_host_smoothed(int i, int M, double khat, double sigma, double expc) { return ps_smoothed(i, M, khat, sigma, expc); }
double ps_host_norm_cdf(double z) { return ps_norm_cdf(z); }
double ps_host_ll(double g, double lam) { return ps_ll(g, lam); }
// the values merged in order, in runs of `run` values each merged as a pair: ln sum exp
double ps_host_lse(const double *v, int n, int run)
{
    double m = -INFINITY, s = 0.0;
    for (int i = 0; i < n; i += run) {
        double m2 = -INFINITY, s2 = 0.0;
        for (int j = i; j < n && j < i + run; ++j) ps_lse_add(m2, s2, v[j]);
        ps_lse_merge(m, s, m2, s2);
    }
    return ps_lse_value(m, s);
}
}
