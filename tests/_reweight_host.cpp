// The HOST build of csrc/mbb_rwsteps.hip.h for tests/test_reweight_cpu.py: the text the kernels of csrc/mbb_reweight.hip.h run.
#define MBB_MATH_HOST 1
#include "../mbb_emcee_amd/csrc/mbb_rwsteps.hip.h"

using namespace mbbrws;

extern "C" {
void rw_constants(double *c) { c[0] = kTwo32; c[1] = (double)kUnit; }
unsigned long long rw_host_quantise(double lw) { return rw_quantise(lw); }
unsigned long long rw_host_target(double p, unsigned long long U) { return rw_target(p, U); }
void rw_host_quantise_n(const double *lw, int n, unsigned long long *u) { for (int i = 0; i < n; ++i) u[i] = rw_quantise(lw[i]); }
void rw_host_target_n(const double *p, const unsigned long long *U, int n, unsigned long long *t)
{
    for (int i = 0; i < n; ++i) t[i] = rw_target(p[i], U[i]);
}
}
