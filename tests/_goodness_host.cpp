// The host build of csrc/mbb_gammq.hip.h for tests/test_goodness_cpu.py: m_gammq_half on n (nb, chisq) pairs.
#define MBB_MATH_HOST
#include "../mbb_emcee_amd/csrc/mbb_gammq.hip.h"

extern "C" void goodness_host_q(const int *nb, const double *chisq, int n, double *q)
{
    for (int i = 0; i < n; ++i) q[i] = mbbm::m_gammq_half(nb[i], chisq[i]);
}
