// The HOST build of csrc/mbb_popsteps.hip.h for tests/test_population_cpu.py: the text the kernels of csrc/mbb_population.hip.h run.
#define MBB_MATH_HOST 1
#include "../mbb_emcee_amd/csrc/mbb_popsteps.hip.h"

using namespace mbbpops;

namespace {
// One record merge after another over n entries, as one lane does it; then the record as words (m, s, s2, mean, M2)
template <int D> void fold(const double *prep, const double *x, const double *b, int n, double *words)
{
    PopRec<D, true> r;
    pop_clear(r);
    for (int j = 0; j < n; ++j) pop_add(r, pop_logdens<D>(prep, x + (size_t)j * D, b[j]), x + (size_t)j * D);
    pop_store(r, words);
}
template <int D> void merge(double *wa, const double *wb)
{
    PopRec<D, true> a, b;
    pop_load(a, wa); pop_load(b, wb);
    pop_merge(a, b);
    pop_store(a, wa);
}
}

extern "C" {
void pop_constants(double *c) { c[0] = kWallRelWidth; c[1] = kUnderflow; c[2] = kLn10; c[3] = mbbps::kLn2Pi; }
double pop_host_prior_factor(double theta, int has_uplim, double uplim, double lowlim, int has_gprior, double gmean, double givar)
{
    return pop_prior_factor(theta, has_uplim, uplim, lowlim, has_gprior, gmean, givar);
}
double pop_host_transform(double theta, int transform, double *lnjac) { return pop_transform(theta, transform, lnjac); }
// rows [n][5] -> x [n][d], b [n]
void pop_host_entries(const double *rows, int n, int d, const int *col, const int *transform, const int *has_uplim,
                      const int *has_gprior, const double *lowlim, const double *uplim, const double *gmean,
                      const double *givar, double *x, double *b)
{
    PopPrior p;
    for (int k = 0; k < 5; ++k) {
        p.has_uplim[k] = has_uplim[k]; p.has_gprior[k] = has_gprior[k];
        p.lowlim[k] = lowlim[k]; p.uplim[k] = uplim[k]; p.gmean[k] = gmean[k]; p.givar[k] = givar[k];
    }
    for (int j = 0; j < n; ++j) b[j] = pop_entry(rows + (size_t)j * 5, d, col, transform, p, x + (size_t)j * d);
}
int pop_host_prep_len(int d) { return pop_prep_len(d); }
int pop_host_prepare(const double *h, int d, double *prep) { return pop_prepare(h, d, prep) ? 1 : 0; }
// z of L z = y as pop_logdens forms it is not handed out; the log density a [n] of x [n][d] is
void pop_host_logdens(const double *prep, int d, const double *x, const double *b, int n, double *a)
{
    for (int j = 0; j < n; ++j) {
        const double *xj = x + (size_t)j * d;
        switch (d) {
        case 1: a[j] = pop_logdens<1>(prep, xj, b[j]); break;
        case 2: a[j] = pop_logdens<2>(prep, xj, b[j]); break;
        case 3: a[j] = pop_logdens<3>(prep, xj, b[j]); break;
        case 4: a[j] = pop_logdens<4>(prep, xj, b[j]); break;
        default: a[j] = pop_logdens<5>(prep, xj, b[j]); break;
        }
    }
}
int pop_host_words(int d) { return 3 + d + pop_tri(d); }
void pop_host_fold(const double *prep, int d, const double *x, const double *b, int n, double *words)
{
    switch (d) {
    case 1: fold<1>(prep, x, b, n, words); break;
    case 2: fold<2>(prep, x, b, n, words); break;
    case 3: fold<3>(prep, x, b, n, words); break;
    case 4: fold<4>(prep, x, b, n, words); break;
    default: fold<5>(prep, x, b, n, words); break;
    }
}
void pop_host_merge(int d, double *wa, const double *wb)
{
    switch (d) {
    case 1: merge<1>(wa, wb); break;
    case 2: merge<2>(wa, wb); break;
    case 3: merge<3>(wa, wb); break;
    case 4: merge<4>(wa, wb); break;
    default: merge<5>(wa, wb); break;
    }
}
}
