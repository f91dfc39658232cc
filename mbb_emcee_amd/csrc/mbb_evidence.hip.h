// mbb_evidence.hip.h -- the marginal likelihood ln Z of every source of a device-resident chain by bridge sampling
// (gfx950, fp64, wave64).  The step logic is mbb_bridge.hip.h's; include/mbb_hip.h has the definitions.
//
// The window's nkept kept steps are split: the first nfit = nkept / 2 of every walker fit the Gaussian proposal, the
// other n1k = nkept - nfit of every walker are the posterior samples it is bridged to, so that the proposal does not
// depend on the samples.  Fit sample j is (walker j / nfit, step burn + (j % nfit) thin); posterior sample j is
// (walker j / n1k, step burn + (nfit + j % n1k) thin).
//
// Kernels:
//   k_ev_moments   a workgroup per source: mean and covariance (ddof = 1) of the five columns over the fit half in two
//                  passes, min and max of every column over the whole window (a column with min == max is held), the
//                  held values (the first window cell)
//   k_ev_factor    a thread per source: the free set, br_chol, status
//   k_ev_propose   a thread per (source, draw) of a slab: three Philox4x32-10 blocks at counter (draw, first_source +
//                  source, "BRDG", 0..2), key = seed -> five 53-bit uniforms -> br_ppnd -> br_draw; the row and its lnq
//   k_ev_l2        a thread per (source, draw) of a slab: ln l2 = lnP - lnq into the [nsrc][N2] block
//   k_ev_post      a thread per (source, posterior sample): lnq there, ln l1 = lnprob - lnq (NaN: the cell is left out)
//   k_ev_bridge    a workgroup per source: the shift l*, the whole fixed-point iteration, the error; one launch
// Every sum is a per-thread strided partial, wave_sum's fixed tree, then the four waves' totals in order: a source's
// result has the same bits whatever else the call holds.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_device.hip.h"
#include "mbb_chain_view.hip.h"
#include "mbb_stretch.hip.h"   // philox4x32
#include "mbb_bridge.hip.h"

namespace mbbev {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr unsigned int kStreamWord = 0x42524447u;    // "BRDG": the third counter word of every proposal draw
constexpr int kMaxN2 = 1 << 22;                      // proposal draws per source and call
constexpr int kMaxIter = 100000;
// status bits (include/mbb_hip.h: mbb_evidence_status)
constexpr int kConverged = 1, kMaxIterHit = 2, kCovSingular = 4, kPostLeftOut = 8, kNoOverlap = 16, kAllHeld = 32,
              kHeldShift = 8;
// per source, doubles: mean[5] cov[25] L[25] held[5] sumlog
constexpr int kMomMean = 0, kMomCov = 5, kMomL = 30, kMomHeld = 55, kMomSumlog = 60, kMomWords = 61;

struct EvArgs : mbbc::ChainView {
    const double *lnprob;             // [nsrc][nw][nsteps]
    int nfit, n1k;                    // kept steps per walker of the fit half and of the posterior half
    long long n1max;                  // nw * n1k
    int n2;                           // proposal draws per source
    unsigned fixed;                   // lm_fixed_mask: the caller's, lambda0 of a thin model, alpha without one
    int first_source;
    unsigned long long seed;
    double tol;
    int maxiter;
    const double *neff;               // [nsrc] or null
    double *mom;                      // [nsrc][kMomWords]
    int *free_;                       // [nsrc] the free set
    int *status;                      // [nsrc]
    double *l1, *l2;                  // ln l1 [nsrc][n1max], ln l2 [nsrc][n2]
    double *post_lnq;                 // [nsrc][n1max] or null
    // a slab: draws [i0, i0 + m) of every source
    int i0, m;
    double *s_rows, *s_lnq;           // [nsrc][m][5], [nsrc][m]
    const double *s_lnl;              // [nsrc][m] their lnP
    // results
    double *o_lnz, *o_err;            // [nsrc]
    int *o_niter;
    long long *o_n1, *o_inside;
};

// the workgroup's total of v in every thread; lds: kWaves doubles.  (Two barriers: lds may be reused at once.)
__device__ __forceinline__ double block_sum(double v, double *lds)
{
    v = mbbd::wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = lds[0];
    for (int w = 1; w < kWaves; ++w) t += lds[w];
    return t;
}

__device__ __forceinline__ long long fit_flat(const EvArgs &a, int src, long long j)
{
    const long long w = j / a.nfit, step = a.burn + (j - w * a.nfit) * a.thin;
    return ((long long)src * a.nw + w) * a.nsteps + step;
}

__device__ __forceinline__ long long post_flat(const EvArgs &a, int src, long long j)
{
    const long long w = j / a.n1k, step = a.burn + (a.nfit + (j - w * a.n1k)) * a.thin;
    return ((long long)src * a.nw + w) * a.nsteps + step;
}

static __global__ __launch_bounds__(kThreads) void k_ev_moments(const EvArgs a)
{
    __shared__ double lds[kWaves];
    __shared__ double s_min[kThreads], s_max[kThreads];
    const int src = blockIdx.x, t = threadIdx.x;
    double *const mom = a.mom + (size_t)src * kMomWords;
    const long long nf = (long long)a.nw * a.nfit;
    // min and max of every column over the whole window
    unsigned held = 0;
    for (int k = 0; k < 5; ++k) {
        double mn = __builtin_inf(), mx = -__builtin_inf();
        bool nan = false;
        for (long long j = t; j < a.n; j += kThreads) {
            const double v = a.chain[mbbc::sample_flat(a, src, j) * 5 + k];
            if (v != v) nan = true;
            mn = fmin(mn, v); mx = fmax(mx, v);
        }
        if (nan) { mn = -__builtin_inf(); mx = __builtin_inf(); }      // (a NaN column is not a constant one)
        __syncthreads();
        s_min[t] = mn; s_max[t] = mx;
        __syncthreads();
        for (int w = kThreads / 2; w > 0; w >>= 1) {
            if (t < w) { s_min[t] = fmin(s_min[t], s_min[t + w]); s_max[t] = fmax(s_max[t], s_max[t + w]); }
            __syncthreads();
        }
        if (s_min[0] == s_max[0]) held |= 1u << k;
    }
    // the mean over the fit half
    double mu[5];
    for (int k = 0; k < 5; ++k) {
        double acc = 0.0;
        for (long long j = t; j < nf; j += kThreads) acc += a.chain[fit_flat(a, src, j) * 5 + k];
        mu[k] = block_sum(acc, lds) / (double)nf;
    }
    // the covariance about it
    for (int p = 0; p < 5; ++p)
        for (int q = p; q < 5; ++q) {
            double acc = 0.0;
            for (long long j = t; j < nf; j += kThreads) {
                const double *row = a.chain + fit_flat(a, src, j) * 5;
                acc = fma(row[p] - mu[p], row[q] - mu[q], acc);
            }
            const double c = block_sum(acc, lds) / (double)(nf - 1);
            if (t == 0) { mom[kMomCov + p * 5 + q] = c; mom[kMomCov + q * 5 + p] = c; }
        }
    if (t == 0) {
        const double *first = a.chain + mbbc::sample_flat(a, src, 0) * 5;
        for (int k = 0; k < 5; ++k) {
            mom[kMomHeld + k] = first[k];
            mom[kMomMean + k] = mu[k];
        }
        a.free_[src] = (int)mbbbr::br_free_mask(a.fixed, held);
    }
}

// one thread per source
static __global__ __launch_bounds__(64) void k_ev_factor(const EvArgs a)
{
    const int src = blockIdx.x * 64 + threadIdx.x;
    if (src >= a.nsrc) return;
    double *const mom = a.mom + (size_t)src * kMomWords;
    const unsigned free_ = (unsigned)a.free_[src];
    int st = 0;
    for (int k = 0; k < 5; ++k)
        if (!((free_ >> k) & 1u)) {
            st |= 1 << (kHeldShift + k);
            mom[kMomMean + k] = mom[kMomHeld + k];
        }
    double cov[25], L[25], sumlog;
    for (int i = 0; i < 25; ++i) cov[i] = mom[kMomCov + i];
    if (free_ == 0) st |= kAllHeld;
    if (!mbbbr::br_chol(cov, free_, L, &sumlog)) st |= kCovSingular;
    for (int i = 0; i < 25; ++i) mom[kMomL + i] = L[i];
    mom[kMomSumlog] = sumlog;
    const double qnan = __builtin_nan("");
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j)
            if (!((free_ >> i) & 1u) || !((free_ >> j) & 1u)) mom[kMomCov + i * 5 + j] = qnan;
    a.status[src] = st;
}

static __global__ __launch_bounds__(kThreads) void k_ev_propose(const EvArgs a)
{
    const long long tt = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (tt >= (long long)a.nsrc * a.m) return;
    const int src = (int)(tt / a.m), ii = (int)(tt - (long long)src * a.m);
    const int i = a.i0 + ii;
    const double *mom = a.mom + (size_t)src * kMomWords;
    const unsigned free_ = (unsigned)a.free_[src];
    unsigned int w[12];
    for (int b = 0; b < 3; ++b) {
        unsigned int c4[4] = {(unsigned int)i, (unsigned int)(a.first_source + src), kStreamWord, (unsigned int)b};
        philox4x32(c4, (unsigned int)a.seed, (unsigned int)(a.seed >> 32));
        for (int k = 0; k < 4; ++k) w[4 * b + k] = c4[k];
    }
    double z[5], theta[5];
    for (int k = 0; k < 5; ++k) z[k] = mbbbr::br_ppnd(mbbbr::br_centered(mbbbr::br_bits53(w[2 * k], w[2 * k + 1])));
    mbbbr::br_draw(mom + kMomMean, mom + kMomL, z, free_, mom + kMomHeld, theta);
    double *const row = a.s_rows + (size_t)tt * 5;
    for (int k = 0; k < 5; ++k) row[k] = theta[k];
    a.s_lnq[tt] = mbbbr::br_lnq(theta, mom + kMomMean, mom + kMomL, free_, mom[kMomSumlog]);
}

static __global__ __launch_bounds__(kThreads) void k_ev_l2(const EvArgs a)
{
    const long long tt = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (tt >= (long long)a.nsrc * a.m) return;
    const int src = (int)(tt / a.m), ii = (int)(tt - (long long)src * a.m);
    a.l2[(size_t)src * a.n2 + a.i0 + ii] = a.s_lnl[tt] - a.s_lnq[tt];
}

static __global__ __launch_bounds__(kThreads) void k_ev_post(const EvArgs a)
{
    const long long tt = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (tt >= (long long)a.nsrc * a.n1max) return;
    const int src = (int)(tt / a.n1max);
    const long long j = tt - (long long)src * a.n1max;
    const long long flat = post_flat(a, src, j);
    const double *mom = a.mom + (size_t)src * kMomWords;
    double theta[5];
    for (int k = 0; k < 5; ++k) theta[k] = a.chain[flat * 5 + k];
    const double lq = mbbbr::br_lnq(theta, mom + kMomMean, mom + kMomL, (unsigned)a.free_[src], mom[kMomSumlog]);
    const double lp = a.lnprob[flat];
    if (a.post_lnq) a.post_lnq[tt] = lq;
    a.l1[tt] = mbbbr::br_finite(lp) ? lp - lq : __builtin_nan("");
}

static __global__ __launch_bounds__(kThreads) void k_ev_bridge(const EvArgs a)
{
    __shared__ double lds[kWaves];
    const int src = blockIdx.x, t = threadIdx.x;
    const double *const l1 = a.l1 + (size_t)src * a.n1max, *const l2 = a.l2 + (size_t)src * a.n2;
    const double qnan = __builtin_nan("");
    int st = a.status[src];
    // the posterior cells that count, their mean ln l1; the draws inside the support
    double sum = 0.0, cnt = 0.0, inside = 0.0;
    for (long long j = t; j < a.n1max; j += kThreads) {
        const double v = l1[j];
        if (mbbbr::br_finite(v)) { sum += v; cnt += 1.0; }
    }
    for (int i = t; i < a.n2; i += kThreads) {
        const double v = l2[i];
        if (v > -mbbbr::kDblMax) inside += 1.0;
    }
    sum = block_sum(sum, lds); cnt = block_sum(cnt, lds); inside = block_sum(inside, lds);
    const long long n1 = (long long)cnt;
    if (n1 < a.n1max) st |= kPostLeftOut;
    double lnz = qnan, err = qnan;
    int niter = 0;
    if (st & kAllHeld) {
        lnz = a.lnprob[mbbc::sample_flat(a, src, 0)];
        err = 0.0;
    } else if (st & kCovSingular) {
    } else if (inside == 0.0) {
        st |= kNoOverlap;
    } else if (n1 > 0) {
        const double lstar = sum / cnt;
        double n1e = cnt;
        if (a.neff) n1e = fmin(fmax(a.neff[src], 1.0), cnt);
        const double n2 = (double)a.n2;
        const double s1 = n1e / (n1e + n2), s2 = n2 / (n1e + n2);
        double rho = 1.0;
        bool conv = false;
        while (niter < a.maxiter && !conv) {
            double sn = 0.0, sd = 0.0;
            for (int i = t; i < a.n2; i += kThreads) sn += mbbbr::br_term_num(l2[i] - lstar, rho, s1, s2);
            for (long long j = t; j < a.n1max; j += kThreads) {
                const double v = l1[j];
                if (mbbbr::br_finite(v)) sd += mbbbr::br_term_den(v - lstar, rho, s1, s2);
            }
            sn = block_sum(sn, lds); sd = block_sum(sd, lds);
            const double rho_new = (sn / n2) / (sd / cnt);
            ++niter;
            conv = mbbbr::br_converged(rho_new, rho, a.tol);
            rho = rho_new;
            if (!(rho > 0.0) || !mbbbr::br_finite(rho)) break;
        }
        st |= conv ? kConverged : kMaxIterHit;
        // the terms' means and variances (ddof = 1) at the final rho
        double sn = 0.0, sd = 0.0;
        for (int i = t; i < a.n2; i += kThreads) sn += mbbbr::br_term_num(l2[i] - lstar, rho, s1, s2);
        for (long long j = t; j < a.n1max; j += kThreads) {
            const double v = l1[j];
            if (mbbbr::br_finite(v)) sd += mbbbr::br_term_den(v - lstar, rho, s1, s2);
        }
        const double m1 = block_sum(sn, lds) / n2, m2 = block_sum(sd, lds) / cnt;
        double vn = 0.0, vd = 0.0;
        for (int i = t; i < a.n2; i += kThreads) {
            const double d = mbbbr::br_term_num(l2[i] - lstar, rho, s1, s2) - m1;
            vn = fma(d, d, vn);
        }
        for (long long j = t; j < a.n1max; j += kThreads) {
            const double v = l1[j];
            if (mbbbr::br_finite(v)) {
                const double d = mbbbr::br_term_den(v - lstar, rho, s1, s2) - m2;
                vd = fma(d, d, vd);
            }
        }
        const double v1 = block_sum(vn, lds) / (n2 - 1.0), v2 = block_sum(vd, lds) / (cnt - 1.0);
        if (rho > 0.0 && mbbbr::br_finite(rho)) {
            lnz = mbbm::m_log(rho) + lstar;
            err = sqrt(mbbbr::br_relerr2(m1, v1, n2, m2, v2, n1e));
        }
    }
    if (t == 0) {
        a.o_lnz[src] = lnz; a.o_err[src] = err; a.o_niter[src] = niter;
        a.o_n1[src] = n1; a.o_inside[src] = (long long)inside;
        a.status[src] = st;
    }
}

}   // namespace mbbev
