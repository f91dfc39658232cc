// mbb_pointwise.hip.h -- out-of-sample fit of a device-resident chain: WAIC and PSIS-LOO per source and band
// (gfx950, fp64, wave64).  The definitions are in include/mbb_hip.h; the step logic in mbb_psis.hip.h.
//
// Per chain entry theta and band b the kernels keep g_b = (Lambda r)_b, r = f - m(theta), one column [cells] per band of
// a group; the pointwise term ll_b = ps_ll(g_b, Lambda_bb) is formed from it wherever it is needed, by the same
// expression, and so has the same bits everywhere.  A second column per band holds the log weights lw.
//
// Kernels:
//   k_pw_g       a lane per row: g of the group's bands from a chunk's band fluxes (k_good_flux's); for
//                mbb_pointwise_rows ll of every band row by row.  C^-1 in LDS up to mbbq::kLdsCov bands.
//   k_pw_stat1   per (source, band, split): count, sum, (max, sum exp) and minimum of the finite ll
//   k_pw_begin   per (source, band): merges the splits in order; S, mean, lppd, M; asks the summary's select for the
//                cutoff, the entry of ascending rank n - M - 1 of the lw column
//   k_pw_stat2   per (source, band, split): sum (ll - mean)^2; writes lw = -ll - max(-ll), -inf for an entry left out
//   (mbbs::k_sum_hist / k_sum_pick, eight passes: the cutoff's key and its place among the entries equal to it)
//   k_pw_tail    one workgroup per (source, band): gathers the M tail entries in window order, sorts them by
//                (lw, index) in LDS, fits the generalised Pareto distribution (a grid point per thread), writes the
//                smoothed tail back into the lw column, then the weighted pass for elpd_loo and loo_pit; every output
// Every sum has a fixed order: a thread's entries in order, a binary tree over the threads, the splits in order.
// No kernel holds an array in registers: none uses scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_device.hip.h"
#include "mbb_summary.hip.h"
#include "mbb_goodness.hip.h"
#include "mbb_psis.hip.h"

namespace mbbpw {

using mbbq::kThreads;
constexpr int kPartWords = 5;         // doubles per (source, band, split) of k_pw_stat1: count, sum, max, sum exp, minimum
constexpr int kSelCols = 3;           // bands per launch of the summary's select: its derived-column slots
// status bits beside the summary's (include/mbb_hip.h: mbb_pointwise_status)
constexpr int kStKHigh = 16, kStTailShort = 32, kStTailFlat = 64, kStWaicVarHigh = 128;

struct GArgs {
    const double *mf;                 // band fluxes [nb][n]
    const int32_t *status;            // row status [n]
    int n, nb;
    long long off;                    // the first row's number among all rows of the call
    long long rows_per_src;           // row (off + i) belongs to source ((off + i) / rows_per_src) % nsrc_data
    int nsrc_data;
    const double *flux, *ivar;        // [nsrc_data][nb]
    const double *invcov;             // [nb][nb] or null
    int cov_in_lds;
    int b0, ng;                       // the group: bands b0 .. b0 + ng - 1
    double *gcol;                     // [ng][cells] or null: row i goes to element off + i of each
    long long cells;
    double *ll_rows;                  // [n][nb] or null: ll row by row (b0 = 0, ng = nb)
    int32_t *row_status;              // [n] or null
    int *gstatus;                     // [nsrc] row-status bits, or null
    int nw, nsteps, burn, thin;       // (gstatus: the chain's shape and window)
};

static __global__ __launch_bounds__(kThreads) void k_pw_g(const GArgs a)
{
    extern __shared__ double sh_pwcov[];
    const double *cinv = a.invcov;
    if (a.invcov && a.cov_in_lds) {
        for (int i = threadIdx.x; i < a.nb * a.nb; i += kThreads) sh_pwcov[i] = a.invcov[i];
        __syncthreads();
        cinv = sh_pwcov;
    }
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const long long row = a.off + i;
    const int st = a.status[i];
    const int src = (int)((row / a.rows_per_src) % a.nsrc_data);
    const double *f = a.flux + (size_t)src * a.nb, *iv = a.ivar + (size_t)src * a.nb;
    const double qnan = __builtin_nan("");
    for (int gb = 0; gb < a.ng; ++gb) {
        const int b = a.b0 + gb;
        double g = qnan, lam;
        if (!a.invcov) {
            lam = iv[b];
            if (st == mbbd::ROW_OK) g = lam * (f[b] - a.mf[(size_t)b * a.n + i]);
        } else {
            // every lane reads the same element of C^-1 at the same time: one LDS broadcast
            lam = cinv[b * a.nb + b];
            if (st == mbbd::ROW_OK) {
                double t = 0.0;
                for (int j = 0; j < a.nb; ++j) t = fma(cinv[b * a.nb + j], f[j] - a.mf[(size_t)j * a.n + i], t);
                g = t;
            }
        }
        if (a.gcol) a.gcol[(size_t)gb * a.cells + row] = g;
        if (a.ll_rows) a.ll_rows[(size_t)i * a.nb + b] = mbbps::ps_ll(g, lam);
    }
    if (a.row_status) a.row_status[i] = st;
    if (a.gstatus && st != mbbd::ROW_OK) {
        const long long per = (long long)a.nw * a.nsteps;
        const int csrc = (int)(row / per), step = (int)(row % a.nsteps);
        if (step >= a.burn && (step - a.burn) % a.thin == 0)
            atomicOr(&a.gstatus[csrc], 1 << (mbbs::kStRowShift + (st & 7)));
    }
}

struct PwState {
    long long S;                      // finite entries of the window
    double mean, lppd, mx;            // mean of ll, lppd, max(-ll)
    int M;
};

struct PwArgs : mbbc::ChainView {     // (the window, a column's splits: der and col are not used here)
    int nb, b0, ng;
    long long cells;
    double *gcol, *lwcol;             // [ng][cells] each
    const double *ivar, *invcov;      // the context's data: [nsrc_data][nb], [nb][nb] or null
    int nsrc_data;
    double *part, *part2;             // [nsrc * ng][splits][kPartWords], [nsrc * ng][splits]
    PwState *state;                   // [nsrc * ng]
    mbbs::ColState *sel;              // the select's columns: launch q holds [nsrc][bands of the launch], kSelCols apart
    const int *gstatus;               // [nsrc]
    // results [nsrc][nb]
    long long *o_nused;
    int *o_tail, *o_status;
    double *o_lppd, *o_pwaic, *o_elpdwaic, *o_elpdloo, *o_ploo, *o_khat, *o_pit;
};

__device__ __forceinline__ double lam_of(const PwArgs &a, int src, int b)
{
    if (a.invcov) return a.invcov[(size_t)b * a.nb + b];
    return a.ivar[(size_t)(a.nsrc_data == 1 ? 0 : src) * a.nb + b];
}

__device__ __forceinline__ mbbs::ColState &sel_of(const PwArgs &a, int src, int gb)
{
    const int q = gb / kSelCols, k = gb - q * kSelCols, nbat = min(kSelCols, a.ng - q * kSelCols);
    return a.sel[(size_t)q * a.nsrc * kSelCols + (size_t)src * nbat + k];
}

static __global__ __launch_bounds__(kThreads) void k_pw_stat1(const PwArgs a)
{
    __shared__ double lds[kThreads], lds2[kThreads];
    __shared__ long long ldsn[kThreads];
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const int src = cid / a.ng, gb = cid - src * a.ng;
    const double lam = lam_of(a, src, a.b0 + gb);
    const double *col = a.gcol + (size_t)gb * a.cells;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    long long cnt = 0;
    double sum = 0.0, m = -INFINITY, s = 0.0, mn = INFINITY;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const double ll = mbbps::ps_ll(col[mbbc::sample_flat(a, src, j)], lam);
        if (mbbps::ps_finite(ll)) {
            ++cnt;
            sum += ll;
            mbbps::ps_lse_add(m, s, ll);
            mn = fmin(mn, ll);
        }
    }
    const double bsum = mbbs::block_tree(sum, lds, [](double x, double y) { return x + y; });
    const double bmn = mbbs::block_tree(mn, lds, [](double x, double y) { return fmin(x, y); });
    const long long bc = mbbs::block_tree(cnt, ldsn, [](long long x, long long y) { return x + y; });
    __syncthreads();
    lds[t] = m; lds2[t] = s;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) mbbps::ps_lse_merge(lds[t], lds2[t], lds[t + w], lds2[t + w]);
        __syncthreads();
    }
    if (t == 0) {
        double *p = a.part + ((size_t)cid * a.splits + split) * kPartWords;
        p[0] = (double)bc; p[1] = bsum; p[2] = lds[0]; p[3] = lds2[0]; p[4] = bmn;
    }
}

// one thread per (source, band)
static __global__ __launch_bounds__(64) void k_pw_begin(const PwArgs a)
{
    const int cid = blockIdx.x * 64 + threadIdx.x;
    if (cid >= a.nsrc * a.ng) return;
    const int src = cid / a.ng, gb = cid - src * a.ng;
    const double *p = a.part + (size_t)cid * a.splits * kPartWords;
    long long cnt = 0;
    double sum = 0.0, m = -INFINITY, s = 0.0, mn = INFINITY;
    for (int i = 0; i < a.splits; ++i) {
        cnt += (long long)p[i * kPartWords + 0];
        sum += p[i * kPartWords + 1];
        mbbps::ps_lse_merge(m, s, p[i * kPartWords + 2], p[i * kPartWords + 3]);
        mn = fmin(mn, p[i * kPartWords + 4]);
    }
    PwState &st = a.state[cid];
    const double qnan = __builtin_nan("");
    st.S = cnt;
    st.mean = cnt > 0 ? sum / (double)cnt : qnan;
    st.lppd = cnt > 0 ? mbbps::ps_lse_value(m, s) - log((double)cnt) : qnan;
    st.mx = -mn;
    st.M = (int)mbbps::ps_tail_len(cnt);
    mbbs::ColState &cs = sel_of(a, src, gb);
    cs.nranks = st.M >= 5 ? 1 : 0;
    cs.prefix[0] = 0ull;
    cs.rank[0] = (unsigned int)(a.n - st.M - 1);      // (M <= n / 5: never negative)
    cs.n_used = cnt; cs.nan = 0;
}

static __global__ __launch_bounds__(kThreads) void k_pw_stat2(const PwArgs a)
{
    __shared__ double lds[kThreads];
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const int src = cid / a.ng, gb = cid - src * a.ng;
    const double lam = lam_of(a, src, a.b0 + gb);
    const double *col = a.gcol + (size_t)gb * a.cells;
    double *lw = a.lwcol + (size_t)gb * a.cells;
    const double mean = a.state[cid].mean, mx = a.state[cid].mx;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    double ss = 0.0;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const long long flat = mbbc::sample_flat(a, src, j);
        const double ll = mbbps::ps_ll(col[flat], lam);
        double w = -INFINITY;
        if (mbbps::ps_finite(ll)) {
            const double d = ll - mean;
            ss += d * d;
            w = -ll - mx;
        }
        lw[flat] = w;
    }
    const double bss = mbbs::block_tree(ss, lds, [](double x, double y) { return x + y; });
    if (t == 0) a.part2[(size_t)cid * a.splits + split] = bss;
}

// The place of a thread's flag among the workgroup's set flags, in thread order, and their number.  Every thread of
// the workgroup calls it.
__device__ __forceinline__ int block_rank(bool flag, int *wcnt, int &total)
{
    const unsigned long long bal = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wcnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        const int c = wcnt[w];
        if (w < wave) base += c;
        total += c;
    }
    return base + before;
}

// (value, index) pairs in ascending order
__device__ __forceinline__ bool pair_gt(double v1, int i1, double v2, int i2) { return v1 > v2 || (v1 == v2 && i1 > i2); }

static __global__ __launch_bounds__(kThreads) void k_pw_tail(const PwArgs a)
{
    __shared__ double tv[mbbps::kTailMax];            // the tail's lw, then its x
    __shared__ int ti[mbbps::kTailMax];               // ... and window indices
    __shared__ double ra[kThreads], rb[kThreads], rc[kThreads];
    __shared__ double th[mbbps::kGridMax + 2], lp[mbbps::kGridMax + 2];
    __shared__ double s_fit[3];
    __shared__ int s_why;
    __shared__ int wcnt[kThreads / 64];
    const int cid = blockIdx.x, t = threadIdx.x;
    const int src = cid / a.ng, gb = cid - src * a.ng, b = a.b0 + gb;
    const PwState st = a.state[cid];
    const double lam = lam_of(a, src, b);
    const double *col = a.gcol + (size_t)gb * a.cells;
    double *lw = a.lwcol + (size_t)gb * a.cells;
    const double qnan = __builtin_nan("");
    const int M = st.M;
    int why = M < 5 ? mbbps::kFitShort : mbbps::kFitOk;
    double khat = INFINITY;

    if (why == mbbps::kFitOk) {
        // the tail, in window order: what is above the cutoff, and of the entries equal to it those after the cutoff's own
        const mbbs::ColState &cs = sel_of(a, src, gb);
        const unsigned long long ckey = cs.prefix[0];
        const long long want = (long long)cs.rank[0];
        long long eq_seen = 0;
        int tail_n = 0;
        for (long long base = 0; base < a.n; base += kThreads) {
            const long long j = base + t;
            bool gt = false, eq = false;
            double v = 0.0;
            if (j < a.n) {
                v = lw[mbbc::sample_flat(a, src, j)];
                const unsigned long long key = mbbs::to_key(v);
                gt = key > ckey;
                eq = key == ckey;
            }
            int tot_eq, tot_in;
            const int r_eq = block_rank(eq, wcnt, tot_eq);
            const bool in = gt || (eq && eq_seen + r_eq > want);
            const int pos = tail_n + block_rank(in, wcnt, tot_in);
            if (in && pos < mbbps::kTailMax) { tv[pos] = v; ti[pos] = (int)j; }
            eq_seen += tot_eq;
            tail_n += tot_in;
        }
        if (tail_n != M) why = mbbps::kFitFlat;        // (cannot happen: the select is exact)
    }
    if (why == mbbps::kFitOk) {                         // (workgroup-uniform)
        int P = 1;
        while (P < M) P <<= 1;
        for (int i = M + t; i < P; i += kThreads) { tv[i] = INFINITY; ti[i] = 0x7fffffff; }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = t; i < P; i += kThreads) {
                    const int o = i ^ j;
                    if (o > i) {
                        const double v1 = tv[i], v2 = tv[o];
                        const int i1 = ti[i], i2 = ti[o];
                        if (pair_gt(v1, i1, v2, i2) == ((i & k) == 0)) { tv[i] = v2; tv[o] = v1; ti[i] = i2; ti[o] = i1; }
                    }
                }
                __syncthreads();
            }
        const double expc = exp(mbbs::from_key(sel_of(a, src, gb).prefix[0]));
        for (int i = t; i < M; i += kThreads) tv[i] = exp(tv[i]) - expc;
        __syncthreads();
        const double xs = mbbps::ps_xstar(tv, M), xM = tv[M - 1];
        if (!(xM > tv[0]) || !(xs > 0.0)) why = mbbps::kFitFlat;
        if (why == mbbps::kFitOk) {
            const int m = mbbps::ps_grid_len(M);
            if (t < m) {
                const double theta = mbbps::ps_theta(t + 1, m, xM, xs);
                th[t] = theta;
                lp[t] = mbbps::ps_profile(theta, tv, M);
            }
            __syncthreads();
            if (t == 0) s_why = mbbps::ps_combine(th, lp, m, tv, M, &s_fit[0], &s_fit[1], &s_fit[2]);
            __syncthreads();
            why = s_why;
            if (why == mbbps::kFitOk) {
                khat = s_fit[2];
                const double sigma = s_fit[1];
                for (int i = t; i < M; i += kThreads)
                    lw[mbbc::sample_flat(a, src, (long long)ti[i])] = mbbps::ps_smoothed(i, M, khat, sigma, expc);
                __threadfence_block();
            }
        }
        __syncthreads();
    }

    // the weighted pass: LSE(ll + lw), LSE(lw) and sum exp(lw) Phi, the last two on one running maximum
    double m1 = -INFINITY, s1 = 0.0, m2 = -INFINITY, s2 = 0.0, p2 = 0.0;
    const double rsl = 1.0 / sqrt(lam);
    for (long long j = t; j < a.n; j += kThreads) {
        const long long flat = mbbc::sample_flat(a, src, j);
        const double g = col[flat];
        const double ll = mbbps::ps_ll(g, lam);
        if (!mbbps::ps_finite(ll)) continue;
        const double w = lw[flat];
        mbbps::ps_lse_add(m1, s1, ll + w);
        const double phi = mbbps::ps_norm_cdf(g * rsl);
        if (s2 == 0.0) { m2 = w; s2 = 1.0; p2 = phi; }
        else if (w <= m2) { const double e = exp(w - m2); s2 += e; p2 += e * phi; }
        else { const double e = exp(m2 - w); s2 = s2 * e + 1.0; p2 = p2 * e + phi; m2 = w; }
    }
    __syncthreads();
    ra[t] = m1; rb[t] = s1;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) mbbps::ps_lse_merge(ra[t], rb[t], ra[t + w], rb[t + w]);
        __syncthreads();
    }
    const double lse1 = mbbps::ps_lse_value(ra[0], rb[0]);
    __syncthreads();
    ra[t] = m2; rb[t] = s2; rc[t] = p2;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w && rb[t + w] != 0.0) {
            const double ma = ra[t], mb = ra[t + w];
            if (rb[t] == 0.0) { ra[t] = mb; rb[t] = rb[t + w]; rc[t] = rc[t + w]; }
            else if (mb <= ma) { const double e = exp(mb - ma); rb[t] += rb[t + w] * e; rc[t] += rc[t + w] * e; }
            else { const double e = exp(ma - mb); rb[t] = rb[t] * e + rb[t + w]; rc[t] = rc[t] * e + rc[t + w]; ra[t] = mb; }
        }
        __syncthreads();
    }
    if (t != 0) return;
    const double lse2 = mbbps::ps_lse_value(ra[0], rb[0]);
    double ss = 0.0;
    for (int i = 0; i < a.splits; ++i) ss += a.part2[(size_t)cid * a.splits + i];
    const double pwaic = st.S >= 2 ? ss / (double)(st.S - 1) : qnan;
    const double elpdloo = st.S > 0 ? lse1 - lse2 : qnan;
    const size_t o = (size_t)src * a.nb + b;
    a.o_nused[o] = st.S;
    a.o_tail[o] = M;
    a.o_lppd[o] = st.lppd;
    a.o_pwaic[o] = pwaic;
    a.o_elpdwaic[o] = st.lppd - pwaic;
    a.o_elpdloo[o] = elpdloo;
    a.o_ploo[o] = st.lppd - elpdloo;
    a.o_khat[o] = khat;
    a.o_pit[o] = st.S > 0 ? rc[0] / rb[0] : qnan;
    a.o_status[o] = a.gstatus[src] | (st.S == 0 ? mbbs::kStEmpty : 0) | (st.S < a.n ? mbbs::kStNaN : 0) |
                    (khat > 0.7 ? kStKHigh : 0) | (why == mbbps::kFitShort ? kStTailShort : 0) |
                    (why == mbbps::kFitFlat ? kStTailFlat : 0) | (pwaic > 0.4 ? kStWaicVarHigh : 0);
}

}   // namespace mbbpw
