// mbb_reweight.hip.h -- a device-resident chain reweighted under another posterior density: Pareto-smoothed importance
// weights per source, and the weighted statistics of the summary's columns (gfx950, fp64, wave64).  The definitions are
// in include/mbb_hip.h; the step logic in mbb_psis.hip.h and mbb_rwsteps.hip.h.
//
// Per window entry the kernels keep three columns in the chain's cell layout [nsrc][nw][nsteps], so that ChainView and the
// summary's select read them as derived slots: lq (the target's lnprob of the row), lw (r = lq - lp, then the log weight;
// -inf for an entry that is not used) and u (the integer weight, with the entry's class in its two top bits).
//
// Kernels:
//   k_rw_gather   a thread per (source, entry) of a slab [nsrc][m][5]: the window's rows in the likelihood's multi-source
//                 row grouping (launch_rows then runs on the slab)
//   k_rw_ratio    a thread per slab row: r = lq - lp and the entry's class into the columns; row-status bits
//   k_rw_count    per (source, split): used, zero and left-out entries, max r
//   k_rw_begin    per source: merges the splits; S, M; asks the summary's select for the cutoff (as k_pw_begin)
//   k_rw_shift    per (source, split): lw = r - max r
//   (mbbs::k_sum_hist / k_sum_pick, eight passes, unchanged)
//   k_rw_tail     one workgroup per source: the tail in window order, sorted by (lw, index) in LDS, the Pareto fit with a
//                 grid point per thread, the smoothed lw; then sum e^lw, sum e^2lw, the u column and U = sum u
//   k_rw_wstats   per (source, column, split): sum u x, NaN count among the used entries
//   k_rw_wbegin   per (source, column): the weighted mean, the targets t = rw_target(p, U)
//   k_rw_whist    one radix pass of the WEIGHTED select: 256-bin histograms of sums of u (64-bit words in LDS), one per
//                 distinct prefix still followed
//   k_rw_wpick    merges the splits' histograms, finds each target's bin, extends its prefix
//   k_rw_cov      per (source, split): 15 weighted sums of products about the weighted means, and the used entry of
//                 largest lq
//   k_rw_finish   a thread per (source, column slot): every output of the call
//   k_rw_entries  the per-entry outputs [nsrc][n] in window order
// Every floating-point sum has a fixed order: a thread's entries in order, a binary tree over the threads, the splits in
// order or by the summary's split tree.  Every accumulation of weights is an integer one; the only atomics are integer
// ones (histogram sums in LDS, status bits).  No kernel holds an array in registers: none uses scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_device.hip.h"
#include "mbb_summary.hip.h"
#include "mbb_psis.hip.h"
#include "mbb_rwsteps.hip.h"

namespace mbbrw {

using mbbc::kCols;
using mbbc::kMaxSplits;
using mbbs::kThreads;
constexpr int kMaxPct = mbbs::kMaxPct;
constexpr int kCountWords = 4;        // 64-bit words per (source, split) of k_rw_count: used, zero, left out, max r's bits
constexpr int kWStatWords = 2;        // doubles per (column, split) of k_rw_wstats: sum u x, NaN count
constexpr int kCovWords = 18;         // doubles per (source, split) of k_rw_cov: 15 products, best lq, best index, pad
// status bits beside the summary's (include/mbb_hip.h: mbb_reweight_status)
constexpr int kStKHigh = 16, kStTailShort = 32, kStTailFlat = 64, kStHasZero = 128, kStAllZero = 1 << 16;
// an entry's class, in the two top bits of its word of the u column
constexpr int kUsed = 0, kZero = 1, kLeftOut = 2, kClsShift = 62;
constexpr unsigned long long kWeightMask = (1ull << kClsShift) - 1ull;

struct RwState {
    long long S, nzero, nleft;        // used, zero and left-out entries of the window
    double mx;                        // max r over the used entries
    unsigned long long U;             // sum u (k_rw_tail)
    double khat, ess, lnz;
    int M, why;
};

struct WColState {
    unsigned long long prefix[kMaxPct];     // the key bits found so far, right-aligned
    unsigned long long target[kMaxPct];     // the cumulative weight wanted among the samples that share the prefix
    double mean;
    int nranks;                             // 0: nothing to select (no weight, or a NaN among the used entries)
    int nan;
};

struct RwArgs : mbbc::ChainView {
    const double *lnprob;             // [nsrc][nw][nsteps]
    double *lqcol, *lwcol;            // [cells] each
    unsigned long long *ucol;         // [cells]
    // the slab: entries i0 .. i0 + m - 1 of every source
    double *s_rows;                   // [nsrc][m][5]
    const double *s_lnl;              // [nsrc][m]
    const int32_t *s_status;
    long long i0;
    int m;
    int smooth;
    int npct;
    double pct[kMaxPct];
    // work
    unsigned long long *count;        // [nsrc][splits][kCountWords]
    RwState *state;                   // [nsrc]
    mbbs::ColState *sel;              // [nsrc]: the select's column
    int *gstatus;                     // [nsrc] row-status bits of the entries left out
    double *wpart;                    // [nsrc * ncol][splits][kWStatWords]
    WColState *wstate;                // [nsrc * ncol]
    unsigned long long *whist;        // [nsrc * ncol][splits][kMaxPct][256]
    double *covpart;                  // [nsrc][splits][kCovWords]
    const int *colstatus;             // [nsrc][kCols] status bits gathered while the derived columns were filled
    // results
    long long *o_nused, *o_nzero, *o_nleft, *o_wsum;      // [nsrc]
    double *o_khat, *o_ess, *o_lnz;                       // [nsrc]
    double *o_mean, *o_pct;                               // [nsrc][kCols], [nsrc][kCols][npct]
    double *o_cov, *o_best;                               // [nsrc][25], [nsrc][6]
    int *o_tail, *o_status, *o_colstatus, *o_bestidx;     // [nsrc], [nsrc], [nsrc][kCols], [nsrc][2]
};

__device__ __forceinline__ int cls_of(unsigned long long w) { return (int)(w >> kClsShift); }

static __global__ __launch_bounds__(kThreads) void k_rw_gather(const RwArgs a)
{
    const long long tt = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (tt >= (long long)a.nsrc * a.m) return;
    const int src = (int)(tt / a.m);
    const long long j = a.i0 + (tt - (long long)src * a.m);
    const double *x = a.chain + mbbc::sample_flat(a, src, j) * 5;
    double *o = a.s_rows + tt * 5;
#pragma unroll
    for (int k = 0; k < 5; ++k) o[k] = x[k];
}

static __global__ __launch_bounds__(kThreads) void k_rw_ratio(const RwArgs a)
{
    const long long tt = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (tt >= (long long)a.nsrc * a.m) return;
    const int src = (int)(tt / a.m);
    const long long j = a.i0 + (tt - (long long)src * a.m);
    const long long flat = mbbc::sample_flat(a, src, j);
    const double lq = a.s_lnl[tt], lp = a.lnprob[flat];
    const double r = lq - lp;
    int cls = kLeftOut;
    if (mbbps::ps_finite(r)) cls = kUsed;
    else if (mbbps::ps_finite(lp) && lq == -INFINITY) cls = kZero;
    a.lqcol[flat] = lq;
    a.lwcol[flat] = cls == kUsed ? r : -INFINITY;
    a.ucol[flat] = (unsigned long long)cls << kClsShift;
    const int st = a.s_status[tt];
    if (cls == kLeftOut && st != mbbd::ROW_OK) atomicOr(&a.gstatus[src], 1 << (mbbs::kStRowShift + (st & 7)));
}

static __global__ __launch_bounds__(kThreads) void k_rw_count(const RwArgs a)
{
    __shared__ double lds[kThreads];
    __shared__ long long ldsn[kThreads];
    const int src = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    long long nu = 0, nz = 0, nl = 0;
    double mx = -INFINITY;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const long long flat = mbbc::sample_flat(a, src, j);
        const int cls = cls_of(a.ucol[flat]);
        if (cls == kUsed) { ++nu; mx = fmax(mx, a.lwcol[flat]); }
        else if (cls == kZero) ++nz;
        else ++nl;
    }
    const auto addn = [](long long x, long long y) { return x + y; };
    const long long bu = mbbs::block_tree(nu, ldsn, addn), bz = mbbs::block_tree(nz, ldsn, addn),
                    bl = mbbs::block_tree(nl, ldsn, addn);
    const double bmx = mbbs::block_tree(mx, lds, [](double x, double y) { return fmax(x, y); });
    if (t == 0) {
        unsigned long long *p = a.count + ((size_t)src * a.splits + split) * kCountWords;
        p[0] = (unsigned long long)bu; p[1] = (unsigned long long)bz; p[2] = (unsigned long long)bl;
        p[3] = (unsigned long long)__double_as_longlong(bmx);
    }
}

// one thread per source
static __global__ __launch_bounds__(64) void k_rw_begin(const RwArgs a)
{
    const int src = blockIdx.x * 64 + threadIdx.x;
    if (src >= a.nsrc) return;
    const unsigned long long *p = a.count + (size_t)src * a.splits * kCountWords;
    long long nu = 0, nz = 0, nl = 0;
    double mx = -INFINITY;
    for (int i = 0; i < a.splits; ++i) {
        nu += (long long)p[i * kCountWords + 0];
        nz += (long long)p[i * kCountWords + 1];
        nl += (long long)p[i * kCountWords + 2];
        mx = fmax(mx, __longlong_as_double((long long)p[i * kCountWords + 3]));
    }
    RwState &st = a.state[src];
    st.S = nu; st.nzero = nz; st.nleft = nl; st.mx = mx;
    st.M = (int)mbbps::ps_tail_len(nu);
    mbbs::ColState &cs = a.sel[src];
    cs.nranks = st.M >= 5 ? 1 : 0;
    cs.prefix[0] = 0ull;
    cs.rank[0] = (unsigned int)(a.n - st.M - 1);      // (M <= n / 5: never negative)
    cs.n_used = nu; cs.nan = 0;
}

static __global__ __launch_bounds__(kThreads) void k_rw_shift(const RwArgs a)
{
    const int src = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const double mx = a.state[src].mx;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const long long flat = mbbc::sample_flat(a, src, j);
        if (cls_of(a.ucol[flat]) == kUsed) a.lwcol[flat] = a.lwcol[flat] - mx;
    }
}

// The place of a thread's flag among the workgroup's set flags, in thread order, and their number.  Every thread of
// the workgroup calls it.  (mbb_pointwise.hip.h's, copied.)
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

static __global__ __launch_bounds__(kThreads) void k_rw_tail(const RwArgs a)
{
    __shared__ double tv[mbbps::kTailMax];            // the tail's lw, then its x
    __shared__ int ti[mbbps::kTailMax];               // ... and window indices
    __shared__ double ra[kThreads];
    __shared__ unsigned long long ru[kThreads];
    __shared__ double th[mbbps::kGridMax + 2], lp[mbbps::kGridMax + 2];
    __shared__ double s_fit[3];
    __shared__ int s_why;
    __shared__ int wcnt[kThreads / 64];
    const int src = blockIdx.x, t = threadIdx.x;
    RwState &st = a.state[src];
    double *lw = a.lwcol;
    const int M = st.M;
    int why = M < 5 ? mbbps::kFitShort : mbbps::kFitOk;
    double khat = INFINITY;

    if (why == mbbps::kFitOk) {
        // the tail, in window order: what is above the cutoff, and of the entries equal to it those after the cutoff's own
        const mbbs::ColState &cs = a.sel[src];
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
        const double expc = exp(mbbs::from_key(a.sel[src].prefix[0]));
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
                if (a.smooth)
                    for (int i = t; i < M; i += kThreads)
                        lw[mbbc::sample_flat(a, src, (long long)ti[i])] = mbbps::ps_smoothed(i, M, khat, sigma, expc);
                __threadfence_block();
            }
        }
        __syncthreads();
    }

    // the weights: sum e^lw, sum e^2lw (lw <= 0: neither overflows), the u column and U
    double s1 = 0.0, s2 = 0.0;
    unsigned long long usum = 0ull;
    for (long long j = t; j < a.n; j += kThreads) {
        const long long flat = mbbc::sample_flat(a, src, j);
        const unsigned long long w = a.ucol[flat];
        if (cls_of(w) != kUsed) { a.ucol[flat] = w & ~kWeightMask; continue; }
        const double v = lw[flat];
        const double e = exp(v);
        s1 += e;
        s2 += e * e;
        const unsigned long long u = mbbrws::rw_quantise(v);
        usum += u;
        a.ucol[flat] = u;                               // (class kUsed: top bits 0)
    }
    const auto add = [](double x, double y) { return x + y; };
    const double b1 = mbbs::block_tree(s1, ra, add);
    const double b2 = mbbs::block_tree(s2, ra, add);
    const unsigned long long bu = mbbs::block_tree(usum, ru, [](unsigned long long x, unsigned long long y) { return x + y; });
    if (t != 0) return;
    const double qnan = __builtin_nan("");
    const long long N = st.S + st.nzero;
    st.U = bu;
    st.khat = khat;
    st.why = why;
    st.ess = st.S > 0 ? (b1 * b1) / b2 : qnan;
    st.lnz = st.S > 0 ? st.mx + log(b1) - log((double)N) : (st.nzero > 0 ? -INFINITY : qnan);
}

// ---- weighted statistics of the summary's columns -----------------------------------------------
static __global__ __launch_bounds__(kThreads) void k_rw_wstats(const RwArgs a)
{
    __shared__ double lds[kThreads];
    __shared__ long long ldsn[kThreads];
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const int src = cid / a.ncol, slot = a.col[cid - src * a.ncol];
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    double sum = 0.0;
    long long nan = 0;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const unsigned long long w = a.ucol[mbbc::sample_flat(a, src, j)];
        if (cls_of(w) != kUsed) continue;
        const double v = mbbc::sample(a, src, slot, j);
        if (v != v) ++nan;
        if (w) sum += (double)w * v;                    // (u = 0: no part in any sum, whatever the value)
    }
    const double bsum = mbbs::block_tree(sum, lds, [](double x, double y) { return x + y; });
    const long long bn = mbbs::block_tree(nan, ldsn, [](long long x, long long y) { return x + y; });
    if (t == 0) {
        double *p = a.wpart + ((size_t)cid * a.splits + split) * kWStatWords;
        p[0] = bsum; p[1] = (double)bn;
    }
}

// one thread per column: merge the splits, place the targets
static __global__ __launch_bounds__(64) void k_rw_wbegin(const RwArgs a)
{
    __shared__ double sh[64][kMaxSplits + 1];          // (split_tree's row per thread)
    const int cid = blockIdx.x * 64 + threadIdx.x;
    if (cid >= a.nsrc * a.ncol) return;
    const int src = cid / a.ncol;
    const double *p = a.wpart + (size_t)cid * a.splits * kWStatWords;
    long long nan = 0;
    for (int i = 0; i < a.splits; ++i) nan += (long long)p[i * kWStatWords + 1];
    const double sum = mbbs::split_tree(p, a.splits, kWStatWords, sh[threadIdx.x]);
    const unsigned long long U = a.state[src].U;
    WColState &ws = a.wstate[cid];
    ws.nan = nan > 0;
    ws.mean = U > 0ull && nan == 0 ? sum / (double)U : __builtin_nan("");
    ws.nranks = 0;
    if (U > 0ull && nan == 0) {
        for (int k = 0; k < a.npct; ++k) {
            ws.prefix[k] = 0ull;
            ws.target[k] = mbbrws::rw_target(a.pct[k], U);
        }
        ws.nranks = a.npct;
    }
}

// The distinct prefixes among a column's targets, in order of first appearance (the same list in k_rw_whist and
// k_rw_wpick).  Returns their number; grp[r] = the list entry target r follows.
__device__ __forceinline__ int distinct_prefixes(const WColState &st, unsigned long long *pre, int *grp)
{
    int ng = 0;
    for (int r = 0; r < st.nranks; ++r) {
        int g = 0;
        while (g < ng && pre[g] != st.prefix[r]) ++g;
        if (g == ng) pre[ng++] = st.prefix[r];
        grp[r] = g;
    }
    return ng;
}

static __global__ __launch_bounds__(kThreads) void k_rw_whist(const RwArgs a, int pass)
{
    __shared__ unsigned long long h[kMaxPct * 256];
    __shared__ unsigned long long pre[kMaxPct];
    __shared__ int grp[kMaxPct];
    __shared__ int s_ng;
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const WColState &st = a.wstate[cid];
    if (st.nranks == 0) return;                          // (the whole workgroup)
    const int src = cid / a.ncol, slot = a.col[cid - src * a.ncol];
    if (t == 0) s_ng = distinct_prefixes(st, pre, grp);
    __syncthreads();
    const int ng = s_ng;
    for (int i = t; i < ng * 256; i += kThreads) h[i] = 0ull;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const unsigned long long w = a.ucol[mbbc::sample_flat(a, src, j)];
        if (cls_of(w) != kUsed || w == 0ull) continue;
        const unsigned long long key = mbbs::to_key(mbbc::sample(a, src, slot, j));
        const unsigned long long top = pass ? key >> (shift + 8) : 0ull;
        for (int g = 0; g < ng; ++g)
            if (top == pre[g]) { atomicAdd(&h[g * 256 + (int)((key >> shift) & 255ull)], w); break; }
    }
    __syncthreads();
    unsigned long long *out = a.whist + ((size_t)cid * a.splits + split) * kMaxPct * 256;
    for (int i = t; i < ng * 256; i += kThreads) out[i] = h[i];
}

static __global__ __launch_bounds__(kThreads) void k_rw_wpick(const RwArgs a)
{
    __shared__ unsigned long long scan[kThreads];
    __shared__ unsigned long long pre[kMaxPct], npre[kMaxPct], ntarget[kMaxPct];
    __shared__ int grp[kMaxPct];
    __shared__ int s_ng;
    const int cid = blockIdx.x, t = threadIdx.x;
    WColState &st = a.wstate[cid];
    if (st.nranks == 0) return;
    if (t == 0) s_ng = distinct_prefixes(st, pre, grp);
    __syncthreads();
    const int ng = s_ng, nr = st.nranks;
    for (int g = 0; g < ng; ++g) {
        unsigned long long c = 0ull;
        for (int s = 0; s < a.splits; ++s) c += a.whist[(((size_t)cid * a.splits + s) * kMaxPct + g) * 256 + t];
        // inclusive scan over the 256 bins
        scan[t] = c;
        __syncthreads();
        for (int w = 1; w < kThreads; w *= 2) {
            const unsigned long long add = t >= w ? scan[t - w] : 0ull;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        const unsigned long long incl = scan[t], excl = incl - c;
        // the smallest value whose cumulative weight reaches the target: the bin with excl < target <= incl
        for (int r = 0; r < nr; ++r)
            if (grp[r] == g && excl < st.target[r] && st.target[r] <= incl) {
                npre[r] = (pre[g] << 8) | (unsigned long long)t;
                ntarget[r] = st.target[r] - excl;
            }
        __syncthreads();
    }
    if (t < nr) {
        st.prefix[t] = npre[t];
        st.target[t] = ntarget[t];
    }
}

// per source and split: weighted sums of products about the weighted means of the five parameters, and the used entry
// of largest lq (mbbs::better's tie rule: the smaller index)
static __global__ __launch_bounds__(kThreads) void k_rw_cov(const RwArgs a)
{
    __shared__ double lds[kThreads];
    __shared__ long long ldsi[kThreads];
    const int src = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    // (slots 0..4 are always active and come first)
    const WColState *ws = a.wstate + (size_t)src * a.ncol;
    const double m0 = ws[0].mean, m1 = ws[1].mean, m2 = ws[2].mean, m3 = ws[3].mean, m4 = ws[4].mean;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    double c00 = 0, c01 = 0, c02 = 0, c03 = 0, c04 = 0, c11 = 0, c12 = 0, c13 = 0, c14 = 0, c22 = 0, c23 = 0, c24 = 0,
           c33 = 0, c34 = 0, c44 = 0;
    double bv = 0.0;
    long long bi = -1;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        long long w, step;
        mbbc::sample_cell(a, j, w, step);
        const long long flat = ((long long)src * a.nw + w) * a.nsteps + step;
        const unsigned long long uw = a.ucol[flat];
        if (cls_of(uw) != kUsed) continue;
        const double lq = a.lqcol[flat];
        const long long idx = w * a.nsteps + step;
        if (mbbs::better(lq, idx, bv, bi)) { bv = lq; bi = idx; }
        if (uw == 0ull) continue;
        const double u = (double)uw;
        const double *x = a.chain + flat * 5;
        const double d0 = x[0] - m0, d1 = x[1] - m1, d2 = x[2] - m2, d3 = x[3] - m3, d4 = x[4] - m4;
        const double u0 = u * d0, u1 = u * d1, u2 = u * d2, u3 = u * d3, u4 = u * d4;
        c00 += u0 * d0; c01 += u0 * d1; c02 += u0 * d2; c03 += u0 * d3; c04 += u0 * d4;
        c11 += u1 * d1; c12 += u1 * d2; c13 += u1 * d3; c14 += u1 * d4;
        c22 += u2 * d2; c23 += u2 * d3; c24 += u2 * d4;
        c33 += u3 * d3; c34 += u3 * d4;
        c44 += u4 * d4;
    }
    double *out = a.covpart + ((size_t)src * a.splits + split) * kCovWords;
    const auto add = [](double x, double y) { return x + y; };
#define MBB_RW_COV_OUT(I, C)                                 \
    {                                                        \
        const double s_ = mbbs::block_tree(C, lds, add);     \
        if (t == 0) out[I] = s_;                             \
    }
    MBB_RW_COV_OUT(0, c00) MBB_RW_COV_OUT(1, c01) MBB_RW_COV_OUT(2, c02) MBB_RW_COV_OUT(3, c03) MBB_RW_COV_OUT(4, c04)
    MBB_RW_COV_OUT(5, c11) MBB_RW_COV_OUT(6, c12) MBB_RW_COV_OUT(7, c13) MBB_RW_COV_OUT(8, c14)
    MBB_RW_COV_OUT(9, c22) MBB_RW_COV_OUT(10, c23) MBB_RW_COV_OUT(11, c24)
    MBB_RW_COV_OUT(12, c33) MBB_RW_COV_OUT(13, c34) MBB_RW_COV_OUT(14, c44)
#undef MBB_RW_COV_OUT
    // the best entry: a tree over (value, index) pairs
    __syncthreads();
    lds[t] = bv; ldsi[t] = bi;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w && mbbs::better(lds[t + w], ldsi[t + w], lds[t], ldsi[t])) { lds[t] = lds[t + w]; ldsi[t] = ldsi[t + w]; }
        __syncthreads();
    }
    if (t == 0) { out[15] = lds[0]; out[16] = (double)ldsi[0]; }
}

// one thread per (source, column slot): every output of the call
static __global__ __launch_bounds__(64) void k_rw_finish(const RwArgs a)
{
    __shared__ double sh[64][kMaxSplits + 1];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.nsrc * kCols) return;
    const int src = i / kCols, slot = i - src * kCols;
    const double qnan = __builtin_nan("");
    const RwState &rs = a.state[src];
    int ci = -1;
    for (int k = 0; k < a.ncol; ++k) if (a.col[k] == slot) ci = k;
    if (ci < 0) {
        a.o_mean[i] = qnan; a.o_colstatus[i] = mbbs::kStAbsent;
        for (int k = 0; k < a.npct; ++k) a.o_pct[(size_t)i * a.npct + k] = qnan;
    } else {
        const WColState &ws = a.wstate[(size_t)src * a.ncol + ci];
        a.o_mean[i] = ws.mean;
        a.o_colstatus[i] = a.colstatus[i] | (rs.U == 0ull ? mbbs::kStEmpty : 0) | (ws.nan ? mbbs::kStNaN : 0);
        for (int k = 0; k < a.npct; ++k)
            a.o_pct[(size_t)i * a.npct + k] = ws.nranks ? mbbs::from_key(ws.prefix[k]) : qnan;
    }
    if (slot != 0) return;
    // per source: the scalars, the covariance (no ddof correction) and the best entry
    a.o_nused[src] = rs.S; a.o_nzero[src] = rs.nzero; a.o_nleft[src] = rs.nleft; a.o_wsum[src] = (long long)rs.U;
    a.o_khat[src] = rs.khat; a.o_ess[src] = rs.ess; a.o_lnz[src] = rs.lnz;
    a.o_tail[src] = rs.M;
    a.o_status[src] = a.gstatus[src] | (rs.S == 0 ? mbbs::kStEmpty : 0) | (rs.nleft > 0 ? mbbs::kStNaN : 0) |
                      (rs.khat > 0.7 ? kStKHigh : 0) | (rs.why == mbbps::kFitShort ? kStTailShort : 0) |
                      (rs.why == mbbps::kFitFlat ? kStTailFlat : 0) | (rs.nzero > 0 ? kStHasZero : 0) |
                      (rs.S == 0 && rs.nzero > 0 ? kStAllZero : 0);
    const double *cp = a.covpart + (size_t)src * a.splits * kCovWords;
    int e = 0;
    for (int p = 0; p < 5; ++p)
        for (int q = p; q < 5; ++q, ++e) {
            const double s = mbbs::split_tree(cp + e, a.splits, kCovWords, sh[threadIdx.x]);
            const double c = rs.U > 0ull ? s / (double)rs.U : qnan;
            a.o_cov[(size_t)src * 25 + p * 5 + q] = c;
            a.o_cov[(size_t)src * 25 + q * 5 + p] = c;
        }
    double bv = 0.0;
    long long bi = -1;
    for (int s = 0; s < a.splits; ++s) {
        const double sv = cp[(size_t)s * kCovWords + 15];
        const long long si = (long long)cp[(size_t)s * kCovWords + 16];
        if (mbbs::better(sv, si, bv, bi)) { bv = sv; bi = si; }
    }
    if (bi < 0) {                                       // no used entry
        for (int k = 0; k < 6; ++k) a.o_best[(size_t)src * 6 + k] = qnan;
        a.o_bestidx[src * 2 + 0] = a.o_bestidx[src * 2 + 1] = -1;
        return;
    }
    const long long flat = (long long)src * a.nw * a.nsteps + bi;
    for (int k = 0; k < 5; ++k) a.o_best[(size_t)src * 6 + k] = a.chain[flat * 5 + k];
    a.o_best[(size_t)src * 6 + 5] = a.lqcol[flat];
    a.o_bestidx[src * 2 + 0] = (int)(bi / a.nsteps);
    a.o_bestidx[src * 2 + 1] = (int)(bi - (bi / a.nsteps) * a.nsteps);
}

// A per-entry output [nsrc][n] in window order: what = 0 lq, 1 r = lq - lp, 2 lw, 3 u (as a 64-bit integer).
static __global__ __launch_bounds__(kThreads) void k_rw_entries(const RwArgs a, int what, double *out)
{
    const long long tt = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (tt >= (long long)a.nsrc * a.n) return;
    const int src = (int)(tt / a.n);
    const long long flat = mbbc::sample_flat(a, src, tt - (long long)src * a.n);
    if (what == 0) out[tt] = a.lqcol[flat];
    else if (what == 1) out[tt] = a.lqcol[flat] - a.lnprob[flat];
    else if (what == 2) out[tt] = a.lwcol[flat];
    else reinterpret_cast<long long *>(out)[tt] = (long long)(a.ucol[flat] & kWeightMask);
}

}   // namespace mbbrw
