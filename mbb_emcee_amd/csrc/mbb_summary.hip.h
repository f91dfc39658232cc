// mbb_summary.hip.h -- posterior summaries of a device-resident chain (gfx950, fp64, wave64).
//
// What the reference's mbb_results makes of a chain on the host (results.py:160-165 best fit,
// :314-369 _parcen_internal: mean and numpy.percentile of the flattened chain with optional
// clipping, :433-493 one-sided limits), computed where the chain is: per (source, column)
// n_used / mean / min / max and EXACT order statistics by a radix select, per source the 5 x 5
// sample covariance and the sample of largest lnprob.
//
// The chain is in emcee's layout, chain [nsrc][nw][nsteps][5] and lnprob [nsrc][nw][nsteps]
// (k_chain_reorder's output); derived columns are [nsrc][nw][nsteps] each.  A column's samples are
// the steps burn, burn + thin, ... of every walker, in [nw][nkept] order (numpy's flatten()).
//
// Kernels (256 threads; grid.x = nsrc * active columns, grid.y = splits of the column):
//   k_sum_stats   count, NaN count, sum (clipped and unclipped), min, max of a split
//   k_sum_begin   merges the splits; ranks of the order statistics numpy's "linear" percentile needs
//   k_sum_hist    one radix pass: 256-bin histograms of the next 8 key bits, one per distinct prefix
//                 still followed (at most 16: two ranks per percentile), in LDS, then to global
//   k_sum_pick    merges the splits' histograms, finds each rank's bin, extends its prefix
//   k_sum_cov     per source and split: 15 sums of products about the mean, and the best sample
//   k_sum_finish  interpolates the percentiles as numpy does, writes every output
//   k_sum_take / k_sum_lir / k_sum_dustmass   fill the derived columns from the SED kernels' outputs
//   k_sum_lir_src / k_sum_dustmass_src        ... with a redshift and a luminosity distance per source (SrcConst)
// Eight radix passes over the order-preserving 64-bit image of the doubles select every rank at
// once.  All floating-point sums are fixed-order trees (eight interleaved partial sums per thread,
// a binary tree over the threads in LDS, a binary tree over the splits): the same chain gives the
// same bits.  The only atomics are integer ones (histogram counts in LDS, status bits).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_chain_view.hip.h"

namespace mbbs {

using mbbc::kCols;
using mbbc::kMaxSplits;
constexpr int kMaxPct = 8;       // percentiles per call
constexpr int kMaxRanks = 2 * kMaxPct;
constexpr int kThreads = 256;
constexpr int kStatWords = 8;    // doubles per (column, split) of k_sum_stats
constexpr int kCovWords = 18;    // doubles per (source, split) of k_sum_cov: 15 products, best lnprob, best index, pad

// column status bits (include/mbb_hip.h: mbb_summary_status)
constexpr int kStEmpty = 1, kStNaN = 2, kStAbsent = 4, kStRowShift = 8;

struct ColState {
    unsigned long long prefix[kMaxRanks];   // the key bits found so far, right-aligned
    unsigned int rank[kMaxRanks];           // the rank wanted among the samples that share the prefix
    double gamma[kMaxPct];                  // numpy's interpolation weight of each percentile
    double mean, umean, vmin, vmax;         // (umean: the unclipped mean, for the covariance)
    long long n_used;
    int nranks;                             // 0: nothing to select (empty column, or one holding a NaN)
    int nan;
};

struct SumArgs : mbbc::ChainView {
    const double *lnprob;                   // [nsrc][nw][nsteps]
    int npct;
    double pct[kMaxPct];
    int has_lo[kCols], has_hi[kCols];
    double lo[kCols], hi[kCols];
    // work
    double *part;                           // [nsrc*ncol][splits][kStatWords]
    ColState *state;                        // [nsrc*ncol]
    unsigned int *hist;                     // [nsrc*ncol][splits][kMaxRanks][256]
    double *covpart;                        // [nsrc][splits][kCovWords]
    int *colstatus;                         // [nsrc][kCols] status bits gathered while the derived columns were filled
    // results [nsrc][kCols]...
    long long *o_nused;
    double *o_mean, *o_min, *o_max, *o_pct; // o_pct [nsrc][kCols][npct]
    int *o_status;
    double *o_cov, *o_best;                 // [nsrc][25], [nsrc][6]
    int *o_bestidx;                         // [nsrc][2] walker, step
};

__device__ __forceinline__ unsigned long long to_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_key(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ bool kept(const SumArgs &a, int slot, double v)
{
    // _parcen_internal's clipping (results.py:351-367): a NaN fails either comparison and is dropped
    bool k = true;
    if (a.has_lo[slot]) k = k && v >= a.lo[slot];
    if (a.has_hi[slot]) k = k && v <= a.hi[slot];
    return k;
}

// binary tree over the workgroup's 256 values in LDS, fixed order; the result in every thread
template <typename T, typename F>
__device__ __forceinline__ T block_tree(T v, T *lds, F op)
{
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w) lds[t] = op(lds[t], lds[t + w]);
        __syncthreads();
    }
    return lds[0];
}

// binary tree over the splits' values (stride doubles apart), fixed order, in a row of LDS of the caller's
__device__ __forceinline__ double split_tree(const double *p, int splits, int stride, double *v)
{
    // (kept as loops over LDS: unrolled, the 64 values go to registers, 256 of them)
#pragma nounroll
    for (int i = 0; i < kMaxSplits; ++i) v[i] = i < splits ? p[(size_t)i * stride] : 0.0;
#pragma nounroll
    for (int w = 1; w < kMaxSplits; w *= 2) {
#pragma nounroll
        for (int i = 0; i + w < kMaxSplits; i += 2 * w) v[i] += v[i + w];
    }
    return v[0];
}

__global__ __launch_bounds__(kThreads) void k_sum_stats(const SumArgs a)
{
    __shared__ double lds[kThreads];
    __shared__ long long ldsn[kThreads];
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const int src = cid / a.ncol, slot = a.col[cid - src * a.ncol];
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0;
    double u0 = 0, u1 = 0, u2 = 0, u3 = 0, u4 = 0, u5 = 0, u6 = 0, u7 = 0;
    double mn = INFINITY, mx = -INFINITY;
    long long cnt = 0, nan = 0;
#define MBB_SUM_ONE(Q, S, U)                               \
    {                                                      \
        const long long j = base + (Q) * kThreads + t;     \
        if (j < j1) {                                      \
            const double v = sample(a, src, slot, j);      \
            U += v;                                        \
            if (kept(a, slot, v)) {                        \
                S += v;                                    \
                ++cnt;                                     \
                if (v != v) ++nan;                         \
                mn = fmin(mn, v);                          \
                mx = fmax(mx, v);                          \
            }                                              \
        }                                                  \
    }
    for (long long base = j0; base < j1; base += 8 * kThreads) {
        MBB_SUM_ONE(0, s0, u0) MBB_SUM_ONE(1, s1, u1) MBB_SUM_ONE(2, s2, u2) MBB_SUM_ONE(3, s3, u3)
        MBB_SUM_ONE(4, s4, u4) MBB_SUM_ONE(5, s5, u5) MBB_SUM_ONE(6, s6, u6) MBB_SUM_ONE(7, s7, u7)
    }
#undef MBB_SUM_ONE
    const auto add = [](double x, double y) { return x + y; };
    const double sum = block_tree(((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), lds, add);
    const double usum = block_tree(((u0 + u1) + (u2 + u3)) + ((u4 + u5) + (u6 + u7)), lds, add);
    const double bmn = block_tree(mn, lds, [](double x, double y) { return fmin(x, y); });
    const double bmx = block_tree(mx, lds, [](double x, double y) { return fmax(x, y); });
    const long long bc = block_tree(cnt, ldsn, [](long long x, long long y) { return x + y; });
    const long long bn = block_tree(nan, ldsn, [](long long x, long long y) { return x + y; });
    if (t == 0) {
        double *p = a.part + ((size_t)cid * a.splits + split) * kStatWords;
        p[0] = (double)bc; p[1] = (double)bn; p[2] = sum; p[3] = usum; p[4] = bmn; p[5] = bmx;
    }
}

// one thread per column: merge the splits, place the ranks
__global__ __launch_bounds__(64) void k_sum_begin(const SumArgs a)
{
    __shared__ double sh[64][kMaxSplits + 1];          // (split_tree's row per thread)
    const int cid = blockIdx.x * 64 + threadIdx.x;
    if (cid >= a.nsrc * a.ncol) return;
    const double *p = a.part + (size_t)cid * a.splits * kStatWords;
    long long cnt = 0, nan = 0;
    double mn = INFINITY, mx = -INFINITY;
    for (int i = 0; i < a.splits; ++i) {
        cnt += (long long)p[i * kStatWords + 0];
        nan += (long long)p[i * kStatWords + 1];
        mn = fmin(mn, p[i * kStatWords + 4]);
        mx = fmax(mx, p[i * kStatWords + 5]);
    }
    const double sum = split_tree(p + 2, a.splits, kStatWords, sh[threadIdx.x]);
    const double usum = split_tree(p + 3, a.splits, kStatWords, sh[threadIdx.x]);
    ColState &st = a.state[cid];
    const double qnan = __builtin_nan("");
    st.n_used = cnt;
    st.nan = nan > 0;
    st.mean = cnt > 0 ? sum / (double)cnt : qnan;
    st.umean = usum / (double)a.n;
    st.vmin = cnt > 0 && nan == 0 ? mn : qnan;
    st.vmax = cnt > 0 && nan == 0 ? mx : qnan;
    st.nranks = 0;
    if (cnt > 0 && nan == 0) {
        // numpy's method "linear" (Hyndman & Fan 7), in numpy's own arithmetic: virtual index (n - 1) (q / 100),
        // the two bracketing order statistics, gamma = virtual - floor(virtual); at or beyond the last index
        // both are the last
        const double nn = (double)cnt;
        for (int k = 0; k < a.npct; ++k) {
            const double q = a.pct[k] / 100.0;
            const double vi = (nn - 1.0) * q;
            const double fl = floor(vi);
            long long lo = (long long)fl, hi = lo + 1;
            if (vi >= nn - 1.0) lo = hi = cnt - 1;
            if (vi < 0.0) lo = hi = 0;
            st.gamma[k] = vi - fl;
            st.prefix[2 * k] = st.prefix[2 * k + 1] = 0ull;
            st.rank[2 * k] = (unsigned int)lo;
            st.rank[2 * k + 1] = (unsigned int)hi;
        }
        st.nranks = 2 * a.npct;
    }
}

// The distinct prefixes among a column's ranks, in order of first appearance (the same list in k_sum_hist
// and k_sum_pick).  Returns their number; grp[r] = the list entry rank r follows.
__device__ __forceinline__ int distinct_prefixes(const ColState &st, unsigned long long *pre, int *grp)
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

__global__ __launch_bounds__(kThreads) void k_sum_hist(const SumArgs a, int pass)
{
    __shared__ unsigned int h[kMaxRanks * 256];
    __shared__ unsigned long long pre[kMaxRanks];
    __shared__ int grp[kMaxRanks];
    __shared__ int s_ng;
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const ColState &st = a.state[cid];
    if (st.nranks == 0) return;                          // (the whole workgroup)
    const int src = cid / a.ncol, slot = a.col[cid - src * a.ncol];
    if (t == 0) s_ng = distinct_prefixes(st, pre, grp);
    __syncthreads();
    const int ng = s_ng;
    for (int i = t; i < ng * 256; i += kThreads) h[i] = 0u;
    __syncthreads();
    const int shift = 56 - 8 * pass;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    // (every lane makes every trip, so that the wave-wide vote below sees whole waves)
    for (long long base = j0; base < j1; base += kThreads) {
        const long long j = base + t;
        int bin = -1;
        if (j < j1) {
            const double v = sample(a, src, slot, j);
            if (kept(a, slot, v)) {
                const unsigned long long key = to_key(v);
                const unsigned long long top = pass ? key >> (shift + 8) : 0ull;
                for (int g = 0; g < ng; ++g)
                    if (top == pre[g]) { bin = g * 256 + (int)((key >> shift) & 255ull); break; }
            }
        }
        // the leading bytes of a column's doubles are nearly all alike: a wave whose lanes all count into one
        // bin adds its 64 at once instead of queueing 64 atomics on one LDS word
        const int first = __builtin_amdgcn_readfirstlane(bin);
        if (__all(bin == first)) {
            if (first >= 0 && (t & 63) == 0) atomicAdd(&h[first], 64u);
        } else if (bin >= 0) {
            atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    unsigned int *out = a.hist + ((size_t)cid * a.splits + split) * kMaxRanks * 256;
    for (int i = t; i < ng * 256; i += kThreads) out[i] = h[i];
}

__global__ __launch_bounds__(kThreads) void k_sum_pick(const SumArgs a)
{
    __shared__ unsigned int scan[kThreads];
    __shared__ unsigned long long pre[kMaxRanks], npre[kMaxRanks];
    __shared__ unsigned int nrank[kMaxRanks];
    __shared__ int grp[kMaxRanks];
    __shared__ int s_ng;
    const int cid = blockIdx.x, t = threadIdx.x;
    ColState &st = a.state[cid];
    if (st.nranks == 0) return;
    if (t == 0) s_ng = distinct_prefixes(st, pre, grp);
    __syncthreads();
    const int ng = s_ng, nr = st.nranks;
    for (int g = 0; g < ng; ++g) {
        unsigned int c = 0;
        for (int s = 0; s < a.splits; ++s) c += a.hist[(((size_t)cid * a.splits + s) * kMaxRanks + g) * 256 + t];
        // inclusive scan over the 256 bins
        scan[t] = c;
        __syncthreads();
        for (int w = 1; w < kThreads; w *= 2) {
            const unsigned int add = t >= w ? scan[t - w] : 0u;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        const unsigned int incl = scan[t], excl = incl - c;
        for (int r = 0; r < nr; ++r)
            if (grp[r] == g && excl <= st.rank[r] && st.rank[r] < incl) {
                npre[r] = (pre[g] << 8) | (unsigned long long)t;
                nrank[r] = st.rank[r] - excl;
            }
        __syncthreads();
    }
    if (t < nr) {
        st.prefix[t] = npre[t];
        st.rank[t] = nrank[t];
    }
}

// numpy's argmax order: a NaN beats everything, then the larger value, then the smaller index (index < 0: none yet)
__device__ __forceinline__ bool better(double v1, long long i1, double v2, long long i2)
{
    const bool n1 = v1 != v1, n2 = v2 != v2;
    if (i1 < 0) return false;
    if (i2 < 0) return true;
    if (n1 != n2) return n1;
    if (!n1 && v1 != v2) return v1 > v2;
    return i1 < i2;
}

// per source and split: sums of products about the (unclipped) means of the five parameters, and the best sample
__global__ __launch_bounds__(kThreads) void k_sum_cov(const SumArgs a)
{
    __shared__ double lds[kThreads];
    __shared__ long long ldsi[kThreads];
    const int src = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    // (slots 0..4 are always active and come first)
    const ColState *st = a.state + (size_t)src * a.ncol;
    const double m0 = st[0].umean, m1 = st[1].umean, m2 = st[2].umean, m3 = st[3].umean, m4 = st[4].umean;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    double c00 = 0, c01 = 0, c02 = 0, c03 = 0, c04 = 0, c11 = 0, c12 = 0, c13 = 0, c14 = 0, c22 = 0, c23 = 0, c24 = 0,
           c33 = 0, c34 = 0, c44 = 0;
    double bv = 0.0;
    long long bi = -1;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const long long w = j / a.nkept, k = j - w * a.nkept;
        const long long step = a.burn + k * a.thin;
        const long long flat = ((long long)src * a.nw + w) * a.nsteps + step;
        const double *x = a.chain + flat * 5;
        const double d0 = x[0] - m0, d1 = x[1] - m1, d2 = x[2] - m2, d3 = x[3] - m3, d4 = x[4] - m4;
        c00 += d0 * d0; c01 += d0 * d1; c02 += d0 * d2; c03 += d0 * d3; c04 += d0 * d4;
        c11 += d1 * d1; c12 += d1 * d2; c13 += d1 * d3; c14 += d1 * d4;
        c22 += d2 * d2; c23 += d2 * d3; c24 += d2 * d4;
        c33 += d3 * d3; c34 += d3 * d4;
        c44 += d4 * d4;
        const double lp = a.lnprob[flat];
        const long long idx = w * a.nsteps + step;
        if (better(lp, idx, bv, bi)) { bv = lp; bi = idx; }
    }
    double *out = a.covpart + ((size_t)src * a.splits + split) * kCovWords;
    const auto add = [](double x, double y) { return x + y; };
#define MBB_COV_OUT(I, C)                              \
    {                                                  \
        const double s_ = block_tree(C, lds, add);     \
        if (t == 0) out[I] = s_;                       \
    }
    MBB_COV_OUT(0, c00) MBB_COV_OUT(1, c01) MBB_COV_OUT(2, c02) MBB_COV_OUT(3, c03) MBB_COV_OUT(4, c04)
    MBB_COV_OUT(5, c11) MBB_COV_OUT(6, c12) MBB_COV_OUT(7, c13) MBB_COV_OUT(8, c14)
    MBB_COV_OUT(9, c22) MBB_COV_OUT(10, c23) MBB_COV_OUT(11, c24)
    MBB_COV_OUT(12, c33) MBB_COV_OUT(13, c34) MBB_COV_OUT(14, c44)
#undef MBB_COV_OUT
    // the best sample: a tree over (value, index) pairs
    __syncthreads();
    lds[t] = bv; ldsi[t] = bi;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w && better(lds[t + w], ldsi[t + w], lds[t], ldsi[t])) { lds[t] = lds[t + w]; ldsi[t] = ldsi[t + w]; }
        __syncthreads();
    }
    if (t == 0) { out[15] = lds[0]; out[16] = (double)ldsi[0]; }
}

// one thread per (source, column slot): every output of the call
__global__ __launch_bounds__(64) void k_sum_finish(const SumArgs a)
{
    __shared__ double sh[64][kMaxSplits + 1];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.nsrc * kCols) return;
    const int src = i / kCols, slot = i - src * kCols;
    const double qnan = __builtin_nan("");
    int ci = -1;
    for (int k = 0; k < a.ncol; ++k) if (a.col[k] == slot) ci = k;
    if (ci < 0) {
        a.o_nused[i] = 0; a.o_mean[i] = a.o_min[i] = a.o_max[i] = qnan; a.o_status[i] = kStAbsent;
        for (int k = 0; k < a.npct; ++k) a.o_pct[(size_t)i * a.npct + k] = qnan;
    } else {
        const ColState &st = a.state[(size_t)src * a.ncol + ci];
        a.o_nused[i] = st.n_used; a.o_mean[i] = st.mean; a.o_min[i] = st.vmin; a.o_max[i] = st.vmax;
        a.o_status[i] = a.colstatus[i] | (st.n_used == 0 ? kStEmpty : 0) | (st.nan ? kStNaN : 0);
        for (int k = 0; k < a.npct; ++k) {
            double r = qnan;
            if (st.nranks) {
                // numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) from t = 0.5 on
                const double lo = from_key(st.prefix[2 * k]), hi = from_key(st.prefix[2 * k + 1]), g = st.gamma[k];
                const double diff = hi - lo;
                r = lo + diff * g;
                if (g >= 0.5) r = hi - diff * (1.0 - g);
            }
            a.o_pct[(size_t)i * a.npct + k] = r;
        }
    }
    if (slot != 0) return;
    // per source: covariance (ddof = 1) and best fit
    const double *cp = a.covpart + (size_t)src * a.splits * kCovWords;
    int e = 0;
    for (int p = 0; p < 5; ++p)
        for (int q = p; q < 5; ++q, ++e) {
            const double c = split_tree(cp + e, a.splits, kCovWords, sh[threadIdx.x]) / (double)(a.n - 1);
            a.o_cov[(size_t)src * 25 + p * 5 + q] = c;
            a.o_cov[(size_t)src * 25 + q * 5 + p] = c;
        }
    double bv = 0.0;
    long long bi = -1;
    for (int s = 0; s < a.splits; ++s) {
        const double sv = cp[(size_t)s * kCovWords + 15];
        const long long si = (long long)cp[(size_t)s * kCovWords + 16];
        if (better(sv, si, bv, bi)) { bv = sv; bi = si; }
    }
    const long long flat = (long long)src * a.nw * a.nsteps + bi;
    for (int k = 0; k < 5; ++k) a.o_best[(size_t)src * 6 + k] = a.chain[flat * 5 + k];
    a.o_best[(size_t)src * 6 + 5] = a.lnprob[flat];
    a.o_bestidx[src * 2 + 0] = (int)(bi / a.nsteps);
    a.o_bestidx[src * 2 + 1] = (int)(bi - (bi / a.nsteps) * a.nsteps);
}

// ---- derived columns --------------------------------------------------------------------------
// rows off .. off + n - 1 of the flat chain [nsrc * nw * nsteps]; a row's status counts for its column when
// the row is inside the window
__device__ __forceinline__ void note_status(int *colstatus, int slot, long long row, int st, int nw, int nsteps,
                                            int burn, int thin)
{
    if (st == 0) return;
    const long long per = (long long)nw * nsteps;
    const int src = (int)(row / per), step = (int)(row % nsteps);
    if (step >= burn && (step - burn) % thin == 0) atomicOr(&colstatus[src * kCols + slot], 1 << (kStRowShift + (st & 7)));
}

// peak wavelength: element 5 of the prologue's six outputs per row
__global__ void k_sum_take(const double *out6, const int32_t *status, int n, long long off, double *col, int *colstatus,
                           int nw, int nsteps, int burn, int thin)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    col[off + i] = out6[(size_t)i * 6 + 5];
    note_status(colstatus, 5, off + i, status[i], nw, nsteps, burn, thin);
}

// L_IR = prefac * (1e-17 * integral)    (postprocess.lir; results.py:627-674)
__global__ void k_sum_lir(const double *integ, const int32_t *status, int n, long long off, double prefac, double *col,
                          int *colstatus, int nw, int nsteps, int burn, int thin)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    col[off + i] = prefac * (1e-17 * integ[i]);
    note_status(colstatus, 6, off + i, status[i], nw, nsteps, burn, thin);
}

// What of L_IR and dust mass depends on a source's redshift and luminosity distance (mbb_summary_spec's src_redshift /
// src_lumdist_mpc): the bounds of the L_IR integral in GHz and its prefactor, and DustArgs' members of the same names.
// summary_fill_derived forms one entry per source on the host, in the scalar path's own expressions.  An entry of NaNs
// is a source whose redshift or distance is unknown: its L_IR and dust mass are NaN in every cell.
struct SrcConst { double numin, numax, prefac, opz, dl2, temp_fac, bnu_fac, knu_fac; };

// ... with the prefactor of the row's source, (off + i) / (nw * nsteps).  An unknown source gets its NaN written here,
// whatever the integral's slot holds, and its rows' status is not looked at.
__global__ void k_sum_lir_src(const double *integ, const int32_t *status, int n, long long off, const SrcConst *src,
                              double *col, int *colstatus, int nw, int nsteps, int burn, int thin)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double prefac = src[(off + i) / ((long long)nw * nsteps)].prefac;
    if (prefac != prefac) { col[off + i] = __builtin_nan(""); return; }
    col[off + i] = prefac * (1e-17 * integ[i]);
    note_status(colstatus, 6, off + i, status[i], nw, nsteps, burn, thin);
}

// dust mass in 1e8 solar masses: the closed form of results.py:726-801 (postprocess.dustmass) per chain row
struct DustArgs { double opz, dl2, temp_fac, bnu_fac, knu_fac, k10, msolar8, wavenorm; int opthin; };
__device__ __forceinline__ double dustmass_row(const double *row, const DustArgs &d)
{
    const double T = row[0] * d.opz, beta = row[1], S = row[4] * 1e-26;
    const double B = d.bnu_fac / expm1(d.temp_fac / T);
    const double K = d.k10 * pow(d.knu_fac, -beta);
    double m = d.dl2 * S / (d.opz * K * B * d.msolar8);
    if (!d.opthin) {
        const double tau = pow(row[2] / d.wavenorm, beta);
        m = m * (-tau / expm1(-tau));
    }
    return m;
}
__global__ void k_sum_dustmass(const double *chain, long long n, DustArgs d, double *col)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    col[i] = dustmass_row(chain + i * 5, d);
}

// ... with the redshift-dependent members of d taken from the row's source, i / per_src
__global__ void k_sum_dustmass_src(const double *chain, long long n, long long per_src, const SrcConst *src, DustArgs d,
                                   double *col)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const SrcConst s = src[i / per_src];
    if (s.opz != s.opz) { col[i] = __builtin_nan(""); return; }
    d.opz = s.opz; d.dl2 = s.dl2; d.temp_fac = s.temp_fac; d.bnu_fac = s.bnu_fac; d.knu_fac = s.knu_fac;
    col[i] = dustmass_row(chain + i * 5, d);
}

}   // namespace mbbs
