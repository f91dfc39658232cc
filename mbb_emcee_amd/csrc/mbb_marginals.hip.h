// mbb_marginals.hip.h -- binned posterior marginals of a device-resident chain (gfx950, fp64, wave64).
//
// What a user of the reference makes on the host with numpy.histogram / numpy.histogram2d / corner of
// mbb_results.parameter_chain, computed where the chain is: per (source, column) a 1-D histogram of nbins bins, per
// (source, requested pair of columns) a 2-D histogram of nbins2 x nbins2 bins.  Counts are integers and the bin
// of a sample is decided by comparisons with numpy's own edges, so the result is numpy's EXACTLY.
//
// The chain is in emcee's layout [nsrc][nw][nsteps][5]; the derived columns (slots 5, 6, 7: peak wavelength, L_IR,
// dust mass) are [nsrc][nw][nsteps] each, filled by the summary's summary_fill_derived.  A column's samples are the
// steps burn, burn + thin, ... of every walker, as in mbb_summary.hip.h.
//
// Definition, per (source, column), nb bins over [lo, hi]:
//   range  given: one pair for the call;  automatic: min and max of the column's FINITE samples, min - 0.5 and
//          max + 0.5 when they are equal (numpy.histogram's rule);
//   edges  numpy.linspace(lo, hi, nb + 1) bit for bit: step = (hi - lo) / nb, e[i] = i * step + lo with the product and
//          the sum rounded separately, e[nb] = hi;
//   bin    sample x is in bin i iff e[i] <= x < e[i + 1], the last bin also takes x == e[nb]: a first guess
//          (x - lo) / (hi - lo) * nb is corrected against the edges, the comparisons decide;
//   x < lo, x > hi, x not finite: counted in n_below, n_above, n_nonfinite, never binned.
// A 2-D table of (a, b) counts the samples that are binned in BOTH columns' ranges, at [bin of a][bin of b].
//
// Kernels (256 threads; a column is cut into splits of whole samples as the summary cuts it):
//   k_marg_extent   grid (nsrc * active columns, splits): min and max of a split's finite samples
//   k_marg_edges    grid nsrc * 8: merges the splits' extents, settles [lo, hi] of the slot, writes the edges of
//                   both tables and the slot's part of the status
//   k_marg_hist1    grid (nsrc * active columns, splits): the split's 1-D table in LDS (16 KB at 4096 bins), integer
//                   atomicAdd, a wave whose 64 lanes meet in one bin adding its 64 at once (k_sum_hist's vote: a fixed
//                   parameter sends every lane to one bin); then the table and the three outside counts to global
//   k_marg_hist2    grid (nsrc * pairs, splits): the same for a pair, 40 KB of LDS at 100 x 100
//   k_marg_merge    adds the splits' tables and counts, integer adds in split order, and writes every output
// One workgroup per (source, column or pair, split): a table is private to its workgroup, nothing is shared across
// workgroups but the read-only chain.  All accumulation is integer: the same chain gives the same bits every time.
// No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_chain_view.hip.h"

namespace mbbm {

using mbbc::kCols;
using mbbc::kMaxSplits;
constexpr int kThreads = 256;
constexpr int kSplitSamples = 4096;   // a split has at most this many samples (16 per thread) until kMaxSplits are reached
constexpr int kMaxBins = 4096;    // 1-D: 16 KB of LDS
constexpr int kMaxBins2 = 100;    // 2-D, per axis: 40 KB of LDS
constexpr int kMaxPairs = 28;     // all pairs of eight columns
constexpr int kTail = 4;          // words behind a split's 1-D table: n_below, n_above, n_nonfinite, pad

// status bits of a column (include/mbb_hip.h: mbb_marginals_status; the summary's values and row shift)
constexpr int kStEmpty = 1, kStNonfinite = 2, kStAbsent = 4, kStRowShift = 8;

struct Range { double lo, hi; };   // NaNs: nothing of the column is binned (absent, or no finite sample)

struct MargArgs : mbbc::ChainView {
    int nbins, nbins2, npairs;
    int pair[kMaxPairs][2];                 // slots (a, b), a < b
    int has_range[kCols];
    double lo[kCols], hi[kCols];
    // work
    double *extent;                         // [nsrc*ncol][splits][2]: min, max of the finite samples
    Range *range;                           // [nsrc][kCols]
    unsigned int *part1;                    // [nsrc*ncol][splits][nbins + kTail]
    unsigned int *part2;                    // [nsrc*npairs][splits][nbins2 * nbins2]
    const int *colstatus;                   // [nsrc][kCols]: the row-status bits summary_fill_derived gathered
    // results
    unsigned int *o_counts1, *o_counts2;    // [nsrc][kCols][nbins], [nsrc][npairs][nbins2][nbins2]
    double *o_edges1, *o_edges2;            // [nsrc][kCols][nbins + 1], [nsrc][kCols][nbins2 + 1]
    long long *o_used, *o_below, *o_above, *o_nonfinite;   // [nsrc][kCols]
    int *o_status;                          // [nsrc][kCols]
};

__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }   // (v - v: NaN for a NaN and for an infinity)

// numpy.linspace(lo, hi, nb + 1)[i]: the product and the sum are rounded separately, the last edge is hi itself
struct Edges {
    double lo, hi, step, scale;
    int nb;
    __device__ __forceinline__ Edges(Range r, int nbins)
        : lo(r.lo), hi(r.hi), step((r.hi - r.lo) / (double)nbins), scale(r.hi - r.lo), nb(nbins) {}
    __device__ __forceinline__ double at(int i) const
    {
        return i == nb ? hi : __dadd_rn(__dmul_rn((double)i, step), lo);
    }
    // The bin of x, lo <= x <= hi: e[i] <= x < e[i + 1], the last bin closed.  The guess is numpy.histogram's own; the
    // edges decide (they do not decrease with i, so the two walks end at the one bin that holds x).
    __device__ __forceinline__ int bin(double x) const
    {
        int g = (int)(((x - lo) / scale) * (double)nb);
        g = g < 0 ? 0 : (g > nb - 1 ? nb - 1 : g);
        while (g > 0 && x < at(g)) --g;
        while (g < nb - 1 && x >= at(g + 1)) ++g;
        return g;
    }
};

// where a sample goes: a bin, or one of the three counts beside the table
constexpr int kBelow = -1, kAbove = -2, kNonfinite = -3, kNone = -4;
__device__ __forceinline__ int place(const Edges &e, double x)
{
    if (!finite(x)) return kNonfinite;
    if (x < e.lo) return kBelow;
    if (x > e.hi) return kAbove;
    if (!(x >= e.lo)) return kNone;                       // (a NaN range: an absent or empty column bins nothing)
    return e.bin(x);
}

// One count into an LDS table, wave-aggregated: a wave whose lanes all count into one word adds its 64 at once
// instead of queueing 64 atomics on it.  Every lane of the wave calls this on every trip (idx < 0: nothing to count).
__device__ __forceinline__ void count(unsigned int *h, int idx)
{
    const int first = __builtin_amdgcn_readfirstlane(idx);
    if (__all(idx == first)) {
        if (first >= 0 && (threadIdx.x & 63) == 0) atomicAdd(&h[first], 64u);
    } else if (idx >= 0) {
        atomicAdd(&h[idx], 1u);
    }
}

__global__ __launch_bounds__(kThreads) void k_marg_extent(const MargArgs a)
{
    __shared__ double smn[kThreads / 64], smx[kThreads / 64];
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const int src = cid / a.ncol, slot = a.col[cid - src * a.ncol];
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    double mn = INFINITY, mx = -INFINITY;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        const double v = sample(a, src, slot, j);
        if (finite(v)) { mn = fmin(mn, v); mx = fmax(mx, v); }
    }
    // (min and max are exact: any order gives the same bits)
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, w, 64));
        mx = fmax(mx, __shfl_xor(mx, w, 64));
    }
    if ((t & 63) == 0) { smn[t >> 6] = mn; smx[t >> 6] = mx; }
    __syncthreads();
    if (t == 0) {
        double *p = a.extent + ((size_t)cid * a.splits + split) * 2;
        p[0] = fmin(fmin(smn[0], smn[1]), fmin(smn[2], smn[3]));
        p[1] = fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3]));
    }
}

// one workgroup per (source, column slot): the slot's range, the edges of both tables
__global__ __launch_bounds__(kThreads) void k_marg_edges(const MargArgs a)
{
    __shared__ Range s_r;
    const int i = blockIdx.x, t = threadIdx.x;
    const int src = i / kCols, slot = i - src * kCols;
    if (t == 0) {
        const double qnan = __builtin_nan("");
        Range r = {qnan, qnan};
        int ci = -1;
        for (int k = 0; k < a.ncol; ++k) if (a.col[k] == slot) ci = k;
        if (ci >= 0) {
            const double *p = a.extent + ((size_t)src * a.ncol + ci) * a.splits * 2;
            double mn = INFINITY, mx = -INFINITY;
            for (int s = 0; s < a.splits; ++s) { mn = fmin(mn, p[2 * s]); mx = fmax(mx, p[2 * s + 1]); }
            if (mn <= mx) {                               // a finite sample exists
                if (a.has_range[slot]) { r.lo = a.lo[slot]; r.hi = a.hi[slot]; }
                else if (mn == mx) { r.lo = mn - 0.5; r.hi = mx + 0.5; }
                else { r.lo = mn; r.hi = mx; }
            }
        }
        s_r = r;
        a.range[i] = r;
    }
    __syncthreads();
    const Edges e1(s_r, a.nbins);
    for (int k = t; k <= a.nbins; k += kThreads) a.o_edges1[(size_t)i * (a.nbins + 1) + k] = e1.at(k);
    if (a.nbins2 > 0) {
        const Edges e2(s_r, a.nbins2);
        for (int k = t; k <= a.nbins2; k += kThreads) a.o_edges2[(size_t)i * (a.nbins2 + 1) + k] = e2.at(k);
    }
}

__global__ __launch_bounds__(kThreads) void k_marg_hist1(const MargArgs a)
{
    __shared__ unsigned int h[kMaxBins + kTail];
    const int cid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const int src = cid / a.ncol, slot = a.col[cid - src * a.ncol];
    const int nb = a.nbins, len = nb + kTail;
    for (int i = t; i < len; i += kThreads) h[i] = 0u;
    __syncthreads();
    const Edges e(a.range[src * kCols + slot], nb);
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    // (every lane makes every trip, so that count()'s vote sees whole waves)
    for (long long base = j0; base < j1; base += kThreads) {
        const long long j = base + t;
        int idx = -1;
        if (j < j1) {
            const int p = place(e, sample(a, src, slot, j));
            idx = p >= 0 ? p : (p == kNone ? -1 : nb + (-1 - p));      // below, above, non-finite: the words behind the table
        }
        count(h, idx);
    }
    __syncthreads();
    unsigned int *out = a.part1 + ((size_t)cid * a.splits + split) * len;
    for (int i = t; i < len; i += kThreads) out[i] = h[i];
}

__global__ __launch_bounds__(kThreads) void k_marg_hist2(const MargArgs a)
{
    __shared__ unsigned int h[kMaxBins2 * kMaxBins2];
    const int pid = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const int src = pid / a.npairs, pr = pid - src * a.npairs;
    const int sa = a.pair[pr][0], sb = a.pair[pr][1];
    const int nb = a.nbins2, len = nb * nb;
    for (int i = t; i < len; i += kThreads) h[i] = 0u;
    __syncthreads();
    const Edges ea(a.range[src * kCols + sa], nb), eb(a.range[src * kCols + sb], nb);
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    for (long long base = j0; base < j1; base += kThreads) {
        const long long j = base + t;
        int idx = -1;
        if (j < j1) {
            const int pa = place(ea, sample(a, src, sa, j)), pb = place(eb, sample(a, src, sb, j));
            if (pa >= 0 && pb >= 0) idx = pa * nb + pb;
        }
        count(h, idx);
    }
    __syncthreads();
    unsigned int *out = a.part2 + ((size_t)pid * a.splits + split) * len;
    for (int i = t; i < len; i += kThreads) out[i] = h[i];
}

// grid nsrc * 8 + nsrc * npairs: a (source, slot)'s 1-D table, counts and status, or a (source, pair)'s 2-D table
__global__ __launch_bounds__(kThreads) void k_marg_merge(const MargArgs a)
{
    const int t = threadIdx.x;
    const int n1 = a.nsrc * kCols;
    if ((int)blockIdx.x >= n1) {
        const size_t pid = blockIdx.x - n1, len = (size_t)a.nbins2 * a.nbins2;
        const unsigned int *p = a.part2 + pid * a.splits * len;
        for (size_t i = t; i < len; i += kThreads) {
            unsigned int c = 0;
            for (int s = 0; s < a.splits; ++s) c += p[(size_t)s * len + i];
            a.o_counts2[pid * len + i] = c;
        }
        return;
    }
    __shared__ unsigned long long s_used[kThreads / 64];
    const int i = blockIdx.x, src = i / kCols, slot = i - src * kCols;
    const int nb = a.nbins, len = nb + kTail;
    int ci = -1;
    for (int k = 0; k < a.ncol; ++k) if (a.col[k] == slot) ci = k;
    unsigned int *o = a.o_counts1 + (size_t)i * nb;
    if (ci < 0) {
        for (int k = t; k < nb; k += kThreads) o[k] = 0u;
        if (t == 0) {
            a.o_used[i] = a.o_below[i] = a.o_above[i] = a.o_nonfinite[i] = 0;
            a.o_status[i] = kStAbsent;
        }
        return;
    }
    const unsigned int *p = a.part1 + ((size_t)src * a.ncol + ci) * a.splits * len;
    unsigned long long used = 0;
    for (int k = t; k < nb; k += kThreads) {
        unsigned int c = 0;
        for (int s = 0; s < a.splits; ++s) c += p[(size_t)s * len + k];
        o[k] = c;
        used += c;
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) used += __shfl_xor(used, w, 64);
    if ((t & 63) == 0) s_used[t >> 6] = used;
    __syncthreads();
    if (t == 0) {
        long long tail[3] = {0, 0, 0};
        for (int s = 0; s < a.splits; ++s)
            for (int k = 0; k < 3; ++k) tail[k] += p[(size_t)s * len + nb + k];
        const Range r = a.range[i];
        a.o_used[i] = (long long)(s_used[0] + s_used[1] + s_used[2] + s_used[3]);
        a.o_below[i] = tail[0]; a.o_above[i] = tail[1]; a.o_nonfinite[i] = tail[2];
        a.o_status[i] = a.colstatus[i] | (r.lo != r.lo ? kStEmpty : 0) | (tail[2] > 0 ? kStNonfinite : 0);
    }
}

}   // namespace mbbm
