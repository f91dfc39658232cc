// mbb_chain_view.hip.h -- the columns of a device-resident chain as its summary and its marginals read them.
//
// The chain is in emcee's layout, chain [nsrc][nw][nsteps][5] (k_chain_reorder's output); the derived columns (slots
// 5, 6, 7) are [nsrc][nw][nsteps] each.  A column's samples are the steps burn, burn + thin, ... of every walker, in
// [nw][nkept] order (numpy's flatten()).  SumArgs, MargArgs and DrawArgs begin with this view; sample_cell() is the one
// mapping from a sample's number j to its walker and step, sample() from (source, slot, j) to a value.
#pragma once
#include <hip/hip_runtime.h>

namespace mbbc {

constexpr int kCols = 8;         // column slots: T, beta, lambda0, alpha, fnorm, peak wavelength, L_IR, dust mass
constexpr int kMaxSplits = 64;   // a column is cut into at most this many splits

struct ChainView {
    const double *chain;
    const double *der[3];                   // the derived columns (slots 5, 6, 7) or null
    int nsrc, nw, nsteps, burn, thin, nkept;
    long long n;                            // samples per column: nw * nkept
    int ncol, col[kCols];                   // the active column slots
    int splits;                             // a column is cut into this many runs of per_split samples
    long long per_split;
};

// sample j of a source: its walker w and its step
__device__ __forceinline__ void sample_cell(const ChainView &a, long long j, long long &w, long long &step)
{
    w = j / a.nkept;
    step = a.burn + (j - w * a.nkept) * a.thin;
}

// ... and the flat index of that cell in [nsrc][nw][nsteps]
__device__ __forceinline__ long long sample_flat(const ChainView &a, int src, long long j)
{
    long long w, step;
    sample_cell(a, j, w, step);
    return ((long long)src * a.nw + w) * a.nsteps + step;
}

// sample j of (source, column slot): its value
__device__ __forceinline__ double sample(const ChainView &a, int src, int slot, long long j)
{
    const long long flat = sample_flat(a, src, j);
    return slot < 5 ? a.chain[flat * 5 + slot] : a.der[slot - 5][flat];
}

}  // namespace mbbc
