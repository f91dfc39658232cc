// mbb_draws.hip.h -- posterior draws of a device-resident chain (gfx950).
//
// What the reference's mbb_results.choice() does on the host (results.py:803-893: nsamples cells of the chain, uniform
// over walkers x steps with replacement, with their peak wavelength, L_IR and dust mass), done where the chain is: per
// source n cells of the burn / thin window are picked and their rows, lnprob and (walker, step) gathered into a
// compact block [nsrc][n]; the derived columns are then filled for that block alone by the summary's own kernels
// (summary_fill_derived over the block seen as a chain of nsrc x 1 x n).
//
// A source's population is the N = nw * nkept kept cells of the window in mbb_chain_view.hip.h's order (sample j ->
// walker j / nkept, step burn + (j % nkept) thin).  Draw i of source src picks
//   random   j = (u N) >> 64 with u the first 64 bits of Philox4x32-10 at counter (i, src, "DRAW", 1), key = seed:
//            uniform with replacement, no rejection loop (the bias of the multiply-shift is below N / 2^64).  The
//            stretch move's draws of the same seed have counters (row, half, 0, 0): the streams never meet.
//   even     j = floor(i N / n): spread over the window, no repeats while n <= N
// Kernels (256 threads, one thread per (source, draw)):
//   k_draw_gather   rows [nsrc][n][5], lnprob [nsrc][n] (NaN without one), index [nsrc][n][2] -- copies, never recomputed
//   k_draw_index    index alone: the picks without a chain
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_chain_view.hip.h"
#include "mbb_stretch.hip.h"   // philox4x32

namespace mbbw {

constexpr int kThreads = 256;
constexpr int kMaxDraws = 1 << 24;            // draws per source and call
constexpr int kRandom = 0, kEven = 1;         // include/mbb_hip.h: mbb_draws_how
constexpr unsigned int kStreamWord = 0x44524157u;   // "DRAW": the third counter word of every draw

struct DrawArgs : mbbc::ChainView {
    const double *lnprob;                   // [nsrc][nw][nsteps] or null
    int ndraw, how;
    unsigned long long seed;
    // results
    double *o_rows;                         // [nsrc][ndraw][5] or null (k_draw_index)
    double *o_lnprob;                       // [nsrc][ndraw] or null
    int *o_index;                           // [nsrc][ndraw][2] walker, step
};

// the high 64 bits of a * b, from four 32 x 32 -> 64 products: no 128-bit type, nothing signed
__device__ __forceinline__ unsigned long long mulhi64(unsigned long long a, unsigned long long b)
{
    const unsigned long long a0 = (unsigned int)a, a1 = a >> 32, b0 = (unsigned int)b, b1 = b >> 32;
    const unsigned long long p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const unsigned long long mid = (p00 >> 32) + (unsigned int)p01 + (unsigned int)p10;       // < 3 * 2^32
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// The pick: which of a source's N window samples draw i of n is.  N >= 1, i < n <= kMaxDraws, N < 2^32.
__device__ __forceinline__ long long pick(int how, unsigned long long seed, int src, int i, int n, long long N)
{
    if (how == kEven) return (long long)((unsigned long long)i * (unsigned long long)N / (unsigned long long)n);
    unsigned int c4[4] = {(unsigned int)i, (unsigned int)src, kStreamWord, 1u};
    philox4x32(c4, (unsigned int)seed, (unsigned int)(seed >> 32));
    const unsigned long long u = (unsigned long long)c4[0] | ((unsigned long long)c4[1] << 32);
    return (long long)mulhi64(u, (unsigned long long)N);
}

// (source, draw) of a thread, or false beyond the last
__device__ __forceinline__ bool draw_of_thread(const DrawArgs &a, int &src, int &i)
{
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)a.nsrc * a.ndraw) return false;
    src = (int)(t / a.ndraw);
    i = (int)(t - (long long)src * a.ndraw);
    return true;
}

__device__ __forceinline__ void write_index(const DrawArgs &a, int src, int i, long long j)
{
    long long w, step;
    mbbc::sample_cell(a, j, w, step);
    int *const o = a.o_index + ((size_t)src * a.ndraw + i) * 2;
    o[0] = (int)w;
    o[1] = (int)step;
}

__global__ __launch_bounds__(kThreads) void k_draw_gather(const DrawArgs a)
{
    int src, i;
    if (!draw_of_thread(a, src, i)) return;
    const long long j = pick(a.how, a.seed, src, i, a.ndraw, a.n);
    const long long flat = mbbc::sample_flat(a, src, j);
    const size_t o = (size_t)src * a.ndraw + i;
    for (int k = 0; k < 5; ++k) a.o_rows[o * 5 + k] = a.chain[flat * 5 + k];
    a.o_lnprob[o] = a.lnprob ? a.lnprob[flat] : __builtin_nan("");
    write_index(a, src, i, j);
}

__global__ __launch_bounds__(kThreads) void k_draw_index(const DrawArgs a)
{
    int src, i;
    if (!draw_of_thread(a, src, i)) return;
    write_index(a, src, i, pick(a.how, a.seed, src, i, a.ndraw, a.n));
}

}  // namespace mbbw
