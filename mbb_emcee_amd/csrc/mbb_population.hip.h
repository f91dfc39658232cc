// mbb_population.hip.h -- the population of a catalogue: the hyper-likelihood of a chain's sources under Gaussian
// population candidates (include/mbb_hip.h: "the population of a catalogue"; the step logic is mbb_popsteps.hip.h).
//
//   k_pop_build    a thread per (source, entry), a workgroup within one source: the chain row of the window (mbb_chain_view.hip.h's order) becomes
//                  x[d] of the compact block [nsrc][n][d] and b of [nsrc][n] (-inf: left out); the used entries are
//                  counted per source (a block fold, one integer atomic per workgroup).
//   k_pop_status   a thread per source: n_left_out and the status bits from the count.
//   k_pop_eval     a workgroup of 256 per (source, split of its entries, tile of candidates).  Thread t < tile prepares
//                  candidate t of the tile into LDS (pop_prepare: the same text whatever the candidate's place); every
//                  lane then walks its entries of the split, j = first + lane, + 256, ..., loads x_j and b_j ONCE and
//                  folds a_j of every candidate of the tile into that candidate's record, which lives in registers.  The
//                  candidate's constants are read from LDS at a wave-uniform address (a broadcast).  The 64 records of a
//                  wave are folded by cross-lane moves in the fixed tree 32, 16, 8, 4, 2, 1, the four waves' through LDS
//                  in wave order by thread t, which writes the split's record.
//   k_pop_merge    a thread per (candidate, source): the splits' records in split order, then lnl_src, ess, mean, cov.
//   k_pop_total    a wave per candidate: 64 lnl_src at a time into LDS, lane 0 adds them in source order: lnl, n_src_used,
//                  cand_status.
//
// Which lane and which split an entry belongs to depends on n alone, a candidate's constants on the candidate alone, a
// tile's unused slots evaluate the call's last candidate and are not written: the arithmetic of a (candidate, source)
// does not depend on what shares the call, nor on the candidate's place in it.
//
// Registers.  A record is 3 doubles, with moments 3 + d + d (d + 1) / 2 (23 at d = 5), and the candidates of a tile are
// independent chains that the compiler interleaves, each with the temporaries of its exponential.  kTile = 8 candidates
// without moments, kTileMom = 4 with (kTileMomWide = 2 from d = 4 on) keep every instantiation free of spills; 16 / 4 / 4
// spilled from d = 2 on (up to 364 VGPRs at d = 5).  A larger tile would only save reads of a block that streams far
// below the HBM rate: the evaluation is bound by the exponential, one per entry and candidate.
#pragma once
#include <hip/hip_runtime.h>
#include "mbb_chain_view.hip.h"
#include "mbb_popsteps.hip.h"

namespace mbbpop {

using namespace mbbpops;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTile = 8, kTileMom = 4, kTileMomWide = 2;       // candidates per tile: plain, with moments, with moments at d >= 4
constexpr int pop_tile(int d, bool mom) { return mom ? (d >= 4 ? kTileMomWide : kTileMom) : kTile; }
constexpr int kSplitEntries = 8192;       // a source's entries are cut into ceil(n / 8192) splits, at most kMaxSplits
constexpr int kMaxSplits = 64;
constexpr int kChunk = 64;                // candidates per launch of k_pop_eval (a multiple of both tiles)
constexpr int kMaxCand = 1024;

// status bits: per source (beside the summary's EMPTY = 1 and HAS_NAN = 2) and per candidate
constexpr int kStEmpty = 1, kStHasNan = 2;
constexpr int kCandBad = 1, kCandUnderflow = 2, kCandHasEmpty = 4;

struct PopBuildArgs : mbbc::ChainView {
    int d, pcol[kMaxD], transform[kMaxD];
    PopPrior prior;
    double *x, *b;                        // the compact block
    unsigned long long *count;            // [nsrc] used entries
    unsigned int blocks_per_src;          // the grid is [nsrc][blocks_per_src] workgroups, flat
    long long *o_nused, *o_nleft;
    int *o_status;
};

struct PopEvalArgs {
    const double *x, *b;
    const unsigned long long *count;
    const double *hyper;                  // [H][d + d (d + 1) / 2]
    int nsrc, d, H, h0, hn;               // the candidates h0 .. h0 + hn - 1 of this launch
    long long n, per_split;
    int splits, moments;
    double *part;                         // [hn][nsrc][splits][words]
    double *lnl_src, *ess;                // [H][nsrc]
    double *mean, *cov;                   // [H][nsrc][d], [H][nsrc][d][d], or null
    double *o_lnl;                        // [H]
    int *o_nsrc_used, *o_cand_status;     // [H]
};

__global__ __launch_bounds__(kThreads) void k_pop_build(PopBuildArgs a)
{
    __shared__ unsigned int s_used[kWaves];
    const int src = (int)(blockIdx.x / a.blocks_per_src);
    const long long j = (long long)(blockIdx.x - (unsigned)src * a.blocks_per_src) * kThreads + threadIdx.x;
    bool used = false;
    if (j < a.n) {
        const long long flat = mbbc::sample_flat(a, src, j);
        double th[5], x[kMaxD];
        for (int k = 0; k < 5; ++k) th[k] = a.chain[flat * 5 + k];
        const double b = pop_entry(th, a.d, a.pcol, a.transform, a.prior, x);
        const long long at = (long long)src * a.n + j;
        for (int i = 0; i < a.d; ++i) a.x[at * a.d + i] = x[i];
        a.b[at] = b;
        used = b > -INFINITY;
    }
    const unsigned long long ball = __ballot(used);
    if ((threadIdx.x & 63) == 0) s_used[threadIdx.x >> 6] = (unsigned int)__popcll(ball);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int t = 0;
        for (int w = 0; w < kWaves; ++w) t += s_used[w];
        if (t) atomicAdd(&a.count[src], (unsigned long long)t);
    }
}

__global__ void k_pop_status(PopBuildArgs a)
{
    const int src = blockIdx.x * blockDim.x + threadIdx.x;
    if (src >= a.nsrc) return;
    const long long used = (long long)a.count[src];
    a.o_nused[src] = used;
    a.o_nleft[src] = a.n - used;
    a.o_status[src] = (used == 0 ? kStEmpty : 0) | (used < a.n ? kStHasNan : 0);
}

template <int D, bool MOM> __device__ __forceinline__ void pop_shift_merge(PopRec<D, MOM> &r, int off)
{
    PopRec<D, MOM> o;
    o.m = __shfl_down(r.m, off); o.s = __shfl_down(r.s, off); o.s2 = __shfl_down(r.s2, off);
    for (int i = 0; i < r.kMean; ++i) o.mean[i] = __shfl_down(r.mean[i], off);
    for (int i = 0; i < r.kM2; ++i) o.M2[i] = __shfl_down(r.M2[i], off);
    pop_merge(r, o);
}

template <int D, bool MOM> __global__ __launch_bounds__(kThreads) void k_pop_eval(PopEvalArgs a)
{
    constexpr int TILE = pop_tile(D, MOM);
    constexpr int W = PopRec<D, MOM>::kWords;
    constexpr int P = pop_prep_len(D);
    __shared__ double s_prep[TILE][P];
    __shared__ int s_good[TILE];
    __shared__ double s_rec[kWaves][TILE][W];
    const int src = blockIdx.x, split = blockIdx.y, tile0 = blockIdx.z * TILE;      // (tile0 counts within the launch)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < TILE) {
        // a slot beyond the launch's candidates evaluates the call's last one and is not written
        const int h = min(a.h0 + tile0 + tid, a.H - 1);
        double prep[P];
        for (int i = 0; i < P; ++i) prep[i] = 0.0;
        const bool good = pop_prepare(a.hyper + (size_t)h * pop_hyper_len(D), D, prep);
        for (int i = 0; i < P; ++i) s_prep[tid][i] = prep[i];
        s_good[tid] = good;
    }
    __syncthreads();
    PopRec<D, MOM> rec[TILE];
#pragma unroll
    for (int t = 0; t < TILE; ++t) pop_clear(rec[t]);
    const long long first = (long long)split * a.per_split;
    const long long last = min(first + a.per_split, a.n);
    const double *const xs = a.x + (size_t)src * a.n * D;
    const double *const bs = a.b + (size_t)src * a.n;
    for (long long j = first + tid; j < last; j += kThreads) {
        // (the tile's constants are read from LDS anew for every entry: hoisted out of the loop they would take
        // TILE x (2 d + d (d - 1) / 2 + 1) doubles of registers and spill)
        asm volatile("" ::: "memory");
        const double b = bs[j];
        if (!(b > -INFINITY)) continue;           // left out
        double x[D];
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = xs[j * D + i];
#pragma unroll
        for (int t = 0; t < TILE; ++t) pop_add(rec[t], pop_logdens<D>(s_prep[t], x, b), x);
    }
#pragma unroll
    for (int t = 0; t < TILE; ++t) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) pop_shift_merge(rec[t], off);
        if (lane == 0) pop_store(rec[t], s_rec[wave][t]);
    }
    __syncthreads();
    if (tid < TILE && tile0 + tid < a.hn) {
        PopRec<D, MOM> r, o;
        pop_load(r, s_rec[0][tid]);
        for (int w = 1; w < kWaves; ++w) { pop_load(o, s_rec[w][tid]); pop_merge(r, o); }
        if (!s_good[tid]) { pop_clear(r); r.m = NAN; }          // a bad candidate: its record says so
        pop_store(r, a.part + (((size_t)(tile0 + tid) * a.nsrc + src) * a.splits + split) * W);
    }
}

template <int D, bool MOM> __global__ void k_pop_merge(PopEvalArgs a)
{
    constexpr int W = PopRec<D, MOM>::kWords;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)a.hn * a.nsrc) return;
    const int hl = (int)(i / a.nsrc), src = (int)(i - (long long)hl * a.nsrc);
    const double *const p = a.part + ((size_t)hl * a.nsrc + src) * a.splits * W;
    PopRec<D, MOM> r, o;
    pop_load(r, p);
    const bool bad = r.m != r.m;
    if (!bad)
        for (int s = 1; s < a.splits; ++s) { pop_load(o, p + (size_t)s * W); pop_merge(r, o); }
    const size_t at = (size_t)(a.h0 + hl) * a.nsrc + src;
    const long long used = (long long)a.count[src];
    double lnl = NAN, ess = NAN;
    bool moments = false;
    if (!bad && used > 0) {
        if (r.s == 0.0 || r.m < kUnderflow) lnl = -INFINITY;     // every e^a_j is below the smallest float64
        else {
            lnl = r.m + mbbm::m_log(r.s) - mbbm::m_log((double)used);
            ess = r.s * r.s / r.s2;
            moments = true;
        }
    }
    a.lnl_src[at] = lnl;
    a.ess[at] = ess;
    if (MOM) {
        int o2 = 0;
        for (int k = 0; k < D; ++k) {
            a.mean[at * D + k] = moments ? r.mean[k] : NAN;
            for (int l = 0; l <= k; ++l, ++o2) {
                const double c = moments ? r.M2[MOM ? o2 : 0] / r.s : NAN;
                a.cov[(at * D + k) * D + l] = c;
                a.cov[(at * D + l) * D + k] = c;
            }
        }
    }
}

__global__ __launch_bounds__(64) void k_pop_total(PopEvalArgs a)
{
    __shared__ double s_l[64];
    __shared__ int s_empty[64];
    const int h = blockIdx.x, lane = threadIdx.x;
    const double *const l = a.lnl_src + (size_t)h * a.nsrc;
    double total = 0.0;
    int used = 0, status = 0;
    // 64 sources at a time into LDS, then lane 0 adds them in source order
    for (int s0 = 0; s0 < a.nsrc; s0 += 64) {
        const int src = s0 + lane;
        if (src < a.nsrc) { s_l[lane] = l[src]; s_empty[lane] = a.count[src] == 0ull; }
        __syncthreads();
        if (lane == 0) {
            const int m = min(64, a.nsrc - s0);
            for (int k = 0; k < m; ++k) {
                if (s_empty[k]) { status |= kCandHasEmpty; continue; }
                const double v = s_l[k];
                if (v == -INFINITY) status |= kCandUnderflow;
                total += v;
                ++used;
            }
        }
        __syncthreads();
    }
    if (lane != 0) return;
    // a bad candidate is told from its hyper-parameters, as pop_prepare tells it
    bool bad = false;
    const double *const hy = a.hyper + (size_t)h * pop_hyper_len(a.d);
    for (int i = 0; i < pop_hyper_len(a.d); ++i) if (!mbbps::ps_finite(hy[i])) bad = true;
    for (int i = 0; i < a.d; ++i) if (!(hy[a.d + pop_tri(i) + i] > 0.0)) bad = true;
    if (bad) { total = NAN; status = kCandBad; used = 0; }
    else if (used == 0) total = NAN;
    a.o_lnl[h] = total;
    a.o_nsrc_used[h] = used;
    a.o_cand_status[h] = status;
}

}  // namespace mbbpop
