// mbb_predict.hip.h -- predicted fluxes of a device-resident chain (gfx950, fp64, wave64).
//
// What mbb_results.predflux_cen makes of a chain on the host (results.py:895-985: the model flux of every chain entry at a
// wavelength or through a passband, then _parcen_internal's mean and percentiles), computed where the chain is.  A
// prediction target ("spec") is a list of quadrature samples (nu [GHz], weight): a passband's response.quadrature(), or
// the one sample (um_to_GHz / lambda, 1) of a wavelength.
//
// Columns are made a few at a time: a group of at most kGroup specs is filled into the derived-column block of the
// summary ([nsrc][nw][nsteps] doubles each), a chunk of chain rows at a time, and summarised by the summary's own
// kernels (k_sum_stats, k_sum_begin, k_sum_hist, k_sum_pick of mbb_summary.hip.h, driven unchanged with the group's
// columns in slots 5, 6, 7); k_pred_finish writes the group's results.  Nothing about a column depends on the columns
// beside it: a spec's results are the same bits whatever else the call asks for.
//
// Kernels:
//   k_pred_lnnu    m_log of every sample frequency, once per call
//   k_pred_fill    a chunk's rows x the group's specs: f_nu or the band sum of every (row, spec), into the columns
//   k_pred_finish  one thread per (source, spec of the group): interpolates the percentiles, writes every output
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_device.hip.h"
#include "mbb_summary.hip.h"

namespace mbbp {

constexpr int kGroup = 3;             // specs filled and summarised together: the columns of the derived-column block
constexpr int kMaxSpecs = 128;        // specs per call (MBB_PRED_MAX_SPECS)
constexpr int kMaxSamples = 32768;    // quadrature samples per call, all specs together (MBB_PRED_MAX_SAMPLES)
constexpr int kLdsSamples = 2560;     // a group's many-sample lists are staged in LDS up to this many samples: 24 bytes
                                      // each, dynamic LDS of just the group's size, 60 KB at the most
constexpr int kThreads = 256;         // four waves; a workgroup takes kThreads rows, a wave 64 of them

struct FillArgs {
    const WalkerK *wk;                // the chunk's records (k_prologue)
    const int32_t *status;            // ... and row status
    int n;                            // rows of the chunk
    long long off;                    // the chunk's first row in the flat chain [nsrc * nw * nsteps]
    const double *nu, *lnnu, *wt;     // every sample of the call
    int ng;                           // specs of the group, 1 .. kGroup
    int s0[kGroup], s1[kGroup];       // a spec's samples: s0 <= i < s1
    int single[kGroup];               // one sample of weight 1: the value is f_nu itself
    int l0[kGroup];                   // where a many-sample spec's list starts in LDS (STAGE)
    int nstaged;                      // samples in LDS: three arrays of that many doubles
    double *col[kGroup];              // the spec's column [nsrc][nw][nsteps]
    int *pstatus;                     // [nsrc][nspec] row-status bits
    int nspec, spec0;                 // specs of the call; the group's first
    int nw, nsteps, burn, thin;
};

__global__ void k_pred_lnnu(const double *nu, int n, double *lnnu)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lnnu[i] = m_log(nu[i]);
}

// mbbs::note_status for a (source, spec) table: a failing row counts when its step is inside the window
__device__ __forceinline__ void note_row(const FillArgs &a, int g, long long row, int st)
{
    const long long per = (long long)a.nw * a.nsteps;
    const int src = (int)(row / per), step = (int)(row % a.nsteps);
    if (step >= a.burn && (step - a.burn) % a.thin == 0)
        atomicOr(&a.pstatus[(size_t)src * a.nspec + a.spec0 + g], 1 << (mbbs::kStRowShift + (st & 7)));
}

// Rows blockIdx.x * kThreads ... of the chunk.  A many-sample spec takes a wave per row: lane l accumulates samples
// l, l + 64, ... in that order and the 64 partial sums go through wave_sum's fixed tree; the wave walks its 64 rows and
// lane r keeps row r's total.  A single-sample spec takes a lane per row.  Then every lane stores its row's values:
// consecutive lanes, consecutive doubles of a column.
template <bool OPTHIN, bool NOALPHA, bool STAGE>
__global__ __launch_bounds__(kThreads) void k_pred_fill(const FillArgs a)
{
    extern __shared__ double sh_pred[];                            // (STAGE: nu, log nu, weight of the staged samples)
    double *const sh_nu = sh_pred, *const sh_ln = sh_pred + a.nstaged, *const sh_wt = sh_pred + 2 * a.nstaged;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int base = blockIdx.x * kThreads + wave * 64;            // the wave's first row (wave-uniform)
    if (STAGE) {
#pragma unroll
        for (int g = 0; g < kGroup; ++g)
            if (g < a.ng && !a.single[g])
                for (int i = a.s0[g] + (int)threadIdx.x; i < a.s1[g]; i += kThreads) {
                    const int l = a.l0[g] + i - a.s0[g];
                    sh_nu[l] = a.nu[i]; sh_ln[l] = a.lnnu[i]; sh_wt[l] = a.wt[i];
                }
        __syncthreads();
    }
    const double qnan = __builtin_nan("");
    double res[kGroup] = {qnan, qnan, qnan};
    const int rows = min(64, a.n - base);                          // (<= 0: a wave beyond the chunk's end)
    bool many = false;
#pragma unroll
    for (int g = 0; g < kGroup; ++g) many = many || (g < a.ng && !a.single[g]);
    if (many) {
        for (int r = 0; r < rows; ++r) {
            const WalkerK k = a.wk[base + r];                      // wave-uniform
            if (k.status != ROW_OK) continue;
#pragma unroll
            for (int g = 0; g < kGroup; ++g) {
                if (g >= a.ng || a.single[g]) continue;
                double acc = 0.0;
                const int cnt = a.s1[g] - a.s0[g];
                if (STAGE) {
                    const int l0 = a.l0[g];
                    for (int i = lane; i < cnt; i += 64)
                        acc = fma(fnu_sample<OPTHIN, NOALPHA>(k, sh_nu[l0 + i], sh_ln[l0 + i]), sh_wt[l0 + i], acc);
                } else {
                    const int s0 = a.s0[g];
                    for (int i = lane; i < cnt; i += 64)
                        acc = fma(fnu_sample<OPTHIN, NOALPHA>(k, a.nu[s0 + i], a.lnnu[s0 + i]), a.wt[s0 + i], acc);
                }
                const double total = wave_sum(acc);
                if (lane == r) res[g] = total;
            }
        }
    }
    if (lane >= rows) return;
    const int row = base + lane;
    const int st = a.status[row];
    bool one = false;
#pragma unroll
    for (int g = 0; g < kGroup; ++g) one = one || (g < a.ng && a.single[g]);
    if (one && st == ROW_OK) {
        const WalkerK k = a.wk[row];
#pragma unroll
        for (int g = 0; g < kGroup; ++g)
            if (g < a.ng && a.single[g]) res[g] = fnu_sample<OPTHIN, NOALPHA>(k, a.nu[a.s0[g]], a.lnnu[a.s0[g]]);
    }
#pragma unroll
    for (int g = 0; g < kGroup; ++g)
        if (g < a.ng) {
            a.col[g][a.off + row] = res[g];
            if (st != ROW_OK) note_row(a, g, a.off + row, st);
        }
}

struct FinishArgs {
    int spec0, nspec;                 // the group's first spec; specs of the call
    const int *pstatus;               // [nsrc][nspec]
    long long *o_nused;               // results [nsrc][nspec] ...
    double *o_mean, *o_min, *o_max, *o_pct;   // o_pct [nsrc][nspec][npct]
    int *o_status;
};

// one thread per (source, column of the group): what k_sum_finish writes of a column, into the call's [nsrc][nspec] tables
__global__ __launch_bounds__(64) void k_pred_finish(const mbbs::SumArgs a, const FinishArgs f)
{
    const int cid = blockIdx.x * 64 + threadIdx.x;
    if (cid >= a.nsrc * a.ncol) return;
    const int src = cid / a.ncol, g = cid - src * a.ncol;
    const size_t i = (size_t)src * f.nspec + f.spec0 + g;
    const mbbs::ColState &st = a.state[cid];
    const double qnan = __builtin_nan("");
    f.o_nused[i] = st.n_used; f.o_mean[i] = st.mean; f.o_min[i] = st.vmin; f.o_max[i] = st.vmax;
    f.o_status[i] = f.pstatus[i] | (st.n_used == 0 ? mbbs::kStEmpty : 0) | (st.nan ? mbbs::kStNaN : 0);
    for (int k = 0; k < a.npct; ++k) {
        double r = qnan;
        if (st.nranks) {
            // numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) from t = 0.5 on
            const double lo = mbbs::from_key(st.prefix[2 * k]), hi = mbbs::from_key(st.prefix[2 * k + 1]), t = st.gamma[k];
            const double diff = hi - lo;
            r = lo + diff * t;
            if (t >= 0.5) r = hi - diff * (1.0 - t);
        }
        f.o_pct[i * a.npct + k] = r;
    }
}

}   // namespace mbbp
