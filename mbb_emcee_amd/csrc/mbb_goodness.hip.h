// mbb_goodness.hip.h -- goodness of fit of a device-resident chain (gfx950, fp64, wave64).
//
// Per chain entry theta the data term of the likelihood and its tail probability:
//   chisq(theta) = sum_b (f_b - m_b(theta))^2 ivar_b,  or  r^T C^-1 r  with r = f - m  when the data has a covariance;
//   q(theta)     = Q(nb/2, chisq/2)   (mbb_gammq.hip.h),
// m_b the model flux through band b of the context (the samples mbb_set_bands was given, the context's model), f, ivar
// and C^-1 the context's data.  Neither knows limits or priors: a row below a lower limit has a chisq like any other;
// a row the SED constructor fails on gives NaN.  The two columns go into slots 0 and 1 of the summary's derived-column
// block and through the summary's own statistics kernels (mbb_summary.hip.h, driven as for the predicted fluxes); the
// kernels here fill them, find the entry of smallest chisq and of largest lnprob, and write the results.
//
// Kernels:
//   k_good_lnnu    m_log of every band sample, once per call
//   k_good_flux    n rows x the context's bands: the band fluxes, band-major [nb][n] -- a wave per row for a band of
//                  many samples (lane-strided fma, wave_sum's fixed tree), a lane per row for a band of one sample
//   k_good_chi     a lane per row: chisq (bands in order; the quadratic form row by row of C^-1), q, status notes, stores
//   k_good_mean    per source: theta-bar, the window's means of the five parameters, as a parameter row
//   k_good_best    per (source, split): the window's entry of smallest chisq and of largest lnprob
//   k_good_pick    per source: merges the splits, writes those entries' parameters, indices and values
//   k_good_finish  per (source, column): n_used, mean, min, max, percentiles, status
// A row's band fluxes, chisq and q are functions of the row and of its source's data alone: the same bits whatever
// chunk the row is in, however many sources the call has, wherever the chain came from.  Every sum has a fixed order.
// No kernel holds an array in registers: none uses scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_device.hip.h"
#include "mbb_summary.hip.h"
#include "mbb_gammq.hip.h"

namespace mbbq {

constexpr int kMaxBands = mbbm::kGammqMaxNb;   // bands of a goodness call
constexpr int kLdsSamples = 2560;     // the bands' samples are staged in LDS up to this many: 24 bytes each, 60 KB
constexpr int kLdsCov = 64;           // C^-1 is held in LDS up to this many bands: 32 KB
constexpr int kThreads = 256;         // four waves; a workgroup takes kThreads rows, a wave 64 of them
constexpr int kBestWords = 4;         // doubles per (source, split) of k_good_best: chisq, its index, lnprob, its index

struct FluxArgs {
    const mbbd::WalkerK *wk;          // the rows' records (k_prologue)
    const int32_t *status;            // ... and row status
    int n;                            // rows
    const double *nu, *lnnu, *wt;     // every sample of the context's bands
    const int32_t *band;              // [nb][3]: first sample, one past the last, whether it is one sample of weight 1
    int nb, nmany, nsingle;           // bands; of many samples; of one sample of weight 1
    int nsamples;                     // samples of all bands (STAGE: in LDS, three arrays of that many doubles)
    double *mf;                       // band fluxes [nb][n]
};

static __global__ void k_good_lnnu(const double *nu, int n, double *lnnu)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) lnnu[i] = mbbm::m_log(nu[i]);
}

// Rows blockIdx.x * kThreads ... .  A band of many samples takes a wave per row: lane l accumulates samples l, l + 64,
// ... in that order, the 64 partial sums go through wave_sum's fixed tree and lane 0 stores the total.  A band of one
// sample of weight 1 is f_nu itself, a lane per row; a row the constructor failed on gets NaN in every band.
template <bool OPTHIN, bool NOALPHA, bool STAGE>
static __global__ __launch_bounds__(kThreads) void k_good_flux(const FluxArgs a)
{
    extern __shared__ double sh_good[];                            // (STAGE: nu, log nu, weight of every sample)
    const double *nu = a.nu, *ln = a.lnnu, *wt = a.wt;
    if (STAGE) {
        double *const s_nu = sh_good, *const s_ln = sh_good + a.nsamples, *const s_wt = sh_good + 2 * a.nsamples;
        for (int i = threadIdx.x; i < a.nsamples; i += kThreads) { s_nu[i] = a.nu[i]; s_ln[i] = a.lnnu[i]; s_wt[i] = a.wt[i]; }
        __syncthreads();
        nu = s_nu; ln = s_ln; wt = s_wt;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int base = blockIdx.x * kThreads + wave * 64;            // the wave's first row (wave-uniform)
    const int rows = min(64, a.n - base);                          // (<= 0: a wave beyond the last row)
    if (a.nmany) {
        for (int r = 0; r < rows; ++r) {
            const mbbd::WalkerK k = a.wk[base + r];                // wave-uniform
            if (k.status != mbbd::ROW_OK) continue;
            for (int b = 0; b < a.nb; ++b) {
                const int s0 = a.band[3 * b], s1 = a.band[3 * b + 1];
                if (a.band[3 * b + 2]) continue;
                double acc = 0.0;
                for (int i = s0 + lane; i < s1; i += 64)
                    acc = fma(mbbd::fnu_sample<OPTHIN, NOALPHA>(k, nu[i], ln[i]), wt[i], acc);
                const double total = mbbd::wave_sum(acc);
                if (lane == 0) a.mf[(size_t)b * a.n + base + r] = total;
            }
        }
    }
    if (lane >= rows) return;
    const int row = base + lane;
    if (a.status[row] != mbbd::ROW_OK) {
        const double qnan = __builtin_nan("");
        for (int b = 0; b < a.nb; ++b) a.mf[(size_t)b * a.n + row] = qnan;
    } else if (a.nsingle) {
        const mbbd::WalkerK k = a.wk[row];
        for (int b = 0; b < a.nb; ++b)
            if (a.band[3 * b + 2]) {
                const int s0 = a.band[3 * b];
                a.mf[(size_t)b * a.n + row] = mbbd::fnu_sample<OPTHIN, NOALPHA>(k, nu[s0], ln[s0]);
            }
    }
}

struct ChiArgs {
    const double *mf;                 // band fluxes [nb][n]
    const int32_t *status;            // row status [n]
    int n, nb;
    long long off;                    // the first row's number among all rows of the call
    long long rows_per_src;           // row (off + i) belongs to source ((off + i) / rows_per_src) % nsrc_data
    int nsrc_data;                    // sources of the context's data (1: it serves every row)
    const double *flux, *ivar;        // [nsrc_data][nb]
    const double *invcov;             // [nb][nb] or null
    int cov_in_lds;
    double *chisq, *q;                // row i goes to element out + i: of the columns (out = off), or of a block of n
    long long out;
    int32_t *row_status;              // [n] or null: a copy of the row status
    double *mf_rows;                  // [n][nb] or null: the band fluxes row by row
    int *gstatus;                     // [nsrc][2] row-status bits of the two columns, or null
    int nw, nsteps, burn, thin;       // (gstatus: the chain's shape and window)
};

// chisq of one row from its band fluxes, lane i of the launch: bands in order.  With a covariance the quadratic form is
// sum_i r_i (sum_j C^-1_ij r_j), both sums in order; every lane of a wave reads the same element of C^-1 at the same
// time, which LDS serves as one broadcast: no two lanes ever ask one bank for different words.
__device__ __forceinline__ double chisq_row(const ChiArgs &a, int i, int src, const double *cinv)
{
    const double *f = a.flux + (size_t)src * a.nb, *iv = a.ivar + (size_t)src * a.nb;
    double acc = 0.0;
    if (!a.invcov) {
        for (int b = 0; b < a.nb; ++b) {
            const double d = f[b] - a.mf[(size_t)b * a.n + i];
            acc = fma(d * d, iv[b], acc);
        }
    } else {
        for (int p = 0; p < a.nb; ++p) {
            double t = 0.0;
            for (int b = 0; b < a.nb; ++b) t = fma(cinv[p * a.nb + b], f[b] - a.mf[(size_t)b * a.n + i], t);
            acc = fma(f[p] - a.mf[(size_t)p * a.n + i], t, acc);
        }
    }
    return acc;
}

static __global__ __launch_bounds__(kThreads) void k_good_chi(const ChiArgs a)
{
    extern __shared__ double sh_cov[];
    const double *cinv = a.invcov;
    if (a.invcov && a.cov_in_lds) {
        for (int i = threadIdx.x; i < a.nb * a.nb; i += kThreads) sh_cov[i] = a.invcov[i];
        __syncthreads();
        cinv = sh_cov;
    }
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.n) return;
    const long long row = a.off + i;
    const int st = a.status[i];
    const int src = (int)((row / a.rows_per_src) % a.nsrc_data);
    double chi = __builtin_nan("");
    if (st == mbbd::ROW_OK) chi = chisq_row(a, i, src, cinv);
    const double q = mbbm::m_gammq_half(a.nb, chi);
    a.chisq[a.out + i] = chi;
    a.q[a.out + i] = q;
    if (a.row_status) a.row_status[i] = st;
    if (a.mf_rows)
        for (int b = 0; b < a.nb; ++b) a.mf_rows[(size_t)i * a.nb + b] = a.mf[(size_t)b * a.n + i];
    if (a.gstatus && st != mbbd::ROW_OK) {
        // mbbs::note_status for a [nsrc][2] table: a failing row counts when its step is inside the window
        const long long per = (long long)a.nw * a.nsteps;
        const int csrc = (int)(row / per), step = (int)(row % a.nsteps);
        if (step >= a.burn && (step - a.burn) % a.thin == 0) {
            const int bit = 1 << (mbbs::kStRowShift + (st & 7));
            atomicOr(&a.gstatus[csrc * 2 + 0], bit);
            atomicOr(&a.gstatus[csrc * 2 + 1], bit);
        }
    }
}

// theta-bar of every source as a parameter row: the means k_sum_begin left of columns 0 .. 4 (a.ncol == 5: the splits,
// and so the bits, of a summary of the window with neither clipping nor derived columns)
static __global__ __launch_bounds__(64) void k_good_mean(const mbbs::SumArgs a, double *rows)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.nsrc * 5) return;
    rows[i] = a.state[i].mean;
}

// smaller chisq first, then the smaller index; a NaN never wins (index < 0: none yet)
__device__ __forceinline__ bool smaller(double v1, long long i1, double v2, long long i2)
{
    if (i1 < 0 || v1 != v1) return false;
    if (i2 < 0) return true;
    if (v1 != v2) return v1 < v2;
    return i1 < i2;
}

// per source and split of the window (the columns' own splits): the entry of smallest chisq and, where there is an
// lnprob, the entry of largest lnprob in the summary's order (mbbs::better).  Indices are walker * nsteps + step.
static __global__ __launch_bounds__(kThreads) void k_good_best(const mbbs::SumArgs a, double *part)
{
    __shared__ double lds[kThreads];
    __shared__ long long ldsi[kThreads];
    const int src = blockIdx.x, split = blockIdx.y, t = threadIdx.x;
    const long long j0 = (long long)split * a.per_split, j1 = min(a.n, j0 + a.per_split);
    double cv = 0.0, bv = 0.0;
    long long ci = -1, bi = -1;
    for (long long j = j0 + t; j < j1; j += kThreads) {
        long long w, step;
        mbbc::sample_cell(a, j, w, step);
        const long long idx = w * a.nsteps + step, flat = (long long)src * a.nw * a.nsteps + idx;
        const double c = a.der[0][flat];
        if (smaller(c, idx, cv, ci)) { cv = c; ci = idx; }
        if (a.lnprob) {
            const double lp = a.lnprob[flat];
            if (mbbs::better(lp, idx, bv, bi)) { bv = lp; bi = idx; }
        }
    }
    double *out = part + ((size_t)src * a.splits + split) * kBestWords;
    __syncthreads();
    lds[t] = cv; ldsi[t] = ci;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w && smaller(lds[t + w], ldsi[t + w], lds[t], ldsi[t])) { lds[t] = lds[t + w]; ldsi[t] = ldsi[t + w]; }
        __syncthreads();
    }
    if (t == 0) { out[0] = lds[0]; out[1] = (double)ldsi[0]; }
    __syncthreads();
    lds[t] = bv; ldsi[t] = bi;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (t < w && mbbs::better(lds[t + w], ldsi[t + w], lds[t], ldsi[t])) { lds[t] = lds[t + w]; ldsi[t] = ldsi[t + w]; }
        __syncthreads();
    }
    if (t == 0) { out[2] = lds[0]; out[3] = (double)ldsi[0]; }
}

struct PickArgs {
    const double *part;               // [nsrc][splits][kBestWords]
    double *ml_row;                   // [nsrc][5] the maximum-likelihood entry as a parameter row (NaN: none)
    double *o_ml;                     // [nsrc][7]: slots 0 .. 4 are written here, 5 and 6 by the rows' evaluation
    int *o_mlidx, *o_bestidx;         // [nsrc][2] walker, step; -1, -1: none
    double *o_best;                   // [nsrc][2] chisq and q of the entry of largest lnprob
};

// one thread per source
static __global__ __launch_bounds__(64) void k_good_pick(const mbbs::SumArgs a, const PickArgs p)
{
    const int src = blockIdx.x * 64 + threadIdx.x;
    if (src >= a.nsrc) return;
    const double *pp = p.part + (size_t)src * a.splits * kBestWords;
    const double qnan = __builtin_nan("");
    double cv = 0.0, bv = 0.0;
    long long ci = -1, bi = -1;
    for (int s = 0; s < a.splits; ++s) {
        const double *e = pp + (size_t)s * kBestWords;
        if (smaller(e[0], (long long)e[1], cv, ci)) { cv = e[0]; ci = (long long)e[1]; }
        if (mbbs::better(e[2], (long long)e[3], bv, bi)) { bv = e[2]; bi = (long long)e[3]; }
    }
    const long long first = (long long)src * a.nw * a.nsteps;
    for (int k = 0; k < 5; ++k) {
        const double v = ci >= 0 ? a.chain[(first + ci) * 5 + k] : qnan;
        p.ml_row[(size_t)src * 5 + k] = v;
        p.o_ml[(size_t)src * 7 + k] = v;
    }
    p.o_mlidx[src * 2 + 0] = ci >= 0 ? (int)(ci / a.nsteps) : -1;
    p.o_mlidx[src * 2 + 1] = ci >= 0 ? (int)(ci % a.nsteps) : -1;
    p.o_bestidx[src * 2 + 0] = bi >= 0 ? (int)(bi / a.nsteps) : -1;
    p.o_bestidx[src * 2 + 1] = bi >= 0 ? (int)(bi % a.nsteps) : -1;
    p.o_best[src * 2 + 0] = bi >= 0 ? a.der[0][first + bi] : qnan;
    p.o_best[src * 2 + 1] = bi >= 0 ? a.der[1][first + bi] : qnan;
}

struct FinishArgs {
    const int *gstatus;               // [nsrc][2]
    long long *o_nused;               // results [nsrc][2] ...
    double *o_mean, *o_min, *o_max, *o_pct;   // o_pct [nsrc][2][npct]
    int *o_status;
    // the evaluation of the rows [theta-bar of every source][maximum-likelihood entry of every source]
    const double *tbar;               // [nsrc][5]
    const double *ev_chisq, *ev_q;    // [2 nsrc]
    double *o_atmean, *o_ml;          // [nsrc][7]
};

// one thread per (source, column): what k_sum_finish writes of a column; the thread of column 0 also puts the rows'
// evaluation into at_mean and ml
static __global__ __launch_bounds__(64) void k_good_finish(const mbbs::SumArgs a, const FinishArgs f)
{
    const int cid = blockIdx.x * 64 + threadIdx.x;
    if (cid >= a.nsrc * 2) return;
    const mbbs::ColState &st = a.state[cid];
    const double qnan = __builtin_nan("");
    f.o_nused[cid] = st.n_used; f.o_mean[cid] = st.mean; f.o_min[cid] = st.vmin; f.o_max[cid] = st.vmax;
    f.o_status[cid] = f.gstatus[cid] | (st.n_used == 0 ? mbbs::kStEmpty : 0) | (st.nan ? mbbs::kStNaN : 0);
    for (int k = 0; k < a.npct; ++k) {
        double r = qnan;
        if (st.nranks) {
            // numpy's _lerp: a + (b - a) t, and b - (b - a) (1 - t) from t = 0.5 on
            const double lo = mbbs::from_key(st.prefix[2 * k]), hi = mbbs::from_key(st.prefix[2 * k + 1]), t = st.gamma[k];
            const double diff = hi - lo;
            r = lo + diff * t;
            if (t >= 0.5) r = hi - diff * (1.0 - t);
        }
        f.o_pct[(size_t)cid * a.npct + k] = r;
    }
    if (cid & 1) return;
    const int src = cid >> 1;
    for (int k = 0; k < 5; ++k) f.o_atmean[(size_t)src * 7 + k] = f.tbar[(size_t)src * 5 + k];
    f.o_atmean[(size_t)src * 7 + 5] = f.ev_chisq[src];
    f.o_atmean[(size_t)src * 7 + 6] = f.ev_q[src];
    f.o_ml[(size_t)src * 7 + 5] = f.ev_chisq[a.nsrc + src];
    f.o_ml[(size_t)src * 7 + 6] = f.ev_q[a.nsrc + src];
}

}   // namespace mbbq
