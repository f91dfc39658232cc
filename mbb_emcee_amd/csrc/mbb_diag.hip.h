// mbb_diag.hip.h -- convergence diagnostics of a device-resident chain (gfx950, fp64, wave64).
//
// Per (source, parameter), over the steps burn <= t < nsteps of a chain in emcee's layout
// [nsrc][nw][nsteps][5]: the integrated autocorrelation time tau with Sokal's automatic window M
// (ensemble.integrated_time's definition), the effective sample size nw n / tau, the split R-hat of
// Gelman & Rubin across walkers, and optionally the first nacf values of the autocorrelation function.
//
//   rho_k = c_k / c_0,  c_k = sum_{i < n - k} y_i y_{i+k},  y = the series minus its mean
//   tau(m) = 2 sum_{k <= m} rho_k - 1;  M = the first m with m >= c tau(m), else n - 1;  tau = tau(M)
// method 0 ("mean"):    the series is the ensemble mean over walkers at each step
// method 1 ("walkers"): each walker's own rho_k, averaged over walkers, windowed once (emcee >= 3)
//
// Kernels (256 threads):
//   k_diag_mean   method 0: the ensemble-mean series [nsrc][n][5]; a thread owns one (step, parameter), consecutive
//                 threads consecutive addresses, the walkers added in order 0 .. nw - 1 (numpy's mean(axis=0))
//   k_diag_acf    one workgroup per (source, parameter): a series is staged, centred, in LDS; lags are taken in
//                 ascending blocks of kLagBlock, a thread owning ONE lag of the block: at index i the read of y[i]
//                 is a broadcast and the reads of y[i + k] are 256 consecutive doubles (conflict-free).  After a
//                 block thread 0 scans tau(m) in ascending m and tests the window; the workgroup leaves, all of
//                 it at once, when M is found and nacf lags are out: the cost is n M, not n^2.
//   k_diag_seq    split R-hat, first pass: mean and variance (ddof 1) of both halves of every walker; a wave owns a
//                 walker, its lanes consecutive steps
//   k_diag_rhat   W, B and R of a (source, parameter) from its 2 nw sequences
// A walker's part of the chain is contiguous along step x parameter; a series is every fifth double of it, and the
// five workgroups of a source (adjacent block indices) use the five fifths of every line that is fetched.  No thread
// pattern strides across walkers.
//
// Sums are fixed-order: a lag's products go, four interleaved partial sums at a time, through chunks of kChunk
// indices that are added in ascending order; sums over a series are per-thread strided partial sums, a butterfly
// over the wave's lanes and a fixed tree over the four waves; walkers are added in order.  No floating-point
// atomics: the same chain gives the same bits.
//
// Limit: a series may have kMaxSteps = 16384 kept steps (the staged series and its zero padding, 133 KB, fit the
// CU's 160 KB of LDS); a longer one is an argument error.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mbbg {

constexpr int kThreads = 256;
constexpr int kLagBlock = 256;      // lags per block: one per thread
constexpr int kChunk = 64;          // indices per inner chunk of a lag's sum
constexpr int kPad = kLagBlock + 8; // zeros behind the staged series: y[i + k] beyond the end reads 0
constexpr int kMaxSteps = 16384;
constexpr int kMinSteps = 8;        // ensemble.integrated_time: shorter series give NaN

// status bits (include/mbb_hip.h: mbb_diag_status)
constexpr int kStShort = 1, kStConst = 2, kStNaN = 4, kStUnreliable = 8;

struct DiagArgs {
    const double *chain;            // [nsrc][nw][nsteps][5]
    int nsrc, nw, nsteps, burn, n;  // n = nsteps - burn
    int method, nacf;
    double c, tol;
    // work
    double *mean;                   // [nsrc][n][5]: the ensemble-mean series (method 0)
    double *seq;                    // [nsrc * 5][nw][2 halves][mean, variance]
    // results [nsrc][5]...
    double *o_tau, *o_ess, *o_rhat, *o_acf;   // o_acf [nsrc][5][nacf] or null
    int *o_window, *o_status;
};

inline size_t acf_lds_bytes(int n) { return ((size_t)n + kPad) * sizeof(double); }

// butterfly over the wave's 64 lanes: every lane ends with the same sum (a + b and b + a are the same bits)
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    return v;
}

// ... and a fixed tree over the workgroup's four waves; the result in every thread
__device__ __forceinline__ double block_sum(double v, double *w4)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) w4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (w4[0] + w4[1]) + (w4[2] + w4[3]);
}

__global__ __launch_bounds__(kThreads) void k_diag_mean(const DiagArgs a)
{
    const long long len = (long long)a.n * 5;
    const int per = (int)((len + kThreads - 1) / kThreads), src = blockIdx.x / per;   // workgroups per source
    const long long j = (long long)(blockIdx.x - src * per) * kThreads + threadIdx.x;
    if (j >= len) return;
    const double *p = a.chain + ((long long)src * a.nw * a.nsteps + a.burn) * 5 + j;
    const long long stride = (long long)a.nsteps * 5;
    double s = 0.0;
    for (int w = 0; w < a.nw; ++w) s += p[w * stride];
    a.mean[(long long)src * len + j] = s / (double)a.nw;
}

// Stage series x[0], x[5], ... x[5 (n - 1)] in y, minus its mean; c_0 in every thread.  flags (the same in every
// thread): 1 the series holds a NaN or an infinity, 2 it is constant.
__device__ __forceinline__ double stage_series(const double *x, int n, double *y, double *w4, int &flags)
{
    const int t = threadIdx.x;
    const double first = x[0];
    double s = 0.0;
    int f = 0;
    __syncthreads();                                      // (the last block's readers of y are done)
    for (int i = t; i < n; i += kThreads) {
        const double v = x[(long long)i * 5];
        y[i] = v;
        s += v;
        f |= (v - v != 0.0 ? 1 : 0) | (v != first ? 2 : 0);   // (v - v: NaN for a NaN and for an infinity)
    }
    // (__syncthreads_or answers whether ANY thread's argument was non-zero, not the OR of the arguments: a vote per flag)
    const int bad = __syncthreads_or(f & 1), differs = __syncthreads_or(f & 2);
    flags = (bad ? 1 : 0) | (differs ? 0 : 2);
    const double mean = block_sum(s, w4) / (double)n;
    double q = 0.0;
    for (int i = t; i < n; i += kThreads) {
        const double d = y[i] - mean;
        y[i] = d;
        q += d * d;
    }
    const double c0 = block_sum(q, w4);                   // (its barriers also publish y)
    return c0;
}

__global__ __launch_bounds__(kThreads) void k_diag_acf(const DiagArgs a)
{
    extern __shared__ __align__(16) unsigned char diag_smem[];
    double *y = reinterpret_cast<double *>(diag_smem);    // [n + kPad]
    __shared__ double rho_b[kLagBlock];
    __shared__ double w4[4];
    __shared__ double s_tau;
    __shared__ int s_m;
    const int col = blockIdx.x, src = col / 5, par = col - src * 5, t = threadIdx.x;
    const int n = a.n, nacf = a.o_acf ? a.nacf : 0;
    const double qnan = __builtin_nan("");
    double *acf = a.o_acf ? a.o_acf + (size_t)col * a.nacf : nullptr;
    int status = 0;
    if (n < kMinSteps) status = kStShort;
    // the series: one (the ensemble mean) or one per walker
    const int nser = a.method == 0 ? 1 : a.nw;
    const double *base = a.method == 0 ? a.mean + (long long)src * n * 5 + par
                                       : a.chain + ((long long)src * a.nw * a.nsteps + a.burn) * 5 + par;
    const long long sstride = (long long)a.nsteps * 5;
    for (int i = n + t; i < n + kPad; i += kThreads) y[i] = 0.0;
    int found = -1;                                        // M once it is known
    double tau = qnan, csum = 0.0, c0 = 0.0;
    for (int k0 = 0; status == 0; k0 += kLagBlock) {
        const int k = k0 + t, lim = n - k0;
        double racc = 0.0;
        for (int s = 0; s < nser; ++s) {
            if (nser > 1 || k0 == 0) {
                int flags;
                c0 = stage_series(base + s * sstride, n, y, w4, flags);
                if (flags & 1) status |= kStNaN;
                else if ((flags & 2) || !(c0 > 0.0)) status |= kStConst;
            }
            if (status) continue;                          // (uniform; the flags of the walkers behind still count)
            double o = 0.0;
            for (int i0 = 0; i0 < lim; i0 += kChunk) {
                const int e = min(kChunk, lim - i0);
                const double *p = y + i0, *q = y + i0 + k;
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
                for (int i = 0; i < e; i += 4) {           // (indices past the end meet the zeros behind the series)
                    a0 += p[i] * q[i];
                    a1 += p[i + 1] * q[i + 1];
                    a2 += p[i + 2] * q[i + 2];
                    a3 += p[i + 3] * q[i + 3];
                }
                o += (a0 + a1) + (a2 + a3);
            }
            racc += k == 0 ? 1.0 : o / c0;                 // (rho_0 is 1: c_0 is the tree's, this thread's sum rounds otherwise)
        }
        if (status) break;                                 // (only in the first block: every series is staged there)
        const double rho = nser > 1 ? racc / (double)nser : racc;
        rho_b[t] = rho;
        if (k < nacf) acf[k] = rho;
        __syncthreads();
        if (t == 0 && found < 0) {
            int m = -1;
            double tm = qnan;
            for (int j = 0; j < kLagBlock && k0 + j < n; ++j) {
                csum += rho_b[j];
                tm = 2.0 * csum - 1.0;
                if ((double)(k0 + j) >= a.c * tm) { m = k0 + j; break; }
            }
            if (m < 0 && k0 + kLagBlock >= n) m = n - 1;   // no window: all of the series (tm is tau(n - 1))
            s_m = m;
            s_tau = tm;
        }
        __syncthreads();
        if (found < 0) {
            found = s_m;
            tau = s_tau;
        }
        if (found >= 0 && k0 + kLagBlock >= nacf) break;
    }
    if (status) {
        tau = qnan;
        found = -1;
        for (int k = t; k < nacf; k += kThreads) acf[k] = qnan;
    }
    if (t == 0) {
        if (status == 0 && (double)n < a.tol * tau) status |= kStUnreliable;
        a.o_tau[col] = tau;
        a.o_ess[col] = (double)a.nw * (double)n / tau;
        a.o_window[col] = found;
        a.o_status[col] = status;
    }
}

// Split R-hat, first pass.  grid (nsrc * 5, y): wave g of the row's 4 y takes walkers g, g + 4 y, ...
__global__ __launch_bounds__(kThreads) void k_diag_seq(const DiagArgs a)
{
    const int col = blockIdx.x, src = col / 5, par = col - src * 5;
    const int lane = threadIdx.x & 63, g = blockIdx.y * (kThreads / 64) + (threadIdx.x >> 6);
    const int h = a.n / 2;
    if (h < 2) return;
    for (int w = g; w < a.nw; w += gridDim.y * (kThreads / 64)) {
        const double *x = a.chain + (((long long)src * a.nw + w) * a.nsteps + a.burn) * 5 + par;
        for (int half = 0; half < 2; ++half) {
            const double *xh = x + (long long)(half ? a.n - h : 0) * 5;   // (n odd: the middle step is in neither)
            double s = 0.0;
            for (int i = lane; i < h; i += 64) s += xh[(long long)i * 5];
            const double mean = wave_sum(s) / (double)h;
            double q = 0.0;
            for (int i = lane; i < h; i += 64) {
                const double d = xh[(long long)i * 5] - mean;
                q += d * d;
            }
            const double var = wave_sum(q) / (double)(h - 1);
            if (lane == 0) {
                double *o = a.seq + (((size_t)col * a.nw + w) * 2 + half) * 2;
                o[0] = mean;
                o[1] = var;
            }
        }
    }
}

// W = mean of the sequences' variances, B = h var(their means), R = sqrt(((h - 1) / h W + B / h) / W)
__global__ __launch_bounds__(kThreads) void k_diag_rhat(const DiagArgs a)
{
    __shared__ double w4[4];
    const int col = blockIdx.x, t = threadIdx.x, h = a.n / 2, nseq = 2 * a.nw;
    if (h < 2) {
        if (t == 0) a.o_rhat[col] = __builtin_nan("");
        return;
    }
    const double *sq = a.seq + (size_t)col * nseq * 2;
    double sm = 0.0, sv = 0.0;
    for (int i = t; i < nseq; i += kThreads) { sm += sq[2 * i]; sv += sq[2 * i + 1]; }
    const double mm = block_sum(sm, w4) / (double)nseq;
    const double W = block_sum(sv, w4) / (double)nseq;
    double sb = 0.0;
    for (int i = t; i < nseq; i += kThreads) { const double d = sq[2 * i] - mm; sb += d * d; }
    const double B = (double)h * (block_sum(sb, w4) / (double)(nseq - 1));
    if (t == 0) a.o_rhat[col] = sqrt((((double)(h - 1) / (double)h) * W + B / (double)h) / W);
}

}   // namespace mbbg
