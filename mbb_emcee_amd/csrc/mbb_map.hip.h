// mbb_map.hip.h -- the maximum of the posterior per (source, start) by Levenberg-Marquardt (gfx950, fp64, wave64).
//
// The posterior is a sum of squares: -2 ln P = F(p) = data term + soft upper walls + Gaussian priors behind the hard
// lower limits (mbb_walker_consts.inc), so each source is a small non-linear least-squares problem and all of them are
// independent.  k_map_lm gives a workgroup to one (source, start) and runs the whole search inside one launch: no host
// round trip, no traffic between workgroups, no atomics, no spins; every loop is bounded by maxiter and kTries.  The
// step logic is mbb_lm.hip.h's (the host tests run the same text).
//
// An iteration at p:
//   rows      p and, per active parameter, two more rows: p -+ h_i e_i (central difference), or p + h_i e_i and
//             p + 2 h_i e_i (the second-order one-sided difference) where p_i - h_i would be below the lower limit;
//             h_i = kHRel max(|p_i|, kXFloor).  At most 11 rows.
//   records   a lane per row: the SED constructor as k_prologue has it (sed_prologue<.., false>, make_walker_k), and
//             sed_peak_wave when a wall or a prior of the peak wavelength is set; the WalkerK records go to LDS
//   fluxes    a wave per row, rows dealt to the waves in turn: a band of many samples by lane-strided fma and wave_sum's
//             fixed tree, a band of one sample of weight 1 is fnu_sample itself (k_good_flux's two shapes); with STAGE
//             the samples (nu, ln nu, w) are in dynamic LDS
//   F         a wave per row: d = f - m, then sum d^2 ivar, or d^T C^-1 d, lanes striding the bands, wave_sum; lane 0
//             adds the walls and priors.  A row the constructor fails on, or below a lower limit, has F = +inf.
//   J, A, g   J_m = d m / d p by the differences above (LDS); A = J_m^T W J_m, g = J_m^T W d with W = diag(ivar) or
//             C^-1 (through U = C^-1 J_m in LDS), a wave per element, plus the walls' and priors' own terms: those of
//             the five parameters analytically, the peak wavelength's through the same differences
//   trials    kCand damped steps at once (lm_candidates), a lane each for the 5 x 5 solve, a wave each for the
//             evaluation: this is where waves that would idle shorten the dependent chain.  The best one lm_accept
//             admits is taken; if none, the next kCand, up to kTries times.
// After the search one more Jacobian at the final point gives the Laplace covariance A^-1 (lm_laplace).
// Band fluxes, Jacobian and records live in LDS, nothing a thread indexes at run time is in registers: no scratch.
// Every sum has a fixed order and a workgroup reads its own source's data and its own start alone: a result has the
// same bits whatever else the call holds, and from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mbb_device.hip.h"
#include "mbb_lm.hip.h"

namespace mbbmap {

// Four waves: one per damping candidate, and the 11 rows of a Jacobian in three turns.  -DMBB_MAP_THREADS=512 or 704
// builds the kernel with 8 or 11 waves for a measurement (tools/bench_map.py --lib; DESIGN.md 4.3h has what came of it).
#ifndef MBB_MAP_THREADS
#define MBB_MAP_THREADS 256
#endif
constexpr int kThreads = MBB_MAP_THREADS;
static_assert(kThreads % 64 == 0 && kThreads >= 256 && kThreads <= 704, "4 to 11 waves");
constexpr int kWaves = kThreads / 64;
constexpr int kRows = 11;             // p and two per parameter
constexpr int kMaxBands = 256;        // bands of a map fit (mbb_map_fit checks it)
constexpr int kLdsSamples = 2560;     // as the goodness and prediction fills
constexpr int kLdsCov = 64;
constexpr double kHRel = 7.62939453125e-06;   // 2^-17 ~ eps^(1/3): truncation and rounding of a central difference meet

enum Status : int { ST_CONV_F = 1, ST_CONV_X = 2, ST_MAXITER = 4, ST_START_INVALID = 8, ST_COV_SINGULAR = 16,
                    ST_ALL_FIXED = 32, ST_STENCIL_FAILED = 64, ST_LOWLIM_SHIFT = 8 };

constexpr int kOutDoubles = 31;       // per (source, start): params[5], F, cov[25]
constexpr int kOutInts = 4;           // niter, nfev, status, 0

struct MapArgs {
    const double *start;              // [nsrc][nstart][5]
    int nstart;
    int nsrc_data;                    // sources of the context's data (1: it serves every source)
    const double *nu, *lnnu, *wt;     // every sample of the context's bands
    const int32_t *band;              // [nb][3]: first sample, one past the last, whether it is one sample of weight 1
    int nb, nsamples;
    const double *flux, *ivar;        // [nsrc_data][nb]
    const double *invcov;             // [nb][nb] or null
    int cov_in_lds;
    double nunorm, lnunorm;
    double lowlim[5], uplim[6], gmean[6], givar[6];
    uint32_t has_uplim, has_gprior;
    uint32_t fixed;                   // lm_fixed_mask
    int maxiter;
    double ftol, xtol;
    double *outd;                     // [nsrc][nstart][kOutDoubles]
    int32_t *outi;                    // [nsrc][nstart][kOutInts]
};

// dynamic LDS in doubles: [samples 3 ns if STAGE][C^-1 nb^2 if in LDS][mf kRows nb][jm 5 nb][d nb][u 5 nb if cov]
__host__ __device__ inline size_t lds_doubles(int nb, int nsamples, bool stage, bool cov, bool cov_in_lds)
{
    return (stage ? (size_t)3 * nsamples : 0) + (cov && cov_in_lds ? (size_t)nb * nb : 0) + (size_t)(kRows + 5 + 1) * nb +
           (cov ? (size_t)5 * nb : 0);
}

template <bool OPTHIN, bool NOALPHA, bool STAGE>
static __global__ __launch_bounds__(kThreads) void k_map_lm(const MapArgs a)
{
    using namespace mbblm;
    extern __shared__ double sh_map[];
    __shared__ mbbd::WalkerK s_wk[kRows];
    __shared__ double s_rows[kRows][5];
    __shared__ double s_peak[kRows], s_F[kRows];
    __shared__ double s_p[5], s_h[5], s_A[25], s_g[5], s_dpeak[5], s_cov[25];
    __shared__ double s_work[kCand][25], s_delta[kCand][5], s_cand[kCand], s_pred[kCand], s_step[kCand];
    __shared__ int s_solved[kCand], s_clipped[kCand];
    __shared__ double s_Fcur, s_lam, s_nu;
    __shared__ int s_rowp[5], s_rowm[5], s_onesided[5];
    __shared__ int s_nrows, s_stop, s_status, s_niter, s_nfev, s_moved;
    __shared__ unsigned s_active;
    // the limits and priors as LDS arrays: an argument block indexed at run time would be copied to scratch
    __shared__ double s_low[5], s_up[6], s_gm[6], s_gi[6];

    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(t >> 6));
    const int nb = a.nb;
    const int src = blockIdx.x / a.nstart;
    const double *const flux = a.flux + (size_t)(src % a.nsrc_data) * nb;
    const double *const ivar = a.ivar + (size_t)(src % a.nsrc_data) * nb;
    const bool cov = a.invcov != nullptr;
    const bool want_peak = ((a.has_uplim | a.has_gprior) >> 5) & 1u;

    // the carve of the dynamic LDS
    double *carve = sh_map;
    const double *nu = a.nu, *ln = a.lnnu, *wt = a.wt;
    if (STAGE) {
        double *const st_freq = carve, *const st_ln = carve + a.nsamples, *const st_wt = carve + 2 * a.nsamples;
        carve += 3 * (size_t)a.nsamples;
        for (int i = t; i < a.nsamples; i += kThreads) { st_freq[i] = a.nu[i]; st_ln[i] = a.lnnu[i]; st_wt[i] = a.wt[i]; }
        nu = st_freq; ln = st_ln; wt = st_wt;
    }
    const double *cinv = a.invcov;
    if (cov && a.cov_in_lds) {
        double *const s_c = carve;
        carve += (size_t)nb * nb;
        for (int i = t; i < nb * nb; i += kThreads) s_c[i] = a.invcov[i];
        cinv = s_c;
    }
    double *const s_mf = carve;                      // [kRows][nb]
    double *const s_jm = s_mf + (size_t)kRows * nb;  // [5][nb]
    double *const s_d = s_jm + (size_t)5 * nb;       // [nb]: f - m at p
    double *const s_u = s_d + nb;                    // [5][nb]: C^-1 J_m (with a covariance)

    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 5; ++i) s_low[i] = a.lowlim[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) { s_up[i] = a.uplim[i]; s_gm[i] = a.gmean[i]; s_gi[i] = a.givar[i]; }
    }
    if (t < 5) s_p[t] = a.start[(size_t)blockIdx.x * 5 + t];
    if (t == 0) { s_lam = kLamStart; s_nu = 2.0; s_stop = 0; s_status = 0; s_niter = 0; s_nfev = 0; s_moved = 1; }
    __syncthreads();

    // ---- F of rows 0 .. n - 1 of s_rows into s_F; the band fluxes stay in s_mf, the peaks in s_peak ----
    auto evaluate = [&](int n) __attribute__((always_inline)) {
        if (t < n) {
            const double T = s_rows[t][0], beta = s_rows[t][1], lambda0 = s_rows[t][2], alpha = s_rows[t][3], fnorm = s_rows[t][4];
            bool ok = true;
            ok = ok && !(T < s_low[0]); ok = ok && !(beta < s_low[1]); ok = ok && !(lambda0 < s_low[2]);
            ok = ok && !(alpha < s_low[3]); ok = ok && !(fnorm < s_low[4]);
            const double big = 1.7976931348623157e308;
            const bool fin = fabs(T) <= big && fabs(beta) <= big && fabs(lambda0) <= big && fabs(alpha) <= big && fabs(fnorm) <= big;
            mbbd::SedScalars s;
            mbbd::WalkerK k = {};                                   // (a failing row's record is zeros and its status)
            int st = !ok ? (int)mbbd::ROW_BELOW_LOWLIM : (int)mbbd::ROW_NONFINITE;
            double peak = __builtin_nan("");
            if (ok && fin) {
                st = mbbd::sed_prologue<OPTHIN, NOALPHA, false>(T, beta, alpha, fnorm, mbbm::m_log(T),
                                                                OPTHIN ? 0.0 : mbbm::m_log(lambda0), a.nunorm, a.lnunorm, s);
                if (st == mbbd::ROW_OK) {
                    mbbd::make_walker_k<OPTHIN, NOALPHA>(beta, alpha, s, k);
                    if (want_peak) {
                        int pst;
                        peak = mbbd::sed_peak_wave<OPTHIN, false>(T, beta, k.lx0, s.hcokt, pst);
                        if (pst != mbbd::ROW_OK) st = pst;
                    }
                }
            }
            k.status = st;
            k.peak = peak;
            s_wk[t] = k;
            s_peak[t] = peak;
        }
        __syncthreads();
        for (int r = wave; r < n; r += kWaves) {
            const mbbd::WalkerK &k = s_wk[r];
            if (k.status != mbbd::ROW_OK) continue;                 // wave-uniform
            for (int b = 0; b < nb; ++b) {
                const int s0 = a.band[3 * b], s1 = a.band[3 * b + 1];
                if (a.band[3 * b + 2]) continue;
                double acc = 0.0;
                for (int i = s0 + lane; i < s1; i += 64)
                    acc = fma(mbbd::fnu_sample<OPTHIN, NOALPHA>(k, nu[i], ln[i]), wt[i], acc);
                const double total = mbbd::wave_sum(acc);
                if (lane == 0) s_mf[(size_t)r * nb + b] = total;
            }
            for (int b = lane; b < nb; b += 64)
                if (a.band[3 * b + 2]) {
                    const int s0 = a.band[3 * b];
                    s_mf[(size_t)r * nb + b] = mbbd::fnu_sample<OPTHIN, NOALPHA>(k, nu[s0], ln[s0]);
                }
        }
        __syncthreads();
        for (int r = wave; r < n; r += kWaves) {
            const double inf = __builtin_inf();
            if (s_wk[r].status != mbbd::ROW_OK) { if (lane == 0) s_F[r] = inf; continue; }
            const double *m = s_mf + (size_t)r * nb;
            double acc = 0.0;
            if (!cov) {
                for (int b = lane; b < nb; b += 64) { const double d = flux[b] - m[b]; acc = fma(d * d, ivar[b], acc); }
            } else {
                for (int p = lane; p < nb; p += 64) {
                    double tt = 0.0;
                    for (int b = 0; b < nb; ++b) tt = fma(cinv[p * nb + b], flux[b] - m[b], tt);
                    acc = fma(flux[p] - m[p], tt, acc);
                }
            }
            double f = mbbd::wave_sum(acc);
            if (lane == 0) {
                // the walls and the priors, as mbb_walker_consts.inc has them
                for (int i = 0; i < 5; ++i) {
                    const double pi = s_rows[r][i];
                    if (((a.has_uplim >> i) & 1u) && pi > s_up[i]) {
                        const double lw = 0.02 * (s_up[i] - s_low[i]), d = pi - s_up[i];
                        f += d * d / (lw * lw);
                    }
                    if ((a.has_gprior >> i) & 1u) { const double d = pi - s_gm[i]; f = fma(s_gi[i] * d, d, f); }
                }
                if (want_peak) {
                    const double pk = s_peak[r];
                    if (((a.has_uplim >> 5) & 1u) && pk > s_up[5]) {
                        const double lw = 0.02 * s_up[5], d = pk - s_up[5];
                        f += d * d / (lw * lw);
                    }
                    if ((a.has_gprior >> 5) & 1u) { const double d = pk - s_gm[5]; f = fma(s_gi[5] * d, d, f); }
                }
                s_F[r] = f;
            }
        }
        __syncthreads();
    };

    // ---- the rows of a Jacobian at s_p over the parameters of `over`, evaluated; A, g (and s_d, s_dpeak) from them ----
    auto jacobian = [&](unsigned over) __attribute__((always_inline)) {
        if (t == 0) {
            int n = 1;
            for (int i = 0; i < 5; ++i) {
                s_rows[0][i] = s_p[i];
                s_rowp[i] = s_rowm[i] = -1;
                if (!((over >> i) & 1u)) continue;
                const double h = kHRel * fmax(fabs(s_p[i]), kXFloor);
                s_onesided[i] = s_p[i] - h < s_low[i];
                s_rowm[i] = n++; s_rowp[i] = n++;
                s_h[i] = h;
            }
            for (int i = 0; i < 5; ++i) {
                if (s_rowp[i] < 0) continue;
                for (int j = 0; j < 5; ++j) s_rows[s_rowm[i]][j] = s_rows[s_rowp[i]][j] = s_p[j];
                // (the step actually taken, as the rounded rows have it, is what the difference is divided by)
                s_rows[s_rowm[i]][i] = s_onesided[i] ? s_p[i] + s_h[i] : s_p[i] - s_h[i];
                s_rows[s_rowp[i]][i] = s_onesided[i] ? s_p[i] + 2.0 * s_h[i] : s_p[i] + s_h[i];
            }
            s_nrows = n;
            s_nfev += n;
        }
        __syncthreads();
        evaluate(s_nrows);
        // J_m, d and the peak's derivative; a row of the stencil that failed gives NaN, which stops the search below
        for (int e = t; e < 5 * nb; e += kThreads) {
            const int i = e / nb, b = e - i * nb;
            double v = 0.0;
            if (s_rowp[i] >= 0) {
                const double m0 = s_mf[b], m1 = s_mf[(size_t)s_rowm[i] * nb + b], m2 = s_mf[(size_t)s_rowp[i] * nb + b];
                const bool bad = s_wk[s_rowm[i]].status != mbbd::ROW_OK || s_wk[s_rowp[i]].status != mbbd::ROW_OK;
                const double x1 = s_rows[s_rowm[i]][i], x2 = s_rows[s_rowp[i]][i];
                if (s_onesided[i]) v = (fma(4.0, m1, -3.0 * m0) - m2) / (x2 - s_p[i]);      // (-3 f0 + 4 f1 - f2) / 2h
                else v = (m2 - m1) / (x2 - x1);
                if (bad) v = __builtin_nan("");
            }
            s_jm[(size_t)i * nb + b] = v;
        }
        for (int b = t; b < nb; b += kThreads) s_d[b] = flux[b] - s_mf[b];
        if (t < 5) {
            double v = 0.0;
            if (want_peak && s_rowp[t] >= 0) {
                const double k0 = s_peak[0], k1 = s_peak[s_rowm[t]], k2 = s_peak[s_rowp[t]];
                const double x1 = s_rows[s_rowm[t]][t], x2 = s_rows[s_rowp[t]][t];
                if (s_onesided[t]) v = (fma(4.0, k1, -3.0 * k0) - k2) / (x2 - s_p[t]);
                else v = (k2 - k1) / (x2 - x1);
            }
            s_dpeak[t] = v;
        }
        __syncthreads();
        if (cov) {
            for (int e = t; e < 5 * nb; e += kThreads) {
                const int i = e / nb, p = e - i * nb;
                double tt = 0.0;
                for (int b = 0; b < nb; ++b) tt = fma(cinv[p * nb + b], s_jm[(size_t)i * nb + b], tt);
                s_u[(size_t)i * nb + p] = tt;
            }
            __syncthreads();
        }
        // the 15 elements of A's upper triangle and the 5 of g, dealt to the waves in turn
        for (int e = wave; e < 20; e += kWaves) {
            int i, j;
            if (e < 15) {
                i = 0; int rest = e;
                while (rest >= 5 - i) { rest -= 5 - i; ++i; }
                j = i + rest;
            } else { i = e - 15; j = -1; }
            const double *ji = s_jm + (size_t)i * nb;
            double acc = 0.0;
            if (!cov) {
                if (j >= 0) { const double *jj = s_jm + (size_t)j * nb; for (int b = lane; b < nb; b += 64) acc = fma(ji[b] * ivar[b], jj[b], acc); }
                else for (int b = lane; b < nb; b += 64) acc = fma(ji[b] * ivar[b], s_d[b], acc);
            } else {
                const double *ui = s_u + (size_t)i * nb;
                if (j >= 0) { const double *jj = s_jm + (size_t)j * nb; for (int b = lane; b < nb; b += 64) acc = fma(ui[b], jj[b], acc); }
                else for (int b = lane; b < nb; b += 64) acc = fma(ui[b], s_d[b], acc);
            }
            const double total = mbbd::wave_sum(acc);
            if (lane == 0) {
                if (j >= 0) { s_A[i * 5 + j] = total; s_A[j * 5 + i] = total; }
                else s_g[i] = total;
            }
        }
        __syncthreads();
        if (t == 0) {
            for (int i = 0; i < 5; ++i) {
                if (s_rowp[i] < 0) continue;
                const double pi = s_p[i];
                if (((a.has_uplim >> i) & 1u) && pi > s_up[i]) {
                    const double lw = 0.02 * (s_up[i] - s_low[i]), il = 1.0 / (lw * lw);
                    s_A[i * 5 + i] += il;
                    s_g[i] -= (pi - s_up[i]) * il;
                }
                if ((a.has_gprior >> i) & 1u) {
                    s_A[i * 5 + i] += s_gi[i];
                    s_g[i] -= (pi - s_gm[i]) * s_gi[i];
                }
            }
            if (want_peak) {
                const double pk = s_peak[0];
                double w = 0.0, r = 0.0;                                // sum of weights; sum of weight x residual
                if (((a.has_uplim >> 5) & 1u) && pk > s_up[5]) {
                    const double lw = 0.02 * s_up[5], il = 1.0 / (lw * lw);
                    w += il; r += (pk - s_up[5]) * il;
                }
                if ((a.has_gprior >> 5) & 1u) { w += s_gi[5]; r += (pk - s_gm[5]) * s_gi[5]; }
                for (int i = 0; i < 5; ++i) {
                    for (int j = 0; j < 5; ++j) s_A[i * 5 + j] = fma(w * s_dpeak[i], s_dpeak[j], s_A[i * 5 + j]);
                    s_g[i] = fma(-r, s_dpeak[i], s_g[i]);
                }
            }
        }
        __syncthreads();
    };

    const unsigned free0 = ~a.fixed & 31u;

    // ---- the start ----
    if (t < 5) s_rows[0][t] = s_p[t];
    if (t == 0) s_nfev = 1;
    __syncthreads();
    evaluate(1);
    if (t == 0) {
        s_Fcur = s_F[0];
        if (!lm_finite(s_F[0])) { s_status |= ST_START_INVALID; s_stop = 1; }
        else if (!free0) { s_status |= ST_ALL_FIXED; s_stop = 1; }
    }
    // the flags thread 0 keeps in LDS steer every thread's loops: each reads them into registers between two barriers,
    // so that no thread can still be looking at a flag when thread 0 writes it again
    int stop, moved;
    auto read_flags = [&]() __attribute__((always_inline)) { __syncthreads(); stop = s_stop; moved = s_moved; __syncthreads(); };
    read_flags();
    const bool searched = !stop;

    // ---- the search ----
    for (int it = 0; it < a.maxiter && !stop; ++it) {
        if (moved) jacobian(free0);
        if (t == 0) {
            ++s_niter;
            s_moved = 0;
            bool fin = true;
            for (int i = 0; i < 25; ++i) fin = fin && lm_finite(s_A[i]);
            for (int i = 0; i < 5; ++i) fin = fin && lm_finite(s_g[i]);
            s_active = fin ? lm_active(s_p, s_low, s_g, a.fixed) : 0u;
            // no direction left (every free parameter held on its limit): converged.  A row of the difference stencil
            // failed (the constructor found no merge point or no peak beside p): no Jacobian here, the search ends where
            // it is and says so
            if (!s_active) { s_status |= fin ? ST_CONV_F : ST_STENCIL_FAILED; s_stop = 1; }
        }
        read_flags();
        for (int tr = 0; tr < kTries && !stop && !moved; ++tr) {
            if (t == 0) lm_candidates(s_lam, s_nu, s_cand);
            __syncthreads();
            if (t < kCand) {
                s_solved[t] = lm_solve(s_A, s_g, s_cand[t], s_active, s_work[t], s_delta[t]);
                lm_project(s_p, s_delta[t], s_low, s_active, s_rows[t]);
                s_clipped[t] = lm_clipped(s_p, s_delta[t], s_low, s_active);
                s_pred[t] = lm_predicted(s_A, s_g, s_p, s_rows[t]);
                s_step[t] = lm_scaled_step(s_p, s_rows[t]);
            }
            if (t == 0) s_nfev += kCand;
            __syncthreads();
            evaluate(kCand);
            if (t == 0) {
                for (int c = 0; c < kCand; ++c) if (!s_solved[c] || !(s_pred[c] > 0.0)) s_F[c] = __builtin_inf();
                const int best = lm_pick(s_Fcur, s_F, kCand);
                // The boldest step says how much there is still to gain -- but only a step the projection left alone:
                // a step clipped onto a lower limit is not the model's minimiser, and its predicted reduction (often
                // negative) says nothing about convergence.  When every candidate is clipped or unsolved nothing is
                // concluded from this try: it is a rejection, lam rises, and shorter steps follow.
                double pmax = 0.0, smin = __builtin_inf();
                bool judged = false;
                for (int c = 0; c < kCand; ++c) {
                    if (!s_solved[c]) continue;
                    smin = fmin(smin, s_step[c]);
                    if (!s_clipped[c]) { pmax = fmax(pmax, s_pred[c]); judged = true; }
                }
                if (best >= 0) {
                    const double rho = lm_gain(s_Fcur, s_F[best], s_pred[best]);
                    for (int i = 0; i < 5; ++i) s_p[i] = s_rows[best][i];
                    lm_lambda_accept(s_cand[best], rho, &s_lam, &s_nu);
                    if (lm_converged_x(s_step[best], a.xtol)) { s_status |= ST_CONV_X; s_stop = 1; }
                    s_Fcur = s_F[best];
                    s_moved = 1;
                } else {
                    lm_lambda_reject(&s_lam, &s_nu);
                    if (lm_converged_x(smin, a.xtol)) { s_status |= ST_CONV_X; s_stop = 1; }
                }
                if (judged && lm_converged_f(pmax, s_Fcur, a.ftol)) { s_status |= ST_CONV_F; s_stop = 1; }
            }
            read_flags();
        }
    }
    if (t == 0 && searched && !(s_status & (ST_CONV_F | ST_CONV_X | ST_MAXITER | ST_STENCIL_FAILED))) s_status |= ST_MAXITER;
    __syncthreads();

    // ---- the Laplace covariance at the final point ----
    if (searched) {
        jacobian(free0);
        if (t == 0) {
            unsigned fr = 0;
            bool fin = true;
            for (int i = 0; i < 25; ++i) fin = fin && lm_finite(s_A[i]);
            for (int i = 0; i < 5; ++i) {
                if (s_p[i] <= s_low[i]) s_status |= 1 << (ST_LOWLIM_SHIFT + i);
                else if ((free0 >> i) & 1u) fr |= 1u << i;
            }
            if (!fin) fr = 0;
            if (!lm_laplace(s_A, fr, s_work[0], s_cov)) s_status |= ST_COV_SINGULAR;
        }
    } else if (t < 25) {
        s_cov[t] = __builtin_nan("");
    }
    __syncthreads();
    double *const od = a.outd + (size_t)blockIdx.x * kOutDoubles;
    if (t < 5) od[t] = s_p[t];
    if (t == 5) od[5] = s_Fcur;
    if (t >= 6 && t < 31) od[t] = s_cov[t - 6];
    if (t == 0) {
        int32_t *const oi = a.outi + (size_t)blockIdx.x * kOutInts;
        oi[0] = s_niter; oi[1] = s_nfev; oi[2] = s_status; oi[3] = 0;
    }
}

}   // namespace mbbmap
