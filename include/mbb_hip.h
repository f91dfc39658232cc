/*
 * mbb_hip.h -- C-ABI of the MI355X (gfx950) likelihood hot path.
 *
 * This is the drop-in boundary for the per-walker likelihood of mbb_emcee:
 * plain pointers and sizes, no C++ or framework types.  Every entry point
 * names the reference interface it replaces (paths relative to the
 * reference's mbb_emcee/ directory).  The reference-side binding (ctypes)
 * is shown in INTEGRATION.md; mbb_emcee_amd/_native.py is that binding.
 *
 * Conventions
 *   - all floating point data is IEEE float64, arrays are C-contiguous;
 *   - parameter rows are (T, beta, lambda0, alpha, fnorm)   likelihood.py:20-22;
 *   - the caller owns every buffer passed in; nothing is retained after return
 *     except what the set_* calls copy to the device;
 *   - functions return 0 on success, a negative mbb_error on failure, and never
 *     throw; mbb_last_error() gives the text of the last failure in this thread;
 *   - one context = one device + one HIP stream; a context is not thread-safe,
 *     any number of contexts may coexist;
 *   - per-row status codes (int32): see mbb_row_status.
 */
#ifndef MBB_HIP_H
#define MBB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mbb_ctx mbb_ctx;

enum mbb_error {
    MBB_OK = 0,
    MBB_ERR_HIP = -1,        /* a HIP runtime call failed (no GPU, OOM, ...) */
    MBB_ERR_ARG = -2,        /* invalid argument                             */
    MBB_ERR_STATE = -3,      /* bands / data not set yet                     */
    MBB_ERR_RCCL = -4        /* RCCL missing or a collective failed          */
};

/* Per-row outcome.  Rows with status >= 2 correspond to Python exceptions in
 * the reference's SED constructor (modified_blackbody.py:219-224, :294-316). */
enum mbb_row_status {
    MBB_ROW_OK = 0,
    MBB_ROW_BELOW_LOWLIM = 1, /* lnL = -inf          likelihood.py:806-807   */
    MBB_ROW_BAD_ALPHA = 2,    /* alpha <= 0          modified_blackbody.py:219 */
    MBB_ROW_BAD_BETA = 3,     /* beta < 0            modified_blackbody.py:222 */
    MBB_ROW_NOCONV = 6,       /* merge / peak root not found                 */
    MBB_ROW_NONFINITE = 7     /* NaN/inf parameter: lnL = NaN, as the reference; for the SED-level and chain
                               * calls also a row whose h/kT or normalisation is not finite (T = 0)   */
};

const char *mbb_last_error(void);
int mbb_device_count(void);

/* ---- context ----------------------------------------------------------- */
/* Replaces: construction of `likelihood` + `modified_blackbody` state
 * (likelihood.py:24-117).  opthin / noalpha / wavenorm as in likelihood.py:62-64. */
int mbb_ctx_create(int device, mbb_ctx **out);
void mbb_ctx_destroy(mbb_ctx *ctx);
int mbb_set_model(mbb_ctx *ctx, int opthin, int noalpha, double wavenorm);

/* Replaces: the per-band state built by response.setup (response.py:252-332)
 * and consumed by response.__call__ (response.py:572-576).
 *   freq   [offsets[nb]]  sample frequencies in GHz (response._freq)
 *   weight [offsets[nb]]  response._sedmult * response._normfac; a delta band
 *                         (response.py:336-374) or a plain photometric
 *                         wavelength (likelihood.py:817) is one sample, weight 1
 *   offsets[nb+1]         band b owns samples offsets[b] .. offsets[b+1]-1   */
int mbb_set_bands(mbb_ctx *ctx, const double *freq, const double *weight,
                  const int32_t *offsets, int nb);

/* Replaces: likelihood.set_phot / set_cov state (likelihood.py:158-232, :330-357).
 * is_cov == 0: w is ivar[nb] = 1/unc^2; is_cov != 0: w is inverse covariance [nb*nb]. */
int mbb_set_data(mbb_ctx *ctx, const double *flux, const double *w, int nb, int is_cov);

/* Batched multi-source mode (BASELINE.json configs[4]): nsrc independent SEDs
 * observed through the same bands, flux / ivar [nsrc*nb] (diagonal errors).
 * Afterwards a batch of n rows is read as nsrc groups of n/nsrc consecutive rows,
 * group g being compared with source g's data.  The reference fits one source
 * per process (likelihood.py:158-232 holds one flux vector); this is the same
 * likelihood applied to many. */
int mbb_set_data_multi(mbb_ctx *ctx, const double *flux, const double *ivar, int nb, int nsrc);

/* Replaces: _lowlim / _has_uplim / _uplim (likelihood.py:73, :83-85, :227-229);
 * index 5 is the lambda_peak ghost parameter (likelihood.py:710-715). */
int mbb_set_limits(mbb_ctx *ctx, const double lowlim[5], const int32_t has_uplim[6],
                   const double uplim[6]);
/* Replaces: Gaussian priors (likelihood.py:87-92, :513-541, :719-752). */
int mbb_set_gpriors(mbb_ctx *ctx, const int32_t has[6], const double mean[6],
                    const double ivar[6]);

/* ---- the hot path ------------------------------------------------------- */
/* Replaces: n calls of likelihood.__call__(pars) (likelihood.py:790-834), i.e.
 * what emcee's map(lnprobfn, rows) does per half-step (mbb_fit.py:80-81).
 * pars [n*5] host, lnl [n] host, status [n] host (may be NULL),
 * model_flux [n*nb] host (may be NULL).  Synchronous. */
int mbb_lnlike_batch(mbb_ctx *ctx, const double *pars, int n, double *lnl,
                     int32_t *status, double *model_flux);

/* The same boundary call with the copies taken out (what likelihood.__call__ uses for an (n, 5) array,
 * likelihood.py:790-834, once per emcee half-step).  mbb_boundary_buffers returns host addresses that hold
 * until more than nmax rows are asked for or the context goes: *in -- the caller writes its parameter rows
 * [n x 5] straight INTO it (device memory behind the PCIe BAR where there is a large BAR, else the pinned
 * block the kernel reads); *out / *status (may be NULL) -- pinned blocks the kernel writes lnprob [n] and row
 * status [n] to.  mbb_lnlike_call(ctx, n) evaluates the first n rows of *in: same kernel, same results as
 * mbb_lnlike_batch, bit for bit.  It returns MBB_OK, a negative error (MBB_ERR_STATE: ask for the buffers
 * again -- capacity or the zero_copy / bar_params options changed), or, positive, the row status of the first
 * row the reference would have raised ValueError for (2 alpha <= 0, 3 beta < 0, 6 no merge point:
 * modified_blackbody.py:219-224, :294-316); rows below a lower limit are -inf with status 1, as ever. */
int mbb_boundary_buffers(mbb_ctx *ctx, int nmax, double **in, double **out, int32_t **status);
int mbb_lnlike_call(mbb_ctx *ctx, int n);
/* The address of a word that lives as long as the context and changes whenever the blocks mbb_boundary_buffers
 * handed out are freed (ANY entry point of the context asked to hold more rows than they do: mbb_lnlike_batch,
 * mbb_lnlike_allgather, ...).  A binding that caches the addresses reads the word right after mbb_boundary_buffers
 * and compares it BEFORE every write through them; a different value means: ask for the buffers again. */
const unsigned long long *mbb_boundary_generation(mbb_ctx *ctx);

/* Same computation on device-resident buffers, enqueued on the context's
 * stream, asynchronous.  d_model_flux / d_status may be NULL. */
int mbb_lnlike_batch_device(mbb_ctx *ctx, const double *d_pars, int n,
                            double *d_lnl, int32_t *d_status, double *d_model_flux);

/* Measurement helper: the same launch enqueued `reps` times back to back from
 * C (no host work in between), so that HIP events around the call time the
 * kernel itself.  Asynchronous. */
int mbb_lnlike_repeat_device(mbb_ctx *ctx, const double *d_pars, int n, double *d_lnl,
                             int32_t *d_status, int reps);

/* Measurement helper (bench.py roofline): the sample arithmetic of
 * fnu.pyx:9-108 alone -- every wave of a chip-filling grid walks all passband
 * samples `reps` times with the constants of one parameter row; no prologue, no
 * reductions.  lane_slots = samples evaluated including chunk padding; clock_mhz (may be
 * NULL) = the shader clock the chip held meanwhile, s_memtime against the 100 MHz
 * s_memrealtime over workgroup 0's loop.  Synchronous. */
int mbb_roof_probe(mbb_ctx *ctx, const double pars[5], int reps, double *seconds,
                   double *lane_slots, double *clock_mhz);

/* ---- device-resident ensemble sampler ------------------------------------- */
/* Replaces: emcee.EnsembleSampler(nwalkers, 5, like).run_mcmc(p0, nsteps) as
 * driven by mbb_fitter.run (mbb_fit.py:80-81, :533, :542): the affine-invariant
 * stretch move (Goodman & Weare 2010) with the proposal, the fused likelihood
 * and the accept/reject step of a half-ensemble in ONE kernel launch, 2 nsteps
 * dependent launches per call and no host round trip in between.  emcee is not
 * part of the reference tree, so parity is statistical.
 * chain [nw][nsteps][5] and lnprob [nw][nsteps] use emcee's layout
 * (results.py:154-155).  After mbb_set_data_multi the sampler advances nsrc
 * independent ensembles of nwalkers each in the same launches; every array then
 * has a leading nsrc dimension.  "Fixed" parameters work as in the reference: a column
 * of p0 with zero scatter is preserved exactly by the stretch move
 * (mbb_fit.py:442-443), and the accept test's power of z is (columns of the ensemble
 * that are not constant over its walkers) - 1, counted by mbb_sampler_set_state: the
 * stretch move's Jacobian in the space the walkers span (the reference's dim - 1 = 4
 * widens the posterior of a fit with fixed parameters).  The sources of a multi-source
 * state must agree on that number (MBB_ERR_ARG otherwise). */
int mbb_sampler_create(mbb_ctx *ctx, int nwalkers, unsigned long long seed, void **sampler);
int mbb_sampler_destroy(mbb_ctx *ctx, void *sampler);
int mbb_sampler_reset(mbb_ctx *ctx, void *sampler);          /* zero the acceptance counts */
int mbb_sampler_set_state(mbb_ctx *ctx, void *sampler, const double *pos, const double *lnprob);
int mbb_sampler_run(mbb_ctx *ctx, void *sampler, int nsteps, double stretch_a, double *chain,
                    double *lnprob, double *pos_out, double *lnprob_out, double *naccepted);
int mbb_sampler_advance_async(mbb_ctx *ctx, void *sampler, int nsteps, double stretch_a);
/* The completion counters of the sampler's one-launch runs (the lag guard of sampler forms 7 and 9), one value per
 * counter, [2 sets][*ring][*shards] (cap >= 2 * ring * shards values; 128 is enough): read (store 0) or written
 * (store 1) with the stream idle; *next_set is the set the next launch uses.  MBB_ERR_STATE when the sampler's last run
 * was not of such a form.  A test hook; no reference counterpart. */
int mbb_sampler_flow_counters(mbb_ctx *ctx, void *sampler, unsigned long long *counters, int cap, int store, int *ring,
                              int *shards, int *next_set);
/* Measurement helper (bench.py's timed region on one GPU): nsteps steps as mbb_sampler_advance_async
 * enqueues them, bracketed inside ONE call by the host clock and by two events on the context's stream,
 * recorded right before the run's first launch and right behind its last: clock; enqueue; stream wait; clock.
 * The stream must be idle on entry (mbb_sync before).  wall_s = host seconds from before the enqueue to after
 * the wait; stream_ms = between the events.  No reference counterpart. */
int mbb_sampler_advance_timed(mbb_ctx *ctx, void *sampler, int nsteps, double stretch_a, double *wall_s,
                              float *stream_ms);

/* ---- posterior summaries of a chain, computed where the chain is ---------- */
/* Replaces: what mbb_results makes of a chain (results.py): _parcen_internal (:314-369: mean and
 * numpy.percentile of the flattened chain, optionally clipped to [lowlim, uplim]) behind par_cen, peaklambda_cen,
 * lir_cen and dustmass_cen (:397-431, :507-532, :600-625, :699-724); par_lowlim / par_uplim (:433-493); the best
 * fit of process_fit (:160-165: lnprobability.argmax(), ties to the smallest flat index); compute_peaklambda,
 * compute_lir and compute_dustmass (:570-581, :627-674, :746-801) for the derived columns.
 * Columns ("slots") of a summary: 0-4 the parameters, 5 peak wavelength [um], 6 L_IR [1e12 L_sun], 7 dust mass
 * [1e8 M_sun].  A column's samples are steps burn, burn + thin, ... of every walker.  Percentiles are numpy's
 * (method "linear") of EXACT order statistics; all sums are fixed-order trees, so a chain gives the same bits
 * every time.  Covariance (numpy.cov of the five parameters, ddof 1) and best fit are over the same window,
 * unclipped.
 * L_IR and dust mass need a redshift and a luminosity distance: one of each for the whole call (redshift,
 * lumdist_mpc -- what the reference has, one object per results file), or, for a catalogue of sources fitted in one
 * launch, one per source (src_redshift, src_lumdist_mpc).  There is no cosmology here: distances are passed in.  No
 * reference counterpart for the per-source form. */
#define MBB_SUMMARY_COLS 8
#define MBB_SUMMARY_MAX_PCT 8
enum mbb_summary_derived { MBB_SUM_PEAK = 1, MBB_SUM_LIR = 2, MBB_SUM_DUSTMASS = 4 };
/* status of a column: bits */
enum mbb_summary_status {
    MBB_SUM_EMPTY = 1,        /* no sample survives the clipping: n_used 0, mean and percentiles NaN          */
    MBB_SUM_HAS_NAN = 2,      /* the column holds a NaN: mean and percentiles NaN, as numpy's                 */
    MBB_SUM_ABSENT = 4,       /* a derived column that was not asked for                                      */
    MBB_SUM_ROW_SHIFT = 8     /* bit 8 + s: a sample's SED kernel row had mbb_row_status s (derived columns)  */
};
typedef struct mbb_summary_spec {
    int32_t npct;                          /* percentiles asked for, 1..MBB_SUMMARY_MAX_PCT                   */
    int32_t burn, thin;                    /* window: steps burn <= t < nsteps, every thin-th                 */
    int32_t derived;                       /* mbb_summary_derived bits                                        */
    int32_t peak_model;                    /* 0: the fit's own model; 1: optically thick with alpha, which is
                                              what compute_peaklambda evaluates whatever the fit (:574-581)   */
    int32_t has_lo[MBB_SUMMARY_COLS], has_hi[MBB_SUMMARY_COLS];   /* clip a column: keep lo <= x <= hi       */
    double pct[MBB_SUMMARY_MAX_PCT];       /* numpy's q in [0, 100]                                           */
    double lo[MBB_SUMMARY_COLS], hi[MBB_SUMMARY_COLS];
    double redshift, lumdist_mpc;          /* for L_IR and dust mass                                          */
    double kappa, kappa_wave;              /* dust mass (results.py:746: 2.64 m^2/kg at 125 um)               */
    double lir_wavemin, lir_wavemax;       /* rest-frame range of L_IR in um (results.py:627: 8, 1000)       */
    /* A redshift and a luminosity distance per source, for a catalogue: host arrays [nsrc], both or neither (NULL:
     * the two scalars above serve every source; exactly one NULL is MBB_ERR_ARG).  When given, the scalars are
     * ignored and the L_IR and dust-mass columns of source s are computed with entry s.  An entry is finite with
     * redshift > -1 and distance > 0, or NaN: unknown for this source, whose L_IR and dust-mass columns are then
     * NaN in every cell (MBB_SUM_HAS_NAN, NaN mean and percentiles) while its other columns and all other sources
     * are as ever.  Anything else is MBB_ERR_ARG, the message naming the first such source, before anything is
     * allocated, uploaded or launched.  Looked at only when MBB_SUM_LIR or MBB_SUM_DUSTMASS is asked for; read
     * during the call only.  Clip bounds, kappa, kappa_wave and the L_IR range stay one per call. */
    double *src_redshift, *src_lumdist_mpc;
} mbb_summary_spec;
/* Where a summary goes; every pointer is the caller's, host memory, required. */
typedef struct mbb_summary_out {
    int64_t *n_used;                       /* [nsrc][8]                                                       */
    double *mean, *min, *max;              /* [nsrc][8]                                                       */
    double *pct;                           /* [nsrc][8][npct]                                                 */
    int32_t *status;                       /* [nsrc][8] mbb_summary_status bits                               */
    double *cov;                           /* [nsrc][5][5]                                                    */
    double *best;                          /* [nsrc][6]: the best sample's parameters and lnprob, bit for bit */
    int32_t *best_index;                   /* [nsrc][2]: its walker and step                                  */
} mbb_summary_out;
/* A host chain in emcee's layout, chain [nsrc][nw][nsteps][5] and lnprob [nsrc][nw][nsteps]: upload, summarise on
 * the device, download the summary.  The model flags of the context (mbb_set_model) are the derived columns'. */
int mbb_chain_summary(mbb_ctx *ctx, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                      const mbb_summary_spec *spec, const mbb_summary_out *out);
/* mbb_sampler_run that keeps the chain on the device, summarises it there and copies back the summary and the
 * final ensemble: same run plan, same forms, same redo of a one-launch run that gave up as mbb_sampler_run, so
 * the chain summarised is bit for bit the one mbb_sampler_run returns.  chain / lnprob may be NULL (then no chain
 * crosses the bus) or given to get the chain as well.  nsteps == 0 runs nothing and summarises again, with
 * another spec, the chain the last call with nsteps > 0 left on the device (MBB_ERR_STATE when there is none).
 * A sharded run (a communicator or the one-hop exchange with more than one rank) is refused with
 * MBB_ERR_STATE: a rank holds only its own walkers' chain. */
int mbb_sampler_run_summary(mbb_ctx *ctx, void *sampler, int nsteps, double stretch_a,
                            const mbb_summary_spec *spec, const mbb_summary_out *out, double *chain,
                            double *lnprob, double *pos_out, double *lnprob_out, double *naccepted);

/* ---- convergence diagnostics of a chain, computed where the chain is ------ */
/* Replaces: sampler.acor as the fit driver prints it (mbb_fit.py:548-561), for every source of a catalogue fit and
 * without the chain on the host.  Per (source, parameter), over the steps burn <= t < nsteps (n of them):
 *   tau, window  the integrated autocorrelation time with Sokal's automatic window: rho_k = c_k / c_0 with
 *                c_k = sum_{i < n - k} y_i y_{i+k} of the centred series y, tau(m) = 2 sum_{k <= m} rho_k - 1,
 *                window M = the first m with m >= c tau(m), else n - 1; tau = tau(M).
 *                MBB_DIAG_MEAN: the series is the ensemble mean over walkers at each step.
 *                MBB_DIAG_WALKERS: each walker's own rho_k, averaged over walkers, windowed once (emcee >= 3).
 *   ess          nw n / tau
 *   rhat         split R-hat (Gelman & Rubin, not rank-normalised): every walker's first and last h = n / 2 kept
 *                steps are 2 nw sequences; W the mean of their variances (ddof 1), B = h var(their means) (ddof 1),
 *                R = sqrt(((h - 1) / h W + B / h) / W); NaN when h < 2.
 *   acf          rho_0 .. rho_{nacf-1}
 * All sums are fixed-order: a chain gives the same bits every time, resident or uploaded.  A series may have
 * MBB_DIAG_MAX_STEPS kept steps; a longer one is MBB_ERR_ARG. */
#define MBB_DIAG_MAX_STEPS 16384
enum mbb_diag_method { MBB_DIAG_MEAN = 0, MBB_DIAG_WALKERS = 1 };
/* status of a (source, parameter): bits */
enum mbb_diag_status {
    MBB_DIAG_SHORT = 1,       /* fewer than 8 kept steps: tau, ess NaN, window -1                                  */
    MBB_DIAG_CONSTANT = 2,    /* the series (MEAN) or a walker's series (WALKERS) is constant, or c_0 <= 0: a fixed
                                 parameter; tau, ess NaN, window -1                                                  */
    MBB_DIAG_HAS_NAN = 4,     /* the column holds a NaN or an infinity inside the window: tau, ess NaN, window -1   */
    MBB_DIAG_UNRELIABLE = 8   /* the chain is shorter than tol tau                                                  */
};
typedef struct mbb_diag_spec {
    int32_t burn;                          /* window: steps burn <= t < nsteps                                */
    int32_t method;                        /* mbb_diag_method                                                 */
    int32_t nacf;                          /* values of rho wanted, 0 .. nsteps - burn                        */
    double c;                              /* Sokal's window factor (emcee: 5)                                */
    double tol;                            /* MBB_DIAG_UNRELIABLE below tol tau kept steps (emcee: 50)        */
} mbb_diag_spec;
/* Where diagnostics go; every pointer is the caller's, host memory; acf may be NULL. */
typedef struct mbb_diag_out {
    double *tau, *ess, *rhat;              /* [nsrc][5]                                                       */
    int32_t *window, *status;              /* [nsrc][5]: M, mbb_diag_status bits                              */
    double *acf;                           /* [nsrc][5][nacf] or NULL                                         */
} mbb_diag_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5]: upload, diagnose on the device, download the result. */
int mbb_chain_diagnostics(mbb_ctx *ctx, const double *chain, int nsrc, int nw, int nsteps,
                          const mbb_diag_spec *spec, const mbb_diag_out *out);
/* The same of the chain the sampler's last stored or summarised run (mbb_sampler_run with a chain or lnprob
 * array, mbb_sampler_run_summary) left on the device.  MBB_ERR_STATE when there is none, and for a sharded run (a
 * communicator or the one-hop exchange with more than one rank): a rank holds only its own walkers' chain. */
int mbb_sampler_diagnostics(mbb_ctx *ctx, void *sampler, const mbb_diag_spec *spec, const mbb_diag_out *out);

/* ---- binned posterior marginals of a chain, computed where the chain is ---- */
/* Replaces: numpy.histogram / numpy.histogram2d (or corner) on mbb_results.parameter_chain, which is how a user of
 * the reference gets per-parameter PDFs and the T-beta contours: the reference has no code for it.  Per (source,
 * column slot of a summary) a histogram of nbins bins; per (source, requested pair of slots a < b) a table of
 * nbins2 x nbins2 bins, [bin of a][bin of b].  A column's samples are a summary's: steps burn, burn + thin, ... of
 * every walker; the derived columns are the summary's, with the summary spec's settings.
 *   range   given (has_range[slot]): lo[slot], hi[slot], one pair for every source; else per source the min and max
 *           of the column's finite samples, min - 0.5 and max + 0.5 when they are equal (numpy.histogram's rule)
 *   edges   numpy.linspace(lo, hi, nbins + 1) bit for bit: e[i] = i * ((hi - lo) / nbins) + lo, the product and the sum
 *           rounded separately, e[nbins] = hi
 *   bins    x is counted in bin i iff e[i] <= x < e[i + 1]; the last bin also takes x == hi.  The comparisons decide.
 *   below lo, above hi, not finite (NaN, +-inf): counted in n_below, n_above, n_nonfinite, never binned;
 *           n_used is the number binned, and the four add up to the samples of the column
 *   2-D     over the two columns' own ranges and numpy.linspace(lo, hi, nbins2 + 1): a sample is counted when it is
 *           binned in both; numpy.histogram2d's [i][j]
 * Counts are exactly numpy's.  All accumulation is integer: a chain gives the same bits every time.  A column may
 * have 2^32 - 1 samples. */
#define MBB_MARG_MAX_BINS 4096
#define MBB_MARG_MAX_BINS2 100
#define MBB_MARG_MAX_PAIRS 28
/* status of a column: bits (MBB_MARG_EMPTY, _ABSENT and the row shift are the summary's values) */
enum mbb_marginals_status {
    MBB_MARG_EMPTY = 1,       /* no finite sample: all counts 0, NaN edges                                         */
    MBB_MARG_NONFINITE = 2,   /* the column holds a NaN or an infinity inside the window (n_nonfinite > 0)         */
    MBB_MARG_ABSENT = 4,      /* a derived column that was not asked for: all counts 0, NaN edges                  */
    MBB_MARG_ROW_SHIFT = 8    /* bit 8 + s: a sample's SED kernel row had mbb_row_status s (derived columns)       */
};
typedef struct mbb_marginals_spec {
    int32_t nbins;                         /* 1 .. MBB_MARG_MAX_BINS                                          */
    int32_t nbins2;                        /* 0 .. MBB_MARG_MAX_BINS2 per axis; 0: no 2-D tables               */
    int32_t npairs;                        /* 0 .. MBB_MARG_MAX_PAIRS (0 when nbins2 is 0)                     */
    int32_t pairs[MBB_MARG_MAX_PAIRS][2];  /* slots (a, b), a < b, both columns present                       */
    int32_t has_range[MBB_SUMMARY_COLS];
    double lo[MBB_SUMMARY_COLS], hi[MBB_SUMMARY_COLS];   /* finite, lo < hi, hi - lo finite                    */
    /* burn, thin, derived, peak_model, redshift / lumdist_mpc (scalar or per source), kappa, kappa_wave and the L_IR
     * range are taken from here; its percentiles and clips are ignored.  Required. */
    const mbb_summary_spec *summary;
} mbb_marginals_spec;
/* Where marginals go; every pointer is the caller's, host memory, required (counts2 and edges2 unless nbins2 or
 * npairs is 0). */
typedef struct mbb_marginals_out {
    uint32_t *counts1;                     /* [nsrc][8][nbins]                                                */
    double *edges1;                        /* [nsrc][8][nbins + 1]                                            */
    uint32_t *counts2;                     /* [nsrc][npairs][nbins2][nbins2]                                  */
    double *edges2;                        /* [nsrc][8][nbins2 + 1]                                           */
    int64_t *n_used, *n_below, *n_above, *n_nonfinite;   /* [nsrc][8]                                        */
    int32_t *status;                       /* [nsrc][8] mbb_marginals_status bits                             */
} mbb_marginals_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5]: upload, bin on the device, download the tables.  Arguments
 * are checked before anything is uploaded (MBB_ERR_ARG with a message). */
int mbb_chain_marginals(mbb_ctx *ctx, const double *chain, int nsrc, int nw, int nsteps,
                        const mbb_marginals_spec *spec, const mbb_marginals_out *out);
/* The same of the chain the sampler's last stored or summarised run left on the device.  MBB_ERR_STATE when there is
 * none, and for a sharded run, as mbb_sampler_diagnostics. */
int mbb_sampler_marginals(mbb_ctx *ctx, void *sampler, const mbb_marginals_spec *spec, const mbb_marginals_out *out);

/* ---- predicted fluxes of a chain, computed where the chain is ---- */
/* Replaces: mbb_results.predflux_cen (results.py:895-985): the model flux of every chain entry at a wavelength or
 * through a passband, then _parcen_internal's mean and percentiles of that column.  A prediction target ("spec") is a
 * list of quadrature samples (frequency in GHz, weight): a passband's samples with weight sedmult * normfac
 * (response.py:575-576), or the single sample (um_to_GHz / lambda, 1) of a wavelength or a delta-function band.  Spec
 * s has samples sample_off[s] <= i < sample_off[s + 1] of freq[] and weight[].
 *   value   of (chain row, spec): a single sample of weight 1 gives f_nu at that frequency itself, the bits
 *           mbb_sed_eval_batch gives; any other list gives sum_i f_nu(freq_i) weight_i, summed in a fixed order
 *   model   the context's (mbb_set_model); wavenorm the spec's, or the context's when that is 0
 *   window, statistics, percentiles, clip, status bits: a summary column's (mbb_summary_spec), per (source, spec); a
 *           chain row the SED constructor fails on gives NaN and its row-status bit when it is inside the window
 * A spec's results do not depend on the other specs of the call, nor on whether the chain was uploaded or resident:
 * the same chain gives the same bits.  Columns are made three at a time, whatever nspec is: a call needs the memory of
 * three columns.  A column may have 2^32 - 1 samples. */
#define MBB_PRED_MAX_SPECS 128        /* specs per call                                                       */
#define MBB_PRED_MAX_SAMPLES 32768    /* quadrature samples per call, all specs together                      */
typedef struct mbb_predict_spec {
    int32_t nspec;                         /* 1 .. MBB_PRED_MAX_SPECS                                         */
    int32_t npct;                          /* 1 .. MBB_SUMMARY_MAX_PCT                                        */
    int32_t burn, thin;                    /* window: steps burn, burn + thin, ...                            */
    const int32_t *sample_off;             /* [nspec + 1], sample_off[0] = 0, strictly increasing             */
    const double *freq, *weight;           /* [sample_off[nspec]]: finite and > 0; finite                     */
    double pct[MBB_SUMMARY_MAX_PCT];       /* numpy's q, 0 .. 100                                             */
    double wavenorm;                       /* normalisation wavelength [um] of the SED; 0: the context's      */
    const int32_t *has_lo, *has_hi;        /* [nspec] each, or all four NULL: no clip                         */
    const double *lo, *hi;                 /* [nspec]: samples with lo <= x <= hi are used                    */
} mbb_predict_spec;
/* Where predictions go; every pointer is the caller's, host memory, required. */
typedef struct mbb_predict_out {
    int64_t *n_used;                       /* [nsrc][nspec]                                                   */
    double *mean, *min, *max;              /* [nsrc][nspec]                                                   */
    double *pct;                           /* [nsrc][nspec][npct]                                             */
    int32_t *status;                       /* [nsrc][nspec] mbb_summary_status bits (never MBB_SUM_ABSENT)    */
} mbb_predict_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5]: upload, predict on the device, download the results.
 * Arguments are checked before anything is allocated, uploaded or launched (MBB_ERR_ARG with a message). */
int mbb_chain_predict(mbb_ctx *ctx, const double *chain, int nsrc, int nw, int nsteps,
                      const mbb_predict_spec *spec, const mbb_predict_out *out);
/* The same of the chain the sampler's last stored or summarised run left on the device.  MBB_ERR_STATE when there is
 * none, and for a sharded run, as mbb_sampler_diagnostics. */
int mbb_sampler_predict(mbb_ctx *ctx, void *sampler, const mbb_predict_spec *spec, const mbb_predict_out *out);

/* ---- posterior draws of a chain, taken where the chain is ---- */
/* Replaces: mbb_results.choice() (results.py:803-893): nsamples cells of the chain, uniform over walkers x steps with
 * replacement, with their peak wavelength, L_IR and dust mass.  Per source n cells of the window (steps burn, burn +
 * thin, ... of every walker: N = nw * nkept cells, cell j = walker j / nkept, step burn + (j % nkept) thin) are picked
 * and their rows, lnprob and (walker, step) gathered on the device; the derived columns are computed for the drawn
 * rows alone, by the kernels and with the settings of a summary, so a drawn row's derived values and status bits are
 * those a summary of that one cell reports.  Draw i of source s picks
 *   MBB_DRAWS_RANDOM  j = (u N) >> 64, u = out[0] | out[1] << 32 of Philox4x32-10 with counter (i, s, 0x44524157, 1)
 *                     and key (seed low, seed high): the reference's semantics; apart from every stretch-move draw of
 *                     the same seed (counters (row, half, 0, 0))
 *   MBB_DRAWS_EVEN    j = floor(i N / n): deterministic, spread over the window, no repeats while n <= N
 * Rows and lnprob are copies of the chain's, bit for bit.  The same chain, spec and seed give the same draws, resident
 * or uploaded. */
#define MBB_DRAWS_MAX (1 << 24)       /* draws per source and call; nsrc * n may be 2^31 - 1 at most              */
enum mbb_draws_how { MBB_DRAWS_RANDOM = 0, MBB_DRAWS_EVEN = 1 };
typedef struct mbb_draws_spec {
    int32_t n;                             /* draws per source, 1 .. MBB_DRAWS_MAX                            */
    int32_t how;                           /* mbb_draws_how                                                   */
    uint64_t seed;
    /* burn, thin, derived, peak_model, redshift / lumdist_mpc (scalar or per source), kappa, kappa_wave and the L_IR
     * range are taken from here; its percentiles and clips are ignored.  Required. */
    const mbb_summary_spec *summary;
} mbb_draws_spec;
/* Where draws go; every pointer is the caller's, host memory, required (derived[k] only where bit k of the summary
 * spec's derived is set; others are not written and may be NULL). */
typedef struct mbb_draws_out {
    double *rows;                          /* [nsrc][n][5]                                                    */
    double *lnprob;                        /* [nsrc][n]; NaN when no lnprob was given                         */
    int32_t *index;                        /* [nsrc][n][2]: walker, step                                      */
    double *derived[3];                    /* [nsrc][n] each: peak wavelength, L_IR, dust mass                */
    int32_t *status;                       /* [nsrc][8]: from MBB_SUM_ROW_SHIFT on the row status of drawn rows the
                                              SED kernels failed on, per derived column, as a summary reports them;
                                              MBB_SUM_ABSENT for a derived column not asked for                */
} mbb_draws_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5], lnprob [nsrc][nw][nsteps] or NULL: upload, draw on the
 * device, download the draws.  Arguments are checked before anything is allocated, uploaded or launched. */
int mbb_chain_draws(mbb_ctx *ctx, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                    const mbb_draws_spec *spec, const mbb_draws_out *out);
/* The same of the chain (and its lnprob) the sampler's last stored or summarised run left on the device.
 * MBB_ERR_STATE when there is none, and for a sharded run, as mbb_sampler_diagnostics. */
int mbb_sampler_draws(mbb_ctx *ctx, void *sampler, const mbb_draws_spec *spec, const mbb_draws_out *out);
/* The picks alone, index [nsrc][n][2] (walker, step), with no chain: for a chain the caller holds on the host. */
int mbb_draw_indices(mbb_ctx *ctx, int nsrc, int nw, int nsteps, int burn, int thin, int n, int how,
                     unsigned long long seed, int32_t *index);

/* ---- goodness of fit of a chain, computed where the chain is ---- */
/* New: the reference has nothing comparable (its "ChiSquare of best fit point" is -2 lnprob, which carries the soft
 * upper walls and the Gaussian priors: results.py:261-272, likelihood.py:672-752).  Everything is per source, over a
 * summary's window: steps burn, burn + thin, ... of every walker.
 *   chisq   of a chain row theta: sum_b (f_b - m_b(theta))^2 ivar_b, or r^T C^-1 r with r = f - m when the data has a
 *           covariance matrix; m_b the model flux through band b of the context (mbb_set_bands' samples, mbb_set_model),
 *           f, ivar, C^-1 the context's data (mbb_set_data, mbb_set_data_multi).  Defined for every row the SED
 *           constructor succeeds on, whatever the limits and priors are: a row below a lower limit has one.  A row the
 *           constructor fails on gives NaN and its row-status bit when it is inside the window.
 *   q       = Q(nb/2, chisq/2), Q the regularised upper incomplete gamma function, nb the number of bands: the
 *           probability that data replicated from the model at theta with the stated errors has a larger chisq.  Its
 *           posterior mean is the posterior predictive p-value of the chisq discrepancy.  chisq <= 0 gives 1, +inf 0,
 *           NaN NaN.
 *   columns slot 0 is chisq, slot 1 is q: n_used, mean, min, max, numpy-linear percentiles of exact order statistics
 *           and mbb_summary_status bits, as a summary column without clipping.
 *   at_mean theta-bar, the window's mean of each parameter column (the bits a summary of the same window with neither
 *           clipping nor derived columns reports as mean[0:5]; a summary with derived columns may split its sums
 *           otherwise and differ in the last bits), then chisq(theta-bar) and q(theta-bar).
 *   ml      the window's entry of smallest chisq, ties to the smallest index in [walker][step] order; a NaN never
 *           wins: its parameters (the chain's bits), chisq, q; ml_index (walker, step); ml_model its nb band fluxes.
 *           All NaN and index -1 when every entry is NaN.
 *   best    chisq and q of the window's entry of largest lnprob, best_index the summary's; NaN and -1 without lnprob.
 * A row's chisq and q are the same bits whatever the call's shape and wherever the chain came from.  The chain's nsrc
 * is the context's, or the context holds one source, which then serves every source of the chain; at most 256 bands. */
typedef struct mbb_goodness_spec {
    int32_t npct;                          /* 1 .. MBB_SUMMARY_MAX_PCT                                        */
    int32_t burn, thin;                    /* window: steps burn, burn + thin, ...                            */
    double pct[MBB_SUMMARY_MAX_PCT];       /* numpy's q, 0 .. 100                                             */
} mbb_goodness_spec;
/* Where the results go; every pointer is the caller's, host memory, required. */
typedef struct mbb_goodness_out {
    int64_t *n_used;                       /* [nsrc][2]                                                       */
    double *mean, *min, *max;              /* [nsrc][2]                                                       */
    int32_t *status;                       /* [nsrc][2] mbb_summary_status bits (never MBB_SUM_ABSENT)        */
    double *pct;                           /* [nsrc][2][npct]                                                 */
    double *at_mean;                       /* [nsrc][7] theta-bar, chisq, q                                   */
    double *ml;                            /* [nsrc][7] parameters, chisq, q                                  */
    int32_t *ml_index;                     /* [nsrc][2] walker, step                                          */
    double *ml_model;                      /* [nsrc][nb]                                                      */
    double *best;                          /* [nsrc][2] chisq, q                                              */
    int32_t *best_index;                   /* [nsrc][2] walker, step                                          */
} mbb_goodness_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5], its lnprob [nsrc][nw][nsteps] or NULL: upload, work on the
 * device, download the results.  Arguments are checked before anything is allocated, uploaded or launched:
 * MBB_ERR_STATE with no bands or data set, MBB_ERR_ARG otherwise, with a message. */
int mbb_chain_goodness(mbb_ctx *ctx, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                       const mbb_goodness_spec *spec, const mbb_goodness_out *out);
/* The same of the chain the sampler's last stored or summarised run left on the device.  MBB_ERR_STATE when there is
 * none, and for a sharded run, as mbb_sampler_predict. */
int mbb_sampler_goodness(mbb_ctx *ctx, void *sampler, const mbb_goodness_spec *spec, const mbb_goodness_out *out);
/* chisq, q and the row status of n parameter rows, and their band fluxes model_flux [n*nb] unless NULL: the device
 * function the chain's entries go through.  Rows are grouped by source as for mbb_lnlike_batch. */
int mbb_goodness_rows(mbb_ctx *ctx, const double *pars, int n, double *chisq, double *q, int32_t *status,
                      double *model_flux);

/* ---- out-of-sample fit of a chain: WAIC and PSIS-LOO per source and band ---- */
/* New: the reference has nothing comparable.  Everything is per source and per band b of the context, over a summary's
 * window: steps burn, burn + thin, ... of every walker, in [walker][step] order, which is the window index below.
 * r = f - m(theta), m the band fluxes exactly as mbb_goodness_rows returns them; Lambda = C^-1 when the data has a
 * covariance and diag(ivar) otherwise; g = Lambda r.
 *   ll_b(theta) = (ln Lambda_bb - ln 2 pi) / 2 - g_b^2 / (2 Lambda_bb)
 *           = ln p(f_b | f_-b, theta), the conditional Gaussian (Buerkner, Gabry & Vehtari 2021); without a covariance
 *           the usual -r_b^2 ivar_b / 2 + ln(ivar_b / 2 pi) / 2.  It knows no limits or priors, like chisq.  A row the
 *           SED constructor fails on gives NaN in every band and its row-status bit when it is inside the window.
 * With S the window's entries of finite ll_b:
 *   n_used = S;  lppd = LSE_s ll - ln S;  p_waic = var(ll), ddof 1, in two passes (NaN for S < 2);
 *   elpd_waic = lppd - p_waic.
 * PSIS (Vehtari, Simpson, Gelman, Yao & Gabry; `loo` 2.x psislw): lw = -ll - max(-ll); M = ceil(min(0.2 S, 3 sqrt S));
 * the tail is the M entries largest in (lw, window index) order, the cutoff c the largest lw not in it;
 * x_i = exp(lw_i) - exp(c) ascending; (k, sigma) by Zhang & Stephens (2009): m = 30 + floor(sqrt M),
 * x* = x[floor(M/4 + 1/2)] (1-based), theta_j = 1/x_M + (1 - sqrt(m / (j - 1/2))) / (3 x*), k_j = mean log1p(-theta_j x),
 * l_j = M (ln(-theta_j / k_j) - k_j - 1), w = softmax(l) (maximum subtracted), theta^ = sum theta_j w_j,
 * k = mean log1p(-theta^ x), sigma = -k / theta^, k^ = (k M + 5) / (M + 10).  The tail entry of ascending rank i gets
 * lw = ln(sigma expm1(-k^ log1p(-p_i)) / k^ + exp(c)), p_i = (i - 1/2) / M; every lw is capped at 0.
 * The raw lw are kept (truncated importance sampling) and k^ = +inf when M < 5 (S <= 20: MBB_PW_TAIL_SHORT), or the
 * tail is constant, x* <= 0, or any of k, sigma, k^ is not finite (MBB_PW_TAIL_FLAT).
 *   elpd_loo = LSE(ll + lw) - LSE(lw);  p_loo = lppd - elpd_loo;
 *   loo_pit = sum_s w^_s Phi(g_b / sqrt Lambda_bb), w^ the normalised weights: the leave-one-band-out probability that
 *           a replicated flux lies below the measured one (Phi through erfc);  tail_len = M.
 * Every sum has a fixed order, the tail's ascending; a row's ll is the same bits whatever the call's shape; the results
 * do not depend on how many bands are worked on at a time (option "pointwise_budget_mb").  At most 256 bands.  The tail
 * is sorted by one workgroup: a window of more than MBB_PW_MAX_WINDOW entries per source is MBB_ERR_ARG. */
#define MBB_PW_TAIL_MAX 4096
#define MBB_PW_MAX_WINDOW 1864135          /* the largest S with ceil(3 sqrt S) <= MBB_PW_TAIL_MAX */
enum mbb_pointwise_status {                /* beside the mbb_summary_status bits EMPTY, HAS_NAN (entries left out), ROW_SHIFT */
    MBB_PW_K_HIGH = 16,                    /* k^ > 0.7 (a fallback's +inf included)                            */
    MBB_PW_TAIL_SHORT = 32,
    MBB_PW_TAIL_FLAT = 64,
    MBB_PW_WAIC_VAR_HIGH = 128             /* p_waic > 0.4                                                     */
};
typedef struct mbb_pointwise_spec {
    int32_t burn, thin;                    /* window: steps burn, burn + thin, ...                            */
} mbb_pointwise_spec;
/* Where the results go: [nsrc][nb] each; every pointer is the caller's, host memory, required. */
typedef struct mbb_pointwise_out {
    int64_t *n_used;
    int32_t *tail_len, *status;
    double *lppd, *p_waic, *elpd_waic, *elpd_loo, *p_loo, *khat, *loo_pit;
} mbb_pointwise_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5].  Arguments are checked before anything is allocated, uploaded
 * or launched: MBB_ERR_STATE with no bands or data set, MBB_ERR_ARG otherwise, with a message. */
int mbb_chain_pointwise(mbb_ctx *ctx, const double *chain, int nsrc, int nw, int nsteps, const mbb_pointwise_spec *spec,
                        const mbb_pointwise_out *out);
/* The same of the chain the sampler's last stored or summarised run left on the device.  MBB_ERR_STATE when there is
 * none, and for a sharded run, as mbb_sampler_goodness. */
int mbb_sampler_pointwise(mbb_ctx *ctx, void *sampler, const mbb_pointwise_spec *spec, const mbb_pointwise_out *out);
/* ll [n][nb] and the row status of n parameter rows: the device function the chain's entries go through.  Rows are
 * grouped by source as for mbb_lnlike_batch. */
int mbb_pointwise_rows(mbb_ctx *ctx, const double *pars, int n, double *ll, int32_t *status);

/* ---- the maximum of the posterior, found on the device ---- */
/* New: the reference has no optimiser; its "best fit" is the chain entry of largest lnprob (results.py:160-165).
 * -2 ln P is a sum of squares -- the data term, one square per soft upper wall that is exceeded, one per Gaussian prior
 * (likelihood.py:672-752, :790-834) -- behind the hard lower limits, so a Levenberg-Marquardt search with projection
 * onto the lower limits finds its minimum.  One workgroup runs the whole search of one (source, start) inside one
 * launch (csrc/mbb_map.hip.h; the step logic is csrc/mbb_lm.hip.h); several starts per source because the optically
 * thick models without a prior on lambda0 have more than one optimum.
 *   start    [nsrc][nstart][5]; fixed[i] != 0 holds parameter i at its start value; lambda0 of an optically thin model
 *            and alpha of a model without one never move.  The kernel draws nothing.
 *   stopping predicted reduction of -2 ln P <= ftol max(1, -2 ln P) (MBB_MAP_CONVERGED_F); largest step of a
 *            parameter relative to its value <= xtol (MBB_MAP_CONVERGED_X); maxiter iterations (MBB_MAP_MAXITER).
 *            The predicted reduction is that of a step the projection onto the lower limits left alone: while every
 *            candidate step is clipped onto a limit nothing is concluded, the damping rises and shorter steps follow.
 *            ftol and xtol are finite and >= 0 (0: that test never stops the search).
 *   lnprob   the final points of all (source, start) go through mbb_lnlike_batch's own path, so lnprob_all is bit for
 *            bit what that call gives for params_all; per source the start of largest lnprob is picked, ties to the
 *            lowest index, a NaN never wins (all NaN: index 0).
 *   chisq, q, model_flux   of the picked points, by mbb_goodness_rows' path: its bits.
 *   cov      the Laplace covariance at the picked optimum: the inverse of J^T J (J the Jacobian of the residuals) over
 *            the parameters that are free and off their lower limit, NaN in the rows and columns of the others; all
 *            NaN with MBB_MAP_COV_SINGULAR when that matrix is not positive definite.
 * A start whose lnprob is -inf or NaN (below a lower limit, a failing SED constructor) is MBB_MAP_START_INVALID: its
 * result is the start itself, zero iterations.  A source's result has the same bits whatever other sources or starts
 * the call holds.  nsrc is the context's, or the context holds one source whose data then serves all; at most 256
 * bands; a context that is one rank of a sharded run (mbb_comm_init, mbb_xchg_connect with more than one rank) is
 * refused with MBB_ERR_STATE. */
#define MBB_MAP_MAX_STARTS 64
#define MBB_MAP_MAX_ITER 1000
enum mbb_map_status {
    MBB_MAP_CONVERGED_F = 1,
    MBB_MAP_CONVERGED_X = 2,
    MBB_MAP_MAXITER = 4,
    MBB_MAP_START_INVALID = 8,
    MBB_MAP_COV_SINGULAR = 16,
    MBB_MAP_ALL_FIXED = 32,       /* no parameter is free: the result is the start, zero iterations               */
    MBB_MAP_STENCIL_FAILED = 64,  /* the SED constructor failed on a row of the difference stencil beside the current
                                     point (no merge point, no peak): no Jacobian there, the search ended where it was;
                                     the result is the best point reached, its covariance NaN (MBB_MAP_COV_SINGULAR)  */
    MBB_MAP_AT_LOWLIM_SHIFT = 8   /* bit 8 + i: parameter i of the result sits on its lower limit                 */
};
typedef struct mbb_map_spec {
    int32_t nsrc;
    int32_t nstart;                        /* 1 .. MBB_MAP_MAX_STARTS                                         */
    int32_t maxiter;                       /* 1 .. MBB_MAP_MAX_ITER                                           */
    int32_t fixed[5];
    double ftol, xtol;
    const double *start;                   /* [nsrc][nstart][5], finite                                       */
} mbb_map_spec;
/* Where the results go; every pointer is the caller's, host memory; model_flux, lnprob_all, params_all and status_all
 * may be NULL, the others are required. */
typedef struct mbb_map_out {
    double *params;                        /* [nsrc][5]                                                       */
    double *lnprob, *chisq, *q;            /* [nsrc]                                                          */
    double *model_flux;                    /* [nsrc][nb] or NULL                                              */
    double *cov;                           /* [nsrc][5][5]                                                    */
    int32_t *niter, *nfev, *start_index;   /* [nsrc]: iterations and row evaluations of the picked start      */
    int32_t *status;                       /* [nsrc] mbb_map_status bits of the picked start                  */
    double *lnprob_all;                    /* [nsrc][nstart] or NULL                                          */
    double *params_all;                    /* [nsrc][nstart][5] or NULL                                       */
    int32_t *status_all;                   /* [nsrc][nstart] or NULL                                          */
} mbb_map_out;
int mbb_map_fit(mbb_ctx *ctx, const mbb_map_spec *spec, const mbb_map_out *out);

/* ---- the evidence of a chain: bridge-sampled ln Z per source ---- */
/* New: the reference has nothing comparable.  Z is the integral of what like(theta) returns -- likelihood x hard lower
 * limits x soft upper walls x Gaussian priors, unnormalised -- over the free parameters: every parameter but the
 * caller's fixed ones, lambda0 of an optically thin model, alpha of a model without one, and any whose column is
 * constant over the window (min == max; what a stretch move started with zero scatter leaves).  Such a parameter is
 * HELD at the value of the chain's first window cell.  Meng & Wong's optimal bridge with a Gaussian proposal, the
 * recipe of Gronau et al. 2017 (csrc/mbb_evidence.hip.h; the step logic is csrc/mbb_bridge.hip.h):
 *   window     of the nkept kept steps (burn, burn + thin, ...) the first nfit = nkept / 2 of every walker fit the
 *              proposal: mean and covariance (ddof = 1) of the five columns.  The other nkept - nfit of every walker
 *              are the posterior samples; those whose lnprob is NaN or +-inf are left out, n1 are used.
 *   proposal   draw i of source s: three Philox4x32-10 blocks at counter (i, first_source + s, 0x42524447, 0..2),
 *              key = seed; word pairs (0,1) .. (8,9) give five k of 53 bits, u = (k + 1/2) 2^-53, z = PPND16(u)
 *              (Wichura's AS 241), theta = mean + L z over the free set.  lnP of the draws is mbb_lnlike_batch_device's,
 *              bit for bit; a draw below a lower limit has lnP = -inf and contributes nothing, which is correct: the
 *              proposal is normalised over the whole space.  n2 draws per source (0: as many as posterior samples).
 *   ln l       ln l1_j = lnprob_j - lnq(theta*_j) at the posterior samples, ln l2_i = lnP(theta~_i) - lnq(theta~_i) at
 *              the draws; l* is the mean of the ln l1 used.
 *   weights    n1e = neff[s] clamped to [1, n1] when given, otherwise n1; s1 = n1e / (n1e + n2), s2 = n2 / (n1e + n2).
 *   iteration  rho_0 = 1, rho <- [mean_i l2_i / (s1 l2_i + s2 rho)] / [mean_j 1 / (s1 l1_j + s2 rho)] with l shifted
 *              by l*; it stops when |rho_new - rho| <= tol rho_new (MBB_EV_CONVERGED) or after maxiter iterations
 *              (MBB_EV_MAXITER).  lnz = ln rho + l*.
 *   error      lnz_err = sqrt(RE^2), RE^2 = Var(f1) / (n2 mean(f1)^2) + Var(f2) / (n1e mean(f2)^2) with
 *              f1 = p / (s1 p + s2) over the draws, f2 = 1 / (s1 p + s2) over the posterior samples, p = l / z
 *              (Fruehwirth-Schnatter 2004).  Dividing by n1e stands in for the spectral-density term of the original
 *              formula: the caller says how many independent samples the n1 correlated ones are worth.
 * A source's result has the same bits whatever other sources the call holds (first_source names it among them).
 * Refused with MBB_ERR_ARG: fewer than 2 kept steps, n2 < 0 or above 2^22, tol not finite or negative, maxiter
 * outside 1 .. 100000, a neff that is not finite or not positive.  MBB_ERR_STATE without bands or data, and for a
 * context that is one rank of a sharded run.  nsrc is the context's, or the context holds one source for all. */
#define MBB_EV_MAX_N2 (1 << 22)
#define MBB_EV_MAX_ITER 100000
enum mbb_evidence_status {
    MBB_EV_CONVERGED = 1,
    MBB_EV_MAXITER = 2,
    MBB_EV_COV_SINGULAR = 4,      /* the covariance has no Cholesky factor; lnz is NaN                            */
    MBB_EV_POST_LEFT_OUT = 8,     /* some posterior cells were not finite and excluded                            */
    MBB_EV_NO_OVERLAP = 16,       /* no proposal draw has finite lnP; lnz is NaN                                  */
    MBB_EV_ALL_HELD = 32,         /* no free parameter: lnz is the lnprob of the first window cell, error 0       */
    MBB_EV_HELD_SHIFT = 8         /* bit 8 + i: parameter i was held                                              */
};
typedef struct mbb_evidence_spec {
    int32_t burn, thin, n2, maxiter, first_source, fixed[5];
    double tol;
    uint64_t seed;
    const double *neff;                    /* [nsrc] or NULL                                                  */
} mbb_evidence_spec;
/* Where the results go: host memory of the caller's.  prop, prop_lnprob, prop_lnq and post_lnq may be NULL.  N1 is
 * nw (nkept - nkept / 2), N2 the draws per source. */
typedef struct mbb_evidence_out {
    double *lnz, *lnz_err;                 /* [nsrc]                                                          */
    int32_t *niter, *status;               /* [nsrc]                                                          */
    int64_t *n1, *n2_inside;               /* [nsrc]: posterior cells used; draws of finite lnP               */
    double *prop_mean;                     /* [nsrc][5]                                                       */
    double *prop_cov;                      /* [nsrc][5][5], NaN in held rows and columns                      */
    double *prop;                          /* [nsrc][N2][5] or NULL                                           */
    double *prop_lnprob, *prop_lnq;        /* [nsrc][N2] or NULL                                              */
    double *post_lnq;                      /* [nsrc][N1] or NULL                                              */
} mbb_evidence_out;
int mbb_chain_evidence(mbb_ctx *ctx, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                       const mbb_evidence_spec *spec, const mbb_evidence_out *out);
int mbb_sampler_evidence(mbb_ctx *ctx, void *sampler, const mbb_evidence_spec *spec, const mbb_evidence_out *out);

/* ---- a chain reweighted under another density: Pareto-smoothed importance weights and weighted statistics ---- */
/* New: the reference has nothing comparable.  What the posterior of a chain would look like under the density of
 * another context, the TARGET -- other priors or limits, a measurement more or less, another model variant -- without
 * running the sampler again (csrc/mbb_reweight.hip.h; the step logic is csrc/mbb_psis.hip.h and csrc/mbb_rwsteps.hip.h).
 * Per source over a summary's window: steps burn, burn + thin, ... of every walker, entries j = 0 .. n - 1 in
 * [walker][step] order, n = nw nkept <= MBB_PW_MAX_WINDOW (a larger window is MBB_ERR_ARG, as for the out-of-sample fit).
 *   densities  lp_j is the chain's stored lnprob; lq_j the target's lnprob of row theta_j, mbb_lnlike_batch_device's bit
 *              for bit; r_j = lq_j - lp_j, one IEEE subtraction.
 *   classes    an entry is USED when r_j is finite; ZERO when lp_j is finite and lq_j = -inf (the target excludes the
 *              point: weight 0, counted in n_zero); LEFT OUT otherwise (lp_j not finite, lq_j NaN or +inf, a row the SED
 *              constructor fails on: counted in n_left_out, MBB_SUM_HAS_NAN, and the row's status bit from
 *              MBB_SUM_ROW_SHIFT on).  S = used entries, N = S + n_zero.
 *   weights    lw is the out-of-sample fit's PSIS recipe with -r in the place of ll: lw = r - max r over the used
 *              entries, M = ceil(min(0.2 S, 3 sqrt S)), the cutoff by the summary's exact select, the M tail entries in
 *              (lw, window index) order, the generalised Pareto fit and the smoothed tail capped at 0, the fallbacks
 *              MBB_RW_TAIL_SHORT and MBB_RW_TAIL_FLAT (raw weights, k^ = +inf).  smooth == 0 keeps the raw weights of
 *              every entry; k^ is still the fit's.
 *   scalars    khat, tail_len = M;  ess = (sum e^lw)^2 / sum e^2lw;
 *              lnz_ratio = max r + ln sum e^lw - ln N, an estimate of ln(Z_target / Z_run): added to an evidence's lnz
 *              it gives the target's.  -inf when every entry is zero.
 *   integers   u_j = floor(e^lw_j 2^32 + 1/2) in [0, MBB_RW_WEIGHT_ONE], 0 for an entry that is not used; U = sum u_j
 *              < 2^53, exact as an integer and as a double.  Every accumulation of weights is an integer one.
 *   columns    per column slot 0 .. 7 of a summary (the derived columns by the summary's own fill, from spec->summary,
 *              with the TARGET's model):  mean = sum u_j x_j / U;  the weighted quantile at percent p is the smallest
 *              sample value x with sum_{x_j <= x} u_j >= t, t = (uint64) ceil((p / 100.0) (double) U) clamped to
 *              [1, U] -- the "inverted CDF" (Hyndman & Fan 1) with weights, NOT the summary's "linear" rule; with equal
 *              weights it is numpy.quantile(..., method="inverted_cdf").  It is found by a weighted radix select: eight
 *              passes of 256-bin histograms of sums of u.  A column holding a NaN among its used entries has NaN mean
 *              and quantiles and MBB_SUM_HAS_NAN in col_status.
 *   per source cov = sum u_j d d^T / U about the weighted means, d the five parameters: no ddof correction (the weights
 *              are not counts).  best: the used entry of largest lq, the first in [walker][step] order among equals.
 * With no used entry the statistics are NaN and best_index -1 (MBB_SUM_EMPTY; MBB_RW_ALL_ZERO when every entry that
 * is not left out is zero).  Every floating-point sum has a fixed order: the same chain gives the same bits.
 * The target's number of sources is the chain's, or 1 (one density for all).  Its model variant may differ from the
 * run's: the five columns keep their meaning.  The summary spec's clips are ignored.  Every work buffer is the target's.
 * Refused before anything is allocated, uploaded or launched: null arguments, a target on another device, a sharded
 * context (MBB_ERR_STATE), wrong sources, a window above MBB_PW_MAX_WINDOW, more than MBB_SUMMARY_MAX_PCT percentiles,
 * bad burn / thin, no resident chain (MBB_ERR_STATE). */
#define MBB_RW_WEIGHT_ONE 4294967296ll     /* u of lw = 0: 2^32                                                 */
enum mbb_reweight_status {                 /* [nsrc]; beside the mbb_summary_status bits EMPTY, HAS_NAN (entries left out), ROW_SHIFT */
    MBB_RW_K_HIGH = 16,                    /* k^ > 0.7 (a fallback's +inf included)                            */
    MBB_RW_TAIL_SHORT = 32,
    MBB_RW_TAIL_FLAT = 64,
    MBB_RW_HAS_ZERO = 128,                 /* n_zero > 0                                                       */
    MBB_RW_ALL_ZERO = 65536                /* no used entry and n_zero > 0: the statistics are NaN, lnz_ratio -inf */
};
typedef struct mbb_reweight_spec {
    int32_t smooth;                        /* 0: raw weights                                                   */
    const mbb_summary_spec *summary;       /* the window, the percentiles, the derived columns and redshifts   */
} mbb_reweight_spec;
/* Where the results go: host memory of the caller's.  The four per-entry arrays may be NULL. */
typedef struct mbb_reweight_out {
    int64_t *n_used, *n_zero, *n_left_out, *weight_sum;     /* [nsrc]; weight_sum = U                          */
    double *khat, *ess, *lnz_ratio;        /* [nsrc]                                                          */
    double *mean;                          /* [nsrc][8]                                                       */
    double *pct;                           /* [nsrc][8][npct]                                                 */
    double *cov;                           /* [nsrc][5][5]                                                    */
    double *best;                          /* [nsrc][6]: the parameters and lq                                */
    int32_t *tail_len, *status;            /* [nsrc]                                                          */
    int32_t *col_status;                   /* [nsrc][8]: mbb_summary_status bits                              */
    int32_t *best_index;                   /* [nsrc][2]: walker, step                                         */
    double *target_lnprob, *log_ratio, *log_weight;         /* [nsrc][n] in window order, or NULL; lw is -inf where not used */
    int64_t *weight;                       /* [nsrc][n] u_j, or NULL                                          */
} mbb_reweight_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5] with its lnprob [nsrc][nw][nsteps]. */
int mbb_chain_reweight(mbb_ctx *target, const double *chain, const double *lnprob, int nsrc, int nw, int nsteps,
                       const mbb_reweight_spec *spec, const mbb_reweight_out *out);
/* The same of the chain the sampler's last stored or summarised run left on the device.  ctx owns the sampler and the
 * chain; target may be ctx or another context of this process on the same device.  ctx's stream is synchronised before
 * the target's first launch, the target's before the call returns. */
int mbb_sampler_reweight(mbb_ctx *ctx, void *sampler, mbb_ctx *target, const mbb_reweight_spec *spec,
                         const mbb_reweight_out *out);

/* ---- the population of a catalogue: the hyper-likelihood of its sources' chains under Gaussian candidates ---- */
/* New: the reference has nothing comparable.  Every other analysis answers a question about one source; this one asks
 * how chosen parameters are distributed OVER the sources, by the importance-sampling form of a hierarchical model
 * (Hogg, Myers & Bovy 2010): each source's chain was sampled under the run's own "interim" prior pi0, and for a
 * population density phi(. | h) the catalogue's likelihood is prod_n mean_j phi(x_nj | h) / pi0(x_nj) over the source's
 * window (csrc/mbb_population.hip.h; the step logic is csrc/mbb_popsteps.hip.h).
 *   columns    d of the five parameters (T, beta, lambda0, alpha, fnorm: 0 .. 4), 1 <= d <= 5, each at most once, with a
 *              transform g each: MBB_POP_IDENTITY or MBB_POP_LOG10.  The derived columns (peak wavelength, L_IR, dust
 *              mass) cannot be chosen: their interim prior density is not known in closed form.
 *   entries    source n has the entries j = 0 .. n - 1 of the window, steps burn, burn + thin, ... of every walker in
 *              [walker][step] order (csrc/mbb_chain_view.hip.h);  x_j = g(theta_j[columns]).
 *   interim    ln pi0(x_j) is the sum over the chosen columns of the likelihood's own separable prior factor of that
 *              parameter, unnormalised: 0 up to the upper limit, -1/2 ((theta - uplim) / (0.02 (uplim - lowlim)))^2
 *              beyond it where the parameter has one, plus -1/2 givar (theta - gmean)^2 where it has a Gaussian prior,
 *              plus for a log10 column the Jacobian ln(theta ln 10).  The limits and priors are the spec's, not the
 *              context's.  b_j = -ln pi0(x_j).  (A limit or prior on the peak wavelength is not separable and has no
 *              place here.)
 *   used       an entry is USED when every chosen theta is finite, every log10 column has theta > 0 and b_j is finite;
 *              otherwise it is LEFT OUT (n_left_out, MBB_SUM_HAS_NAN).  No lnprob is needed.
 *   candidate  h = (mu[d], L): L the lower Cholesky factor of the covariance, row by row, d (d + 1) / 2 values.  A
 *              candidate with a value that is not finite or an L_ii <= 0 is bad: MBB_POP_CAND_BAD, NaN results, and the
 *              other candidates of the call are unaffected.
 *              a_j(h) = -1/2 |L^-1 (x_j - mu)|^2 - sum_i ln L_ii - (d / 2) ln 2 pi + b_j, by forward substitution.
 *   per (candidate, source), with A = sum_j e^a_j over the used entries, every sum kept as a pair (max, sum e^(. - max)):
 *              lnl_src = ln A - ln n_used;   ess = A^2 / sum_j e^(2 a_j);
 *              with moments: mean = sum e^a_j x_j / A and cov = sum e^a_j (x_j - mean)(x_j - mean)^T / A, the source's
 *              posterior shrunk by that population.
 *              When every a_j is below -745 (e^a_j is below the smallest float64): lnl_src = -inf, ess and the moments
 *              NaN, MBB_POP_CAND_UNDERFLOW.  A source with no used entry: lnl_src NaN, MBB_SUM_EMPTY in its status and
 *              MBB_POP_CAND_HAS_EMPTY in every candidate's; it is left out of the total.
 *   per candidate  lnl = sum_n lnl_src over the sources used, in source order; n_src_used their number.
 * The population Gaussian is NOT renormalised over the hard lower limits: results mean little where its mass below a
 * limit is not small (population.py reports it as mass_below).
 * The arithmetic of one (candidate, source) depends on neither the other candidates or sources of a call nor on the
 * candidate's place in it: the same bits alone and in company.
 * mbb_*_population_build turns the window into a compact block [nsrc][n][d] of x and [nsrc][n] of b that the CONTEXT
 * keeps (one block per context: the next build replaces it, mbb_population_drop or the context's end frees it), and
 * hands back a serial number that every build increases; mbb_population_eval of another serial than the current block's
 * is MBB_ERR_STATE.  Refused before anything is allocated: null arguments, an empty chain or window, d outside 1 .. 5, a
 * repeated or unknown column or transform, H outside 1 .. MBB_POP_MAX_CAND, a sharded context (MBB_ERR_STATE).  A block
 * that cannot be allocated fails with the allocator's status; thin the window then. */
#define MBB_POP_MAX_CAND 1024
enum mbb_population_transform { MBB_POP_IDENTITY = 0, MBB_POP_LOG10 = 1 };
enum mbb_population_cand_status {          /* cand_status [H]                                                   */
    MBB_POP_CAND_BAD = 1,                  /* a value not finite or an L_ii <= 0: NaN results                   */
    MBB_POP_CAND_UNDERFLOW = 2,            /* a source's lnl_src is -inf, and so is lnl                         */
    MBB_POP_CAND_HAS_EMPTY = 4             /* a source without a used entry was left out of lnl                 */
};
typedef struct mbb_population_spec {
    int32_t d;                             /* 1 .. 5 columns                                                    */
    int32_t col[5], transform[5];          /* [d]: the parameter 0 .. 4 and its transform                       */
    int32_t burn, thin;                    /* the window                                                        */
    int32_t has_uplim[5], has_gprior[5];   /* by parameter: the likelihood's limits and priors                  */
    double lowlim[5], uplim[5], gmean[5], givar[5];
} mbb_population_spec;
typedef struct mbb_population_build_out {
    int64_t *n_used, *n_left_out;          /* [nsrc]                                                            */
    int32_t *status;                       /* [nsrc]: MBB_SUM_EMPTY, MBB_SUM_HAS_NAN (entries left out)         */
    int64_t *serial;                       /* [1]: the block's serial number                                    */
} mbb_population_build_out;
typedef struct mbb_population_eval_out {
    double *lnl;                           /* [H]                                                               */
    int32_t *n_src_used, *cand_status;     /* [H]                                                               */
    double *lnl_src, *ess;                 /* [H][nsrc], or NULL                                                */
    double *mean, *cov;                    /* [H][nsrc][d], [H][nsrc][d][d]: both given with moments, else unused */
} mbb_population_eval_out;
/* A host chain in emcee's layout [nsrc][nw][nsteps][5]. */
int mbb_chain_population_build(mbb_ctx *ctx, const double *chain, int nsrc, int nw, int nsteps,
                               const mbb_population_spec *spec, const mbb_population_build_out *out);
/* The same of the chain the sampler's last stored or summarised run left on the device. */
int mbb_sampler_population_build(mbb_ctx *ctx, void *sampler, const mbb_population_spec *spec,
                                 const mbb_population_build_out *out);
/* H candidates [H][d + d (d + 1) / 2] against the block of that serial. */
int mbb_population_eval(mbb_ctx *ctx, int64_t serial, const double *hyper, int H, int moments,
                        const mbb_population_eval_out *out);
/* Frees the context's block; a serial handed out before is MBB_ERR_STATE from then on. */
int mbb_population_drop(mbb_ctx *ctx);

/* ---- SED-level entry points (parity + the modified_blackbody class) ----- */
/* Replaces: modified_blackbody.__init__ (modified_blackbody.py:168-337) and
 * max_wave (:581-637) for n parameter rows.
 * out [n*6] = normfac, xmerge, kappa, x0, wavemerge, max_wave (NaN where the
 * reference has None); want_peak == 0 skips max_wave. */
int mbb_sed_prologue_batch(mbb_ctx *ctx, const double *pars, int n, int opthin,
                           int noalpha, double wavenorm, int want_peak,
                           double *out, int32_t *status);

/* Replaces: modified_blackbody.__call__ / f_nu (modified_blackbody.py:441-554)
 * for n parameter rows on a common grid of m frequencies (GHz): out [n*m]. */
int mbb_sed_eval_batch(mbb_ctx *ctx, const double *pars, int n, int opthin,
                       int noalpha, double wavenorm, const double *freq, int m,
                       double *out, int32_t *status);

/* Replaces: modified_blackbody.freq_integrate (modified_blackbody.py:639-674, scipy
 * quad of f_nu) for n rows: out[n] = integral of f_nu d nu over [numin, numax] GHz,
 * in mJy GHz (the reference multiplies by 1e-17 to get erg/s/cm^2).  Used by the
 * chain post-processing (results.py:627-674, L_IR). */
int mbb_sed_integrate_batch(mbb_ctx *ctx, const double *pars, int n, int opthin, int noalpha,
                            double wavenorm, double numin, double numax, double *out,
                            int32_t *status);

/* Replaces: fnu.fnueval_{thin,thick}_{noalpha,walpha} (fnu.pyx:9-108) with the
 * same explicit scalars; unused ones are ignored. */
int mbb_fnu_eval(mbb_ctx *ctx, int opthin, int noalpha, const double *freq, int n,
                 double T, double beta, double x0, double alpha, double normfac,
                 double xmerge, double kappa, double *out);

/* ---- device plumbing for callers that keep data resident ---------------- */
int mbb_malloc(mbb_ctx *ctx, size_t bytes, void **dptr);
int mbb_free(mbb_ctx *ctx, void *dptr);
int mbb_memcpy_h2d(mbb_ctx *ctx, void *dst, const void *src, size_t bytes);
int mbb_memcpy_d2h(mbb_ctx *ctx, void *dst, const void *src, size_t bytes);
int mbb_sync(mbb_ctx *ctx);
void *mbb_stream(mbb_ctx *ctx);             /* hipStream_t of the context     */
/* HIP events on the context's stream, for timing launches where they run */
int mbb_event_create(mbb_ctx *ctx, void **ev);
int mbb_event_record(mbb_ctx *ctx, void *ev);
int mbb_event_elapsed_ms(mbb_ctx *ctx, void *start, void *stop, float *ms);
int mbb_event_destroy(mbb_ctx *ctx, void *ev);

/* ---- tunables and counters of a context ---------------------------------- */
/* Options (mbb_set_option).  A value beyond its range is set to the nearer end, never refused; a name that is not here is
 * MBB_ERR_ARG.  Setting any option sends a resident server (below) away first.  The table in code, which
 * tests/test_host_cpu.py holds this one to: csrc/mbb_options.h.
 *
 *   name                    default   range         meaning
 *   "walkers_per_group"     0         any           walkers per workgroup of a likelihood launch; 0 = auto
 *   "block_threads"         0         any           threads per workgroup of a likelihood launch; 0 = auto
 *   "zero_copy"             1         any           host path: the kernel reads and writes pinned host memory
 *   "seg_chunks"            4         any           most chunks of 64 samples to a band segment; from the next mbb_set_bands
 *   "debug"                 0         any           a row's status carries the walker's pad bits too
 *   "stage_tables"          -1        any           band tables staged in LDS: -1 auto, 0 never, 1 whenever they fit
 *   "spin_wait"             2         any           how mbb_lnlike_batch waits (Waiting): 0 blocks, 1 polls the stream, 2 watches
 *   "spin_budget"           20000000  >= 0          polls of the watch before it blocks on the stream; 0 forces that
 *   "pack_tails"            1         any           band leftovers share chunks; from the next mbb_set_bands
 *   "bar_params"            1         any           host path: parameter rows written into device memory through the PCIe BAR
 *   "serve_overlap"         1         any           the served kernel's quadrature beside its constructor (Serve overlap); 0, 1, 2
 *   "serve"                 1         any           the served boundary: 0 a launch per call, 1 on, 2 whoever else is there (tests)
 *   "serve_after"           3         >= 1          boundary calls in a row before a server is started
 *   "serve_idle_us"         1000      any           a server leaves by itself this long after the last request
 *   "serve_budget_us"       400       >= 1          a served request not answered within this goes by a launch
 *   "serve_lease_us"        50000     >= 0          a server is sent away after this long in one go; 0 = never
 *   "serve_grid"            0         0 .. 1048576  workgroups of a server; 0 = as many as the calls have rows, in eights
 *   "serve_prefetch"        32        0 .. 256      record lines the host asks for ahead of its scan; 0 = none
 *   "prepass"               -1        any           k_walker_pre before a likelihood launch (Prepass): -1 auto, 0 never, 1 always
 *   "virtual_ranks"         0         any           testing: a sampler run as this many shards on one GPU
 *   "xchg_spin_max"         4000000   any           polls before a launch waiting for a peer gives up; default again at mbb_xchg_close
 *   "lookahead_sampler"     1         any           0: the plain train of one launch per half-step (Sampler forms)
 *   "flow_sampler"          1         any           one launch per 4096 steps; 0: the plain train as well
 *   "merged_flow_sampler"   1         any           form 7 (k_flowm) for ensembles of up to two walkers per CU; 0: the resident form
 *   "resident_sampler"      1         any           form 9 (k_flowa) for larger ensembles; 0: off, 2: every eligible ensemble
 *   "resident_walkers"      0         any           walkers per workgroup and half of the resident forms; 0 = the host's choice
 *   "flow_spin_log2"        0         any           log2 of the polls before a wait in a one-launch run gives up; 0 = 22, 63 = none
 *   "flow_min_steps"        2         any           runs shorter than this take the plain train
 *   "sharded_flow_sampler"  1         any           a sharded run with the one-hop exchange is one launch per 4096 steps too; 0: not
 *   "roof_wgs_per_cu"       0         any           measurement only: workgroups per CU of mbb_roof_probe; 0 = 2
 *   "roof_threads"          0         any           measurement only: threads per workgroup of mbb_roof_probe; 0 = 512
 *   "pointwise_budget_mb"   16384     >= 0          out-of-sample fit: memory the two columns per band of a group may take
 *
 * Info keys (mbb_get_info); any other name is MBB_ERR_ARG.
 *
 *   name                     meaning
 *   "device"                 the context's HIP device
 *   "cu_count"               its compute units
 *   "nb"                     bands set by mbb_set_bands
 *   "nseg"                   ... their segments
 *   "nunit"                  ... the entries of the unit table
 *   "nchunk"                 ... its chunks of 64 samples
 *   "nq"                     ... its quadrature samples
 *   "simd_chunks_max"        most chunks the unit table deals to one of the four SIMD positions
 *   "simd_chunks_min"        ... and fewest
 *   "last_prep_ns"           last mbb_lnlike_batch: time to prepare
 *   "last_launch_ns"         ... to launch
 *   "last_wait_ns"           ... to wait
 *   "last_watch_seen"        ... 1 the watch saw the results, 0 it fell back to the stream, -1 no watch
 *   "last_prepass"           whether the last likelihood launch was preceded by k_walker_pre
 *   "last_wpb"               last likelihood launch: walkers per workgroup
 *   "last_threads"           ... threads per workgroup
 *   "last_grid"              ... workgroups
 *   "last_smem"              ... bytes of dynamic LDS
 *   "last_stage"             ... whether the band tables were staged in LDS
 *   "last_kernel_form"       which form the last launch ran (Sampler forms; 0: a plain likelihood launch)
 *   "last_workgroups_ahead"  workgroups of the last sampler launch that worked ahead
 *   "serving"                1 while a server is resident
 *   "serve_enabled"          option "serve" as it stands
 *   "serve_requests"         boundary calls handed to a server
 *   "serve_fallbacks"        ... of which the answer did not come in time and a launch evaluated them
 *   "serve_rests"            how often the served boundary has had to rest
 *   "serve_resting"          boundary calls it still rests for
 *   "serve_grid"             workgroups of the resident server; 0 without one
 *   "serve_resizes"          servers that left because they were the wrong width
 *   "serve_peer_yields"      servers not started, or sent away, because another process is on the device
 *   "serve_lease_yields"     servers sent away because their lease was up
 *   "device_peers"           other processes of this library registered on the device
 *   "device_busy"            ... making boundary calls on it, as the latest boundary call counted them
 *   "flow_fallbacks"         one-launch sampler runs that gave up and were redone as a launch train
 *   "flow_resting"           runs the one-launch forms still rest for
 *   "nranks"                 ranks of the exchange when connected, else of the communicator
 *   "rank"                   ... and this context's
 *   "xchg_launches"          launches posted to the one-hop exchange so far
 *
 * Waiting.  "spin_wait" says how mbb_lnlike_batch waits: 0 blocks on the stream, 1 polls it, 2
 * watches the result slots in pinned memory, which are final before the kernel's completion signal
 * is.  After "spin_budget" polls the watch falls back to blocking on the stream.
 *
 * The served boundary.  With "serve" on, after "serve_after" boundary calls in a row with nothing
 * else in between -- a sampler's loop -- mbb_lnlike_call hands its rows to a kernel that STAYS on
 * the GPU between the calls and is rung through the BAR (k_serve: no launch per call; same results
 * bit for bit), while a batch is at most two rows per CU (a workgroup of the kernel takes a row; a
 * call of more rows than it has workgroups, two).  It leaves by itself "serve_idle_us" after the
 * last request.  mbb_get_info "serving", "serve_requests", "serve_fallbacks" tell what happened.
 *
 * Sharing inside a process.  One such kernel per device and process: any other entry point on the
 * context, and any entry point of ANOTHER context of the process that comes to the device, tells it
 * to leave first.  Such a visit also ends this context's run of calls, and doubles, up to 64, the
 * calls in a row it needs before its next server -- back to "serve_after" once a server has
 * answered 256 requests: likelihoods used in turns do not spend their time starting and stopping
 * kernels.
 *
 * Sharing between processes.  A server holds a CU per workgroup, and nothing of another PROCESS
 * fits on those (emcee's pool, mbb_fit.py:80-81 with threads > 1).  So it is as wide as the calls
 * have rows (in eights; "serve_grid" > 0: that many workgroups; mbb_get_info "serve_grid": the
 * resident one's) and no wider than this process's share of the device: the CUs divided (in whole
 * rows of the 8 XCDs) by the processes of this library that are making boundary calls on it right
 * now.  Those are read from a table in POSIX shared memory keyed by the device's PCI address, each
 * process noting its calls (csrc/mbb_registry.h; mbb_get_info "device_peers": registered,
 * "device_busy": calling).  Two workers of 125 rows have their servers side by side; a server
 * narrower than a call has rows takes two rows a workgroup (three workers: 80 CUs each); a call of
 * more than twice the share's rows goes by a launch ("serve_peer_yields"); a server too wide for
 * the share or too narrow for the call leaves and the next starts with the same call
 * ("serve_resizes").  For processes that table cannot show, a server is sent away after
 * "serve_lease_us" in one go -- the rows of that call go by a launch, the next server starts after
 * the next few calls in a row ("serve_lease_yields").  "serve" 2: the whole device is this
 * process's share whoever else is there (tests).
 *
 * Give-up and rest of the served boundary.  A request whose results do not appear within
 * "serve_budget_us" is evaluated by a launch instead, and three such in a row rest the feature for
 * the next 4096 boundary calls (mbb_get_info "serve_rests": how often, "serve_resting": calls
 * left).
 *
 * Record prefetch.  Once a request's first record has turned, the host asks for "serve_prefetch"
 * record lines ahead of its scan.
 *
 * Serve overlap.  With "serve_overlap" 1 the served kernel starts a row's passband quadrature
 * beside its SED constructor -- the blackbody-side value of every sample, which needs none of the
 * constructor's merge point, into a buffer in LDS -- and sums the units from the buffer when the
 * constructor is through, when the bands have at least 12 chunks of 64 samples (2: with fewer too);
 * 0: one after the other, as a launch does it; the same results either way.
 *
 * Prepass.  "prepass" -1 (auto: from 64 rows per CU), 0 (never), 1 (always): a likelihood launch of
 * given rows is preceded by k_walker_pre, which works out gate, SED constructor and penalties with
 * a LANE per row (k_lnlike: a row of 16 lanes per walker -- right where a constructor is latency, a
 * quarter of all instructions where a launch is bound by their number); same values bit for bit
 * (mbb_get_info "last_prepass").
 *
 * Sampler forms.  The forms of the single-GPU sampler give the same chains bit for bit (which one a
 * run takes by default, and what each costs: plan_sampler_run in mbb_hip.hip,
 * profiles/r04/walker_sweep.txt); mbb_get_info "last_kernel_form" says which form ran.
 *   - "lookahead_sampler" 0: the plain train of one launch per half-step.
 *   - "flow_sampler" 1: one launch per 4096 steps, every workgroup resident, rows handed over
 *     through check words instead of a launch boundary; 0: the plain train as well.
 *   - "flow_min_steps": runs shorter than this take the plain train: a one-launch run costs ~14 us
 *     beside its steps (default from profiles/r03/flowm_short_runs.txt).
 *   - "merged_flow_sampler" 1: ensembles of up to two walkers per CU take "form 7", k_flowm -- one
 *     workgroup per pair of walkers and candidate; the passband quadrature of both proposals a
 *     walker can end up making, and the SED constructor for every outcome still open, run ahead of
 *     the decisions they depend on; 0: those ensembles take the resident forms below too.
 *   - "resident_sampler" 1: ensembles beyond that run as ONE launch per 4096 steps as well, a
 *     workgroup owning W = ceil(half / CUs) walkers of each half, up to 8; 0: off, the plain train;
 *     2: every eligible ensemble takes it.  That run -- "form 9", k_flowa -- constructs every
 *     walker's proposal a half-step ahead, for both outcomes of its partner's pending move, beside
 *     the quadrature of the half-step before.  "resident_walkers": W, when not 0.
 *   - "sharded_flow_sampler" 1: a sharded run with the one-hop exchange is one launch per 4096
 *     steps on every rank too; 0: one launch per half-step.
 *
 * Give-up and rest of the one-launch forms.  "flow_spin_log2" is log2 of the polls before a wait
 * inside the one-launch run gives up (0 = 22; 63: no polls, the first miss, for tests).
 * mbb_sampler_run then redoes the run as a launch train and counts it in mbb_get_info
 * "flow_fallbacks"; the next run takes the one-launch form again, and only three give-ups in a row
 * rest it for the next 16 runs -- mbb_get_info "flow_resting" says how many of those are left.
 * mbb_sampler_advance_async keeps nothing to redo a run from: there a give-up surfaces at the next
 * mbb_sampler_run as MBB_ERR_STATE and the sampler wants mbb_sampler_set_state again. */
int mbb_set_option(mbb_ctx *ctx, const char *name, long value);
int mbb_get_info(mbb_ctx *ctx, const char *name, long *value);

/* ---- multi-GPU: one process per GPU, lnprob all-gather over RCCL -------- */
/* Replaces: emcee's multiprocessing pool selected by threads= (mbb_fit.py:80-81).
 * id is an opaque 128-byte ncclUniqueId made on rank 0 and handed to the other
 * ranks by the launcher (any side channel).  The collective library is librccl as the process
 * finds it, or -- environment variable MBB_RCCL_LIB -- the one library named there and no other
 * (a name that does not load is MBB_ERR_RCCL; the one-GPU tests name a stand-in that lets ranks
 * share a device: tests/rccl_standin/). */
int mbb_comm_unique_id(char id[128]);
int mbb_comm_init(mbb_ctx *ctx, int nranks, int rank, const char id[128]);
int mbb_comm_destroy(mbb_ctx *ctx);
/* every rank contributes count doubles; d_recv holds nranks*count, rank-major */
int mbb_allgather_f64(mbb_ctx *ctx, const double *d_send, double *d_recv, int count);
/* one sharded half-step: fused kernel on this rank's n rows, then the all-gather
 * of their lnprob into d_all [nranks*n]; asynchronous on the context's stream */
int mbb_lnlike_allgather_device(mbb_ctx *ctx, const double *d_pars, int n, double *d_lnl,
                                int32_t *d_status, double *d_all);
/* the same half-step as one synchronous call on host arrays -- literally what emcee's pool does per
 * half-step (mbb_fit.py:80-81): pars [n x 5] are this rank's rows, all [nranks*n] receives every rank's
 * lnprob (rank-major), status [n] (may be NULL) this rank's row status.  No copy command for the
 * parameters or the status (BAR / pinned memory as in mbb_lnlike_batch), one in-place ncclAllGather,
 * one copy of the gathered vector into a pinned landing buffer, one stream wait.  Without a communicator
 * (one rank) it is mbb_lnlike_batch through the same buffers. */
int mbb_lnlike_allgather(mbb_ctx *ctx, const double *pars, int n, double *all, int32_t *status);

/* ---- multi-GPU, device-resident sampler: one-hop exchange of the moved walkers ----- */
/* Replaces: emcee's multiprocessing pool (mbb_fit.py:80-81) for the device-resident
 * sampler, without a collective library.  Every rank keeps the whole ensemble in a
 * fine-grained buffer that all peers map (hipIpc*): the lane that accepts a move stores
 * the new state row into every rank's copy, and the launch's last walker raises the
 * launch number in every peer's flag word, which the next launch's prologue waits for.
 * Set-up: mbb_xchg_open on every rank -> exchange the 64-byte handles by any side
 * channel -> mbb_xchg_connect on every rank -> mbb_sampler_create (the sampler then lives
 * in the exchange buffer; nwalkers <= max_rows).  The launcher must also synchronise
 * the ranks between mbb_sampler_set_state and the first mbb_sampler_run / advance, and
 * before a later set_state.  In this mode mbb_sampler_run fills chain / lnprob /
 * naccepted for this rank's walkers only (pos_out and lnprob_out are complete).
 * mbb_xchg_close is refused while a sampler created under the exchange is alive. */
int mbb_xchg_open(mbb_ctx *ctx, int nranks, int rank, int max_rows, unsigned char handle[64]);
int mbb_xchg_connect(mbb_ctx *ctx, const unsigned char *handles /* nranks x 64 */);
int mbb_xchg_close(mbb_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MBB_HIP_H */
