"""A chain reweighted under another posterior density, computed on the MI355X where the chain is
(csrc/mbb_reweight.hip.h): Pareto-smoothed importance weights per source and the weighted statistics of a summary's
columns.

The reference has nothing comparable; people who run emcee answer "what would this posterior look like with another
prior, one more flux, one flux less?" by running the sampler again or by reweighting the stored chain on the host.
Here the TARGET -- a second ``likelihood``: other priors or limits, other photometry, another model variant -- is
evaluated on every entry of the window by its own batch path, and with lp the chain's stored lnprob and lq the target's,

    r = lq - lp,   lw = PSIS(r)   (``loo``'s recipe with -r in the place of ll; k-hat says how far to trust it),
    u = floor(e^lw 2^32 + 1/2)    (integer weights: every accumulation is exact and the same bits every time),

give per source ``khat``, ``ess`` = (sum e^lw)^2 / sum e^2lw, ``lnz_ratio`` = ln(Z_target / Z_run) (add it to
``evidence().lnz`` for the target's ln Z), the weighted ``mean``, weighted quantiles, the weighted covariance and the
best entry under the target.  An entry the target excludes (lq = -inf) has weight zero (``n_zero``); one whose lp or lq
is otherwise not finite is left out (``n_left_out``).

The weighted quantile at percent p is the smallest sample value x with sum_{x_j <= x} u_j >= ceil(p / 100 U): the
"inverted CDF" (Hyndman & Fan 1) with weights -- with equal weights ``numpy.quantile(..., method="inverted_cdf")`` --
NOT the "linear" rule of ``results.chain_summary``.  The covariance is sum u d d^T / U with no ddof correction.
The definitions are in include/mbb_hip.h.  The numbers come from ``mbb_chain_reweight`` (a host chain) or
``mbb_sampler_reweight`` (the chain a ``DeviceEnsembleSampler`` run left on the device, which then never crosses the
bus).
"""
import ctypes as C

import numpy as np

from . import _analysis, _native
from . import results

__all__ = ["chain_reweight", "ChainReweight"]

MAX_WINDOW = _native.PW_MAX_WINDOW
COLUMN_NAMES = ("T", "beta", "lambda0", "alpha", "fnorm", "peaklambda", "lir", "dustmass")
_SCALARS = ("khat", "ess", "lnz_ratio")
_ENTRIES = ("target_lnprob", "log_ratio", "log_weight", "weight")


class _Request(_analysis.Window):
    """What one native reweighting is asked for (mbb_reweight_spec); everything is checked here, before the device is
    touched."""

    def __init__(self, target, percentile=68.3, percentiles=(), burn=0, thin=1, smooth=True, derived=(), redshift=None,
                 lumdist_mpc=None, kappa=2.64, kappa_wave=125.0, lir_range=(8.0, 1000.0), peak_model="fit", keep=False,
                 nsources=1):
        if not hasattr(target, "_sync_device"):
            raise TypeError("the target of a reweighting is a mbb_emcee_amd.likelihood")
        if not target.data_read:
            raise Exception("Data not read: reweighting needs the target likelihood's photometry")
        self.target = target
        self.cens, qs = _analysis.quantiles(percentile, percentiles)
        # the window, the percentiles and the derived columns' settings are a summary request's (its clips are not used)
        self.summary = results._Request(qs, burn, thin, None, derived, redshift, lumdist_mpc, kappa, kappa_wave,
                                        lir_range, peak_model, nsources=nsources)
        self.qs, self.derived = self.summary.qs, self.summary.derived
        self.burn, self.thin = self.summary.burn, self.summary.thin
        self.columns = list(range(5)) + sorted(results._DERIVED[d] for d in set(self.derived))
        self.smooth, self.keep = bool(smooth), bool(keep)
        _analysis.check_sources(target.nsources, int(nsources))

    def check_steps(self, nsteps, nwalkers=1):
        """The number of kept steps per walker."""
        nkept = _analysis.Window.check_steps(self, nsteps)
        if int(nwalkers) * nkept > MAX_WINDOW:
            raise ValueError("a window of {:d} entries per source is more than the device reweights: at most {:d} "
                             "(thin the window)".format(int(nwalkers) * nkept, MAX_WINDOW))
        return nkept

    def spec(self):
        s = _native.ReweightSpec()
        s.smooth = 1 if self.smooth else 0
        # (the summary spec lives as long as the spec that points at it)
        s._summary = self.summary.spec()
        s.summary = C.pointer(s._summary)
        return s


class _Raw(object):
    """The arrays of one native reweighting (mbb_reweight_out), nsrc leading."""

    def __init__(self, nsrc, npct, n=0, keep=False):
        nc = _native.SUMMARY_COLS
        self.n_used, self.n_zero, self.n_left_out, self.weight_sum = (np.zeros(nsrc, dtype=np.int64) for _ in range(4))
        for name in _SCALARS:
            setattr(self, name, np.full(nsrc, np.nan))
        self.mean = np.full((nsrc, nc), np.nan)
        self.pct = np.full((nsrc, nc, npct), np.nan)
        self.cov = np.full((nsrc, 5, 5), np.nan)
        self.best = np.full((nsrc, 6), np.nan)
        self.tail_len = np.zeros(nsrc, dtype=np.int32)
        self.status = np.zeros(nsrc, dtype=np.int32)
        self.col_status = np.zeros((nsrc, nc), dtype=np.int32)
        self.best_index = np.zeros((nsrc, 2), dtype=np.int32)
        self.target_lnprob = self.log_ratio = self.log_weight = self.weight = None
        if keep:
            self.target_lnprob, self.log_ratio, self.log_weight = (np.full((nsrc, n), np.nan) for _ in range(3))
            self.weight = np.zeros((nsrc, n), dtype=np.int64)

    def out(self):
        return _analysis.bind_out(_native.ReweightOut, vars(self))


def chain_reweight(target, chain, lnprob, burn=0, thin=1, percentile=68.3, percentiles=(), smooth=True, derived=(),
                   redshift=None, lumdist_mpc=None, kappa=2.64, kappa_wave=125.0, lir_range=(8.0, 1000.0),
                   peak_model="fit", keep=False):
    """A stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) and its lnprob, reweighted under ``target`` over the
    steps ``chain[:, burn::thin]`` on ``target``'s device; returns a ``ChainReweight``.

    target : the ``likelihood`` whose density the chain is reweighted to.  It holds the chain's number of sources, or
        one source for all.  Its model variant may differ from the run's; the five columns keep their meaning.
    percentile : the central interval(s) prepared, a number or a few;  percentiles : further plain percentiles -- at most
        eight q values in all.  Quantiles are weighted "inverted CDF" ones (the module's docstring).
    smooth : False keeps the raw importance weights (k-hat is still the fit's).
    derived, redshift, lumdist_mpc, kappa, kappa_wave, lir_range, peak_model : ``results.chain_summary``'s; the derived
        columns are made with the target's model.
    keep : bring the per-entry arrays back too, [n] in window order each: ``target_lnprob``, ``log_ratio``,
        ``log_weight``, ``weight``."""
    c4, multi = _native.chain4(chain)
    l3 = _analysis.lnprob_like(lnprob, c4, multi)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    req = _Request(target, percentile, percentiles, burn, thin, smooth, derived, redshift, lumdist_mpc, kappa, kappa_wave,
                   lir_range, peak_model, keep, nsources=nsrc)
    nkept = req.check_steps(nsteps, nw)
    ctx = _native.analysis_context(target)
    raw = _Raw(nsrc, len(req.qs), nw * nkept, req.keep)
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_reweight(ctx.h, _native._d(c4), _native._d(l3), nsrc, nw, nsteps, C.byref(spec),
                                                 C.byref(out)), ctx)
    return ChainReweight(req, raw, multi, nw, nkept)


class ChainReweight(_analysis.Result):
    """A chain reweighted under another density (a leading source axis for a multi-source chain).

    Per source: ``khat``, ``ess``, ``lnz_ratio``, ``n_used``, ``n_zero``, ``n_left_out``, ``tail_len``, ``status``,
    ``weight_sum`` (U, the sum of the integer weights).
    Per source and column [..., 8] (T, beta, lambda0, alpha, fnorm, peaklambda, lir, dustmass; NaN where a derived
    column was not asked for): ``mean``; ``percentiles`` [..., 8, len(qs)] at ``qs``; ``column_status``.
    par_cen(i, percentile) : [mean, upper - mean, mean - lower], and ``peaklambda_cen`` / ``lir_cen`` /
        ``dustmass_cen``, in the reference's vocabulary -- the quantiles are weighted "inverted CDF" ones, not numpy's
        "linear" (the module's docstring).
    covariance : sum u d d^T / U of the five parameters about the weighted means; no ddof correction.
    best_fit : (parameters, the target's lnprob, (walker, step)) of the used entry of largest target lnprob.
    With keep=True the per-entry arrays [..., n] in window order: ``target_lnprob``, ``log_ratio``, ``log_weight``
    (-inf where an entry is not used), ``weight`` (int64 u).
    status : the summary's bits -- EMPTY (no used entry), HAS_NAN (entries left out), from ROW_SHIFT on the row status of
    failing SED rows inside the window -- and K_HIGH (k-hat > 0.7: the weights are not to be trusted), TAIL_SHORT (20
    used entries or fewer: raw weights), TAIL_FLAT (no Pareto fit possible: raw weights), HAS_ZERO (the target excludes
    entries), ALL_ZERO (it excludes every one: the statistics are NaN and lnz_ratio is -inf)."""

    EMPTY, HAS_NAN, ABSENT, ROW_SHIFT = _native.SUM_EMPTY, _native.SUM_HAS_NAN, _native.SUM_ABSENT, _native.SUM_ROW_SHIFT
    K_HIGH, TAIL_SHORT, TAIL_FLAT, HAS_ZERO, ALL_ZERO = (_native.RW_K_HIGH, _native.RW_TAIL_SHORT, _native.RW_TAIL_FLAT,
                                                         _native.RW_HAS_ZERO, _native.RW_ALL_ZERO)
    WEIGHT_ONE = _native.RW_WEIGHT_ONE

    def __init__(self, request, raw, multi, nwalkers=0, nkept=0):
        self._req, self._raw, self._multi = request, raw, bool(multi)
        self.qs = list(request.qs)
        self._percentile = request.cens[0]
        self._set_window(request, nwalkers, nkept)

    khat = property(lambda self: self._squeeze(self._raw.khat).copy())
    ess = property(lambda self: self._squeeze(self._raw.ess).copy())
    lnz_ratio = property(lambda self: self._squeeze(self._raw.lnz_ratio).copy())
    n_used = property(lambda self: self._squeeze(self._raw.n_used).copy())
    n_zero = property(lambda self: self._squeeze(self._raw.n_zero).copy())
    n_left_out = property(lambda self: self._squeeze(self._raw.n_left_out).copy())
    tail_len = property(lambda self: self._squeeze(self._raw.tail_len).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())
    column_status = property(lambda self: self._squeeze(self._raw.col_status).copy())
    weight_sum = property(lambda self: self._squeeze(self._raw.weight_sum).copy())
    mean = property(lambda self: self._squeeze(self._raw.mean).copy())
    percentiles = property(lambda self: self._squeeze(self._raw.pct).copy())
    covariance = property(lambda self: self._squeeze(self._raw.cov).copy())

    def _entries(self, name):
        a = getattr(self._raw, name)
        if a is None:
            raise RuntimeError("the per-entry arrays were not kept: ask for them when the chain is reweighted (keep=True)")
        return self._squeeze(a)

    target_lnprob = property(lambda self: self._entries("target_lnprob"))
    log_ratio = property(lambda self: self._entries("log_ratio"))
    log_weight = property(lambda self: self._entries("log_weight"))
    weight = property(lambda self: self._entries("weight"))

    def _cen(self, slot, name, percentile):
        if slot not in self._req.columns:
            raise ValueError("{} was not asked for when the chain was reweighted (derived=)".format(name))
        lo, hi = results._pval(percentile)
        if lo not in self.qs or hi not in self.qs:
            raise RuntimeError("this reweighting was made without the {:g}% interval: ask for it when it is made "
                               "(percentile=, percentiles=)".format(float(percentile)))
        r = self._raw
        mn = r.mean[:, slot]
        return self._squeeze(np.stack([mn, r.pct[:, slot, self.qs.index(hi)] - mn, mn - r.pct[:, slot, self.qs.index(lo)]],
                                      axis=-1))

    def par_cen(self, param, percentile=None):
        """[weighted mean, upper - mean, mean - lower] of a parameter at a central interval that was prepared."""
        slot = results._paridx(param)
        return self._cen(slot, COLUMN_NAMES[slot], self._percentile if percentile is None else percentile)

    def peaklambda_cen(self, percentile=None):
        """Observer-frame peak wavelength [um]."""
        return self._cen(5, "peaklambda", self._percentile if percentile is None else percentile)

    def lir_cen(self, percentile=None):
        """L_IR [1e12 L_sun]."""
        return self._cen(6, "lir", self._percentile if percentile is None else percentile)

    def dustmass_cen(self, percentile=None):
        """Dust mass [1e8 M_sun]."""
        return self._cen(7, "dustmass", self._percentile if percentile is None else percentile)

    @property
    def best_fit(self):
        """(parameters, the target's lnprob, (walker, step)) of the used entry of largest target lnprob, ties to the
        first in [walker][step] order; NaN and (-1, -1) when no entry is used."""
        r = self._raw
        if self._multi:
            return r.best[:, :5].copy(), r.best[:, 5].copy(), r.best_index.copy()
        return r.best[0, :5].copy(), float(r.best[0, 5]), (int(r.best_index[0, 0]), int(r.best_index[0, 1]))

    def arrays(self, prefix="reweight_"):
        """The results as plain arrays (for an .npz)."""
        out = {prefix + "qs": np.array(self.qs), prefix + "columns": np.array(COLUMN_NAMES)}
        for name in ("khat", "ess", "lnz_ratio", "n_used", "n_zero", "n_left_out", "tail_len", "status", "column_status",
                     "weight_sum", "mean", "percentiles", "covariance"):
            out[prefix + name] = np.array(getattr(self, name))
        best, lq, idx = self.best_fit
        out[prefix + "best_fit"], out[prefix + "best_fit_lnprob"] = np.array(best), np.array(lq)
        out[prefix + "best_fit_index"] = np.array(idx)
        if self._raw.weight is not None:
            for name in _ENTRIES:
                out[prefix + name] = np.array(getattr(self, name))
        return out

    def __str__(self):
        """The first source of a multi-source result."""
        r = self._raw
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(r.status.shape[0]))
        lines.append("Reweighted over {:d} steps of {:d} walkers: {:d} entries used, {:d} of weight zero, {:d} left out".format(
            self.nsteps_used, self.nwalkers, int(r.n_used[0]), int(r.n_zero[0]), int(r.n_left_out[0])))
        lines.append("Pareto k-hat: {:0.2f}  effective sample size: {:0.1f}  ln(Z_target / Z_run): {:0.3f}".format(
            r.khat[0], r.ess[0], r.lnz_ratio[0]))
        lo, hi = results._pval(self._percentile)
        for slot in self._req.columns:
            lines.append("  {:10s} {:.6g} +{:.6g} -{:.6g}".format(
                COLUMN_NAMES[slot], r.mean[0, slot], r.pct[0, slot, self.qs.index(hi)] - r.mean[0, slot],
                r.mean[0, slot] - r.pct[0, slot, self.qs.index(lo)]))
        if int(r.status[0]) & self.ALL_ZERO:
            lines.append("Warning: the target excludes every entry of the chain")
        elif r.khat[0] > 0.7:
            lines.append("Warning: k-hat above 0.7: the chain does not cover the target well enough to be reweighted; "
                         "run the sampler on the target")
        return "\n".join(lines)
