"""Goodness of fit of a chain, computed on the MI355X where the chain is (csrc/mbb_goodness.hip.h).

The reference has nothing comparable: its "ChiSquare of best fit point" is ``-2 lnprob`` (reference
mbb_emcee/results.py:261-272), and lnprob carries the soft upper walls and the Gaussian priors.  Here the data term is
evaluated again for every chain entry: ``chisq(theta) = sum_b (f_b - m_b(theta))^2 / sigma_b^2`` (``r^T C^-1 r`` with a
covariance matrix), whatever the limits and priors are, and ``q(theta) = Q(ndata / 2, chisq / 2)``, the probability
that data replicated from the model at theta has a larger chisq.  The posterior mean of q is the posterior predictive
p-value of the chisq discrepancy.  ``ChainGoodness`` has the vocabulary; the numbers come from ``mbb_chain_goodness`` (a
host chain) or ``mbb_sampler_goodness`` (the chain a ``DeviceEnsembleSampler`` run left on the device, which then never
crosses the bus).  Percentiles are numpy's default ("linear") of exact order statistics.
"""
import ctypes as C

import numpy as np

from . import _analysis, _native
from . import results
from ._analysis import quantiles as _quantiles

__all__ = ["chain_goodness", "ChainGoodness"]

MAX_BANDS = 256
CHISQ, Q = 0, 1            # the two columns


class _Request(_analysis.Window):
    """What one native goodness call is asked for (mbb_goodness_spec); everything is checked here, before the device
    is touched."""

    def __init__(self, like, qs, burn=0, thin=1):
        # the data the pulls are formed with: [nsources, ndata]
        self.ndata, self.flux, self.sigma = _analysis.photometry(like, "goodness of fit")
        if self.ndata > MAX_BANDS:
            raise ValueError("at most {:d} bands per goodness call".format(MAX_BANDS))
        self.qs = [float(q) for q in qs]
        if not 1 <= len(self.qs) <= _native.SUMMARY_MAX_PCT:
            raise ValueError("a goodness call takes 1 to {:d} percentiles".format(_native.SUMMARY_MAX_PCT))
        for q in self.qs:
            if not (0 <= q <= 100):
                raise ValueError("Invalid percentile {:f}".format(q))
        self.set_window(burn, thin)

    def spec(self):
        s = _native.GoodnessSpec()
        s.npct, s.burn, s.thin = len(self.qs), self.burn, self.thin
        for i, q in enumerate(self.qs):
            s.pct[i] = q
        return s


class _Raw(object):
    """The arrays of one native goodness call (mbb_goodness_out), nsrc leading."""

    def __init__(self, nsrc, ndata, npct):
        self.n_used = np.zeros((nsrc, 2), dtype=np.int64)
        self.mean = np.full((nsrc, 2), np.nan); self.min = np.full((nsrc, 2), np.nan); self.max = np.full((nsrc, 2), np.nan)
        self.status = np.zeros((nsrc, 2), dtype=np.int32)
        self.pct = np.full((nsrc, 2, npct), np.nan)
        self.at_mean = np.full((nsrc, 7), np.nan)
        self.ml = np.full((nsrc, 7), np.nan)
        self.ml_index = np.full((nsrc, 2), -1, dtype=np.int32)
        self.ml_model = np.full((nsrc, ndata), np.nan)
        self.best = np.full((nsrc, 2), np.nan)
        self.best_index = np.full((nsrc, 2), -1, dtype=np.int32)

    def out(self):
        return _analysis.bind_out(_native.GoodnessOut, vars(self))


def goodness_rows(like, pars, want_flux=False):
    """(chisq [n], q [n], row status [n]) of parameter rows [n, 5] -- and their band fluxes [n, ndata] with want_flux --
    by the device function the chain's entries go through (mbb_goodness_rows).  In multi-source mode the rows are
    nsources equal blocks, as for ``like(pars)``."""
    p = _analysis.rows5(pars)
    ndata = _analysis.photometry(like, "goodness of fit")[0]
    ctx = _native.analysis_context(like)
    n = p.shape[0]
    chisq, q, st = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
    fl = np.empty((n, ndata)) if want_flux else None
    _native.check_arg(ctx.lib.mbb_goodness_rows(ctx.h, _native._d(p), n, _native._d(chisq), _native._d(q), _native._i(st),
                                                _native._d(fl) if want_flux else None), ctx)
    return (chisq, q, st, fl) if want_flux else (chisq, q, st)


def chain_goodness(like, chain, lnprob=None, percentile=68.3, percentiles=(), burn=0, thin=1):
    """Goodness of fit of a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) over the steps
    ``chain[:, burn::thin]``, computed on ``like``'s device against ``like``'s data; returns a ``ChainGoodness``.

    lnprob : [nw, nsteps] ([nsources, nw, nsteps]) or None -- with it, the real chisq of the entry of largest lnprob
        (``best_fit_chisq``);
    percentile : the central interval(s) of chisq prepared, a number or a few;  percentiles : further plain percentiles
        -- at most eight q values in all.
    A chain of many sources may be run through a one-source likelihood: every source is then held against that
    likelihood's data, and the result keeps its leading source axis."""
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    cens, qs = _quantiles(percentile, percentiles)
    req = _Request(like, qs, burn, thin)
    nkept = req.check_steps(nsteps)
    _analysis.check_sources(like.nsources, nsrc)
    lp = None if lnprob is None else _analysis.lnprob_like(lnprob, c4, multi)
    ctx = _native.analysis_context(like)
    raw = _Raw(nsrc, req.ndata, len(req.qs))
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_goodness(ctx.h, _native._d(c4), None if lp is None else _native._d(lp), nsrc, nw,
                                                 nsteps, C.byref(spec), C.byref(out)), ctx)
    return ChainGoodness(req, raw, multi, cens[0], nw, nkept)


class ChainGoodness(_analysis.Result):
    """Goodness of fit of a chain from the device (a leading source axis for a multi-source result).

    chisq_cen() : [mean, upper - mean, mean - lower] of chisq over the window;
    chisq_mean, chisq_min : of the window;  ppp : the mean of q, the posterior predictive p-value;
    chisq_at_mean : chisq at the posterior mean theta-bar (``theta_mean``: bit for bit the ``mean[0:5]`` of a
        ``chain_summary`` of the same window with neither clipping nor derived columns; one with derived columns may
        split its sums otherwise and differ in the last bits);  p_d = chisq_mean - chisq_at_mean, the effective number
        of parameters;  dic = chisq_mean + p_d;
    max_likelihood : (params [5], chisq, (walker, step)) of the window's entry of smallest chisq; ``q_max_likelihood``;
    pulls : (f_b - m_b) / sigma_b of that entry, per band;  ml_model : its band fluxes;
    best_fit_chisq : the real chisq of the entry of largest lnprob (NaN when no lnprob was given), ``best_fit_q``,
        ``best_index``;
    ndata, n_used, status, percentiles;
    status : per column (chisq, q) the summary's bits -- HAS_NAN, and from ROW_SHIFT on the row status of failing SED
        rows inside the window."""

    EMPTY, HAS_NAN, ROW_SHIFT = _native.SUM_EMPTY, _native.SUM_HAS_NAN, _native.SUM_ROW_SHIFT

    def __init__(self, request, raw, multi, percentile=68.3, nwalkers=0, nkept=0):
        self._req, self._raw, self._multi = request, raw, bool(multi)
        self._percentile = float(percentile)
        self._set_window(request, nwalkers, nkept)

    ndata = property(lambda self: self._req.ndata)
    n_used = property(lambda self: self._squeeze(self._raw.n_used[:, CHISQ]).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())
    chisq_mean = property(lambda self: self._squeeze(self._raw.mean[:, CHISQ]).copy())
    chisq_min = property(lambda self: self._squeeze(self._raw.min[:, CHISQ]).copy())
    chisq_max = property(lambda self: self._squeeze(self._raw.max[:, CHISQ]).copy())
    ppp = property(lambda self: self._squeeze(self._raw.mean[:, Q]).copy())
    theta_mean = property(lambda self: self._squeeze(self._raw.at_mean[:, :5]).copy())
    chisq_at_mean = property(lambda self: self._squeeze(self._raw.at_mean[:, 5]).copy())
    q_at_mean = property(lambda self: self._squeeze(self._raw.at_mean[:, 6]).copy())
    p_d = property(lambda self: self._squeeze(self._raw.mean[:, CHISQ] - self._raw.at_mean[:, 5]))
    dic = property(lambda self: self._squeeze(self._raw.mean[:, CHISQ] + (self._raw.mean[:, CHISQ] - self._raw.at_mean[:, 5])))
    q_max_likelihood = property(lambda self: self._squeeze(self._raw.ml[:, 6]).copy())
    ml_model = property(lambda self: self._squeeze(self._raw.ml_model).copy())
    best_fit_chisq = property(lambda self: self._squeeze(self._raw.best[:, 0]).copy())
    best_fit_q = property(lambda self: self._squeeze(self._raw.best[:, 1]).copy())
    best_index = property(lambda self: self._squeeze(self._raw.best_index).copy())

    @property
    def max_likelihood(self):
        """(params [..., 5], chisq, (walker, step) [..., 2]) of the window's entry of smallest chisq"""
        return (self._squeeze(self._raw.ml[:, :5]).copy(), self._squeeze(self._raw.ml[:, 5]).copy(),
                self._squeeze(self._raw.ml_index).copy())

    @property
    def pulls(self):
        """(f_b - m_b) / sigma_b of the maximum-likelihood entry [..., ndata]; one set of data serves every source of
        the chain when the likelihood holds one."""
        return self._squeeze((self._req.flux - self._raw.ml_model) / self._req.sigma)

    def chisq_cen(self, percentile=None):
        """[mean, upper - mean, mean - lower] of chisq over the window, as ``predflux_cen``; raises -- as
        ``postprocess.predict_flux`` does for the same chain -- when an SED row inside the window fails; a NaN
        parameter gives NaN and does not raise."""
        p = self._percentile if percentile is None else float(percentile)
        lo, hi = results._pval(p)
        for q in (lo, hi):
            if q not in self._req.qs:
                raise RuntimeError("this goodness of fit was made without the {:g}% interval: ask for it when it is "
                                   "made (percentile=, percentiles=)".format(p))
        _native.raise_for_status(results.ChainSummary._row_status(self._raw, CHISQ))
        mn = self._raw.mean[:, CHISQ]
        res = np.stack([mn, self._raw.pct[:, CHISQ, self._req.qs.index(hi)] - mn,
                        mn - self._raw.pct[:, CHISQ, self._req.qs.index(lo)]], axis=-1)
        return self._squeeze(res)

    @property
    def percentiles(self):
        """(q values prepared, their values [..., 2, len(q)]: row 0 chisq, row 1 q)"""
        return list(self._req.qs), self._squeeze(self._raw.pct).copy()

    def arrays(self, prefix="goodness_"):
        """The results as plain arrays (for an .npz)."""
        qs, pct = self.percentiles
        r = self._raw
        ml = self.max_likelihood
        return {prefix + "ndata": np.array(self.ndata), prefix + "n_used": self.n_used,
                prefix + "mean": self._squeeze(r.mean).copy(), prefix + "min": self._squeeze(r.min).copy(),
                prefix + "max": self._squeeze(r.max).copy(), prefix + "q": np.array(qs), prefix + "percentiles": pct,
                prefix + "status": self.status, prefix + "theta_mean": self.theta_mean,
                prefix + "chisq_at_mean": self.chisq_at_mean, prefix + "q_at_mean": self.q_at_mean,
                prefix + "p_d": np.array(self.p_d), prefix + "dic": np.array(self.dic),
                prefix + "ml_params": ml[0], prefix + "ml_chisq": ml[1], prefix + "ml_q": self.q_max_likelihood,
                prefix + "ml_index": ml[2], prefix + "ml_model": self.ml_model, prefix + "pulls": np.array(self.pulls),
                prefix + "best_fit_chisq": self.best_fit_chisq, prefix + "best_fit_q": self.best_fit_q,
                prefix + "best_index": self.best_index}

    def __str__(self):
        """The first source of a multi-source result."""
        r = self._raw
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(r.status.shape[0]))
        try:
            c = np.atleast_2d(self.chisq_cen())[0]
            lines.append("ChiSquare over the chain: {:0.2f} +{:0.2f} -{:0.2f} for {:d} data points".format(
                c[0], c[1], c[2], self.ndata))
        except Exception as e:       # noqa -- a line, whatever it raises
            lines.append("ChiSquare over the chain: {}".format(e))
        lines.append("Posterior predictive p-value: {:0.4f}".format(r.mean[0, Q]))
        lines.append("ChiSquare at the posterior mean: {:0.2f}  p_D: {:0.2f}  DIC: {:0.2f}".format(
            r.at_mean[0, 5], r.mean[0, CHISQ] - r.at_mean[0, 5], 2 * r.mean[0, CHISQ] - r.at_mean[0, 5]))
        lines.append("Minimum ChiSquare: {:0.2f} (q = {:0.4g}) at walker {:d}, step {:d}".format(
            r.ml[0, 5], r.ml[0, 6], int(r.ml_index[0, 0]), int(r.ml_index[0, 1])))
        pulls = np.atleast_2d(self.pulls)[0]
        lines.append("Pulls there: " + " ".join("{:+0.2f}".format(p) for p in pulls))
        if r.best_index[0, 0] >= 0:
            lines.append("ChiSquare of best fit point: {:0.2f} (q = {:0.4g})".format(r.best[0, 0], r.best[0, 1]))
        return "\n".join(lines)
