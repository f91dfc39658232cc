"""The maximum of the posterior, found on the MI355X before any chain is run (csrc/mbb_map.hip.h, csrc/mbb_lm.hip.h).

The reference has no optimiser: its "best fit" is the chain entry of largest lnprob (reference
mbb_emcee/results.py:160-165), a random point near the optimum.  ``-2 ln P`` of this library is a sum of squares (the data
term, one square per soft upper wall that is exceeded, one per Gaussian prior), so a Levenberg-Marquardt search finds
its minimum; ``map_fit`` runs one per (source, start), all in one kernel launch, and returns a ``MapFit``: the optimum, its
lnprob (bit for bit ``like(params)``), chisq, q and band fluxes (bit for bit ``goodness.goodness_rows(params)``) and the
Laplace covariance -- the inverse of the curvature of ``-ln P`` at the optimum, the error estimate that needs no chain.
``mbb_fitter.find_map`` and ``mbb_fitter.map_initial_values`` start a fit's walkers from it.
"""
import ctypes as C

import numpy as np

from . import _analysis, _native

__all__ = ["map_fit", "MapFit"]

MAX_STARTS, MAX_ITER = _native.MAP_MAX_STARTS, _native.MAP_MAX_ITER
# the defaults of csrc/mbb_lm.hip.h (kMaxIterDefault, kFtolDefault, kXtolDefault), where their reasons are
MAXITER, FTOL, XTOL = 200, 1e-13, 1e-9
START_SCATTER = 0.25       # starts that are not given are the first one times (1 + START_SCATTER U(-1, 1))


def _limits(like):
    lo = np.array(like._lowlim, dtype=np.float64)
    hi = np.array([like._uplim[i] if like._has_uplim[i] else np.inf for i in range(5)], dtype=np.float64)
    return lo, hi


class _Request(object):
    """What one native map fit is asked for (mbb_map_spec); everything is checked here, before the device is touched."""

    def __init__(self, like, start, nstart=None, fixed=None, maxiter=MAXITER, ftol=FTOL, xtol=XTOL, rng=None):
        if not like.data_read:
            raise Exception("Data not read: a map fit needs the likelihood's photometry")
        self.nsrc = int(like.nsources)
        st = np.array(start, dtype=np.float64)
        if st.ndim not in (1, 2, 3) or st.shape[-1] != 5:
            raise ValueError("start must be [5], [nsources, 5] or [nsources, nstart, 5]")
        self.multi = st.ndim > 1 or self.nsrc > 1
        if st.ndim == 1:
            st = np.broadcast_to(st, (self.nsrc, 1, 5))
        elif st.ndim == 2:
            st = st[:, None, :]
        if st.shape[0] != self.nsrc:
            if like.nsources > 1:
                raise ValueError("start has {:d} sources, the likelihood {:d}".format(st.shape[0], self.nsrc))
            self.nsrc = st.shape[0]            # a one-source likelihood serves every source of the starts
        if not np.all(np.isfinite(st)):
            raise ValueError("start must be finite")
        given = st.shape[1]
        self.nstart = given if nstart is None else int(nstart)
        if not 1 <= self.nstart <= MAX_STARTS:
            raise ValueError("nstart must be 1 to {:d}".format(MAX_STARTS))
        if given > self.nstart:
            raise ValueError("{:d} starts given per source, nstart is {:d}".format(given, self.nstart))
        self.fixed = np.zeros(5, dtype=np.int32) if fixed is None else np.array([int(bool(f)) for f in fixed], dtype=np.int32)
        if self.fixed.shape != (5,):
            raise ValueError("fixed must have five entries")
        self.maxiter = int(maxiter)
        if not 1 <= self.maxiter <= MAX_ITER:
            raise ValueError("maxiter must be 1 to {:d}".format(MAX_ITER))
        self.ftol, self.xtol = float(ftol), float(xtol)
        if not (np.isfinite(self.ftol) and np.isfinite(self.xtol) and self.ftol >= 0 and self.xtol >= 0):
            raise ValueError("ftol and xtol must be finite and not negative")
        self.start = np.empty((self.nsrc, self.nstart, 5))
        self.start[:, :given] = st
        if given < self.nstart:
            self.start[:, given:] = self._draw(like, st[:, 0], self.nstart - given, np.random if rng is None else rng)
        self.ndata = int(like._ndata)
        if like.nsources > 1:
            self.flux = np.array(like._flux_multi, dtype=np.float64)
            self.sigma = 1.0 / np.sqrt(np.asarray(like._ivar_multi, dtype=np.float64))
        else:
            self.flux = np.array(like._flux, dtype=np.float64)[None]
            self.sigma = np.array(like.data_flux_unc, dtype=np.float64)[None]

    def _draw(self, like, first, n, rng):
        """n more starts per source around its first one, by the caller's generator, on the host, inside the limits;
        parameters that do not move (fixed, lambda0 of a thin model, alpha without one) keep the first start's value."""
        lo, hi = _limits(like)
        still = self.fixed.astype(bool) | np.array([False, False, like.opthin, like.noalpha, False])
        scale = np.where(still, 0.0, START_SCATTER)
        shape = (self.nsrc, n, 5)
        centre = first[:, None, :]
        p = centre * (1.0 + scale * rng.uniform(-1.0, 1.0, size=shape))
        for attempt in range(101):
            out = ((p < lo) | (p > hi)) & ~still
            nout = int(out.sum())
            if nout == 0:
                return p
            redraw = centre * (1.0 + scale * rng.uniform(-1.0, 1.0, size=shape))
            p = np.where(out, redraw, p)
        raise Exception("Too many iterations drawing starts inside the limits")

    def spec(self):
        s = _native.MapSpec()
        s.nsrc, s.nstart, s.maxiter = self.nsrc, self.nstart, self.maxiter
        for i in range(5):
            s.fixed[i] = int(self.fixed[i])
        s.ftol, s.xtol = self.ftol, self.xtol
        self.start = np.ascontiguousarray(self.start, dtype=np.float64)
        s.start = _native._d(self.start)
        return s


class _Raw(object):
    """The arrays of one native map fit (mbb_map_out), nsrc leading."""

    def __init__(self, nsrc, nstart, ndata):
        self.params = np.full((nsrc, 5), np.nan)
        self.lnprob = np.full(nsrc, np.nan); self.chisq = np.full(nsrc, np.nan); self.q = np.full(nsrc, np.nan)
        self.model_flux = np.full((nsrc, ndata), np.nan)
        self.cov = np.full((nsrc, 5, 5), np.nan)
        self.niter = np.zeros(nsrc, dtype=np.int32); self.nfev = np.zeros(nsrc, dtype=np.int32)
        self.start_index = np.zeros(nsrc, dtype=np.int32); self.status = np.zeros(nsrc, dtype=np.int32)
        self.lnprob_all = np.full((nsrc, nstart), np.nan)
        self.params_all = np.full((nsrc, nstart, 5), np.nan)
        self.status_all = np.zeros((nsrc, nstart), dtype=np.int32)

    def out(self):
        return _analysis.bind_out(_native.MapOut, vars(self))


def map_fit(like, start, nstart=None, fixed=None, maxiter=MAXITER, ftol=FTOL, xtol=XTOL, rng=None, squeeze=False):
    """The maximum of ``like``'s posterior per source, by Levenberg-Marquardt on the device; returns a ``MapFit``.

    start : [5] (every source starts there), [nsources, 5] or [nsources, nstart, 5];
    nstart : starts per source, 1 to 64 (default: as many as given).  With fewer starts given than nstart the rest are
        the source's first start times (1 + 0.25 U(-1, 1)), drawn on the host by ``rng`` (a numpy Generator or
        RandomState; default the global numpy generator) inside the limits; the kernel draws nothing.  Several starts
        because the optically thick models without a prior on lambda0 have more than one optimum;
    fixed : five flags, parameters held at their start value;
    maxiter, ftol, xtol : the stopping tests (csrc/mbb_lm.hip.h has the defaults' reasons);
    squeeze : drop the result's source axis when there is one source, whatever shape the starts came in."""
    req = _Request(like, start, nstart, fixed, maxiter, ftol, xtol, rng)
    ctx = _native.analysis_context(like)
    raw = _Raw(req.nsrc, req.nstart, req.ndata)
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_map_fit(ctx.h, C.byref(spec), C.byref(out)), ctx)
    return MapFit(req, raw, req.multi and not (squeeze and req.nsrc == 1), opthin=like.opthin, noalpha=like.noalpha)


class MapFit(object):
    """The optimum of the posterior from the device (a leading source axis for a multi-source result).

    params [..., 5], lnprob (bit for bit ``like(params)``), chisq, q, model_flux [..., ndata] (bit for bit
    ``goodness.goodness_rows(like, params, want_flux=True)``), pulls = (f_b - m_b) / sigma_b;
    covariance [..., 5, 5] : the Laplace covariance, NaN in the rows and columns of parameters that are fixed or sit on a
        lower limit, all NaN with COV_SINGULAR;  sigma : the square root of its diagonal;
    niter, nfev, start_index : of the start that was picked (largest lnprob, ties to the lowest index);
    status : bits CONVERGED_F, CONVERGED_X, MAXITER, START_INVALID, COV_SINGULAR, ALL_FIXED, STENCIL_FAILED (the SED
        constructor failed beside the current point: no Jacobian, the search ended there) and, from AT_LOWLIM_SHIFT on,
        one per parameter that sits on its lower limit; ``status_names()`` spells them;
    lnprob_all [..., nstart], params_all [..., nstart, 5], status_all [..., nstart] : every start's result;
    failed : START_INVALID -- the result is the start itself and nothing was searched."""

    CONVERGED_F, CONVERGED_X, MAXITER = _native.MAP_CONVERGED_F, _native.MAP_CONVERGED_X, _native.MAP_MAXITER
    START_INVALID, COV_SINGULAR, ALL_FIXED = _native.MAP_START_INVALID, _native.MAP_COV_SINGULAR, _native.MAP_ALL_FIXED
    AT_LOWLIM_SHIFT = _native.MAP_AT_LOWLIM_SHIFT
    STENCIL_FAILED = _native.MAP_STENCIL_FAILED
    _NAMES = [(1, "CONVERGED_F"), (2, "CONVERGED_X"), (4, "MAXITER"), (8, "START_INVALID"), (16, "COV_SINGULAR"),
              (32, "ALL_FIXED"), (64, "STENCIL_FAILED")]
    _PARS = ["T", "beta", "lambda0", "alpha", "fnorm"]

    def __init__(self, request, raw, multi, opthin=False, noalpha=False):
        self._req, self._raw, self._multi = request, raw, bool(multi)
        self._opthin, self._noalpha = bool(opthin), bool(noalpha)

    def _squeeze(self, a):
        return a if self._multi else a[0]

    nsources = property(lambda self: self._raw.params.shape[0])
    nstart = property(lambda self: self._raw.lnprob_all.shape[1])
    ndata = property(lambda self: self._req.ndata)
    params = property(lambda self: self._squeeze(self._raw.params).copy())
    lnprob = property(lambda self: self._squeeze(self._raw.lnprob).copy())
    chisq = property(lambda self: self._squeeze(self._raw.chisq).copy())
    q = property(lambda self: self._squeeze(self._raw.q).copy())
    model_flux = property(lambda self: self._squeeze(self._raw.model_flux).copy())
    covariance = property(lambda self: self._squeeze(self._raw.cov).copy())
    niter = property(lambda self: self._squeeze(self._raw.niter).copy())
    nfev = property(lambda self: self._squeeze(self._raw.nfev).copy())
    start_index = property(lambda self: self._squeeze(self._raw.start_index).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())
    lnprob_all = property(lambda self: self._squeeze(self._raw.lnprob_all).copy())
    params_all = property(lambda self: self._squeeze(self._raw.params_all).copy())
    status_all = property(lambda self: self._squeeze(self._raw.status_all).copy())
    failed = property(lambda self: self._squeeze((self._raw.status & _native.MAP_START_INVALID) != 0))

    @property
    def sigma(self):
        """The square root of the covariance's diagonal [..., 5]: NaN where the covariance is."""
        with np.errstate(invalid="ignore"):
            return self._squeeze(np.sqrt(np.diagonal(self._raw.cov, axis1=-2, axis2=-1)))

    @property
    def pulls(self):
        """(f_b - m_b) / sigma_b at the optimum [..., ndata]; one set of data serves every source when the likelihood
        holds one."""
        return self._squeeze((self._req.flux - self._raw.model_flux) / self._req.sigma)

    @classmethod
    def names_of(cls, status):
        """The names of one status word's bits."""
        st = int(status)
        names = [n for bit, n in cls._NAMES if st & bit]
        names += ["AT_LOWLIM(" + p + ")" for i, p in enumerate(cls._PARS) if st & (1 << (cls.AT_LOWLIM_SHIFT + i))]
        return names

    def status_names(self):
        """Per source the names of the status bits (a list of lists for a multi-source result)."""
        out = [self.names_of(s) for s in self._raw.status]
        return out if self._multi else out[0]

    def arrays(self, prefix="map_"):
        """The results as plain arrays (for an .npz)."""
        return {prefix + "params": self.params, prefix + "lnprob": self.lnprob, prefix + "chisq": self.chisq,
                prefix + "q": self.q, prefix + "model_flux": self.model_flux, prefix + "pulls": np.array(self.pulls),
                prefix + "covariance": self.covariance, prefix + "sigma": np.array(self.sigma), prefix + "niter": self.niter,
                prefix + "nfev": self.nfev, prefix + "start_index": self.start_index, prefix + "status": self.status}

    def __str__(self):
        """In the vocabulary of mbb_results.__str__; the first source of a multi-source result."""
        r = self._raw
        p, sg = r.params[0], np.atleast_2d(self.sigma)[0]
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(r.params.shape[0]))
        rows = [(0, "T/(1+z)", " [K]", True), (1, "beta", "", True), (4, "fnorm", " [mJy]", True),
                (2, "lambda0 (1+z)", " [um]", not self._opthin), (3, "alpha", "", not self._noalpha)]
        for i, tag, unit, used in rows:
            if not used:
                lines.append("Optically thin case assumed" if i == 2 else "Alpha not used")
            elif self._req.fixed[i]:
                lines.append("{:s}: {:0.2f} (fixed)".format(tag, p[i]))
            elif np.isnan(sg[i]):
                lines.append("{:s}: {:0.2f}{:s}".format(tag, p[i], unit))
            else:
                lines.append("{:s}: {:0.2f} +-{:0.2f}{:s}".format(tag, p[i], sg[i], unit))
        lines.append("Number of data points: {:d}".format(self.ndata))
        lines.append("ChiSquare of best fit point: {:0.2f} (q = {:0.4g})".format(r.chisq[0], r.q[0]))
        lines.append("ln P at the optimum: {:0.4f} (start {:d} of {:d}, {:d} iterations: {:s})".format(
            r.lnprob[0], int(r.start_index[0]), r.lnprob_all.shape[1], int(r.niter[0]),
            ", ".join(self.names_of(r.status[0])) or "-"))
        return "\n".join(lines)
