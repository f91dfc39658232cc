"""Posterior summaries of a chain, computed on the MI355X where the chain is.

The reference's user-facing result is ``mbb_results`` (reference mbb_emcee/results.py): for every
parameter and derived quantity a mean with a central credible interval (``par_cen``,
``peaklambda_cen``, ``lir_cen``, ``dustmass_cen`` -> ``_parcen_internal``, results.py:314-369),
one-sided limits (``par_lowlim`` / ``par_uplim``, :433-493) and the best-fitting sample
(``process_fit``, :160-165).  ``ChainSummary`` has that vocabulary; the numbers come from the
reduction / selection kernels of csrc/mbb_summary.hip.h through ``mbb_chain_summary`` (a host chain)
or ``mbb_sampler_run_summary`` (the chain of a ``DeviceEnsembleSampler`` run, which then never leaves
the device).  Percentiles are numpy's default ("linear") of exact order statistics.

HDF5, astropy and the cosmology stay out of scope, as in ``postprocess``: pass the luminosity
distance in.  For a catalogue (a multi-source chain) ``redshift`` and ``lumdist_mpc`` may each be an
array with one entry per source; NaN marks a source whose value is unknown, and its L_IR and dust
mass are NaN.  Clip bounds, ``kappa`` / ``kappa_wave`` and ``lir_range`` stay one per call, and
``postprocess.lir`` / ``postprocess.dustmass`` stay scalar.
"""
import ctypes as C

import numpy as np

from . import _analysis, _native
from .modified_blackbody import modified_blackbody

__all__ = ["chain_summary", "ChainSummary"]

_PARAM_ORDER = {'t': 0, 't/(1+z)': 0, 'beta': 1, 'lambda0': 2, 'lambda0*(1+z)': 2, 'lambda_0': 2,
                'lambda_0*(1+z)': 2, 'alpha': 3, 'fnorm': 4, 'f500': 4}          # results.py:33-35
_DERIVED = {"peaklambda": 5, "lir": 6, "dustmass": 7}
_DERIVED_BITS = {"peaklambda": _native.SUM_PEAK, "lir": _native.SUM_LIR, "dustmass": _native.SUM_DUSTMASS}
_NO_SURVIVORS = "No elements survive lower/upper limit clipping"                  # results.py:361-362


def _pval(percentile):
    """_parcen_internal's two percentiles (results.py:342-348), in its own arithmetic."""
    pcnt = float(percentile)
    if not (0 <= pcnt <= 100):
        raise ValueError("Invalid percentile {:f}".format(pcnt))
    pval = 0.5 * (100 - pcnt)
    return pval, 100 - pval


def _check_open(percentile):
    if not (0 < percentile < 100.0):                                              # results.py:426, :460, :491
        raise ValueError("percentile needs to be between 0 and 100")


def _paridx(param):
    if isinstance(param, str):
        try:
            return _PARAM_ORDER[param.lower()]
        except KeyError:
            raise ValueError("unknown parameter name {!r}".format(param))
    paridx = int(param)
    if paridx < 0 or paridx > 4:
        raise ValueError("invalid parameter index {:d}".format(paridx))
    return paridx


class _Request(_analysis.Window):
    """What one native summary call is asked for (mbb_summary_spec)."""

    def __init__(self, qs, burn=0, thin=1, clip=None, derived=(), redshift=None, lumdist_mpc=None, kappa=2.64,
                 kappa_wave=125.0, lir_range=(8.0, 1000.0), peak_model="fit", nsources=1):
        self.qs = [float(q) for q in qs]
        if not 1 <= len(self.qs) <= _native.SUMMARY_MAX_PCT:
            raise ValueError("a summary call takes 1 to {:d} percentiles".format(_native.SUMMARY_MAX_PCT))
        for q in self.qs:
            if not (0 <= q <= 100):
                raise ValueError("Invalid percentile {:f}".format(q))
        self.set_window(burn, thin)
        self.clip = {}
        for key, (lo, hi) in (clip or {}).items():
            slot = _DERIVED[key] if key in _DERIVED else _paridx(key)
            self.clip[slot] = (None if lo is None else float(lo), None if hi is None else float(hi))
        if isinstance(derived, str):
            derived = (derived,)
        self.derived = tuple(derived)
        for d in self.derived:
            if d not in _DERIVED:
                raise ValueError("unknown derived quantity {!r}: one of {}".format(d, sorted(_DERIVED)))
        if peak_model not in ("fit", "reference"):
            raise ValueError("model must be 'fit' or 'reference'")
        self.peak_model = peak_model
        if ("lir" in self.derived or "dustmass" in self.derived) and (redshift is None or lumdist_mpc is None):
            raise ValueError("L_IR and dust mass need redshift and lumdist_mpc")
        # one value for the call (as the reference has it), or one per source: then both go to the library as arrays
        # [nsources] (a scalar beside an array is broadcast), which live as long as this request and its copies
        self.nsources = int(nsources)
        z, d = [None if v is None else np.asarray(v, dtype=np.float64) for v in (redshift, lumdist_mpc)]
        for name, v in (("redshift", z), ("lumdist_mpc", d)):
            if v is not None and v.ndim and v.shape != (self.nsources,):
                raise ValueError("{} must be a number or a 1-d array with one entry per source ({:d}), not of shape "
                                 "{}".format(name, self.nsources, v.shape))
        self.src_redshift = self.src_lumdist_mpc = None
        if z is not None and d is not None and (z.ndim or d.ndim):
            self.src_redshift, self.src_lumdist_mpc = [np.ascontiguousarray(np.broadcast_to(v, (self.nsources,))).copy()
                                                       for v in (z, d)]
            self.src_redshift.setflags(write=False)
            self.src_lumdist_mpc.setflags(write=False)
            z = d = None
        self.redshift = 0.0 if z is None or z.ndim else float(z)
        self.lumdist_mpc = 0.0 if d is None or d.ndim else float(d)
        self.kappa, self.kappa_wave = float(kappa), float(kappa_wave)
        if self.kappa <= 0 or self.kappa_wave <= 0:
            raise ValueError("kappa and kappa_wave must be positive")
        self.lir_range = (float(lir_range[0]), float(lir_range[1]))
        if min(self.lir_range) <= 0:
            raise ValueError("wavelengths must be positive")

    def with_(self, qs, slot, lo, hi):
        """The same request for other percentiles and another clipping of one column."""
        import copy
        r = copy.copy(self)
        r.qs = [float(q) for q in qs]
        r.clip = {slot: (lo, hi)} if (lo is not None or hi is not None) else {}
        return r

    def spec(self):
        s = _native.SummarySpec()
        s.npct = len(self.qs)
        for i, q in enumerate(self.qs):
            s.pct[i] = q
        s.burn, s.thin = self.burn, self.thin
        s.derived = sum(_DERIVED_BITS[d] for d in set(self.derived))
        s.peak_model = 1 if self.peak_model == "reference" else 0
        for slot, (lo, hi) in self.clip.items():
            if lo is not None:
                s.has_lo[slot], s.lo[slot] = 1, lo
            if hi is not None:
                s.has_hi[slot], s.hi[slot] = 1, hi
        s.redshift, s.lumdist_mpc = self.redshift, self.lumdist_mpc
        s.kappa, s.kappa_wave = self.kappa, self.kappa_wave
        s.lir_wavemin, s.lir_wavemax = self.lir_range
        if self.src_redshift is not None:
            # (the addresses of this request's own arrays: the request outlives the call the spec is made for)
            s.src_redshift, s.src_lumdist_mpc = _native._d(self.src_redshift), _native._d(self.src_lumdist_mpc)
        return s

    def cosmology(self):
        """(redshift, lumdist_mpc) as used: arrays [nsources] if given per source, else the two numbers."""
        if self.src_redshift is not None:
            return self.src_redshift, self.src_lumdist_mpc
        return self.redshift, self.lumdist_mpc


class _Raw(object):
    """The arrays of one native summary call (mbb_summary_out), nsrc leading."""

    def __init__(self, nsrc, npct):
        nc = _native.SUMMARY_COLS
        self.n_used = np.zeros((nsrc, nc), dtype=np.int64)
        self.mean = np.empty((nsrc, nc)); self.min = np.empty((nsrc, nc)); self.max = np.empty((nsrc, nc))
        self.pct = np.empty((nsrc, nc, npct))
        self.status = np.zeros((nsrc, nc), dtype=np.int32)
        self.cov = np.empty((nsrc, 5, 5))
        self.best = np.empty((nsrc, 6))
        self.best_index = np.zeros((nsrc, 2), dtype=np.int32)

    def out(self):
        return _analysis.bind_out(_native.SummaryOut, vars(self))


def _summarise_host(like, chain, lnprob, req):
    """mbb_chain_summary on a host chain [nsrc, nw, nsteps, 5]."""
    ctx = _native.analysis_context(like)
    nsrc, nw, nsteps = lnprob.shape
    raw = _Raw(nsrc, len(req.qs))
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_summary(ctx.h, _native._d(chain), _native._d(lnprob), nsrc, nw, nsteps,
                                                C.byref(spec), C.byref(out)), ctx)
    return raw


def chain_summary(like, chain, lnprob, percentile=68.3, burn=0, thin=1, derived=(), redshift=None,
                  lumdist_mpc=None, kappa=2.64, kappa_wave=125.0, lir_range=(8.0, 1000.0), peak_model="fit",
                  clip=None, percentiles=(), keep=True):
    """Summary of a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) and its lnprob, computed on
    ``like``'s device.

    percentile : the central interval(s) prepared, a number or a few (68.3: 1 sigma; 95.4: 2 sigma);
    percentiles : further plain percentiles (numpy's q) to prepare, e.g. ``100 - 95`` for ``par_lowlim(p, 95)``
    -- at most eight q values in all; whatever else is asked of the result later costs another call.
    burn, thin : the steps used, ``chain[:, burn::thin]``.
    derived : any of "peaklambda", "lir", "dustmass" (the latter two need ``redshift`` and ``lumdist_mpc``);
    peak_model as ``postprocess.peak_wavelength``'s ``model``.
    redshift, lumdist_mpc : a number each, or a 1-d array with one entry per source of the chain (length 1 for a
    [nw, nsteps, 5] chain); a number beside an array serves every source.  A NaN entry marks a source whose value is
    unknown: its L_IR and dust mass are NaN (status ``SUM_HAS_NAN``), everything else is unaffected.
    clip : ``{param or derived name: (lowlim, uplim)}`` applied as ``_parcen_internal`` does (either may be None).
    keep : keep the chain with the result, so that other percentiles and clip bounds can be computed on demand."""
    c4, multi = _native.chain4(chain)
    l3 = _analysis.lnprob_like(lnprob, c4, multi)
    if int(burn) >= c4.shape[2]:
        raise ValueError("burn leaves no step of the chain")
    cens, qs = _analysis.quantiles(percentile, percentiles)
    req = _Request(qs, burn, thin, clip, derived, redshift, lumdist_mpc, kappa, kappa_wave, lir_range, peak_model,
                   nsources=c4.shape[0])
    raw = _summarise_host(like, c4, l3, req)
    again = (lambda r: _summarise_host(like, c4, l3, r)) if keep else None
    return ChainSummary(like, req, raw, multi, again, cens[0])


class ChainSummary(_analysis.Result):
    """What ``mbb_results`` reports of a chain (results.py), from the device's summary of it.  Results of a
    multi-source chain carry a leading source axis."""

    def __init__(self, like, request, raw, multi, again=None, percentile=68.3):
        self._like, self._req, self._raw, self._multi, self._again = like, request, raw, multi, again
        self._percentile = float(percentile)
        self._cache = {}
        self._opthin, self._noalpha, self._wavenorm = like.opthin, like.noalpha, like.wavenorm
        self._ndata = int(like.ndata) if like.data_read and like.nsources == 1 else None

    # ---- plumbing ---------------------------------------------------------------------------
    def drop_chain(self):
        """Forget how to compute more from the chain (a sampler's next run overwrites it on the device)."""
        self._again = None

    def _lookup(self, slot, qs, lowlim, uplim):
        """(raw arrays, indices of qs in them) for column `slot` clipped to [lowlim, uplim]."""
        lo = None if lowlim is None else float(lowlim)
        hi = None if uplim is None else float(uplim)
        have = self._req.clip.get(slot, (None, None))
        if have == (lo, hi) and all(q in self._req.qs for q in qs):
            return self._raw, [self._req.qs.index(q) for q in qs]
        key = (slot, lo, hi, tuple(qs))
        if key not in self._cache:
            if self._again is None:
                raise RuntimeError("this summary was made without these percentiles / clip bounds and the chain was "
                                   "not kept: ask for them when the summary is made (percentile=, percentiles=, "
                                   "clip=), or keep the chain")
            self._cache[key] = self._again(self._req.with_(qs, slot, lo, hi))
        return self._cache[key], list(range(len(qs)))

    def _column(self, slot, name):
        if slot >= 5 and name not in self._req.derived:
            raise ValueError("{} was not asked for when the summary was made (derived=)".format(name))

    def _cen(self, slot, percentile, lowlim, uplim):
        """[mean, upper - mean, mean - lower] of column `slot`.  A multi-source summary is one result: the statuses of
        all its sources are combined first, so it raises -- nothing surviving the clipping, or the exception of a
        failing SED row as ``postprocess`` raises it for the same chain -- when ANY source's column met that inside
        the burn / thin window, also for the sources whose own column is fine (``status`` says which those are, and
        ``mean`` / ``percentiles`` hold their numbers).  Rows outside the window never count; a NaN parameter gives NaN
        and does not raise.  Nor does a source whose redshift or distance was given as NaN: its L_IR and dust mass are
        NaN rows (also when a clip leaves that source's column empty)."""
        qs = list(_pval(percentile))
        raw, idx = self._lookup(slot, qs, lowlim, uplim)
        empty = (raw.status[:, slot] & _native.SUM_EMPTY) != 0
        if slot in (6, 7) and self._req.src_redshift is not None:
            empty &= ~(np.isnan(self._req.src_redshift) | np.isnan(self._req.src_lumdist_mpc))
        if np.any(empty):
            raise Exception(_NO_SURVIVORS)
        _native.raise_for_status(self._row_status(raw, slot))
        mn = raw.mean[:, slot]
        res = np.stack([mn, raw.pct[:, slot, idx[1]] - mn, mn - raw.pct[:, slot, idx[0]]], axis=-1)
        return self._squeeze(res)

    @staticmethod
    def _row_status(raw, slot):
        """The SED kernels' row status codes a derived column met in any source, as raise_for_status takes them."""
        bits = int(np.bitwise_or.reduce(raw.status[:, slot])) >> _native.SUM_ROW_SHIFT
        return np.array([s for s in range(8) if bits & (1 << s)] or [0], dtype=np.int32)

    # ---- the reference's vocabulary -----------------------------------------------------------
    def par_cen(self, param, percentile=68.3, lowlim=None, uplim=None):
        """[mean, upper - mean, mean - lower] of a parameter (results.py:397-431)."""
        _check_open(percentile)
        return self._cen(_paridx(param), percentile, lowlim, uplim)

    def par_lowlim(self, param, percentile=68.3):
        """Lower limit at that confidence: the (100 - percentile)-th percentile (results.py:433-462)."""
        slot = _paridx(param)
        _check_open(percentile)
        raw, idx = self._lookup(slot, [float(100 - percentile)], None, None)
        return self._squeeze(raw.pct[:, slot, idx[0]])

    def par_uplim(self, param, percentile=68.3):
        """Upper limit at that confidence: the percentile-th percentile (results.py:464-493)."""
        slot = _paridx(param)
        _check_open(percentile)
        raw, idx = self._lookup(slot, [float(percentile)], None, None)
        return self._squeeze(raw.pct[:, slot, idx[0]])

    def peaklambda_cen(self, percentile=68.3, lowlim=None, uplim=None):
        """Observer-frame peak wavelength [um] (results.py:507-532)."""
        self._column(5, "peaklambda")
        return self._cen(5, percentile, lowlim, uplim)

    def lir_cen(self, percentile=68.3, lowlim=None, uplim=None):
        """L_IR [1e12 L_sun] (results.py:600-625)."""
        self._column(6, "lir")
        return self._cen(6, percentile, lowlim, uplim)

    def dustmass_cen(self, percentile=68.3, lowlim=None, uplim=None):
        """Dust mass [1e8 M_sun] (results.py:699-724)."""
        self._column(7, "dustmass")
        return self._cen(7, percentile, lowlim, uplim)

    @property
    def par_central_values(self):
        return np.stack([self.par_cen(i, self._percentile) for i in range(5)], axis=-2)

    @property
    def best_fit(self):
        """(parameters, lnprob, (walker, step)) of the sample of largest lnprob, ties to the first in
        [walker][step] order (results.py:160-165)."""
        r = self._raw
        if self._multi:
            return r.best[:, :5].copy(), r.best[:, 5].copy(), r.best_index.copy()
        return r.best[0, :5].copy(), float(r.best[0, 5]), (int(r.best_index[0, 0]), int(r.best_index[0, 1]))

    @property
    def best_fit_chisq(self):
        """-2 lnprob of the best sample (results.py:261-272)."""
        return -2.0 * self.best_fit[1]

    def best_fit_sed(self, wave):
        """The best-fitting SED at wavelengths `wave` [um] (results.py:274-296)."""
        pars = self._raw.best[:, :5]
        seds = [modified_blackbody(p[0], p[1], p[2], p[3], p[4], wavenorm=self._wavenorm, noalpha=self._noalpha,
                                   opthin=self._opthin, context=self._like.context)(wave) for p in pars]
        return np.array(seds) if self._multi else seds[0]

    @property
    def covariance(self):
        """numpy.cov of the five parameters over the summarised steps (ddof 1)."""
        return self._squeeze(self._raw.cov).copy()

    @property
    def n_used(self):
        """Samples per column [8]: the five parameters, peak wavelength, L_IR, dust mass (0 where not asked for)."""
        return self._squeeze(self._raw.n_used).copy()

    @property
    def mean(self):
        return self._squeeze(self._raw.mean).copy()

    @property
    def min(self):
        return self._squeeze(self._raw.min).copy()

    @property
    def max(self):
        return self._squeeze(self._raw.max).copy()

    @property
    def status(self):
        return self._squeeze(self._raw.status).copy()

    @property
    def percentiles(self):
        """(q values prepared, their values [..., 8, len(q)])"""
        return list(self._req.qs), self._squeeze(self._raw.pct).copy()

    def arrays(self, prefix="summary_"):
        """The summary as plain arrays (for an .npz)."""
        qs, pct = self.percentiles
        extra = {}
        if "lir" in self._req.derived or "dustmass" in self._req.derived:
            z, d = self._req.cosmology()
            nsrc = (self._raw.mean.shape[0],)
            extra = {prefix + "redshift": np.array(self._squeeze(np.broadcast_to(z, nsrc))),
                     prefix + "lumdist_mpc": np.array(self._squeeze(np.broadcast_to(d, nsrc)))}
        return {**extra, prefix + "n_used": self.n_used, prefix + "mean": self.mean, prefix + "min": self.min,
                prefix + "max": self.max, prefix + "q": np.array(qs), prefix + "percentiles": pct,
                prefix + "covariance": self.covariance, prefix + "best_fit": self._squeeze(self._raw.best[:, :5]).copy(),
                prefix + "best_fit_lnprob": self._squeeze(self._raw.best[:, 5]).copy(),
                prefix + "best_fit_index": self._squeeze(self._raw.best_index).copy(),
                prefix + "status": self.status}

    def __str__(self):
        """In the spirit of mbb_results.__str__ (results.py:1160-1262); the first source of a multi-source summary."""
        cen = self.par_central_values if not self._multi else self.par_central_values[0]
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(self._raw.mean.shape[0]))
        rows = [(0, "T/(1+z)", " [K]", True), (1, "beta", "", True), (4, "fnorm", " [mJy]", True),
                (2, "lambda0 (1+z)", " [um]", not self._opthin), (3, "alpha", "", not self._noalpha)]
        for i, tag, unit, used in rows:
            if not used:
                lines.append("Optically thin case assumed" if i == 2 else "Alpha not used")
            elif self._raw.min[0, i] == self._raw.max[0, i]:
                lines.append("{:s}: {:0.2f} (fixed)".format(tag, cen[i][0]))
            else:
                lines.append("{:s}: {:0.2f} +{:0.2f} -{:0.2f}{:s}".format(tag, cen[i][0], cen[i][1], cen[i][2], unit))
        first = (lambda a: a[0] if self._multi else a)
        if "peaklambda" in self._req.derived:
            lines.append("Lambda peak: {:0.1f} +{:0.1f} -{:0.1f} [um]".format(*first(self.peaklambda_cen(self._percentile))))
        if "lir" in self._req.derived:
            lines.append("L_IR({:0.1f} to {:0.1f}um): {:0.2f} +{:0.2f} -{:0.2f} [10^12 L_sun]".format(
                *(self._req.lir_range + tuple(first(self.lir_cen(self._percentile))))))
        if "dustmass" in self._req.derived:
            lines.append("M_d(kappa={0:0.2f}, lam={1:0.1f}um): {2:0.2f} +{3:0.2f} -{4:0.2f} [10^8 M_sun]".format(
                self._req.kappa, self._req.kappa_wave, *first(self.dustmass_cen(self._percentile))))
        if self._ndata is not None:
            lines.append("Number of data points: {:d}".format(self._ndata))
        lines.append("ChiSquare of best fit point: {:0.2f}".format(float(first(np.atleast_1d(self.best_fit_chisq))
                                                                         if self._multi else self.best_fit_chisq)))
        return "\n".join(lines)
