"""Predicted fluxes of a chain, computed on the MI355X where the chain is (csrc/mbb_predict.hip.h).

The reference's ``mbb_results.predflux_cen`` (reference mbb_emcee/results.py:895-985) is the posterior interval of the
model flux at a wavelength or through a passband: ``_predict_flux`` for every chain entry, then ``_parcen_internal``'s
mean and percentiles.  ``ChainPredictions`` has that vocabulary; the numbers come from ``mbb_chain_predict`` (a host
chain) or ``mbb_sampler_predict`` (the chain a ``DeviceEnsembleSampler`` run left on the device, which then never
crosses the bus).  Percentiles are numpy's default ("linear") of exact order statistics.

A prediction target reaches the library as a plain list of quadrature samples (frequency in GHz, weight): a
passband's ``response.quadrature()``, or the one frequency ``um_to_GHz / wavelength`` with weight 1.  Any band of the
fit's wheel can be predicted, whether the fit used it or not.
"""
import ctypes as C

import numpy as np

from . import _analysis, _native
from . import results
from ._analysis import quantiles as _quantiles
from .modified_blackbody import um_to_GHz

__all__ = ["chain_predictions", "ChainPredictions"]


def _key(spec):
    """A spec as the results name it: a band's name, or the wavelength as a float."""
    return str(spec) if isinstance(spec, str) else float(spec)


def parse_specs(like, specs):
    """(list of spec keys, whether one spec was given alone), refused as ``postprocess.predict_flux`` refuses."""
    single = isinstance(specs, str) or np.isscalar(specs)
    given = [specs] if single else list(specs)
    for s in given:
        if isinstance(s, (bool, np.bool_)):
            raise ValueError("a prediction spec is a wavelength in um or a passband name, not {!r}".format(bool(s)))
    keys = [_key(s) for s in given]
    if not keys:
        raise ValueError("no prediction spec given")
    for k in keys:
        if not isinstance(k, str) and not k > 0:
            raise ValueError("Invalid wavelength {:f}".format(k))
    names = [k for k in keys if isinstance(k, str)]
    if names:
        if not like.response_integrate:
            raise Exception("Asked for response integration, but no response functions "
                            "available from original fit")
        for nm in names:
            if nm not in like._responsewheel:
                raise ValueError("Do not have response function matching {:s}".format(nm))
    if len(set(keys)) != len(keys):
        raise ValueError("a prediction spec is given twice")
    return keys, single


def sample_lists(like, keys):
    """(sample_off [nspec + 1] int32, freq [GHz], weight) of parsed specs."""
    off, freq, weight = [0], [], []
    for k in keys:
        if isinstance(k, str):
            f, w = like._responsewheel[k].quadrature()
        else:
            f, w = np.array([um_to_GHz / k]), np.ones(1)
        freq.append(np.asarray(f, dtype=np.float64).ravel())
        weight.append(np.asarray(w, dtype=np.float64).ravel())
        off.append(off[-1] + freq[-1].size)
    return np.array(off, dtype=np.int32), np.concatenate(freq), np.concatenate(weight)


class _Request(_analysis.Window):
    """What one native prediction call is asked for (mbb_predict_spec); everything is checked here, before the
    device is touched."""

    def __init__(self, like, specs, qs, burn=0, thin=1, clip=None, wavenorm=None):
        self.keys, self.single = parse_specs(like, specs)
        if len(self.keys) > _native.PRED_MAX_SPECS:
            raise ValueError("at most {:d} specs per prediction call".format(_native.PRED_MAX_SPECS))
        self.sample_off, self.freq, self.weight = sample_lists(like, self.keys)
        if self.freq.size > _native.PRED_MAX_SAMPLES:
            raise ValueError("at most {:d} quadrature samples per prediction call".format(_native.PRED_MAX_SAMPLES))
        if not (np.all(np.isfinite(self.freq)) and np.all(self.freq > 0) and np.all(np.isfinite(self.weight))):
            raise ValueError("a spec's frequencies must be finite and positive, its weights finite")
        self.qs = [float(q) for q in qs]
        if not 1 <= len(self.qs) <= _native.SUMMARY_MAX_PCT:
            raise ValueError("a prediction call takes 1 to {:d} percentiles".format(_native.SUMMARY_MAX_PCT))
        for q in self.qs:
            if not (0 <= q <= 100):
                raise ValueError("Invalid percentile {:f}".format(q))
        self.set_window(burn, thin)
        self.wavenorm = 0.0 if wavenorm is None else float(wavenorm)
        if wavenorm is not None and not (0 < self.wavenorm < np.inf):
            raise ValueError("wavenorm must be positive")
        self.clip = {}
        for key, (lo, hi) in (clip or {}).items():
            self.clip[self.index(key)] = (None if lo is None else float(lo), None if hi is None else float(hi))

    def index(self, spec):
        k = _key(spec)
        if k not in self.keys:
            raise ValueError("{} was not asked for when the predictions were made".format(spec))
        return self.keys.index(k)

    def only(self, i, qs, lo, hi):
        """The same request for spec i alone, other percentiles and another clipping."""
        import copy
        r = copy.copy(self)
        s0, s1 = int(self.sample_off[i]), int(self.sample_off[i + 1])
        r.keys = [self.keys[i]]
        r.sample_off = np.array([0, s1 - s0], dtype=np.int32)
        r.freq, r.weight = self.freq[s0:s1].copy(), self.weight[s0:s1].copy()
        r.qs = [float(q) for q in qs]
        r.clip = {0: (lo, hi)} if (lo is not None or hi is not None) else {}
        return r

    def spec(self):
        s = _native.PredictSpec()
        n = len(self.keys)
        s.nspec, s.npct, s.burn, s.thin = n, len(self.qs), self.burn, self.thin
        for i, q in enumerate(self.qs):
            s.pct[i] = q
        s.wavenorm = self.wavenorm
        # (the arrays live as long as the spec that points at them)
        s._keep = [np.ascontiguousarray(self.sample_off, dtype=np.int32), _native._f64(self.freq), _native._f64(self.weight)]
        s.sample_off, s.freq, s.weight = _native._i(s._keep[0]), _native._d(s._keep[1]), _native._d(s._keep[2])
        if self.clip:
            has_lo, has_hi = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
            lo, hi = np.zeros(n), np.zeros(n)
            for i, (a, b) in self.clip.items():
                if a is not None:
                    has_lo[i], lo[i] = 1, a
                if b is not None:
                    has_hi[i], hi[i] = 1, b
            s._keep += [has_lo, has_hi, lo, hi]
            s.has_lo, s.has_hi, s.lo, s.hi = _native._i(has_lo), _native._i(has_hi), _native._d(lo), _native._d(hi)
        return s


class _Raw(object):
    """The arrays of one native prediction call (mbb_predict_out), nsrc leading."""

    def __init__(self, nsrc, nspec, npct):
        self.n_used = np.zeros((nsrc, nspec), dtype=np.int64)
        self.mean = np.full((nsrc, nspec), np.nan); self.min = np.full((nsrc, nspec), np.nan)
        self.max = np.full((nsrc, nspec), np.nan)
        self.pct = np.full((nsrc, nspec, npct), np.nan)
        self.status = np.zeros((nsrc, nspec), dtype=np.int32)

    def out(self):
        return _analysis.bind_out(_native.PredictOut, vars(self))


def _predict_host(like, c4, req):
    """mbb_chain_predict on a host chain [nsrc, nw, nsteps, 5]."""
    ctx = _native.analysis_context(like)
    nsrc, nw, nsteps = c4.shape[:3]
    raw = _Raw(nsrc, len(req.keys), len(req.qs))
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_predict(ctx.h, _native._d(c4), nsrc, nw, nsteps, C.byref(spec), C.byref(out)), ctx)
    return raw


def chain_predictions(like, chain, specs, percentile=68.3, percentiles=(), burn=0, thin=1, clip=None, wavenorm=None,
                      keep=True):
    """Predicted fluxes [mJy] of a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) over the steps
    ``chain[:, burn::thin]``, computed on ``like``'s device; returns a ``ChainPredictions``.

    specs : a wavelength in um, the name of a passband of ``like``'s filter wheel (in the fit or not), or a list mixing
        both -- ``postprocess.predict_flux``'s, with its refusals;
    percentile : the central interval(s) prepared, a number or a few;  percentiles : further plain percentiles -- at
        most eight q values in all; whatever else is asked of the result later costs another call;
    clip : ``{spec: (lowlim, uplim)}`` applied as ``_parcen_internal`` does (either may be None);
    wavenorm : None for the fit's own normalisation wavelength (``postprocess.predict_flux``'s note);
    keep : keep the chain with the result, so that other percentiles and clip bounds can be computed on demand."""
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    cens, qs = _quantiles(percentile, percentiles)
    req = _Request(like, specs, qs, burn, thin, clip, wavenorm)
    nkept = req.check_steps(nsteps)
    raw = _predict_host(like, c4, req)
    again = (lambda r: _predict_host(like, c4, r)) if keep else None
    return ChainPredictions(req, raw, multi, again, cens[0], nw, nkept)


class ChainPredictions(_analysis.Result):
    """What ``mbb_results.predflux_cen`` reports of a chain, from the device's prediction (a leading source axis for
    a multi-source chain).  A spec is named as it was asked for: the band's name, or the wavelength.

    predflux_cen(spec) : [mean, upper - mean, mean - lower];
    sed_band() : (wavelengths, lower, mean, upper) over the wavelength specs;
    mean, min, max, n_used, status : per spec [nspec]; percentiles : (q values prepared, values [..., nspec, len(q)]);
    status : the summary's bits -- EMPTY (nothing survives the clip), HAS_NAN, and from ROW_SHIFT on the row status
        of failing SED rows inside the window."""

    EMPTY, HAS_NAN, ROW_SHIFT = _native.SUM_EMPTY, _native.SUM_HAS_NAN, _native.SUM_ROW_SHIFT

    def __init__(self, request, raw, multi, again=None, percentile=68.3, nwalkers=0, nkept=0):
        self._req, self._raw, self._multi, self._again = request, raw, multi, again
        self._percentile = float(percentile)
        self._cache = {}
        self._set_window(request, nwalkers, nkept)

    def drop_chain(self):
        """Forget how to compute more from the chain (a sampler's next run overwrites it on the device)."""
        self._again = None

    @property
    def specs(self):
        return list(self._req.keys)

    def _lookup(self, i, qs, lowlim, uplim):
        """(raw arrays, column in them, indices of qs in them) for spec i clipped to [lowlim, uplim]."""
        lo = None if lowlim is None else float(lowlim)
        hi = None if uplim is None else float(uplim)
        have = self._req.clip.get(i, (None, None))
        if have == (lo, hi) and all(q in self._req.qs for q in qs):
            return self._raw, i, [self._req.qs.index(q) for q in qs]
        key = (i, lo, hi, tuple(qs))
        if key not in self._cache:
            if self._again is None:
                raise RuntimeError("these predictions were made without these percentiles / clip bounds and the chain "
                                   "was not kept: ask for them when the predictions are made (percentile=, "
                                   "percentiles=, clip=), or keep the chain")
            self._cache[key] = self._again(self._req.only(i, qs, lo, hi))
        return self._cache[key], 0, list(range(len(qs)))

    def predflux_cen(self, spec, percentile=68.3, lowlim=None, uplim=None):
        """[mean, upper - mean, mean - lower] of the predicted flux (results.py:946-985).  As ``ChainSummary``'s
        intervals: raises when nothing survives the clipping, or -- as ``postprocess.predict_flux`` does for the
        same chain -- when an SED row inside the burn / thin window fails, in ANY source of a multi-source chain; a
        NaN parameter gives NaN and does not raise."""
        i = self._req.index(spec)
        qs = list(results._pval(percentile))
        raw, col, idx = self._lookup(i, qs, lowlim, uplim)
        if np.any((raw.status[:, col] & _native.SUM_EMPTY) != 0):
            raise Exception(results._NO_SURVIVORS)
        _native.raise_for_status(results.ChainSummary._row_status(raw, col))
        mn = raw.mean[:, col]
        res = np.stack([mn, raw.pct[:, col, idx[1]] - mn, mn - raw.pct[:, col, idx[0]]], axis=-1)
        return self._squeeze(res)

    def sed_band(self, percentile=68.3):
        """(wavelengths [um] ascending, lower, mean, upper) of the wavelength specs: the SED envelope of a plot;
        lower / mean / upper carry a leading source axis for a multi-source chain."""
        waves = sorted(k for k in self._req.keys if not isinstance(k, str))
        if not waves:
            raise ValueError("no wavelength spec among the predictions")
        cen = np.stack([np.atleast_2d(self.predflux_cen(w, percentile)) for w in waves], axis=1)   # [nsrc, nwave, 3]
        mean = cen[..., 0]
        return np.array(waves), self._squeeze(mean - cen[..., 2]), self._squeeze(mean), self._squeeze(mean + cen[..., 1])

    n_used = property(lambda self: self._squeeze(self._raw.n_used).copy())
    mean = property(lambda self: self._squeeze(self._raw.mean).copy())
    min = property(lambda self: self._squeeze(self._raw.min).copy())
    max = property(lambda self: self._squeeze(self._raw.max).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())

    @property
    def percentiles(self):
        """(q values prepared, their values [..., nspec, len(q)])"""
        return list(self._req.qs), self._squeeze(self._raw.pct).copy()

    def arrays(self, prefix="predict_"):
        """The predictions as plain arrays (for an .npz)."""
        qs, pct = self.percentiles
        return {prefix + "specs": np.array([str(k) for k in self._req.keys]), prefix + "n_used": self.n_used,
                prefix + "mean": self.mean, prefix + "min": self.min, prefix + "max": self.max,
                prefix + "q": np.array(qs), prefix + "percentiles": pct, prefix + "status": self.status}

    def __str__(self):
        """One line per spec; the first source of a multi-source result."""
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(self._raw.status.shape[0]))
        for k in self._req.keys:
            tag = k if isinstance(k, str) else "{:0.1f}um".format(k)
            try:
                c = np.atleast_2d(self.predflux_cen(k, self._percentile))[0]
                lines.append("Predicted flux {:s}: {:0.2f} +{:0.2f} -{:0.2f} [mJy]".format(tag, c[0], c[1], c[2]))
            except Exception as e:       # noqa -- a line per spec, whatever one of them raises
                lines.append("Predicted flux {:s}: {}".format(tag, e))
        return "\n".join(lines)
