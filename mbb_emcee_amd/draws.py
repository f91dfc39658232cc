"""Posterior draws of a chain taken where the chain is (mbb_draws.hip.h): per source n cells of the chain with
their parameters, log-probability, (walker, step) and -- for the drawn rows alone -- peak wavelength, L_IR and dust
mass, without the chain leaving the device.

The reference's ``mbb_results.choice()`` (results.py:803-893) is the model: cells uniform over walkers x steps with
replacement, and its return tuple is ``ChainDraws.choice()``'s.  The derived values are computed by the kernels a
summary uses, so a drawn row's are the bits the summary of that one cell reports.

The random stream is the device's Philox4x32-10 keyed by ``seed`` -- not numpy's global generator, so a draw is not
reproducible against ``np.random.seed`` as the reference's is; it is reproducible against ``seed``.
"""
import ctypes as C

import numpy as np

from . import _analysis, _native
from . import results

__all__ = ["chain_draws", "draw_indices", "ChainDraws"]

_HOW = {"random": _native.DRAWS_RANDOM, "even": _native.DRAWS_EVEN}
_DERIVED_ORDER = ("peaklambda", "lir", "dustmass")
# the reference's messages (results.py:840-845)
_NOT_COMPUTED = {"peaklambda": "Peak lambda not computed", "lir": "LIR not computed", "dustmass": "Dustmass not computed"}


def _check_picks(n, how, seed, nsources):
    """n, how and seed of a request as the library takes them."""
    n = int(n)
    if n < 1:
        raise ValueError("n must be at least 1")
    if n > _native.DRAWS_MAX:
        raise ValueError("at most {:d} draws per source".format(_native.DRAWS_MAX))
    if int(nsources) * n > 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 1 draws per call")
    if how not in _HOW:
        raise ValueError("how must be 'random' or 'even'")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64)")
    return n, how, seed


class _Request(_analysis.Window):
    """What one native draws call is asked for (mbb_draws_spec); everything is checked here, before the device is
    touched."""

    def __init__(self, n=1, how="random", seed=0, burn=0, thin=1, derived=(), redshift=None, lumdist_mpc=None,
                 kappa=2.64, kappa_wave=125.0, lir_range=(8.0, 1000.0), peak_model="fit", nsources=1):
        # burn, thin and the derived columns' settings are a summary request's (its percentiles are not used)
        self.summary = results._Request([50.0], burn, thin, None, derived, redshift, lumdist_mpc, kappa, kappa_wave,
                                        lir_range, peak_model, nsources=nsources)
        self.burn, self.thin, self.derived = self.summary.burn, self.summary.thin, self.summary.derived
        self.n, self.how, self.seed = _check_picks(n, how, seed, nsources)

    def spec(self):
        s = _native.DrawsSpec()
        s.n, s.how, s.seed = self.n, _HOW[self.how], self.seed
        # (the summary spec lives as long as the spec that points at it)
        s._summary = self.summary.spec()
        s.summary = C.pointer(s._summary)
        return s


class _Raw(object):
    """The arrays of one native draws call (mbb_draws_out), nsrc leading."""

    def __init__(self, nsrc, n, derived=()):
        self.rows = np.empty((nsrc, n, 5))
        self.lnprob = np.empty((nsrc, n))
        self.index = np.zeros((nsrc, n, 2), dtype=np.int32)
        self.derived = {d: np.empty((nsrc, n)) for d in _DERIVED_ORDER if d in derived}
        self.status = np.zeros((nsrc, _native.SUMMARY_COLS), dtype=np.int32)

    def out(self):
        return _analysis.bind_out(_native.DrawsOut, dict(vars(self), derived=[self.derived.get(d) for d in _DERIVED_ORDER]))


class ChainDraws(_analysis.Result):
    """Draws from a chain (a leading source axis for a multi-source chain).

    params [n, 5], lnprob [n] (NaN when the chain came without one), index [n, 2] (walker, step) : the drawn cells,
        copies of the chain's bit for bit;
    peaklambda, lir, dustmass [n] : the derived values of the drawn rows; the reference's "... not computed" Exception
        when they were not asked for (derived=);
    status [8] : per column, from ROW_SHIFT on the row status of drawn rows the SED kernels failed on (their derived
        value is NaN), as a summary reports them; ABSENT for a derived column not asked for;
    choice(getpeaklambda, getlir, getdustmass) : the reference's tuple;
    flux(spec) : the model flux of every draw at a wavelength or through a passband."""

    ABSENT, ROW_SHIFT = _native.SUM_ABSENT, _native.SUM_ROW_SHIFT

    def __init__(self, like, request, raw, multi, nwalkers, nkept):
        self._like, self._req, self._raw, self._multi = like, request, raw, multi
        self.n, self.how, self.seed = request.n, request.how, request.seed
        self._set_window(request, nwalkers, nkept)

    def _derived(self, name):
        if name not in self._raw.derived:
            raise Exception(_NOT_COMPUTED[name])
        return self._squeeze(self._raw.derived[name]).copy()

    params = property(lambda self: self._squeeze(self._raw.rows).copy())
    lnprob = property(lambda self: self._squeeze(self._raw.lnprob).copy())
    index = property(lambda self: self._squeeze(self._raw.index).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())
    peaklambda = property(lambda self: self._derived("peaklambda"))
    lir = property(lambda self: self._derived("lir"))
    dustmass = property(lambda self: self._derived("dustmass"))

    def choice(self, getpeaklambda=False, getlir=False, getdustmass=False):
        """The reference's ``choice(nsamples=n, ...)`` tuple (results.py:803-893): the parameters [n, 5], then -- in
        that order -- the peak wavelengths, L_IR and dust masses [n] that were asked for; for n == 1 flattened to a
        5-vector and floats.  A multi-source result has its source axis in front of each.  The draws are the ones
        made when this object was: uniform over walkers x steps with replacement for how="random", from the device's
        Philox stream of ``seed`` and not from numpy's global generator (``np.random.seed`` has no say)."""
        want = [name for name, flag in zip(_DERIVED_ORDER, (getpeaklambda, getlir, getdustmass)) if flag]
        for name in want:
            if name not in self._raw.derived:
                raise Exception(_NOT_COMPUTED[name])
        one = self.n == 1
        ret = (self._squeeze(self._raw.rows[:, 0] if one else self._raw.rows).copy(),)
        for name in want:
            v = self._raw.derived[name]
            if one:
                ret += (v[:, 0].copy() if self._multi else float(v[0, 0]),)
            else:
                ret += (self._squeeze(v).copy(),)
        return ret

    def flux(self, spec, wavenorm=None):
        """Predicted flux density [mJy] of every draw: ``spec`` is a wavelength in um, a passband name of the fit's
        filter wheel, or a list of both (then a trailing axis of that length) -- ``postprocess.predict_flux`` on the
        drawn rows."""
        from . import postprocess
        return postprocess.predict_flux(self._like, self._squeeze(self._raw.rows), spec, wavenorm=wavenorm)

    def arrays(self, prefix="draws_"):
        """The draws as plain arrays (for an .npz): params [..., n, 5], lnprob [..., n], index [..., n, 2], status
        [..., 8], and the derived values [..., n] that were asked for."""
        out = {prefix + "params": self.params, prefix + "lnprob": self.lnprob, prefix + "index": self.index,
               prefix + "status": self.status}
        for name in self._raw.derived:
            out[prefix + name] = self._derived(name)
        return out

    def __str__(self):
        """Mean and standard deviation of every column over the draws; the first source of a multi-source result."""
        r = self._raw
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(r.rows.shape[0]))
        lines.append("{:d} {:s} draws from {:d} steps of {:d} walkers (seed {:d})".format(
            self.n, self.how, self.nsteps_used, self.nwalkers, self.seed))
        cols = [(nm, r.rows[0, :, k]) for k, nm in enumerate(("T", "beta", "lambda0", "alpha", "fnorm"))]
        cols += [(nm, r.derived[nm][0]) for nm in r.derived]
        for nm, v in cols:
            fin = v[np.isfinite(v)]
            if fin.size == 0:
                lines.append("  {:10s} no finite draw".format(nm))
            else:
                lines.append("  {:10s} mean: {:.6g}  std: {:.6g}  not finite: {:d}".format(
                    nm, fin.mean(), fin.std(), int(v.size - fin.size)))
        return "\n".join(lines)


def chain_draws(like, chain, lnprob=None, n=1, how="random", seed=0, burn=0, thin=1, derived=(), redshift=None,
                lumdist_mpc=None, kappa=2.64, kappa_wave=125.0, lir_range=(8.0, 1000.0), peak_model="fit"):
    """``n`` draws per source from a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) over the steps
    ``chain[:, burn::thin]``, made on ``like``'s device; returns a ``ChainDraws``.

    lnprob : the chain's log-probability [nw, nsteps] ([nsources, nw, nsteps]) or None (the draws' is then NaN);
    how : "random" -- the reference's ``choice()``: uniform over walkers x steps, with replacement -- or "even":
        draw i is cell floor(i N / n) of the window's N = nw * nkept cells in flattened order, deterministic and
        without repeats while n <= N;
    seed : of the device's Philox stream (0 .. 2^64 - 1).  Not numpy's global generator: ``np.random.seed`` does not
        make a draw reproducible, ``seed`` does;
    derived, redshift, lumdist_mpc, kappa, kappa_wave, lir_range, peak_model : ``results.chain_summary``'s; the
        derived values are computed for the drawn rows only."""
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    l3 = None if lnprob is None else _analysis.lnprob_like(lnprob, c4, multi)
    req = _Request(n, how, seed, burn, thin, derived, redshift, lumdist_mpc, kappa, kappa_wave, lir_range, peak_model,
                   nsources=nsrc)
    nkept = req.check_steps(nsteps)
    ctx = _native.analysis_context(like)
    raw = _Raw(nsrc, req.n, req.derived)
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_draws(ctx.h, _native._d(c4), None if l3 is None else _native._d(l3), nsrc, nw,
                                              nsteps, C.byref(spec), C.byref(out)), ctx)
    return ChainDraws(like, req, raw, multi, nw, nkept)


def draw_indices(nwalkers, nsteps, n, how="random", seed=0, burn=0, thin=1, nsources=1, like=None):
    """The picks alone: the (walker, step) [n, 2] ([nsources, n, 2] when nsources > 1) that ``chain_draws`` with the
    same n, how, seed, burn and thin draws from a chain of ``nwalkers`` x ``nsteps`` -- for indexing a stored chain on
    the host.  Made on ``like``'s device (the default context's when None)."""
    nsources, nwalkers, nsteps = int(nsources), int(nwalkers), int(nsteps)
    if nsources < 1 or nwalkers < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    n, how, seed = _check_picks(n, how, seed, nsources)
    burn, thin = int(burn), int(thin)
    if burn < 0 or thin < 1:
        raise ValueError("burn must be >= 0 and thin >= 1")
    if burn >= nsteps:
        raise ValueError("burn leaves no step of the chain")
    ctx = like.context if like is not None else _native.default_context()
    index = np.zeros((nsources, n, 2), dtype=np.int32)
    _native.check_arg(ctx.lib.mbb_draw_indices(ctx.h, nsources, nwalkers, nsteps, burn, thin, n, _HOW[how], seed,
                                               _native._i(index)), ctx)
    return index if nsources > 1 else index[0]
