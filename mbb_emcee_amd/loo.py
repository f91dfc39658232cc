"""Out-of-sample fit of a chain, computed on the MI355X where the chain is (csrc/mbb_pointwise.hip.h): WAIC and
Pareto-smoothed importance-sampling leave-one-out cross-validation (PSIS-LOO) per source and band.

The reference has nothing comparable; people who run emcee get these numbers from ``arviz.loo`` / ``arviz.waic`` by
storing a log-likelihood blob per sample.  Here the pointwise term of every chain entry theta and band b,

    ll_b(theta) = ln p(f_b | f_-b, theta) = (ln Lambda_bb - ln 2 pi) / 2 - g_b^2 / (2 Lambda_bb),   g = Lambda (f - m(theta)),

(Lambda the inverse covariance of the data, or diag(1 / sigma^2); Buerkner, Gabry & Vehtari 2021) is formed on the
device and reduced there: lppd, p_waic and elpd_waic; elpd_loo and p_loo with the importance weights' tail smoothed by
a generalised Pareto fit (Vehtari et al., as ``loo`` 2.x ``psislw``; its shape k-hat says how far to trust the band's
number: above 0.7, not); and loo_pit, the leave-one-band-out probability that a replicated flux lies below the
measured one -- near 0 or 1 the band is an outlier.  Like chisq, ll knows no limits or priors, so two fits can be
compared by ``compare`` where improper priors leave ``bayes_factor`` without an answer.  The definitions are in
include/mbb_hip.h.  ``ChainLoo`` has the vocabulary; the numbers come from ``mbb_chain_pointwise`` (a host chain) or
``mbb_sampler_pointwise`` (the chain a ``DeviceEnsembleSampler`` run left on the device, which then never crosses the
bus).
"""
import ctypes as C

import numpy as np

from . import _analysis, _native

__all__ = ["chain_loo", "loo_rows", "ChainLoo"]

MAX_BANDS = 256
MAX_WINDOW = _native.PW_MAX_WINDOW
_TABLES = ("lppd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "khat", "loo_pit")


class _Request(_analysis.Window):
    """What one native pointwise call is asked for (mbb_pointwise_spec); everything is checked here, before the device
    is touched."""

    def __init__(self, like, burn=0, thin=1):
        # what the fit was held against, for compare(): [nsources, ndata]
        self.ndata, self.flux, self.sigma = _analysis.photometry(like, "cross-validation")
        if self.ndata > MAX_BANDS:
            raise ValueError("at most {:d} bands per pointwise call".format(MAX_BANDS))
        self.set_window(burn, thin)

    def check_steps(self, nsteps, nwalkers=1):
        """The number of kept steps per walker."""
        nkept = _analysis.Window.check_steps(self, nsteps)
        if int(nwalkers) * nkept > MAX_WINDOW:
            raise ValueError("a window of {:d} entries per source needs a longer tail than the device sorts: at most "
                             "{:d} (thin the window)".format(int(nwalkers) * nkept, MAX_WINDOW))
        return nkept

    def spec(self):
        s = _native.PointwiseSpec()
        s.burn, s.thin = self.burn, self.thin
        return s


class _Raw(object):
    """The arrays of one native pointwise call (mbb_pointwise_out): [nsrc, ndata] each."""

    def __init__(self, nsrc, ndata):
        self.n_used = np.zeros((nsrc, ndata), dtype=np.int64)
        self.tail_len = np.zeros((nsrc, ndata), dtype=np.int32)
        self.status = np.zeros((nsrc, ndata), dtype=np.int32)
        for name in _TABLES:
            setattr(self, name, np.full((nsrc, ndata), np.nan))

    def out(self):
        return _analysis.bind_out(_native.PointwiseOut, vars(self))


def loo_rows(like, pars):
    """(ll [n, ndata], row status [n]) of parameter rows [n, 5] by the device function the chain's entries go through
    (mbb_pointwise_rows).  In multi-source mode the rows are nsources equal blocks, as for ``like(pars)``."""
    p = _analysis.rows5(pars)
    ndata = _analysis.photometry(like, "cross-validation")[0]
    ctx = _native.analysis_context(like)
    n = p.shape[0]
    ll, st = np.empty((n, ndata)), np.empty(n, dtype=np.int32)
    _native.check_arg(ctx.lib.mbb_pointwise_rows(ctx.h, _native._d(p), n, _native._d(ll), _native._i(st)), ctx)
    return ll, st


def chain_loo(like, chain, burn=0, thin=1):
    """WAIC and PSIS-LOO of a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) over the steps
    ``chain[:, burn::thin]``, computed on ``like``'s device against ``like``'s data; returns a ``ChainLoo``.
    A chain of many sources may be run through a one-source likelihood: every source is then held against that
    likelihood's data, and the result keeps its leading source axis."""
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    req = _Request(like, burn, thin)
    nkept = req.check_steps(nsteps, nw)
    _analysis.check_sources(like.nsources, nsrc)
    ctx = _native.analysis_context(like)
    raw = _Raw(nsrc, req.ndata)
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_pointwise(ctx.h, _native._d(c4), nsrc, nw, nsteps, C.byref(spec), C.byref(out)), ctx)
    return ChainLoo(req, raw, multi, nw, nkept)


def _band_sum(t):
    return np.sum(t, axis=1)


def _band_se(t):
    """sqrt(nb var_b), ddof 1, of a [nsrc, nb] table: NaN for one band"""
    nb = t.shape[1]
    if nb < 2:
        return np.full(t.shape[0], np.nan)
    return np.sqrt(nb * np.var(t, axis=1, ddof=1))


class ChainLoo(_analysis.Result):
    """WAIC and PSIS-LOO of a chain from the device (a leading source axis for a multi-source result).

    Per band [..., ndata]: ``lppd_band``, ``p_waic_band``, ``elpd_waic_band``, ``elpd_loo_band``, ``p_loo_band``,
    ``khat``, ``loo_pit``, ``n_used``, ``tail_len``, ``status``.
    Per source, the sums over bands: ``elpd_loo``, ``elpd_waic``, ``p_loo``, ``p_waic``, ``lppd``; ``se_elpd_loo``,
    ``se_elpd_waic``, ``se_p_loo``, ``se_p_waic`` = sqrt(ndata var_b) with ddof 1 -- the usual error bar of a sum of
    pointwise terms, which with the 4 to 8 bands of a far-infrared SED is crude (NaN for one band); ``khat_max``.
    ``outliers(alpha)`` : which bands have loo_pit outside [alpha / 2, 1 - alpha / 2].
    ``compare(other)`` : (elpd_loo - other's, the error of the paired per-band differences) per source; both fits must
    have been held against the same bands, fluxes and uncertainties.
    status : per band the summary's bits -- EMPTY (no finite entry), HAS_NAN (entries left out), from ROW_SHIFT on the
    row status of failing SED rows inside the window -- and K_HIGH (k-hat > 0.7: the band's elpd_loo is not to be
    trusted), TAIL_SHORT (20 entries or fewer: raw weights), TAIL_FLAT (no Pareto fit possible: raw weights),
    WAIC_VAR_HIGH (p_waic > 0.4: WAIC is not to be trusted for the band)."""

    EMPTY, HAS_NAN, ROW_SHIFT = _native.SUM_EMPTY, _native.SUM_HAS_NAN, _native.SUM_ROW_SHIFT
    K_HIGH, TAIL_SHORT, TAIL_FLAT, WAIC_VAR_HIGH = (_native.PW_K_HIGH, _native.PW_TAIL_SHORT, _native.PW_TAIL_FLAT,
                                                    _native.PW_WAIC_VAR_HIGH)

    def __init__(self, request, raw, multi, nwalkers=0, nkept=0):
        self._req, self._raw, self._multi = request, raw, bool(multi)
        self._set_window(request, nwalkers, nkept)

    ndata = property(lambda self: self._req.ndata)
    n_used = property(lambda self: self._squeeze(self._raw.n_used).copy())
    tail_len = property(lambda self: self._squeeze(self._raw.tail_len).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())
    khat = property(lambda self: self._squeeze(self._raw.khat).copy())
    loo_pit = property(lambda self: self._squeeze(self._raw.loo_pit).copy())
    lppd_band = property(lambda self: self._squeeze(self._raw.lppd).copy())
    p_waic_band = property(lambda self: self._squeeze(self._raw.p_waic).copy())
    elpd_waic_band = property(lambda self: self._squeeze(self._raw.elpd_waic).copy())
    elpd_loo_band = property(lambda self: self._squeeze(self._raw.elpd_loo).copy())
    p_loo_band = property(lambda self: self._squeeze(self._raw.p_loo).copy())
    lppd = property(lambda self: self._squeeze(_band_sum(self._raw.lppd)))
    elpd_loo = property(lambda self: self._squeeze(_band_sum(self._raw.elpd_loo)))
    elpd_waic = property(lambda self: self._squeeze(_band_sum(self._raw.elpd_waic)))
    p_loo = property(lambda self: self._squeeze(_band_sum(self._raw.p_loo)))
    p_waic = property(lambda self: self._squeeze(_band_sum(self._raw.p_waic)))
    se_elpd_loo = property(lambda self: self._squeeze(_band_se(self._raw.elpd_loo)))
    se_elpd_waic = property(lambda self: self._squeeze(_band_se(self._raw.elpd_waic)))
    se_p_loo = property(lambda self: self._squeeze(_band_se(self._raw.p_loo)))
    se_p_waic = property(lambda self: self._squeeze(_band_se(self._raw.p_waic)))
    khat_max = property(lambda self: self._squeeze(np.max(self._raw.khat, axis=1)))

    def outliers(self, alpha=0.01):
        """Boolean [..., ndata]: loo_pit outside [alpha / 2, 1 - alpha / 2] (a NaN is no outlier)."""
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError("alpha must be in (0, 1)")
        pit = self._raw.loo_pit
        with np.errstate(invalid="ignore"):
            return self._squeeze((pit < 0.5 * alpha) | (pit > 1.0 - 0.5 * alpha))

    def compare(self, other):
        """(elpd_loo - other.elpd_loo, se) per source, se = sqrt(ndata var_b) (ddof 1) of the per-band differences.
        Positive: this fit predicts the left-out band better.  Refused unless both were held against the same data."""
        if not isinstance(other, ChainLoo):
            raise TypeError("compare() takes another ChainLoo")
        a, b = self._req, other._req
        if (a.ndata != b.ndata or a.flux.shape != b.flux.shape or not np.array_equal(a.flux, b.flux)
                or not np.array_equal(a.sigma, b.sigma)):
            raise ValueError("the two fits were not held against the same bands, fluxes and uncertainties")
        if self._raw.elpd_loo.shape != other._raw.elpd_loo.shape:
            raise ValueError("the two fits have different numbers of sources")
        d = self._raw.elpd_loo - other._raw.elpd_loo
        return self._squeeze(_band_sum(d)), self._squeeze(_band_se(d))

    def arrays(self, prefix="loo_"):
        """The results as plain arrays (for an .npz)."""
        r = self._raw
        out = {prefix + "ndata": np.array(self.ndata), prefix + "n_used": self.n_used, prefix + "tail_len": self.tail_len,
               prefix + "status": self.status}
        for name in _TABLES:
            out[prefix + name + ("" if name in ("khat", "loo_pit") else "_band")] = self._squeeze(getattr(r, name)).copy()
        for name in ("lppd", "elpd_loo", "elpd_waic", "p_loo", "p_waic", "se_elpd_loo", "se_elpd_waic", "se_p_loo",
                     "se_p_waic", "khat_max"):
            out[prefix + name] = np.array(getattr(self, name))
        return out

    def __str__(self):
        """The first source of a multi-source result."""
        r = self._raw
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(r.status.shape[0]))
        se = _band_se(r.elpd_loo)[0]
        lines.append("elpd_loo: {:0.3f} +- {:0.3f}  p_loo: {:0.3f}  over {:d} bands".format(
            _band_sum(r.elpd_loo)[0], se, _band_sum(r.p_loo)[0], self.ndata))
        lines.append("elpd_waic: {:0.3f}  p_waic: {:0.3f}".format(_band_sum(r.elpd_waic)[0], _band_sum(r.p_waic)[0]))
        lines.append("Pareto k-hat per band: " + " ".join("{:0.2f}".format(k) for k in r.khat[0]))
        lines.append("LOO-PIT per band: " + " ".join("{:0.3f}".format(p) for p in r.loo_pit[0]))
        bad = np.nonzero(np.atleast_2d(self.outliers())[0])[0]
        if len(bad):
            lines.append("Outlying bands (1%): " + " ".join(str(int(b)) for b in bad))
        if np.any(r.status[0] & self.K_HIGH):
            lines.append("Warning: k-hat above 0.7 in band(s) " +
                         " ".join(str(int(b)) for b in np.nonzero(r.status[0] & self.K_HIGH)[0]))
        return "\n".join(lines)
