"""The evidence of a fit, ln Z per source, bridge-sampled on the MI355X where the chain is (csrc/mbb_evidence.hip.h).

The reference has nothing comparable, and DIC (``goodness.ChainGoodness.dic``) is a point-estimate heuristic.  What
decides between two models of the same data -- optically thin or thick, with the alpha power law or without, beta free or
held -- is the marginal likelihood ``Z = integral of P(theta) d theta`` of each fit, P being what ``like(theta)`` returns
before the logarithm: likelihood x hard lower limits x soft upper walls x Gaussian priors, over the parameters that are
free.  Bridge sampling (Meng & Wong 1996; the recipe of Gronau et al. 2017) gets it from a chain and its lnprob: a
Gaussian proposal is fitted to the first half of the window, N2 draws of it are evaluated with the likelihood's own
batch call, and a fixed-point iteration bridges them to the second half of the window.  ``include/mbb_hip.h`` has the
definitions.  ``lnz`` is the integral of the *unnormalised* P; ``ln_prior_norm`` is the closed-form normalisation of
the separable prior factors, and ``ChainEvidence.ln_evidence = lnz - ln_prior_norm`` is what two fits are compared by
(``bayes_factor``).
"""
import ctypes as C
import math

import numpy as np

from . import _analysis, _native

__all__ = ["chain_evidence", "ChainEvidence", "ln_prior_norm"]

TOL, MAXITER = 1e-10, 1000
MAX_N2, MAX_ITER = _native.EV_MAX_N2, _native.EV_MAX_ITER
DEFAULT_SEED = 0x6272696467653031
PARAM_NAMES = ("T", "beta", "lambda0", "alpha", "fnorm")
WALL_REL_WIDTH = 0.02       # the soft upper wall's width over (uplim - lowlim): likelihood._uplim_prior


def _fixed5(fixed):
    f = np.zeros(5, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool).ravel()
    if f.size != 5:
        raise ValueError("fixed must have five entries")
    return f


def _model_held(like):
    return np.array([False, False, bool(like.opthin), bool(like.noalpha), False])


def _ln_factor_norm(lo, up, mean, sigma):
    """ln of the integral over x >= lo of [wall above up] x [Gaussian prior]; up or mean None: that factor is absent."""
    r2 = math.sqrt(2.0)
    hp = math.sqrt(math.pi / 2.0)
    if up is not None and mean is None:
        lw = WALL_REL_WIDTH * (up - lo)
        return math.log((up - lo) + lw * hp)
    if up is None:
        v = sigma * hp * math.erfc((lo - mean) / (sigma * r2))
        return math.log(v) if v > 0.0 else -math.inf
    lw = WALL_REL_WIDTH * (up - lo)
    inner = sigma * hp * (math.erfc((lo - mean) / (sigma * r2)) - math.erfc((up - mean) / (sigma * r2)))
    tau = 1.0 / lw ** 2 + 1.0 / sigma ** 2
    cen, s = (up / lw ** 2 + mean / sigma ** 2) / tau, 1.0 / math.sqrt(tau)
    outer = math.exp(-0.5 * (up - mean) ** 2 / (lw ** 2 + sigma ** 2)) * s * hp * math.erfc((up - cen) / (s * r2))
    v = inner + outer
    return math.log(v) if v > 0.0 else -math.inf


def ln_prior_norm(like, fixed=None):
    """(ln N, improper [5], has_peak_term): N is the integral of the separable prior factors of ``like`` over its free
    parameters -- per parameter ``1[x >= lowlim]`` times the soft upper wall (flat up to uplim, then a half-Gaussian of
    width 0.02 (uplim - lowlim)) where it has an upper limit, times its Gaussian prior where it has one --, in closed
    form with erfc.  ``improper[i]``: parameter i is free and has neither, so its factor cannot be normalised and the
    sum leaves it out.  ``has_peak_term``: an upper limit or a prior on the peak wavelength is set; that term is not
    separable and stays inside ``lnz``."""
    held = _fixed5(fixed) | _model_held(like)
    improper = np.zeros(5, dtype=bool)
    total = 0.0
    for i in range(5):
        if held[i]:
            continue
        has_up, has_g = bool(like._has_uplim[i]), bool(like._has_gprior[i])
        if not has_up and not has_g:
            improper[i] = True
            continue
        total += _ln_factor_norm(float(like._lowlim[i]), float(like._uplim[i]) if has_up else None,
                                 float(like._gprior_mean[i]) if has_g else None,
                                 float(like._gprior_sigma[i]) if has_g else None)
    return total, improper, bool(like._has_uplim[5] or like._has_gprior[5])


class _Request(_analysis.Window):
    """What one native evidence call is asked for (mbb_evidence_spec); everything is checked here, before the device is
    touched."""

    def __init__(self, like, n2=None, fixed=None, seed=DEFAULT_SEED, burn=0, thin=1, tol=TOL, maxiter=MAXITER,
                 first_source=0, keep=False):
        if not like.data_read:
            raise Exception("Data not read: an evidence needs the likelihood's photometry")
        self.fixed = _fixed5(fixed)
        self.n2 = 0 if n2 is None else int(n2)
        if not 0 <= self.n2 <= MAX_N2:
            raise ValueError("n2 must be 0 (as many draws as posterior samples) to {:d}".format(MAX_N2))
        self.seed = int(seed) & 0xffffffffffffffff
        self.set_window(burn, thin)
        self.tol = float(tol)
        if not (np.isfinite(self.tol) and self.tol >= 0):
            raise ValueError("tol must be finite and not negative")
        self.maxiter = int(maxiter)
        if not 1 <= self.maxiter <= MAX_ITER:
            raise ValueError("maxiter must be 1 to {:d}".format(MAX_ITER))
        self.first_source = int(first_source)
        if self.first_source < 0:
            raise ValueError("first_source must not be negative")
        self.keep = bool(keep)
        self.ln_norm, self.improper, self.peak_term = ln_prior_norm(like, self.fixed)
        self.model_held = _model_held(like)
        self.neff = None

    def check_steps(self, nsteps):
        """(kept steps per walker, those that fit the proposal)"""
        nkept = _analysis.Window.check_steps(self, nsteps)
        if nkept < 2:
            raise ValueError("an evidence needs two kept steps at least: one half fits the proposal, the other is "
                             "bridged to")
        return nkept, nkept // 2

    def set_neff(self, neff, nsrc):
        if neff is None:
            self.neff = None
            return
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(neff, dtype=np.float64), (nsrc,)))
        if not np.all(np.isfinite(v) & (v > 0)):
            raise ValueError("neff must be finite and positive")
        self.neff = v

    def neff_from_ess(self, ess, status, n1):
        """The smallest effective sample size over the free parameters per source; a parameter whose series is constant
        or whose ess is not finite is passed over, and n1 stands where none is left."""
        ess = np.atleast_2d(np.asarray(ess, dtype=np.float64))
        status = np.atleast_2d(status)
        use = ~(self.fixed | self.model_held)[None, :] & np.isfinite(ess) & (ess > 0) & ((status & _native.DIAG_CONSTANT) == 0)
        v = np.where(use, ess, np.inf).min(axis=1)
        return np.where(np.isfinite(v), v, float(n1))

    def spec(self):
        s = _native.EvidenceSpec()
        s.burn, s.thin, s.n2, s.maxiter, s.first_source = self.burn, self.thin, self.n2, self.maxiter, self.first_source
        for i in range(5):
            s.fixed[i] = int(self.fixed[i])
        s.tol, s.seed = self.tol, self.seed
        s.neff = _native._d(self.neff) if self.neff is not None else None
        return s


class _Raw(object):
    """The arrays of one native evidence call (mbb_evidence_out), nsrc leading."""

    def __init__(self, nsrc, n1, n2, keep):
        self.lnz = np.full(nsrc, np.nan); self.lnz_err = np.full(nsrc, np.nan)
        self.niter = np.zeros(nsrc, dtype=np.int32); self.status = np.zeros(nsrc, dtype=np.int32)
        self.n1 = np.zeros(nsrc, dtype=np.int64); self.n_inside = np.zeros(nsrc, dtype=np.int64)
        self.prop_mean = np.full((nsrc, 5), np.nan); self.prop_cov = np.full((nsrc, 5, 5), np.nan)
        self.n2 = int(n2)
        self.prop = np.full((nsrc, n2, 5), np.nan) if keep else None
        self.prop_lnprob = np.full((nsrc, n2), np.nan) if keep else None
        self.prop_lnq = np.full((nsrc, n2), np.nan) if keep else None
        self.post_lnq = np.full((nsrc, n1), np.nan) if keep else None

    def out(self):
        # (the draws and their terms: None, and null fields, unless kept)
        return _analysis.bind_out(_native.EvidenceOut, dict(vars(self), n2_inside=self.n_inside))


def chain_evidence(like, chain, lnprob, n2=None, fixed=None, neff="auto", seed=DEFAULT_SEED, burn=0, thin=1, tol=TOL,
                   maxiter=MAXITER, first_source=0, keep=False):
    """ln Z of a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) with its lnprob [nw, nsteps]
    ([nsources, nw, nsteps]) over the steps ``chain[:, burn::thin]``, on ``like``'s device; returns a ``ChainEvidence``.

    The first half of the kept steps of every walker fits the Gaussian proposal, the second half is bridged to.
    n2 : proposal draws per source (None or 0: as many as posterior samples), at most 2^22;
    fixed : five flags, the parameters the fit held (``mbb_fitter`` knows its own); lambda0 of a thin model, alpha of a
        model without one, and any parameter whose column is constant over the window are held as well;
    neff : "auto" -- the smallest ``ess`` over the free parameters from ``diagnostics.chain_diagnostics`` of the bridged
        half --, None (the samples count as independent), a number or one per source.  It weights the two sums and
        scales the second term of the error;
    seed : of the proposal draws (a stream apart from the stretch move's and from ``draws``);
    tol, maxiter : the iteration stops when rho changes by less than tol of itself;
    first_source : the number the call's first source has in the random stream, so that a source run alone repeats what
        it got in a catalogue;
    keep : also bring back the proposal rows, their lnprob and lnq, and lnq at the posterior samples."""
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    req = _Request(like, n2, fixed, seed, burn, thin, tol, maxiter, first_source, keep)
    nkept, nfit = req.check_steps(nsteps)
    _analysis.check_sources(like.nsources, nsrc)
    if lnprob is None:
        raise ValueError("an evidence needs the chain's lnprob")
    lp = _analysis.lnprob_like(lnprob, c4, multi)
    n1 = nw * (nkept - nfit)
    if isinstance(neff, str):
        if neff != "auto":
            raise ValueError("neff must be 'auto', None, a number or one number per source")
        from . import diagnostics
        half = np.ascontiguousarray(c4[:, :, req.burn + nfit * req.thin::req.thin])
        dg = diagnostics.chain_diagnostics(like, half)
        req.set_neff(req.neff_from_ess(dg.ess, dg.status, n1), nsrc)
    else:
        req.set_neff(neff, nsrc)
    ctx = _native.analysis_context(like)
    raw = _Raw(nsrc, n1, req.n2 or n1, req.keep)
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_evidence(ctx.h, _native._d(c4), _native._d(lp), nsrc, nw, nsteps,
                                                 C.byref(spec), C.byref(out)), ctx)
    return ChainEvidence(req, raw, multi, nw, nkept)


class ChainEvidence(_analysis.Result):
    """The evidence of a chain from the device (a leading source axis for a multi-source result).

    lnz, lnz_err : ln of the integral of the unnormalised posterior over the free parameters, and its standard error
        (NaN with COV_SINGULAR or NO_OVERLAP);
    ln_evidence : ``lnz - ln_prior_norm``, the log marginal likelihood under normalised priors; NaN where a free
        parameter is improper (neither an upper limit nor a Gaussian prior);
    niter, status, n1 (posterior samples used), n2 (proposal draws), n_inside (draws of finite lnprob), neff;
    proposal_mean [..., 5], proposal_cov [..., 5, 5] (NaN in held rows and columns);  held [..., 5];
    proposal, proposal_lnprob, proposal_lnq, posterior_lnq : with ``keep=True``, else None;
    status : bits CONVERGED, MAXITER, COV_SINGULAR, POST_LEFT_OUT, NO_OVERLAP, ALL_HELD and, from HELD_SHIFT on, one per
        held parameter."""

    CONVERGED, MAXITER, COV_SINGULAR = _native.EV_CONVERGED, _native.EV_MAXITER, _native.EV_COV_SINGULAR
    POST_LEFT_OUT, NO_OVERLAP, ALL_HELD = _native.EV_POST_LEFT_OUT, _native.EV_NO_OVERLAP, _native.EV_ALL_HELD
    HELD_SHIFT = _native.EV_HELD_SHIFT

    def __init__(self, request, raw, multi, nwalkers=0, nkept=0):
        self._req, self._raw, self._multi = request, raw, bool(multi)
        self._set_window(request, nwalkers, nkept)

    lnz = property(lambda self: self._squeeze(self._raw.lnz).copy())
    lnz_err = property(lambda self: self._squeeze(self._raw.lnz_err).copy())
    niter = property(lambda self: self._squeeze(self._raw.niter).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())
    n1 = property(lambda self: self._squeeze(self._raw.n1).copy())
    n2 = property(lambda self: self._raw.n2)
    n_inside = property(lambda self: self._squeeze(self._raw.n_inside).copy())
    proposal_mean = property(lambda self: self._squeeze(self._raw.prop_mean).copy())
    proposal_cov = property(lambda self: self._squeeze(self._raw.prop_cov).copy())
    ln_prior_norm = property(lambda self: self._req.ln_norm)
    improper = property(lambda self: self._req.improper.copy())
    has_peak_term = property(lambda self: self._req.peak_term)
    converged = property(lambda self: self._squeeze((self._raw.status & _native.EV_CONVERGED) != 0))

    def _kept(self, a):
        return None if a is None else self._squeeze(a).copy()

    proposal = property(lambda self: self._kept(self._raw.prop))
    proposal_lnprob = property(lambda self: self._kept(self._raw.prop_lnprob))
    proposal_lnq = property(lambda self: self._kept(self._raw.prop_lnq))
    posterior_lnq = property(lambda self: self._kept(self._raw.post_lnq))

    @property
    def neff(self):
        """The effective sample count the call was given, per source (n1 where it was given none)."""
        v = self._raw.n1.astype(np.float64) if self._req.neff is None else np.minimum(
            np.maximum(self._req.neff, 1.0), np.maximum(self._raw.n1, 1))
        return self._squeeze(v)

    @property
    def held(self):
        bits = (self._raw.status[:, None] >> (_native.EV_HELD_SHIFT + np.arange(5))[None, :]) & 1
        return self._squeeze(bits.astype(bool))

    def _improper_rows(self):
        """[nsrc, 5]: free in this source and improper"""
        bits = ((self._raw.status[:, None] >> (_native.EV_HELD_SHIFT + np.arange(5))[None, :]) & 1).astype(bool)
        return self._req.improper[None, :] & ~bits

    @property
    def ln_evidence(self):
        bad = self._improper_rows().any(axis=1)
        return self._squeeze(np.where(bad, np.nan, self._raw.lnz - self._req.ln_norm))

    def bayes_factor(self, other):
        """(ln B, its error) per source of this fit against ``other``: the difference of the two ``ln_evidence`` and
        the errors in quadrature.  A parameter that is improper in one fit must be improper in the other too, free in
        both with the same limits: its unknown normalisation then cancels.  Anything else is refused."""
        if not isinstance(other, ChainEvidence):
            raise TypeError("bayes_factor compares two ChainEvidence")
        if self._raw.lnz.shape != other._raw.lnz.shape:
            raise ValueError("the two results have different numbers of sources")
        a, b = self._improper_rows(), other._improper_rows()
        if np.any(a != b):
            which = [PARAM_NAMES[i] for i in range(5) if np.any(a[:, i] != b[:, i])]
            raise ValueError("{} is free without an upper limit or a prior in one fit and not in the other: the "
                             "evidences have no common normalisation".format(", ".join(which)))
        d = (self._raw.lnz - self._req.ln_norm) - (other._raw.lnz - other._req.ln_norm)
        e = np.sqrt(self._raw.lnz_err ** 2 + other._raw.lnz_err ** 2)
        return self._squeeze(d), self._squeeze(e)

    def status_names(self, source=0):
        st = int(np.atleast_1d(self._raw.status)[source])
        names = [n for bit, n in ((1, "CONVERGED"), (2, "MAXITER"), (4, "COV_SINGULAR"), (8, "POST_LEFT_OUT"),
                                  (16, "NO_OVERLAP"), (32, "ALL_HELD")) if st & bit]
        return names + ["HELD_" + PARAM_NAMES[i] for i in range(5) if (st >> (_native.EV_HELD_SHIFT + i)) & 1]

    def arrays(self, prefix="evidence_"):
        """The results as plain arrays (for an .npz)."""
        return {prefix + "lnz": self.lnz, prefix + "lnz_err": self.lnz_err, prefix + "ln_evidence": np.array(self.ln_evidence),
                prefix + "ln_prior_norm": np.array(self._req.ln_norm), prefix + "improper": self.improper,
                prefix + "niter": self.niter, prefix + "status": self.status, prefix + "n1": self.n1,
                prefix + "n2": np.array(self.n2), prefix + "n_inside": self.n_inside, prefix + "neff": np.array(self.neff),
                prefix + "proposal_mean": self.proposal_mean, prefix + "proposal_cov": self.proposal_cov}

    def __str__(self):
        """The first source of a multi-source result."""
        r = self._raw
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(r.lnz.shape[0]))
        lines.append("ln Z: {:0.4f} +- {:0.4f} ({:d} iterations; {})".format(
            r.lnz[0], r.lnz_err[0], int(r.niter[0]), " ".join(self.status_names(0)) or "-"))
        lines.append("Posterior samples: {:d} (effective {:0.1f})  proposal draws: {:d}, {:d} inside the limits".format(
            int(r.n1[0]), float(np.atleast_1d(self.neff)[0]), r.n2, int(r.n_inside[0])))
        le = float(np.atleast_1d(self.ln_evidence)[0])
        if np.isfinite(le):
            lines.append("ln evidence under normalised priors: {:0.4f}".format(le))
        else:
            bad = [PARAM_NAMES[i] for i in range(5) if self._improper_rows()[0, i]]
            lines.append("ln evidence under normalised priors: undefined ({} has neither an upper limit nor a "
                         "prior)".format(", ".join(bad)) if bad else "ln evidence under normalised priors: nan")
        if self._req.peak_term:
            lines.append("(the peak-wavelength limit / prior is not normalised: it stays inside ln Z)")
        return "\n".join(lines)
