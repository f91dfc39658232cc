"""Fit driver: owns the likelihood and the ensemble sampler.

Host-side mirror of the reference's ``mbb_fitter``
(reference mbb_emcee/mbb_fit.py:13-563): same constructor keywords, the same
forwarding setters, the same limit-respecting initial positions and the same
burn-in + main-chain ``run``.  The sampler evaluates each half-step of the
ensemble in one kernel launch through ``likelihood.__call__`` on an (n, 5) array.
"""
from __future__ import print_function

import numpy as np

from .ensemble import EnsembleSampler
from .likelihood import likelihood

__all__ = ["mbb_fitter"]


class mbb_fitter(object):
    """Modified-blackbody MCMC fit."""

    # mbb_fit.py:17-24
    _param_order = {'t': 0, 't/(1+z)': 0, 'beta': 1, 'lambda0': 2,
                    'lambda0*(1+z)': 2, 'lambda_0': 2, 'lambda_0*(1+z)': 2,
                    'alpha': 3, 'fnorm': 4, 'f500': 4, 'lambda_peak': 5, 'peaklam': 5}
    _parnames = np.array(['T/(1+z)', 'Beta', 'Lambda0*(1+z)', 'Alpha', 'Fnorm'])

    def __init__(self, nwalkers=250, photfile=None, covfile=None, covextn=0,
                 response=False, responsefile=None, responsedir=None, wavenorm=500.0,
                 noalpha=False, opthin=False, nthreads=1, device=None, seed=None,
                 sampler="device"):
        """Keywords as mbb_fit.py:26-72.  nthreads is accepted and ignored: the
        walkers of a half-step are evaluated together on the GPU.
        sampler="device" (the default): the whole stretch-move step runs on the GPU
        (DeviceEnsembleSampler; a fit of 50 + 250 steps of 250 walkers takes milliseconds,
        bench.py `fit_wall_s`); sampler="native": host stretch move, one launch per half-step
        through likelihood.__call__ -- the path an external sampler takes;
        sampler="emcee" uses emcee.EnsembleSampler when that package is installed
        (vectorised when it supports it, else through like.map)."""
        self._noalpha = noalpha
        self._opthin = opthin
        self._wavenorm = float(wavenorm)
        self._nwalkers = int(nwalkers)
        self._nthreads = int(nthreads)
        self.like = likelihood(photfile=photfile, covfile=covfile, covextn=covextn,
                               wavenorm=wavenorm, noalpha=noalpha, opthin=opthin,
                               response=response, responsefile=responsefile,
                               responsedir=responsedir, device=device)
        if sampler == "device":
            from .device_sampler import DeviceEnsembleSampler
            self.sampler = DeviceEnsembleSampler(self._nwalkers, 5, self.like, seed=seed)
        elif sampler == "emcee":
            import emcee
            try:
                self.sampler = emcee.EnsembleSampler(self._nwalkers, 5, self.like,
                                                     vectorize=True)
            except TypeError:
                self.sampler = emcee.EnsembleSampler(self._nwalkers, 5, self.like,
                                                     pool=self.like)
        else:
            self.sampler = EnsembleSampler(self._nwalkers, 5, self.like,
                                           threads=self._nthreads, vectorize=True, seed=seed)
        self._random = np.random.RandomState(seed) if seed is not None else np.random
        self._sampled = False
        self._fixed = [False, False, False, False, False]

    # ---- read-only views (mbb_fit.py:87-125) are attached below the class -----

    # ---- data (mbb_fit.py:127-185) --------------------------------------------
    def read_data(self, photfile, covfile=None, covextn=0, responsefile=None,
                  responsedir=None):
        if responsefile is not None:
            self.like.read_responses(responsefile, responsedir=responsedir)
        self.like.read_phot(photfile)
        if covfile is not None:
            self.like.read_cov(covfile, extn=covextn)

    def set_data(self, wave, flux, flux_unc, covmatrix=None):
        self.like.set_phot(wave, flux, flux_unc)
        if covmatrix is not None:
            self.like.set_cov(covmatrix)

    # ---- fixed parameters (mbb_fit.py:187-219); the limit / prior calls of
    # mbb_fit.py:221-360 are forwarded to the likelihood, see _FORWARDED below ----
    def _pidx(self, param):
        return self._param_order[param.lower()] if isinstance(param, str) else int(param)

    def fix_param(self, param):
        """Hold a parameter (index or name) at its initial value."""
        self._fixed[self._pidx(param)] = True

    def unfix_param(self, param):
        self._fixed[self._pidx(param)] = False

    # ---- initial positions (behaviour of mbb_fit.py:362-479) ---------------------
    def generate_initial_values(self, initvals, initsigma):
        """Starting positions [nwalkers, 5]: a Gaussian ball of widths ``initsigma`` around
        ``initvals`` in which every walker respects the parameter limits (the peak-wavelength
        limit is not looked at).  A requested centre that lies outside a parameter's limits is moved
        inside by two sigma, or to the middle of the allowed range when that range is narrower than
        four sigma; a fixed parameter gets no scatter and must itself lie inside its limits."""
        centre = np.array(initvals, dtype=np.float64)
        sigma = np.array(initsigma, dtype=np.float64)
        if centre.shape != (5,):
            raise ValueError("Initial values not expected length")
        if sigma.shape != (5,):
            raise ValueError("Initial sigma values not expected length")
        lo = np.array([self.lowlim(i) for i in range(5)], dtype=np.float64)
        hi = np.array([self.uplim(i) if self.has_uplim(i) else np.inf for i in range(5)], dtype=np.float64)
        fixed = np.asarray(self._fixed, dtype=bool)
        below, above = centre < lo, centre > hi
        stuck = fixed & (below | above)
        if stuck.any():
            raise ValueError("Some fixed parameters outside limits: {:s}".format(', '.join(self._parnames[stuck])))
        width = hi - lo
        crossed = (below | above) & (width <= 0)
        if crossed.any():
            raise ValueError("Limits on parameter {:d} cross".format(int(np.nonzero(crossed)[0][0])))
        # where the ball is centred: as asked for, or two sigma inside the limit that was violated,
        # or mid-range when the range cannot hold that
        narrow = np.isfinite(width) & (2.0 * sigma >= width)
        centre = np.where(below, np.where(narrow, lo + 0.5 * np.where(np.isfinite(width), width, 0.0), lo + 2.0 * sigma), centre)
        centre = np.where(above, np.where(narrow, lo + 0.5 * np.where(np.isfinite(width), width, 0.0), hi - 2.0 * sigma), centre)
        scatter = np.where(fixed, 0.0, sigma)
        p0 = centre + scatter * self._random.randn(self._nwalkers, 5)
        # one rejection loop over the whole array: redraw the entries that fell outside
        for attempt in range(101):
            out = (p0 < lo) | (p0 > hi)
            nout = int(out.sum())
            if nout == 0:
                return p0
            rows, cols = np.nonzero(out)
            p0[rows, cols] = centre[cols] + scatter[cols] * self._random.randn(nout)
        worst = int(np.argmax(out.sum(axis=0)))
        raise Exception("Too many iterations initializing param {:d}: {:d} of {:d} walkers still outside "
                        "[{:g}, {:g}] after 100 redraws".format(worst, int(out[:, worst].sum()), self._nwalkers,
                                                                lo[worst], hi[worst]))

    # ---- the optimum before the chain (optimize.py; no reference counterpart) -----
    def find_map(self, initvals=None, initsigma=None, nstart=8, start=None, **kw):
        """The maximum of the posterior per source, found on the device (``optimize.map_fit``); returns a ``MapFit``.
        The starts are ``nstart`` points of the ``generate_initial_values(initvals, initsigma)`` ball (the same for every
        source of a catalogue), the fixed parameters are the fitter's.  start="best_fit" polishes ``summary.best_fit`` of
        a run made with summary= instead; start=array gives the starts as ``map_fit`` takes them.  Further keywords
        (maxiter, ftol, xtol) go to ``map_fit``."""
        from . import optimize
        if isinstance(start, str):
            if start != "best_fit":
                raise ValueError("start must be \"best_fit\" or an array of starts")
            if self.summary is None:
                raise ValueError("start=\"best_fit\" needs a run made with summary=")
            pts = np.asarray(self.summary.best_fit[0], dtype=np.float64)
            return optimize.map_fit(self.like, pts, nstart=1, fixed=self._fixed, **kw)
        if start is not None:
            return optimize.map_fit(self.like, start, fixed=self._fixed, **kw)
        if initvals is None or initsigma is None:
            raise ValueError("find_map needs initvals and initsigma, or start=")
        nstart = int(nstart)
        if not 1 <= nstart <= optimize.MAX_STARTS:
            raise ValueError("nstart must be 1 to {:d}".format(optimize.MAX_STARTS))
        ball = self.generate_initial_values(initvals, initsigma)
        if ball.shape[0] < nstart:
            raise ValueError("nstart is larger than the number of walkers")
        pts = np.broadcast_to(ball[:nstart], (self.like.nsources, nstart, 5))
        return optimize.map_fit(self.like, pts, nstart=nstart, fixed=self._fixed, squeeze=self.like.nsources == 1, **kw)

    def map_initial_values(self, mapfit, initsigma, scale=1.0):
        """Starting positions [nsources, nwalkers, 5] ([nwalkers, 5] for one source) from a ``MapFit``: per source a
        Gaussian ball around that source's optimum.  Per parameter the width is min(scale x Laplace sigma, initsigma),
        and initsigma where the Laplace sigma is NaN (a parameter on its lower limit, a singular curvature).  Every
        walker respects the limits by ``generate_initial_values``'s rejection rule; a fixed parameter gets no scatter.
        A source whose fit failed (START_INVALID) gets the plain ball around its start, and a warning says so."""
        import warnings
        sigma0 = np.array(initsigma, dtype=np.float64)
        if sigma0.shape != (5,):
            raise ValueError("Initial sigma values not expected length")
        params = np.atleast_2d(mapfit.params)
        lap = np.atleast_2d(mapfit.sigma)
        failed = np.atleast_1d(mapfit.failed)
        out = np.empty((params.shape[0], self._nwalkers, 5))
        for s in range(params.shape[0]):
            with np.errstate(invalid="ignore"):
                width = np.where(np.isfinite(lap[s]) & (lap[s] > 0), np.minimum(float(scale) * lap[s], sigma0), sigma0)
            if failed[s]:
                warnings.warn("the MAP fit of source {:d} failed (START_INVALID): its walkers start from the plain ball "
                              "around its start".format(s))
                width = sigma0
            out[s] = self.generate_initial_values(params[s], width)
        return out if np.ndim(mapfit.params) > 1 else out[0]

    # ---- run (mbb_fit.py:481-563) ------------------------------------------------
    def run(self, nburn, nsteps, p0, verbose=False, summary=None, convergence=None, marginals=None, predict=None,
            draws=None, goodness=None, evidence=None, loo=None, reweight=None, population=None):
        """Burn in for nburn steps, reset, then sample nsteps steps per walker.
        summary (device sampler only): True or a dict of ``results.chain_summary``'s keywords -- the main chain is
        summarised on the device as well, ``mbb_fitter.summary`` (DeviceEnsembleSampler.run_mcmc); for a catalogue
        (``set_phot_multi``) its ``redshift`` and ``lumdist_mpc`` may be arrays with one entry per source.
        convergence (device sampler only): True or a dict of ``diagnostics.chain_diagnostics``'s keywords -- the main
        chain's autocorrelation times, effective sample sizes and split R-hat, ``mbb_fitter.convergence``.
        marginals (device sampler only): True or a dict of ``marginals.chain_marginals``'s keywords -- the main chain's
        1-d and 2-d histograms, ``mbb_fitter.marginals``.
        predict (device sampler only): wavelengths in um and / or passband names, or a dict of
        ``predict.chain_predictions``'s keywords (``specs`` among them) -- the fluxes the main chain predicts there,
        ``mbb_fitter.predictions``.
        draws (device sampler only): a number of draws per source, or a dict of ``draws.chain_draws``'s keywords (``n``
        among them) -- cells drawn from the main chain with their derived values, ``mbb_fitter.draws``.
        goodness (device sampler only): True or a dict of ``goodness.chain_goodness``'s keywords -- the main chain's
        chisq against the data, posterior predictive p-value, DIC and maximum-likelihood entry,
        ``mbb_fitter.goodness``.
        loo (device sampler only): True or a dict of ``loo.chain_loo``'s keywords -- the main chain's WAIC and PSIS-LOO
        per band, ``mbb_fitter.loo``.
        evidence (device sampler only): True or a dict of ``evidence.chain_evidence``'s keywords -- the main chain's
        bridge-sampled ln Z per source, ``mbb_fitter.evidence``; the fitter's own fixed parameters are passed on as
        ``fixed`` unless the dict names others.
        reweight (device sampler only): a target ``likelihood`` (or a ``mbb_fitter``, whose likelihood is meant), or a
        dict of ``reweight.chain_reweight``'s keywords (``target`` among them) -- the main chain reweighted under the
        target's density, ``mbb_fitter.reweight``.
        population (device sampler only): True or a dict of ``population.chain_population``'s keywords -- the main chain
        pooled into a population block, ``mbb_fitter.population_``; the fitter's own fixed parameters are passed on as
        ``fixed`` unless the dict names others."""
        if population is not None and population is not False and not hasattr(self.sampler, "population"):
            raise ValueError("population= needs sampler=\"device\"")
        if reweight is not None and reweight is not False and not hasattr(self.sampler, "reweight"):
            raise ValueError("reweight= needs sampler=\"device\"")
        if evidence is not None and evidence is not False and not hasattr(self.sampler, "evidence"):
            raise ValueError("evidence= needs sampler=\"device\"")
        if loo is not None and loo is not False and not hasattr(self.sampler, "loo"):
            raise ValueError("loo= needs sampler=\"device\"")
        if goodness is not None and goodness is not False and not hasattr(self.sampler, "goodness"):
            raise ValueError("goodness= needs sampler=\"device\"")
        if draws is not None and draws is not False and not hasattr(self.sampler, "draws"):
            raise ValueError("draws= needs sampler=\"device\"")
        if predict is not None and predict is not False and not hasattr(self.sampler, "predictions"):
            raise ValueError("predict= needs sampler=\"device\"")
        if marginals is not None and marginals is not False and not hasattr(self.sampler, "marginals"):
            raise ValueError("marginals= needs sampler=\"device\"")
        if convergence is not None and convergence is not False and not hasattr(self.sampler, "convergence"):
            raise ValueError("convergence= needs sampler=\"device\"")
        if summary is not None and summary is not False and not hasattr(self.sampler, "_summarise_again"):
            raise ValueError("summary= needs sampler=\"device\"")
        if not self.like.data_read:
            raise Exception("Data not read, needed to do fit")
        if verbose:
            print("Starting fit")
            if self.response_integrate:
                print("  Using response integration")
        p0 = np.asarray(p0, dtype=np.float64)
        for i in range(5):
            if (i == 2 and self._opthin) or (i == 3 and self._noalpha):
                continue
            if self.has_uplim(i) and p0[..., i].max() > self.uplim(i):
                raise ValueError("Upper limit initial value violation for "
                                 "{:s}".format(self._parnames[i]))
            if p0[..., i].min() < self.lowlim(i):
                raise ValueError("Lower limit initial value violation for "
                                 "{:s}".format(self._parnames[i]))

        self.sampler.reset()
        self._sampled = False
        if nburn <= 0:
            raise ValueError("Invalid (non-positive) number of burn in steps: {:d}".format(nburn))
        if verbose:
            print("  Doing burn in with {:d} steps".format(nburn))
        pos, prob, rstate = self.sampler.run_mcmc(p0, nburn)[:3]

        self.sampler.reset()
        if nsteps <= 0:
            raise ValueError("Invalid (non-positive) number of main chain steps: "
                             "{:d}".format(nsteps))
        if verbose:
            print("  Doing main chain with {:d} steps".format(nsteps))
        extra = {}
        if summary is not None and summary is not False:
            extra["summary"] = summary
        if convergence is not None and convergence is not False:
            extra["convergence"] = convergence
        if marginals is not None and marginals is not False:
            extra["marginals"] = marginals
        if predict is not None and predict is not False:
            extra["predict"] = predict
        if draws is not None and draws is not False:
            extra["draws"] = draws
        if goodness is not None and goodness is not False:
            extra["goodness"] = goodness
        if loo is not None and loo is not False:
            extra["loo"] = loo
        if reweight is not None and reweight is not False:
            rkw = dict(reweight) if isinstance(reweight, dict) else dict(target=reweight)
            if isinstance(rkw.get("target"), mbb_fitter):
                rkw["target"] = rkw["target"].like
            extra["reweight"] = rkw
        if population is not None and population is not False:
            pkw = {} if population is True else dict(population)
            pkw.setdefault("fixed", [bool(f) for f in self._fixed])
            extra["population"] = pkw
        if evidence is not None and evidence is not False:
            ekw = {} if evidence is True else dict(evidence)
            ekw.setdefault("fixed", [bool(f) for f in self._fixed])
            extra["evidence"] = ekw
        self.sampler.run_mcmc(pos, nsteps, rstate0=rstate, **extra)
        self._sampled = True

        if verbose:
            print("  Fit complete")
            print("   Mean acceptance fraction:", np.mean(self.sampler.acceptance_fraction))
            try:
                acor = self.sampler.acor
                print("   Autocorrelation time: ")
                print("    Number of burn in steps ({:d}) should be larger "
                      "than these".format(nburn))
                print("\tT:        {:f}".format(acor[0]))
                print("\tbeta:     {:f}".format(acor[1]))
                if not self._opthin:
                    print("\tlambda0:  {:f}".format(acor[2]))
                if not self._noalpha:
                    print("\talpha:    {:f}".format(acor[3]))
                print("\tfnorm:    {:f}".format(acor[4]))
            except Exception:
                pass


def _view(attr, doc):
    return property(lambda self: getattr(self, attr), doc=doc)


for _name, _attr, _doc in (("noalpha", "_noalpha", "Not using the blue side power law?"),
                           ("opthin", "_opthin", "Assuming an optically thin model?"),
                           ("wavenorm", "_wavenorm", "Normalisation wavelength [um]"),
                           ("nwalkers", "_nwalkers", "Number of walkers"),
                           ("nthreads", "_nthreads", "Accepted for compatibility, unused"),
                           ("sampled", "_sampled", "Has the distribution been sampled?"),
                           ("fixed", "_fixed", "Which parameters are held fixed")):
    setattr(mbb_fitter, _name, _view(_attr, _doc))
mbb_fitter.summary = property(lambda self: getattr(self.sampler, "summary", None),
                              doc="results.ChainSummary of the main chain when run() was given summary=, else None")
mbb_fitter.convergence = property(lambda self: getattr(self.sampler, "convergence_", None),
                                  doc="diagnostics.ChainDiagnostics of the main chain when run() was given convergence=, "
                                      "else None")
mbb_fitter.marginals = property(lambda self: getattr(self.sampler, "marginals_", None),
                                doc="marginals.ChainMarginals of the main chain when run() was given marginals=, else None")
mbb_fitter.predictions = property(lambda self: getattr(self.sampler, "predictions_", None),
                                  doc="predict.ChainPredictions of the main chain when run() was given predict=, else None")
mbb_fitter.goodness = property(lambda self: getattr(self.sampler, "goodness_", None),
                               doc="goodness.ChainGoodness of the main chain when run() was given goodness=, else None")
mbb_fitter.loo = property(lambda self: getattr(self.sampler, "loo_", None),
                          doc="loo.ChainLoo of the main chain when run() was given loo=, else None")
mbb_fitter.evidence = property(lambda self: getattr(self.sampler, "evidence_", None),
                               doc="evidence.ChainEvidence of the main chain when run() was given evidence=, else None")
mbb_fitter.reweight = property(lambda self: getattr(self.sampler, "reweight_", None),
                               doc="reweight.ChainReweight of the main chain when run() was given reweight=, else None")
mbb_fitter.population_ = property(lambda self: getattr(self.sampler, "population_", None),
                                  doc="population.Population of the main chain when run() was given population=, else None")


def _fitter_population(self, **kw):
    """``population.Population`` of the main chain the last run left on the device (device sampler only); the keywords
    are ``population.chain_population``'s, ``fixed`` defaulting to the fitter's own fixed parameters."""
    if not hasattr(self.sampler, "population"):
        raise ValueError("population() needs sampler=\"device\"")
    kw.setdefault("fixed", [bool(f) for f in self._fixed])
    return self.sampler.population(**kw)


mbb_fitter.population = _fitter_population
mbb_fitter.draws = property(lambda self: getattr(self.sampler, "draws_", None),
                            doc="draws.ChainDraws from the main chain when run() was given draws=, else None")
mbb_fitter.response_integrate = property(lambda self: self.like.response_integrate,
                                         doc="Is passband integration in use?")


def _forward(name):
    def call(self, *args):
        return getattr(self.like, name)(*args)
    call.__name__ = name
    call.__doc__ = "Forwards to likelihood.%s (param: index or name, incl. 'lambda_peak')." % name
    return call


# mbb_fit.py:221-360: the fitter exposes the likelihood's limit and prior calls
_FORWARDED = ("set_lowlim", "lowlim", "set_uplim", "has_uplim", "uplim",
              "set_gaussian_prior", "has_gaussian_prior", "get_gaussian_prior")
for _name in _FORWARDED:
    setattr(mbb_fitter, _name, _forward(_name))
