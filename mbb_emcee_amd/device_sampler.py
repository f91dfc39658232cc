"""Device-resident affine-invariant ensemble sampler.

Plays the role of ``emcee.EnsembleSampler`` in the reference's fit driver
(reference mbb_emcee/mbb_fit.py:80-81, :525-550; results.py:154-155) with the
whole stretch-move step on the MI355X: for each half of the ensemble ONE kernel
draws z and a partner for every walker (counter-based Philox RNG), forms the
proposal, evaluates the fused likelihood and accepts or rejects in place.  A run
of N steps is 2N dependent launches enqueued back to back; the host only sees
the chain at the end.  emcee itself is not part of the reference tree, so parity
with it is statistical.
"""
import collections
import ctypes as C

import numpy as np

from . import _analysis, _native
from .ensemble import integrated_time

__all__ = ["DeviceEnsembleSampler", "accepted_by_step"]


def accepted_by_step(cur, steps, own_rows=None):
    """Every walker's accepted moves after each of a run's steps, rebuilt from its positions: ``cur`` [..., nw, 5] is
    the ensemble before the run, ``steps`` [..., nw, k, 5] the run's chain; the result [..., nw, k] is cumulative.  A
    stretch move that is accepted changes the walker's position, one that is refused leaves every bit of it.
    ``own_rows`` (a boolean mask over the walkers, or their indices): the walkers whose chain this rank holds -- with
    the one-hop exchange the other rows of a rank's chain are zeros, which say nothing about a move, and stay 0."""
    cur, steps = np.asarray(cur, dtype=np.float64), np.asarray(steps, dtype=np.float64)
    if steps.shape[-2] == 0:
        return np.zeros(steps.shape[:-1], dtype=np.int64)
    prev = np.concatenate((cur[..., None, :], steps[..., :-1, :]), axis=-2)
    moved = np.any(steps != prev, axis=-1)
    if own_rows is not None:
        own = np.zeros(steps.shape[-3], dtype=bool)
        own[np.asarray(own_rows)] = True
        moved = moved & own[:, None]
    return np.cumsum(moved, axis=-1)


def _own_rows(nw, rank, nranks):
    """The walkers rank ``rank`` of ``nranks`` moves in a sharded run, as a mask: its block of either half."""
    from .parallel import block_bounds
    half = nw // 2
    lo, hi = block_bounds(half, nranks)[1][rank]
    own = np.zeros(nw, dtype=bool)
    own[lo:hi] = own[half + lo:half + hi] = True
    return own


class _OpenSample(object):
    """What a suspended sample() generator has to leave behind when it ends or is retired."""
    __slots__ = ("live", "it_prev", "n_prev", "made", "acc_made", "storechain", "big_c", "big_l", "kept_c", "kept_l",
                 "single")


def _request_predict(s, kw):
    from . import predict
    return predict._Request(s.lnprobfn, kw["specs"], _analysis.quantiles(kw.get("percentile", 68.3), kw.get("percentiles", ()))[1],
                            kw.get("burn", 0), kw.get("thin", 1), kw.get("clip"), kw.get("wavenorm"))


def _request_loo(s, kw):
    from . import loo
    return loo._Request(s.lnprobfn, kw.get("burn", 0), kw.get("thin", 1))


def _request_goodness(s, kw):
    from . import goodness
    return goodness._Request(s.lnprobfn, _analysis.quantiles(kw.get("percentile", 68.3), kw.get("percentiles", ()))[1],
                             kw.get("burn", 0), kw.get("thin", 1))


def _request_evidence(s, kw):
    from . import evidence
    return evidence._Request(s.lnprobfn, kw.get("n2"), kw.get("fixed"), kw.get("seed", s.seed), kw.get("burn", 0),
                             kw.get("thin", 1), kw.get("tol", evidence.TOL), kw.get("maxiter", evidence.MAXITER))


def _request_marginals(s, kw):
    from . import marginals
    return marginals._Request(nsources=s.nsources, **kw)


def _request_draws(s, kw):
    from . import draws
    kw.setdefault("seed", s.seed)
    return draws._Request(nsources=s.nsources, **kw)


def _request_reweight(s, kw):
    from . import reweight
    return reweight._Request(nsources=s.nsources, **kw)


def _request_population(s, kw):
    from . import population
    return population._Request(s.lnprobfn, **kw)


def _request_convergence(s, kw):
    from . import diagnostics
    return diagnostics._Request(**kw)


def _check_steps(s, req, kw, nsteps):
    req.check_steps(nsteps)


def _check_loo(s, req, kw, nsteps):
    req.check_steps(nsteps, s.k)


def _check_evidence(s, req, kw, nsteps):
    req.check_steps(nsteps)
    if not isinstance(kw.get("neff", "auto"), str):
        req.set_neff(kw["neff"], s.nsources)
    elif kw.get("neff", "auto") != "auto":
        raise ValueError("neff must be 'auto', None, a number or one number per source")


# One analysis of the chain a run leaves on the device, as run_mcmc's keyword of that name is read:
#   first    -- the argument a value that is no dict stands for (None: True stands for no keywords);
#   needs    -- the refusal when ``first`` is missing, where it has to be there;
#   inherits -- the keys of summary= that are the defaults of its own;
#   allowed  -- its keywords, where run_mcmc names the unknown ones itself (None: the request's constructor does);
#   request  -- (sampler, keywords) -> the module's _Request, which checks all it can before a device is touched;
#   check    -- (sampler, request, keywords, nsteps): what the number of steps of the run decides;
#   verb     -- what a sharded run cannot be;
#   attr, method -- the attribute the result goes to, and the method that makes it from the resident chain.
_Analysis = collections.namedtuple("_Analysis", "first needs inherits allowed request check verb attr method")
_WINDOW = ("burn", "thin")
_DERIVED = _WINDOW + ("derived", "redshift", "lumdist_mpc", "kappa", "kappa_wave", "lir_range", "peak_model")
_ANALYSES = {
    "predict": _Analysis("specs", "predict= needs specs: wavelengths in um and / or passband names", _WINDOW,
                         {"specs", "percentile", "percentiles", "burn", "thin", "clip", "wavenorm", "keep"},
                         _request_predict, _check_steps, "predicted from", "predictions_", "predictions"),
    "loo": _Analysis(None, None, _WINDOW, {"burn", "thin"}, _request_loo, _check_loo, "cross-validated", "loo_", "loo"),
    "goodness": _Analysis(None, None, _WINDOW, {"percentile", "percentiles", "burn", "thin"}, _request_goodness,
                          _check_steps, "tested for goodness of fit", "goodness_", "goodness"),
    "evidence": _Analysis(None, None, _WINDOW, {"n2", "fixed", "neff", "seed", "burn", "thin", "tol", "maxiter", "keep"},
                          _request_evidence, _check_evidence, "bridged to an evidence", "evidence_", "evidence"),
    "marginals": _Analysis(None, None, _DERIVED, None, _request_marginals, _check_steps, "binned", "marginals_",
                           "marginals"),
    "draws": _Analysis("n", None, _DERIVED, None, _request_draws, _check_steps, "drawn from", "draws_", "draws"),
    "reweight": _Analysis("target", "reweight= needs a target: the likelihood the chain is reweighted to", _DERIVED, None,
                          _request_reweight, _check_loo, "reweighted", "reweight_", "reweight"),
    "convergence": _Analysis(None, None, (), None, _request_convergence, _check_steps, "diagnosed", "convergence_",
                             "convergence"),
    "population": _Analysis(None, None, _WINDOW, {"columns", "transform", "burn", "thin", "fixed"}, _request_population,
                            _check_steps, "pooled into a population", "population_", "population"),
}
# three orders, each as run_mcmc has always had it: requests are made and checked, a sharded run is refused, and the
# results are made after the run
_REQUEST_ORDER = ("predict", "loo", "goodness", "evidence", "marginals", "draws", "convergence", "population", "reweight")
_SHARDED_ORDER = ("convergence", "marginals", "predict", "loo", "goodness", "evidence", "draws", "population", "reweight")
_RESULT_ORDER = ("convergence", "marginals", "predict", "draws", "goodness", "evidence", "loo", "population", "reweight")


class DeviceEnsembleSampler(object):
    """emcee-2.x-shaped API: run_mcmc, chain [nw, nsteps, 5], lnprobability
    [nw, nsteps], flatchain, acceptance_fraction, acor, reset.

    lnpostfn must be this package's ``likelihood`` (it owns the device context
    and the constant block the kernel reads)."""

    def __init__(self, nwalkers, dim, lnpostfn, a=2.0, threads=1, seed=None, **unused):
        if dim != 5:
            raise ValueError("the modified blackbody model has 5 parameters")
        if nwalkers % 2 != 0:
            raise ValueError("The number of walkers must be even.")
        if nwalkers < 2 * dim:
            raise ValueError("The number of walkers needs to be more than twice the "
                             "dimension of your parameter space.")
        if not hasattr(lnpostfn, "_sync_device"):
            raise TypeError("DeviceEnsembleSampler needs a mbb_emcee_amd.likelihood")
        self.k, self.dim, self.a = int(nwalkers), 5, float(a)
        self.lnprobfn = lnpostfn
        self.seed = int(np.random.SeedSequence(seed).generate_state(1, dtype=np.uint64)[0]) \
            if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
        self._h = None
        self._ctx = None
        self._ns = 1
        self._open = None                     # the state of the sample() generator that is suspended, if one is
        self.reset()

    @property
    def nsources(self):
        return getattr(self.lnprobfn, "nsources", 1)

    def _handle(self):
        ctx = self.lnprobfn._sync_device()
        if self._h is not None and self._ctx is ctx and self._ns != self.nsources:
            ctx.lib.mbb_sampler_destroy(ctx.h, self._h)
            self._h = None
        if self._h is None or self._ctx is not ctx:
            self._ns = self.nsources
            h = C.c_void_p()
            _native._check(ctx.lib.mbb_sampler_create(ctx.h, self.k, self.seed, C.byref(h)))
            self._h, self._ctx = h, ctx
        return ctx, self._h

    def reset(self):
        """Forget the chain: an empty ``chain`` / ``lnprobability``, ``naccepted`` zeros of the ensemble's leading
        shape, ``iterations`` 0, no ``summary``, ``convergence_``, ``marginals_``, ``draws_``, ``goodness_``, ``loo_``, ``evidence_``, ``reweight_``, ``population_`` or ``predictions_``, nothing resident for ``convergence()`` or
        ``marginals()``, and no
        state -- ``run_mcmc(None, n)`` raises until a run has been given positions.  The sampler's life goes on: the
        random stream does not start again (a step's draws are keyed by its number in the sampler's life), so that
        ``pos, lnp, _ = s.run_mcmc(p0, nburn); s.reset(); s.run_mcmc(pos, n, lnprob0=lnp)`` -- emcee's burn-in idiom --
        makes bit for bit the steps ``s.run_mcmc(p0, nburn + n)`` makes.  A sample() generator that is still suspended
        is retired first (see run_mcmc)."""
        self._retire()
        ns = self.nsources
        lead = (ns, self.k) if ns > 1 else (self.k,)
        self.naccepted = np.zeros(lead)
        self.iterations = 0
        self._chain = np.empty(lead + (0, self.dim))
        self._lnprob = np.empty(lead + (0,))
        self._last = None
        if getattr(self, "summary", None) is not None:
            self.summary.drop_chain()
        self.summary = None
        self._drop_predictions()
        for an in _ANALYSES.values():
            setattr(self, an.attr, None)
        self._resident = 0                    # steps of the last run's chain that are resident on the device
        if self._h is not None:
            _native._check(self._ctx.lib.mbb_sampler_reset(self._ctx.h, self._h))

    @property
    def chain(self):
        return self._chain

    @property
    def flatchain(self):
        s = self._chain.shape
        if len(s) == 4:                       # [nsources, nw, nsteps, 5] -> [nsources, nw*nsteps, 5]
            return self._chain.reshape(s[0], s[1] * s[2], s[3])
        return self._chain.reshape(s[0] * s[1], s[2])

    @property
    def lnprobability(self):
        return self._lnprob

    @property
    def flatlnprobability(self):
        return self._lnprob.flatten()

    @property
    def acceptance_fraction(self):
        return self.naccepted / max(self.iterations, 1)

    @property
    def acor(self):
        return self.get_autocorr_time()

    def get_autocorr_time(self, c=5.0):
        ch = self._chain if self._chain.ndim == 3 else self._chain[0]
        mean_chain = ch.mean(axis=0)
        return np.array([integrated_time(mean_chain[:, i], c=c) for i in range(self.dim)])

    @property
    def random_state(self):
        return self.seed

    def _resident_steps(self, name):
        """The steps of the last run's chain that are resident on the device, for the method ``name``."""
        if not getattr(self, "_resident", 0):
            raise ValueError("no chain of this sampler is resident on the device: {}() needs a run with "
                             "storechain=True or summary= (and not a sharded one) since the last reset".format(name))
        return self._resident

    def _analyse(self, entry, req, raw):
        """``mbb_sampler_<entry>`` of the resident chain, asked for what ``req`` says, into the arrays of ``raw``."""
        ctx, h = self._handle()
        spec, out = req.spec(), raw.out()
        _native.check_arg(getattr(ctx.lib, "mbb_sampler_" + entry)(ctx.h, h, C.byref(spec), C.byref(out)), ctx)
        return raw

    def convergence(self, burn=0, c=5.0, tol=50.0, method="mean", nacf=0):
        """``diagnostics.ChainDiagnostics`` (autocorrelation time, ESS, split R-hat per parameter and source) of the
        chain the last run left on the device -- a run with storechain=True or with summary= -- over its steps from
        ``burn`` on; the keywords are ``diagnostics.chain_diagnostics``'s.  No chain crosses the bus."""
        from . import diagnostics
        req = diagnostics._Request(burn, c, tol, method, nacf)
        n = req.check_steps(self._resident_steps("convergence"))
        raw = self._analyse("diagnostics", req, diagnostics._Raw(self.nsources, req.nacf))
        return diagnostics.ChainDiagnostics(req, raw, self.nsources > 1, self.k, n)

    def marginals(self, **kw):
        """``marginals.ChainMarginals`` (1-d and 2-d histograms per source and column) of the chain the last run left on
        the device -- a run with storechain=True or with summary= --; the keywords are ``marginals.chain_marginals``'s.
        No chain crosses the bus."""
        from . import marginals
        req = marginals._Request(nsources=self.nsources, **kw)
        nkept = req.check_steps(self._resident_steps("marginals"))
        raw = self._analyse("marginals", req, marginals._Raw(self.nsources, req.bins, req.bins2d, len(req.pairs)))
        return marginals.ChainMarginals(req, raw, self.nsources > 1, self.k, nkept)

    def draws(self, n=1, **kw):
        """``draws.ChainDraws`` (``n`` cells per source with their parameters, lnprob, (walker, step) and the derived
        values asked for) from the chain the last run left on the device -- a run with storechain=True or with
        summary= --; the keywords are ``draws.chain_draws``'s, ``seed`` defaulting to the sampler's.  A few rows
        cross the bus, no chain."""
        from . import draws
        kw.setdefault("seed", self.seed)
        req = draws._Request(n, nsources=self.nsources, **kw)
        nkept = req.check_steps(self._resident_steps("draws"))
        raw = self._analyse("draws", req, draws._Raw(self.nsources, req.n, req.derived))
        return draws.ChainDraws(self.lnprobfn, req, raw, self.nsources > 1, self.k, nkept)

    def goodness(self, percentile=68.3, percentiles=(), burn=0, thin=1):
        """``goodness.ChainGoodness`` (chisq of every entry against the data whatever the limits and priors, its tail
        probability, the posterior predictive p-value, DIC, the maximum-likelihood entry and its pulls) of the chain
        the last run left on the device -- a run with storechain=True or with summary= --; the keywords are
        ``goodness.chain_goodness``'s.  No chain crosses the bus."""
        from . import goodness
        cens, qs = _analysis.quantiles(percentile, percentiles)
        req = goodness._Request(self.lnprobfn, qs, burn, thin)
        nkept = req.check_steps(self._resident_steps("goodness"))
        raw = self._analyse("goodness", req, goodness._Raw(self.nsources, req.ndata, len(req.qs)))
        return goodness.ChainGoodness(req, raw, self.nsources > 1, cens[0], self.k, nkept)

    def loo(self, burn=0, thin=1):
        """``loo.ChainLoo`` (WAIC and PSIS-LOO per source and band: elpd_loo, p_loo, the Pareto k-hat, LOO-PIT, lppd,
        p_waic, elpd_waic) of the chain the last run left on the device -- a run with storechain=True or with
        summary= --; the keywords are ``loo.chain_loo``'s.  No chain crosses the bus."""
        from . import loo
        req = loo._Request(self.lnprobfn, burn, thin)
        nkept = req.check_steps(self._resident_steps("loo"), self.k)
        raw = self._analyse("pointwise", req, loo._Raw(self.nsources, req.ndata))
        return loo.ChainLoo(req, raw, self.nsources > 1, self.k, nkept)

    def reweight(self, target, **kw):
        """``reweight.ChainReweight`` (Pareto-smoothed importance weights and the weighted statistics of the chain under
        the density of ``target``, another ``likelihood``: k-hat, ess, ln(Z_target / Z_run), weighted means, quantiles,
        covariance and best entry) of the chain the last run left on the device -- a run with storechain=True or with
        summary= --; the keywords are ``reweight.chain_reweight``'s.  ``target`` may be this sampler's own likelihood
        or another of this process on the same device.  No chain crosses the bus."""
        from . import reweight
        req = reweight._Request(target, nsources=self.nsources, **kw)
        nkept = req.check_steps(self._resident_steps("reweight"), self.k)
        ctx, h = self._handle()
        tctx = _native.analysis_context(target)
        raw = reweight._Raw(self.nsources, len(req.qs), self.k * nkept, req.keep)
        spec, out = req.spec(), raw.out()
        _native.check_arg(ctx.lib.mbb_sampler_reweight(ctx.h, h, tctx.h, C.byref(spec), C.byref(out)), ctx)
        return reweight.ChainReweight(req, raw, self.nsources > 1, self.k, nkept)

    def population(self, **kw):
        """``population.Population`` (the block of x = g(theta[columns]) and of the interim prior's weights that the
        hyper-likelihood of Gaussian population candidates is evaluated against) of the chain the last run left on the
        device -- a run with storechain=True or with summary= --; the keywords are ``population.chain_population``'s.
        No chain crosses the bus.  The context keeps one block: the next build replaces it."""
        from . import population
        return population.sampler_population(self, **kw)

    def evidence(self, n2=None, fixed=None, neff="auto", seed=None, burn=0, thin=1, tol=None, maxiter=None, keep=False):
        """``evidence.ChainEvidence`` (bridge-sampled ln Z per source with its error) of the chain the last run left on
        the device -- a run with storechain=True or with summary= --; the keywords are ``evidence.chain_evidence``'s,
        ``seed`` defaulting to the sampler's.  neff="auto" takes the smallest ess over the free parameters from
        ``convergence()`` of the bridged half of the window (of all its steps: with thin > 1 that is an upper bound,
        and the count is clamped to the number of samples).  No chain crosses the bus."""
        from . import evidence
        req = evidence._Request(self.lnprobfn, n2, fixed, self.seed if seed is None else seed, burn, thin,
                                evidence.TOL if tol is None else tol, evidence.MAXITER if maxiter is None else maxiter,
                                0, keep)
        nkept, nfit = req.check_steps(self._resident_steps("evidence"))
        n1 = self.k * (nkept - nfit)
        if isinstance(neff, str):
            if neff != "auto":
                raise ValueError("neff must be 'auto', None, a number or one number per source")
            dg = self.convergence(burn=req.burn + nfit * req.thin)
            req.set_neff(req.neff_from_ess(dg.ess, dg.status, n1), self.nsources)
        else:
            req.set_neff(neff, self.nsources)
        raw = self._analyse("evidence", req, evidence._Raw(self.nsources, n1, req.n2 or n1, req.keep))
        return evidence.ChainEvidence(req, raw, self.nsources > 1, self.k, nkept)

    def predictions(self, specs, percentile=68.3, percentiles=(), burn=0, thin=1, clip=None, wavenorm=None, keep=True):
        """``predict.ChainPredictions`` (predicted fluxes at wavelengths and through passbands, ``predflux_cen``) of the
        chain the last run left on the device -- a run with storechain=True or with summary= --; the arguments are
        ``predict.chain_predictions``'s.  No chain crosses the bus."""
        from . import predict
        cens, qs = _analysis.quantiles(percentile, percentiles)
        req = predict._Request(self.lnprobfn, specs, qs, burn, thin, clip, wavenorm)
        nkept = req.check_steps(self._resident_steps("predictions"))
        res = predict.ChainPredictions(req, self._predict_again(req), self.nsources > 1,
                                       self._predict_again if keep else None, cens[0], self.k, nkept)
        if keep:
            # every result that can go back to the resident chain is known to the sampler, which tells it when that
            # chain goes (_drop_predictions); a result nobody holds any more is forgotten by itself
            import weakref
            if getattr(self, "_handed_predictions", None) is None:
                self._handed_predictions = weakref.WeakSet()
            self._handed_predictions.add(res)
        return res

    def _drop_predictions(self):
        """The resident chain is about to go (the start of a run, reset()): ``predictions_`` is None again, and every
        result ``predictions()`` handed out -- that one included -- forgets how to compute more from the chain, so
        that what it was not made with is a RuntimeError afterwards and never a number from another chain."""
        for res in list(getattr(self, "_handed_predictions", None) or ()) + [getattr(self, "predictions_", None)]:
            if res is not None:
                res.drop_chain()
        self._handed_predictions = None
        self.predictions_ = None

    def _predict_again(self, req):
        """A prediction from the chain the last run left on the device (mbb_sampler_predict)."""
        from . import predict
        return self._analyse("predict", req, predict._Raw(self.nsources, len(req.keys), len(req.qs)))

    def run_mcmc(self, pos0, N, rstate0=None, lnprob0=None, storechain=True, summary=None, convergence=None,
                 marginals=None, predict=None, draws=None, goodness=None, evidence=None, loo=None, reweight=None,
                 population=None, **unused):
        """N stretch-move steps from pos0 [nw, 5] ([nsources, nw, 5]); returns (pos, lnprob, rstate).

        One trajectory: after the first call that was given positions, calls of run_mcmc and sample() with
        ``pos0`` / ``p0`` None walk one trajectory -- that of a single ``run_mcmc(p0, T)`` of a fresh sampler with the
        same seed, bit for bit -- however the steps are grouped into calls, whatever sample()'s chunk and whatever
        ``storechain``.

        ``lnprob0`` (with ``pos0``; ignored without): the log-probabilities of ``pos0``, taken as given and not
        computed again.  Exactly the ensemble's leading shape, (nw,) or (nsources, nw): anything else is a ValueError,
        and so is a NaN; -inf and +inf are legal (a walker at -inf leaves at its first finite proposal, one at +inf
        never moves).

        A sample() generator of this sampler that is still suspended is retired first: ``chain``, ``lnprobability``,
        ``iterations`` and ``naccepted`` are brought to the end of the chunk the device had made for it, as closing it
        would, and this run goes on from there.  The retired generator raises RuntimeError when it is resumed and
        changes nothing when it is closed or collected.  reset() and another sample() do the same.

        summary=True, or a dict of ``results.chain_summary``'s keywords (percentile, burn, thin, derived, redshift,
        lumdist_mpc -- a number each or one entry per source --, kappa, kappa_wave, lir_range, peak_model, clip,
        percentiles): the chain of this run is
        summarised on the device and ``sampler.summary`` is the ``results.ChainSummary`` of it; with
        storechain=False no chain crosses the bus.  The chain stays on the device until the sampler's next run
        (or reset), so that the summary can compute further percentiles on demand.

        convergence=True, or a dict of ``convergence()``'s keywords: the chain of this run is diagnosed on the device
        and ``sampler.convergence_`` is the ``diagnostics.ChainDiagnostics`` of it (None again after reset() and at the
        start of the next run).  With storechain=False it needs summary= too: that is what keeps the chain of a run on
        the device.

        marginals=True, or a dict of ``marginals()``'s keywords: the chain of this run is binned on the device and
        ``sampler.marginals_`` is the ``marginals.ChainMarginals`` of it (None again after reset() and at the start of
        the next run).  With storechain=False it needs summary= too; burn, thin, derived and the derived columns'
        settings default to those given with summary=.

        predict=specs, or a dict of ``predictions()``'s arguments (``specs`` among them): the fluxes the chain of this
        run predicts at those wavelengths and through those passbands are summarised on the device and
        ``sampler.predictions_`` is the ``predict.ChainPredictions`` of them (None again after reset() and at the
        start of the next run).  With storechain=False it needs summary= too; burn and thin default to those given
        with summary=.

        draws=n, or a dict of ``draws()``'s keywords (``n`` among them): that many cells per source are drawn from the
        chain of this run on the device and ``sampler.draws_`` is the ``draws.ChainDraws`` of them (None again after
        reset() and at the start of the next run).  With storechain=False it needs summary= too; burn, thin, derived
        and the derived columns' settings default to those given with summary=.

        loo=True, or a dict of ``loo()``'s keywords (burn, thin): the chain of this run is cross-validated on the device
        and ``sampler.loo_`` is the ``loo.ChainLoo`` of it (None again after reset() and at the start of the next run).
        With storechain=False it needs summary= too; burn and thin default to those given with summary=.

        goodness=True, or a dict of ``goodness()``'s keywords: the chain of this run is held against the data on the
        device and ``sampler.goodness_`` is the ``goodness.ChainGoodness`` of it (None again after reset() and at the
        start of the next run).  With storechain=False it needs summary= too; burn and thin default to those given
        with summary=.

        reweight=target, or a dict of ``reweight()``'s keywords with ``target`` among them: the chain of this run is
        reweighted under the target likelihood's density on the device and ``sampler.reweight_`` is the
        ``reweight.ChainReweight`` of it (None again after reset() and at the start of the next run).  Window and
        derived-column keywords default to summary='s.

        population=True, or a dict of ``population()``'s keywords: the chain of this run is pooled into a population
        block on the device and ``sampler.population_`` is the ``population.Population`` of it (None again after reset()
        and at the start of the next run).  With storechain=False it needs summary= too; burn and thin default to those
        given with summary=.

        evidence=True, or a dict of ``evidence()``'s keywords: ln Z of the chain of this run is bridge-sampled on the
        device and ``sampler.evidence_`` is the ``evidence.ChainEvidence`` of it (None again after reset() and at the
        start of the next run).  With storechain=False it needs summary= too; burn and thin default to those given
        with summary=."""
        self._retire()
        return self._run(pos0, N, lnprob0, storechain, summary, convergence=convergence, marginals=marginals,
                         predict=predict, draws=draws, goodness=goodness, evidence=evidence, loo=loo, reweight=reweight,
                         population=population)

    def _retire(self):
        """End the suspended sample() generator's hold on the attributes (run_mcmc's docstring)."""
        st, self._open = getattr(self, "_open", None), None
        if st is not None and st.live:
            st.live = False
            self._leave(st)

    def _leave(self, st):
        # the device made the whole chunk and run_mcmc(None, n) goes on from its end: the attributes show all of it
        self.iterations, self.naccepted = st.it_prev + st.made, st.acc_made
        if st.storechain:
            self._chain, self._lnprob = st.big_c[..., :st.n_prev + st.made, :], st.big_l[..., :st.n_prev + st.made]
        else:
            self._chain, self._lnprob = st.kept_c, st.kept_l
        if not st.single:
            self._resident = 0                # (what is resident is the last chunk: a part)

    def _run(self, pos0, N, lnprob0=None, storechain=True, summary=None, **asked):
        self._drop_predictions()                    # (the chain they could go back to is about to be overwritten)
        for an in _ANALYSES.values():
            setattr(self, an.attr, None)
        summarised = summary is not None and summary is not False
        kws = {}
        for key in _REQUEST_ORDER:
            value, an = asked.get(key), _ANALYSES[key]
            if value is None or value is False:
                continue
            if isinstance(value, dict):
                kw = dict(value)
            else:
                kw = {} if an.first is None else {an.first: value}
            if an.needs and an.first not in kw:
                raise ValueError(an.needs)
            if summarised and summary is not True:
                for k in an.inherits:
                    if k in summary:
                        kw.setdefault(k, summary[k])
            if an.allowed is not None and set(kw) - an.allowed:
                raise TypeError("{}= got unexpected keyword(s) {}".format(key, sorted(set(kw) - an.allowed)))
            req = an.request(self, kw)
            if not storechain and not summarised:
                raise ValueError("{}= with storechain=False needs summary= too: a run that neither stores "
                                 "nor summarises its chain keeps none on the device".format(key))
            an.check(self, req, kw, int(N))
            kws[key] = kw
        ctx, h = self._handle()
        verbs = [_ANALYSES[key].verb for key in _SHARDED_ORDER if key in kws] + ["summarised"] * summarised
        if verbs and (ctx.info("nranks") > 1 or getattr(ctx, "xchg_barrier", None)):
            raise ValueError("a sharded sampler run cannot be {} on the device: a rank holds only its own walkers' "
                             "chain".format(verbs[0]))
        req = self._summary_request({} if summary is True else dict(summary), int(N)) if summarised else None
        # sharded with the one-hop exchange (parallel.ipc_exchange_setup): the ranks are
        # held together around set_state, because a peer's kernel writes into this rank's
        # copy of the ensemble
        barrier = getattr(ctx, "xchg_barrier", None)
        if pos0 is None:
            if self._last is None:
                raise ValueError("Cannot have pos0=None if run_mcmc has never been called.")
        else:
            if barrier:
                ctx.sync(); barrier()
            p0 = np.ascontiguousarray(pos0, dtype=np.float64)
            want = (self.nsources, self.k, 5) if self.nsources > 1 else (self.k, 5)
            if p0.shape != want:
                raise ValueError("p0 must have shape {}".format(want))
            if np.any(np.isinf(p0)):
                raise ValueError("At least one parameter value was infinite.")
            if np.any(np.isnan(p0)):
                raise ValueError("At least one parameter value was NaN.")
            l0 = None if lnprob0 is None else np.ascontiguousarray(lnprob0, dtype=np.float64)
            if l0 is not None:
                # (the native side reads nsources * nw doubles from it and takes them as they are)
                if l0.shape != want[:-1]:
                    raise ValueError("lnprob0 must have shape {}".format(want[:-1]))
                if np.any(np.isnan(l0)):
                    raise ValueError("The initial lnprob was NaN.")
            try:
                _native._check(ctx.lib.mbb_sampler_set_state(
                    ctx.h, h, _native._d(p0), _native._d(l0) if l0 is not None else None))
            except _native.NativeError as e:
                raise ValueError(str(e))
            if barrier:
                barrier()
        N = int(N)
        lead = (self.nsources, self.k) if self.nsources > 1 else (self.k,)
        # (zeros where a run is sharded over ranks -- the one-hop exchange or a communicator, whether or not a
        # barrier was handed in: only this rank's walkers are filled in there)
        alloc = np.zeros if (barrier or ctx.info("nranks") > 1) else np.empty
        chain = alloc(lead + (N, 5)) if storechain else None
        lnp = alloc(lead + (N,)) if storechain else None
        pos = np.empty(lead + (5,))
        lnprob = np.empty(lead)
        nacc = np.zeros(lead)
        fallbacks = ctx.info("flow_fallbacks")
        self._resident = 0
        if self.summary is not None:
            self.summary.drop_chain()            # (the chain it could go back to is about to be overwritten)
            self.summary = None
        if req is None:
            rc = ctx.lib.mbb_sampler_run(ctx.h, h, N, self.a,
                                         _native._d(chain) if storechain else None,
                                         _native._d(lnp) if storechain else None,
                                         _native._d(pos), _native._d(lnprob), _native._d(nacc))
        else:
            from . import results
            raw = results._Raw(self.nsources, len(req.qs))
            spec, out = req.spec(), raw.out()
            rc = ctx.lib.mbb_sampler_run_summary(ctx.h, h, N, self.a, C.byref(spec), C.byref(out),
                                                 _native._d(chain) if storechain else None,
                                                 _native._d(lnp) if storechain else None,
                                                 _native._d(pos), _native._d(lnprob), _native._d(nacc))
        _native.check_arg(rc, ctx)
        if ctx.info("flow_fallbacks") > fallbacks:
            import warnings
            warnings.warn("the one-launch form of the device sampler gave up waiting (a workgroup was not "
                          "resident: another process on the GPU?) and the run was redone as a train of "
                          "launches, about 2.5x slower; same chain.  %d such run(s) on this context so far%s"
                          % (ctx.info("flow_fallbacks"),
                             "; the one-launch form now rests for %d runs" % ctx.info("flow_resting")
                             if ctx.info("flow_resting") else ""), RuntimeWarning, stacklevel=2)
        self.iterations += N
        self.naccepted = nacc
        if storechain:
            ax = len(lead)
            if self._chain.shape[ax] == 0:            # the usual case (after reset): no second copy of the chain
                self._chain, self._lnprob = chain, lnp
            else:
                self._chain = np.concatenate((self._chain, chain), axis=ax)
                self._lnprob = np.concatenate((self._lnprob, lnp), axis=ax)
        self._last = (pos, lnprob)
        if (storechain or req is not None) and N > 0 and not (barrier or ctx.info("nranks") > 1):
            self._resident = N
        if req is not None:
            self.summary = results.ChainSummary(self.lnprobfn, req, raw, self.nsources > 1, self._summarise_again,
                                                self._summary_percentile)
        for key in _RESULT_ORDER:
            if key in kws:
                an = _ANALYSES[key]
                setattr(self, an.attr, getattr(self, an.method)(**kws[key]))
        return pos, lnprob, self.seed

    def _summary_request(self, kw, nsteps):
        from . import results
        cens, qs = _analysis.quantiles(kw.pop("percentile", 68.3), kw.pop("percentiles", ()))
        self._summary_percentile = cens[0]
        req = results._Request(qs, nsources=self.nsources, **kw)
        req.check_steps(nsteps)
        return req

    def _summarise_again(self, req):
        """Another summary of the chain the last summarised run left on the device (mbb_sampler_run_summary, 0 steps)."""
        from . import results
        ctx, h = self._handle()
        raw = results._Raw(self.nsources, len(req.qs))
        spec, out = req.spec(), raw.out()
        rc = ctx.lib.mbb_sampler_run_summary(ctx.h, h, 0, self.a, C.byref(spec), C.byref(out), None, None, None, None, None)
        _native.check_arg(rc, ctx)
        return raw

    def sample(self, p0, lnprob0=None, rstate0=None, iterations=1, storechain=True, chunk=64):
        """emcee's generator form (``for pos, lnprob, rstate in sampler.sample(p0, iterations=N)``): the ensemble after
        every step.  The steps are made ``chunk`` at a time in one launch on the device -- a launch has a fixed cost of
        ~20 us beside ~6 us per step -- and handed out one by one.  ``rstate0`` is accepted for emcee's call
        convention and ignored: the random stream is the sampler's ``seed`` (Philox, counted by step and row).

        One trajectory.  The chain is run_mcmc(p0, iterations)'s whatever the chunk and whatever ``storechain``: a
        step's draws are keyed by its number in the sampler's life, not by its place in a launch; with ``p0`` None
        the call goes on where the last run or sample() left the device (run_mcmc's docstring).

        While step j is out, ``chain``, ``lnprobability``, ``iterations``, ``naccepted`` and ``acceptance_fraction``
        are those after the steps handed out so far -- as with emcee, where a step exists only once it has been yielded
        -- although the device is up to ``chunk`` - 1 steps ahead.  That holds on top of a chain stored before, and with
        ``storechain=False``, where ``chain`` stays what it was.  On a sampler sharded with the one-hop exchange the
        per-step ``naccepted`` counts this rank's walkers only; the other rows stay 0, as the chain does there.

        Leaving early (``break``, ``close()``) leaves the sampler at the end of the chunk the device made:
        ``run_mcmc(None, n)`` goes on from there, and the attributes then show that whole chunk.

        run_mcmc, reset or another sample() on a sampler whose generator is still suspended retire that generator
        first: the attributes go to the end of the chunk the device made, exactly as closing it would, and the call
        proceeds.  The retired generator raises RuntimeError when it is resumed and changes nothing when it is closed
        or collected.

        ``lnprob0`` is run_mcmc's (exact shape, no NaN, taken as given) and applies to the first chunk only.  What
        run_mcmc refuses -- a wrong shape, NaN or inf in ``p0``, ``p0`` None without a state -- sample() refuses at
        the first ``next()``; ``iterations=0`` sets the state as ``run_mcmc(p0, 0)`` does and yields nothing.

        Afterwards ``summary``, ``convergence_``, ``marginals_`` and ``predictions_`` are None.  ``convergence()`` describes all the steps this call
        made where the whole run was one chunk (``iterations`` <= ``chunk``), which is then resident on the device;
        otherwise it raises its "no chain of this sampler is resident" ValueError: it never describes a part."""
        self._retire()
        return self._sample(p0, lnprob0, max(0, int(iterations)), bool(storechain), max(1, int(chunk)))

    def _sample(self, p0, lnprob0, iterations, storechain, chunk):
        self._retire()                        # (one that was begun between the call and this first next())
        ax = 1 if self.nsources == 1 else 2
        st = _OpenSample()
        st.live, st.storechain, st.single = True, storechain, iterations <= chunk
        st.kept_c, st.kept_l = self._chain, self._lnprob
        n_prev = st.n_prev = st.kept_c.shape[ax]
        it_prev = st.it_prev = self.iterations
        st.big_c = st.big_l = None
        if storechain:
            # (room for the whole run once, filled chunk by chunk: no chain is copied more than that)
            st.big_c = np.empty(st.kept_c.shape[:ax] + (n_prev + iterations, self.dim))
            st.big_l = np.empty(st.kept_l.shape[:ax] + (n_prev + iterations,))
            st.big_c[..., :n_prev, :] = st.kept_c
            st.big_l[..., :n_prev] = st.kept_l
        pos0, l0 = p0, lnprob0
        done = st.made = 0                    # steps handed out / made on the device by this call
        st.acc_made = self.naccepted
        cur = None if p0 is None else np.asarray(p0, dtype=np.float64)
        if cur is None and self._last is not None:
            cur = self._last[0]
        own = None
        self._open = st
        try:
            while True:
                k = min(chunk, iterations - done)
                acc_before = np.array(self.naccepted, dtype=np.float64, copy=True)
                self._chain, self._lnprob = st.kept_c[..., :0, :], st.kept_l[..., :0]
                self._run(pos0, k, lnprob0=l0, storechain=True)
                steps, lnps = self._chain, self._lnprob          # (this chunk's own arrays)
                st.made, st.acc_made = st.made + k, self.naccepted
                if not st.single:
                    self._resident = 0                            # (one chunk of several: a part of the run)
                if st.made == k:
                    # sharded with the one-hop exchange: the rows of the other ranks' walkers are zeros
                    ctx = self._ctx
                    if hasattr(ctx, "xchg_barrier") and ctx.info("nranks") > 1:
                        own = _own_rows(self.k, ctx.info("rank"), ctx.info("nranks"))
                pos0 = l0 = None
                if storechain:
                    st.big_c[..., n_prev + done:n_prev + done + k, :] = steps
                    st.big_l[..., n_prev + done:n_prev + done + k] = lnps
                moved = accepted_by_step(cur, steps, own)
                if k > 0:
                    cur = steps[..., k - 1, :]
                for j in range(k):
                    done += 1
                    if storechain:
                        self._chain, self._lnprob = st.big_c[..., :n_prev + done, :], st.big_l[..., :n_prev + done]
                    else:
                        self._chain, self._lnprob = st.kept_c, st.kept_l
                    self.iterations = it_prev + done
                    self.naccepted = st.acc_made if j == k - 1 else acc_before + moved[..., j]
                    yield steps[..., j, :], lnps[..., j], self.seed
                    if not st.live:
                        raise RuntimeError("this sample() generator was retired by a later run_mcmc, reset or sample() "
                                           "of its sampler: the sampler has gone on from the end of its chunk")
                if done >= iterations:
                    break
        finally:
            # (left early, inside a chunk: the device made the whole chunk and run_mcmc(None, n) goes on from its end --
            # the attributes then show all of it; a retired generator has handed that over already and touches nothing)
            if st.live:
                st.live = False
                self._leave(st)
                if self._open is st:
                    self._open = None

    def advance_async(self, N):
        """Enqueue N steps without storing or synchronising (benchmarks)."""
        ctx, h = self._handle()
        _native._check(ctx.lib.mbb_sampler_advance_async(ctx.h, h, int(N), self.a))

    def flow_counters(self, store=None):
        """The completion counters of the sampler's one-launch runs (the lag guard of forms 7 and 9) as an array
        [2 sets, ring, shards] of uint64, and the set the next launch uses; `store`: such an array, written first.
        A test hook."""
        ctx, h = self._handle()
        buf = (C.c_ulonglong * 256)()
        ring, shards, nxt = C.c_int(), C.c_int(), C.c_int()
        if store is not None:
            flat = np.asarray(store, dtype=np.uint64).reshape(-1)
            for i, v in enumerate(flat):
                buf[i] = int(v)
            _native._check(ctx.lib.mbb_sampler_flow_counters(ctx.h, h, buf, 256, 1, C.byref(ring), C.byref(shards), C.byref(nxt)))
        _native._check(ctx.lib.mbb_sampler_flow_counters(ctx.h, h, buf, 256, 0, C.byref(ring), C.byref(shards), C.byref(nxt)))
        n = 2 * ring.value * shards.value
        return np.array(buf[:n], dtype=np.uint64).reshape(2, ring.value, shards.value), nxt.value

    def advance_timed(self, N):
        """N steps as advance_async enqueues them, timed inside one native call: (wall seconds from an
        idle stream to an idle stream, stream milliseconds between two events).  Benchmarks."""
        ctx, h = self._handle()
        wall, ms = C.c_double(), C.c_float()
        _native._check(ctx.lib.mbb_sampler_advance_timed(ctx.h, h, int(N), self.a, C.byref(wall), C.byref(ms)))
        return wall.value, ms.value

    def __del__(self):
        try:
            if self._h is not None and self._ctx is not None and self._ctx.h:
                self._ctx.lib.mbb_sampler_destroy(self._ctx.h, self._h)
        except Exception:
            pass
