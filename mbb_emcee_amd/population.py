"""The population of a catalogue: how chosen parameters are distributed OVER the sources of a multi-source chain,
computed on the MI355X where the chain is (csrc/mbb_population.hip.h).

Every other analysis of the package answers a question about one source.  The scatter of per-source best fits cannot
say how T and beta are distributed over a catalogue: the T-beta degeneracy of a modified blackbody makes that scatter
anticorrelated even when the population is not.  The cure is a population model fitted THROUGH the per-source
posteriors (Kelly et al. 2012; Hogg, Myers & Bovy 2010 for the importance-sampling form used here): each source's chain
was sampled under the run's own "interim" prior pi0, and for a Gaussian population N(x | mu, Sigma) over
x = g(theta[columns]) the catalogue's likelihood is

    ln L(mu, Sigma) = sum_n ln mean_j N(x_nj | mu, Sigma) / pi0(x_nj),

a log-mean-exp over each source's window.  ``chain_population`` (a stored chain) or ``sampler.population()`` (the chain
a ``DeviceEnsembleSampler`` run left on the device) turn the window into a compact block the context keeps;
``Population.evaluate`` takes up to 1024 candidates at once; ``Population.sample`` runs the package's host ensemble
sampler over the unconstrained vector u = (mu, ln L_ii, off-diagonals of L), one device call per half-step.

What it does not do: derived columns (peak wavelength, L_IR, dust mass) cannot be chosen, because their interim prior
density is not known in closed form; the population Gaussian is not renormalised over the hard lower limits
(``mass_below`` says how much of it lies below them: results mean little where that is not small); a likelihood with a
limit or a prior on the peak wavelength is refused, because that factor is not separable; the hyper-sampler runs on
the host.  The definitions are in include/mbb_hip.h.
"""
import ctypes as C
import math

import numpy as np

from . import _analysis, _native

__all__ = ["chain_population", "Population", "PopulationEval", "PopulationFit"]

PARAM_NAMES = ("T", "beta", "lambda0", "alpha", "fnorm")
_DERIVED_NAMES = ("peaklambda", "lambda_peak", "peaklam", "lir", "dustmass")
MAX_CAND = _native.POP_MAX_CAND
BROAD_SIGMA = 1e10          # source_means(): a candidate so broad that only the 1 / pi0 weights remain
ESS_LOW = 5.0
RHO_MAX = 0.999


def _tri(d):
    return d * (d + 1) // 2


class _Request(_analysis.Window):
    """What one native population build is asked for (mbb_population_spec); everything is checked here, before the
    device is touched."""

    def __init__(self, like, columns=("T", "beta"), transform=None, burn=0, thin=1, fixed=None):
        if not hasattr(like, "_sync_device"):
            raise TypeError("a population is built with the mbb_emcee_amd.likelihood the chain was sampled under")
        if isinstance(columns, (str, int)):
            columns = (columns,)
        cols = []
        for c in columns:
            if isinstance(c, str):
                if c.lower() in _DERIVED_NAMES:
                    raise ValueError("{} is a derived column: its interim prior density is not known in closed form, so it "
                                     "cannot be a population column".format(c))
                if c not in PARAM_NAMES:
                    raise ValueError("unknown population column {!r}: choose among {}".format(c, ", ".join(PARAM_NAMES)))
                c = PARAM_NAMES.index(c)
            c = int(c)
            if not 0 <= c < 5:
                raise ValueError("unknown population column {:d}: the five parameters are 0 to 4".format(c))
            if c in cols:
                raise ValueError("population column {} is given twice".format(PARAM_NAMES[c]))
            cols.append(c)
        if not 1 <= len(cols) <= 5:
            raise ValueError("a population has 1 to 5 columns")
        self.cols = cols
        self.names = [PARAM_NAMES[c] for c in cols]
        if transform is None:
            tr = [None] * len(cols)
        elif isinstance(transform, dict):
            unknown = [k for k in transform if k not in self.names]
            if unknown:
                raise ValueError("transform names column(s) that are not chosen: {}".format(sorted(unknown)))
            tr = [transform.get(n) for n in self.names]
        elif isinstance(transform, str):
            tr = [transform] * len(cols)
        else:
            tr = list(transform)
            if len(tr) != len(cols):
                raise ValueError("transform must give one entry per column")
        self.transform = []
        for t in tr:
            number = isinstance(t, (int, np.integer)) and not isinstance(t, bool)
            if t is None or t == "identity" or (number and t == _native.POP_IDENTITY):
                self.transform.append(_native.POP_IDENTITY)
            elif t == "log10" or (number and t == _native.POP_LOG10):
                self.transform.append(_native.POP_LOG10)
            else:
                raise ValueError("unknown transform {!r}: 'identity' or 'log10'".format(t))
        self.set_window(burn, thin)
        held_fit = np.zeros(5, dtype=bool) if fixed is None else np.asarray(fixed).astype(bool).ravel()
        if held_fit.size != 5:
            raise ValueError("fixed must have five entries")
        held_model = (False, False, bool(like.opthin), bool(like.noalpha), False)
        for c, t in zip(cols, self.transform):
            if held_fit[c]:
                raise ValueError("{} is held fixed by the fit: a constant column has no population".format(PARAM_NAMES[c]))
            if held_model[c]:
                raise ValueError("{} is held by the model variant ({}): it has no population".format(
                    PARAM_NAMES[c], "optically thin" if c == 2 else "noalpha"))
            if t == _native.POP_LOG10 and not float(like._lowlim[c]) > 0.0:
                raise ValueError("log10 of {} needs a lower limit above 0, not {:g}".format(PARAM_NAMES[c],
                                                                                           float(like._lowlim[c])))
        if like._has_uplim[5] or like._has_gprior[5]:
            raise ValueError("the likelihood has a limit or a prior on the peak wavelength: that factor of the interim "
                             "prior is not separable over the parameters, so no population can be built under it")
        self.has_uplim = [int(bool(b)) for b in like._has_uplim[:5]]
        self.has_gprior = [int(bool(b)) for b in like._has_gprior[:5]]
        self.lowlim = [float(v) for v in like._lowlim[:5]]
        self.uplim = [float(v) if h else math.inf for v, h in zip(like._uplim[:5], self.has_uplim)]
        self.gmean = [float(v) for v in like._gprior_mean[:5]]
        self.givar = [float(v) for v in like._gprior_ivar[:5]]
        # g(lowlim) per column, for mass_below
        self.glow = np.array([math.log10(self.lowlim[c]) if t == _native.POP_LOG10 else self.lowlim[c]
                              for c, t in zip(cols, self.transform)])

    @property
    def d(self):
        return len(self.cols)

    def spec(self):
        s = _native.PopulationSpec()
        s.d, s.burn, s.thin = self.d, self.burn, self.thin
        for i, (c, t) in enumerate(zip(self.cols, self.transform)):
            s.col[i], s.transform[i] = c, t
        for k in range(5):
            s.has_uplim[k], s.has_gprior[k] = self.has_uplim[k], self.has_gprior[k]
            s.lowlim[k], s.uplim[k], s.gmean[k], s.givar[k] = self.lowlim[k], self.uplim[k], self.gmean[k], self.givar[k]
        return s


class _BuildRaw(object):
    """The arrays of one native build (mbb_population_build_out)."""

    def __init__(self, nsrc):
        self.n_used, self.n_left_out = np.zeros(nsrc, dtype=np.int64), np.zeros(nsrc, dtype=np.int64)
        self.status = np.zeros(nsrc, dtype=np.int32)
        self.serial = np.zeros(1, dtype=np.int64)

    def out(self):
        return _analysis.bind_out(_native.PopulationBuildOut, vars(self))


def _built(ctx, rc, req, raw, multi, nwalkers, nkept):
    _native.check_arg(rc, ctx)
    ctx._pop_serial = int(raw.serial[0])
    return Population(ctx, req, raw, multi, nwalkers, nkept)


def chain_population(like, chain, columns=("T", "beta"), transform=None, burn=0, thin=1, fixed=None):
    """The population block of a stored chain [nsources, nw, nsteps, 5] (or [nw, nsteps, 5]: one source) over the steps
    ``chain[:, burn::thin]``, built on ``like``'s device; returns a ``Population``.

    like : the ``likelihood`` the chain was sampled under: its limits and priors are the interim prior.
    columns : 1 to 5 of "T", "beta", "lambda0", "alpha", "fnorm" (or 0 .. 4), each at most once.
    transform : None, "log10" for every column, a sequence with an entry per column, or a dict by column name; an
        entry is None / "identity" or "log10".
    fixed : the parameters the fit held fixed [5]; such a column is refused.
    A context keeps one block: the next build in it replaces this one, and this ``Population`` raises from then on."""
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    req = _Request(like, columns, transform, burn, thin, fixed)
    nkept = req.check_steps(nsteps)
    ctx = _native.analysis_context(like)
    raw = _BuildRaw(nsrc)
    spec, out = req.spec(), raw.out()
    rc = ctx.lib.mbb_chain_population_build(ctx.h, _native._d(c4), nsrc, nw, nsteps, C.byref(spec), C.byref(out))
    return _built(ctx, rc, req, raw, multi, nw, nkept)


def sampler_population(sampler, **kw):
    """``DeviceEnsembleSampler.population``: the same of the chain the sampler's last run left on the device."""
    req = _Request(sampler.lnprobfn, **kw)
    nkept = req.check_steps(sampler._resident_steps("population"))
    ctx, h = sampler._handle()
    raw = _BuildRaw(sampler.nsources)
    spec, out = req.spec(), raw.out()
    rc = ctx.lib.mbb_sampler_population_build(ctx.h, h, C.byref(spec), C.byref(out))
    return _built(ctx, rc, req, raw, sampler.nsources > 1, sampler.k, nkept)


def _norm_cdf(z):
    return 0.5 * math.erfc(-z / math.sqrt(2.0))


class PopulationEval(object):
    """Candidates evaluated against a population block.  With H candidates and nsrc sources (no leading axis for a
    single candidate, no source axis for a chain without one):
    ``lnl`` [H]; ``n_sources_used`` [H]; ``status`` [H] (BAD, UNDERFLOW, HAS_EMPTY);
    ``lnl_source``, ``ess`` [H, nsrc];  with moments ``mean`` [H, nsrc, d] and ``covariance`` [H, nsrc, d, d], each
    source's posterior shrunk by that population, else None;
    ``mass_below`` [H, d]: the population's marginal mass below each column's hard lower limit, which the likelihood
    does not renormalise for."""
    BAD, UNDERFLOW, HAS_EMPTY = _native.POP_CAND_BAD, _native.POP_CAND_UNDERFLOW, _native.POP_CAND_HAS_EMPTY

    def __init__(self, lnl, nused, status, lnl_src, ess, mean, cov, mass_below, single, multi):
        def shape(a):
            if a is None:
                return None
            if not multi and a.ndim >= 2:
                a = a[:, 0]
            return a[0] if single else a
        self.lnl, self.n_sources_used, self.status = shape(lnl), shape(nused), shape(status)
        self.lnl_source, self.ess = shape(lnl_src), shape(ess)
        self.mean, self.covariance = shape(mean), shape(cov)
        self.mass_below = mass_below[0] if single else mass_below


class Population(_analysis.Result):
    """The population block of a chain, resident on the device (``chain_population``, ``sampler.population()``).

    ``n_used``, ``n_left_out``, ``status`` per source (EMPTY: no used entry, the source is left out of every total;
    HAS_NAN: entries were left out -- a cell that is not finite, theta <= 0 under log10, or no finite interim prior);
    ``columns``, ``transforms``; ``serial``, the block's number in its context."""
    EMPTY, HAS_NAN = _native.SUM_EMPTY, _native.SUM_HAS_NAN

    def __init__(self, ctx, request, raw, multi, nwalkers=0, nkept=0):
        self._ctx, self._req, self._raw, self._multi = ctx, request, raw, bool(multi)
        self.serial = int(raw.serial[0])
        self.d = request.d
        self.columns = list(request.names)
        self.transforms = ["log10" if t == _native.POP_LOG10 else "identity" for t in request.transform]
        self.nsources = int(raw.status.shape[0])
        self._closed = False
        self._set_window(request, nwalkers, nkept)

    n_used = property(lambda self: self._squeeze(self._raw.n_used).copy())
    n_left_out = property(lambda self: self._squeeze(self._raw.n_left_out).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())

    # ---- (mu, Sigma) <-> u <-> the rows the library takes ------------------------------------------
    def pack(self, mu, cov):
        """u = (mu, ln L_ii, the off-diagonals of L row by row), L the lower Cholesky factor of ``cov``."""
        return pack(mu, cov)

    def unpack(self, u):
        """(mu, Sigma) of u; Sigma = L L^T is positive definite whatever u."""
        return unpack(u, self.d)

    def _rows(self, mu, cov, chol):
        mu = np.asarray(mu, dtype=np.float64)
        single = mu.ndim == 1
        mu = np.atleast_2d(mu)
        H, d = mu.shape
        if d != self.d:
            raise ValueError("mu must have {:d} values per candidate".format(self.d))
        if (cov is None) == (chol is None):
            raise ValueError("give cov or chol, one of the two")
        m = np.asarray(cov if chol is None else chol, dtype=np.float64)
        m = np.broadcast_to(m, (H, d, d)) if m.ndim == 2 else m
        if m.shape != (H, d, d):
            raise ValueError("cov / chol must be [d, d] or [H, d, d]")
        if chol is None:
            L = np.full((H, d, d), np.nan)
            for h in range(H):
                try:
                    L[h] = np.linalg.cholesky(m[h])
                except np.linalg.LinAlgError:
                    pass                                  # (a bad candidate: NaN results, the others unaffected)
        else:
            L = m
        if not 1 <= H <= MAX_CAND:
            raise ValueError("a population evaluation takes 1 to {:d} candidates".format(MAX_CAND))
        il = np.tril_indices(d)
        rows = np.ascontiguousarray(np.concatenate([mu, L[:, il[0], il[1]]], axis=1))
        return rows, L, single

    def _call(self, rows, moments=False, tables=True):
        if self._closed:
            raise RuntimeError("this Population was closed")
        H, ns, d = rows.shape[0], self.nsources, self.d
        lnl = np.full(H, np.nan)
        nused, status = np.zeros(H, dtype=np.int32), np.zeros(H, dtype=np.int32)
        arrays = dict(lnl=lnl, n_src_used=nused, cand_status=status)
        if tables:
            arrays["lnl_src"], arrays["ess"] = np.full((H, ns), np.nan), np.full((H, ns), np.nan)
        if moments:
            arrays["mean"], arrays["cov"] = np.full((H, ns, d), np.nan), np.full((H, ns, d, d), np.nan)
        out = _analysis.bind_out(_native.PopulationEvalOut, arrays)
        ctx = self._ctx
        rc = ctx.lib.mbb_population_eval(ctx.h, self.serial, _native._d(rows), H, 1 if moments else 0, C.byref(out))
        if rc == -3:
            raise RuntimeError("this Population's block is no longer in its context ({}): a later build replaced it; "
                               "build it again".format(ctx.lib.mbb_last_error().decode()))
        _native.check_arg(rc, ctx)
        return arrays

    def _mass_below(self, mu, L):
        sig = np.sqrt(np.einsum("hik,hik->hi", L, L))
        out = np.full(mu.shape, np.nan)
        for h in range(mu.shape[0]):
            for i in range(mu.shape[1]):
                if np.isfinite(sig[h, i]) and sig[h, i] > 0 and np.isfinite(mu[h, i]):
                    out[h, i] = _norm_cdf((self._req.glow[i] - mu[h, i]) / sig[h, i])
        return out

    def evaluate(self, mu, cov=None, chol=None, moments=False):
        """``PopulationEval`` of the candidate(s) (mu [d] or [H, d]; cov [d, d] or [H, d, d], or chol: its lower
        Cholesky factor) -- one device call for all of them."""
        rows, L, single = self._rows(mu, cov, chol)
        a = self._call(rows, moments)
        return PopulationEval(a["lnl"], a["n_src_used"], a["cand_status"], a["lnl_src"], a["ess"], a.get("mean"),
                              a.get("cov"), self._mass_below(rows[:, :self.d], L), single, self._multi)

    def lnlike(self, mu, cov=None, chol=None):
        """The catalogue's ln L of the candidate(s): the totals alone come back."""
        rows, L, single = self._rows(mu, cov, chol)
        lnl = self._call(rows, tables=False)["lnl"]
        return float(lnl[0]) if single else lnl

    def source_means(self):
        """[nsources, d]: each source's mean of x under a candidate so broad (sigma = 1e10) that only the 1 / pi0
        weights remain -- the interim prior divided out, no population imposed.  Used to choose a start."""
        d = self.d
        a = self._call(np.concatenate([np.zeros(d), (BROAD_SIGMA * np.eye(d))[np.tril_indices(d)]])[None], moments=True)
        return a["mean"][0]

    def close(self):
        """Drop the block (if it is still this one) and free its device memory."""
        if not self._closed and getattr(self._ctx, "_pop_serial", None) == self.serial and getattr(self._ctx, "h", None):
            _native._check(self._ctx.lib.mbb_population_drop(self._ctx.h))
            self._ctx._pop_serial = None
        self._closed = True

    # ---- the hyper-posterior -----------------------------------------------------------------------
    def default_bounds(self, means=None):
        """(mu_lo [d], mu_hi [d], s [d]) of the default prior: mu_i within the per-source means' range widened by three
        of their standard deviations s_i; sigma_i within [s_i / 100, 100 s_i]; |rho| < 0.999.  A modelling default."""
        m = self.source_means() if means is None else np.asarray(means, dtype=np.float64)
        m = m[np.all(np.isfinite(m), axis=1)]
        if m.shape[0] < 2:
            raise ValueError("the default prior needs two sources with a finite mean at least; give bounds= or lnprior=")
        s = m.std(axis=0, ddof=1)
        if not np.all(s > 0):
            raise ValueError("the per-source means do not scatter: give bounds= or lnprior=")
        return m.min(axis=0) - 3.0 * s, m.max(axis=0) + 3.0 * s, s

    def _sample_eval(self, mu, L):
        """(lnl [H], the number of sources with ess < 5 [H]) of the candidates, for ``sample``."""
        il = np.tril_indices(self.d)
        a = self._call(np.ascontiguousarray(np.concatenate([mu, L[:, il[0], il[1]]], axis=1)))
        with np.errstate(invalid="ignore"):
            return a["lnl"], np.sum(a["ess"] < ESS_LOW, axis=1)

    def sample(self, nsteps=500, nwalkers=None, nburn=None, start=None, bounds=None, lnprior=None, seed=None):
        """The hyper-posterior of (mu, Sigma) sampled by the package's host ``ensemble.EnsembleSampler`` over
        u = (mu, ln L_ii, off-diagonals of L); each half-step is ONE device call of nwalkers / 2 candidates.  Returns a
        ``PopulationFit`` of the ``nsteps`` steps after ``nburn`` (default nsteps // 4) discarded ones.

        start : u [len(u)] to scatter the walkers about, or [nwalkers, len(u)]; default: the mean and covariance of
            ``source_means()``.
        The prior is flat in u inside a region.  Default (a modelling choice, made from the per-source means; replace it
        where it does not suit): ``default_bounds``.  bounds : [len(u), 2] lower and upper bounds of u itself instead.
        lnprior : a callable u -> ln prior (-inf outside) instead of either."""
        from .ensemble import EnsembleSampler, integrated_time
        d = self.d
        nu = d + _tri(d)
        nwalkers = max(32, 4 * nu) if nwalkers is None else int(nwalkers)
        nsteps = int(nsteps)
        nburn = nsteps // 4 if nburn is None else int(nburn)
        if nsteps < 1 or nburn < 0:
            raise ValueError("nsteps must be positive and nburn not negative")
        rng = np.random.RandomState(seed)
        means = None
        if bounds is not None:
            b = np.asarray(bounds, dtype=np.float64)
            if b.shape != (nu, 2) or not np.all(b[:, 0] < b[:, 1]):
                raise ValueError("bounds must be [{:d}, 2], lower below upper".format(nu))
        if lnprior is None and bounds is None:
            means = self.source_means()
            mlo, mhi, s = self.default_bounds(means)

            def lnprior(u):
                mu, cov = unpack(u, d)
                sig = np.sqrt(np.diag(cov))
                if np.any(mu < mlo) or np.any(mu > mhi) or np.any(sig < s / 100.0) or np.any(sig > 100.0 * s):
                    return -np.inf
                rho = cov / np.outer(sig, sig)
                return 0.0 if np.all(np.abs(rho[np.tril_indices(d, -1)]) < RHO_MAX) else -np.inf
        elif lnprior is None:
            def lnprior(u):
                return 0.0 if np.all(u >= b[:, 0]) and np.all(u <= b[:, 1]) else -np.inf
        if start is None or np.ndim(start) == 1:
            if start is None:
                if bounds is not None:
                    u0, scat = b.mean(axis=1), 0.01 * (b[:, 1] - b[:, 0])
                else:
                    means = self.source_means() if means is None else means
                    ok = means[np.all(np.isfinite(means), axis=1)]
                    u0 = pack(ok.mean(axis=0), np.atleast_2d(np.cov(ok.T, ddof=1)))
                    scat = np.concatenate([0.1 * ok.std(axis=0, ddof=1), np.full(nu - d, 0.05)])
            else:
                u0 = np.asarray(start, dtype=np.float64)
                scat = np.concatenate([0.01 * np.maximum(np.abs(u0[:d]), 1e-3), np.full(nu - d, 0.01)])
            if u0.shape != (nu,):
                raise ValueError("start must have {:d} values".format(nu))
            p0 = u0 + scat * rng.standard_normal((nwalkers, nu))
            for k in range(nwalkers):                      # (inside the prior: pull a walker back towards u0)
                t = 0
                while not np.isfinite(lnprior(p0[k])) and t < 60:
                    p0[k] = u0 + 0.5 * (p0[k] - u0)
                    t += 1
        else:
            p0 = np.array(start, dtype=np.float64)
            if p0.shape != (nwalkers, nu):
                raise ValueError("start must be [{:d}] or [{:d}, {:d}]".format(nu, nwalkers, nu))
        low = {}

        def lnprob(U):
            out = np.full(U.shape[0], -np.inf)
            pri = np.array([lnprior(u) for u in U], dtype=np.float64)
            ok = np.flatnonzero(np.isfinite(pri))
            if ok.size:
                mu, L = _factors(U[ok], d)
                lnl, nlow = self._sample_eval(mu, L)
                v = lnl + pri[ok]
                out[ok] = np.where(np.isnan(v), -np.inf, v)
                for k, i in enumerate(ok):
                    low[U[i].tobytes()] = int(nlow[k])
            return out
        es = EnsembleSampler(nwalkers, nu, lnprob, vectorize=True, seed=rng.randint(0, 2 ** 31 - 1))
        pos = p0
        lnp0 = None
        if nburn:
            pos, lnp0, _ = es.run_mcmc(p0, nburn)
            es.reset()
        es.run_mcmc(pos, nsteps, lnprob0=lnp0)
        chain, lp = es.chain, es.lnprobability
        nlow = sum(low.get(row.tobytes(), 0) for row in chain.reshape(-1, nu))
        tau = np.array([integrated_time(chain[:, :, i].mean(axis=0)) for i in range(nu)])
        return PopulationFit(self.columns, d, chain, lp, es.acceptance_fraction, tau,
                             nlow / float(chain.shape[0] * chain.shape[1] * max(self.nsources, 1)))


def pack(mu, cov):
    """u = (mu, ln L_ii, the off-diagonals of L row by row) of (mu [d], Sigma [d, d])."""
    mu = np.asarray(mu, dtype=np.float64).ravel()
    d = mu.size
    L = np.linalg.cholesky(np.asarray(cov, dtype=np.float64).reshape(d, d))
    return np.concatenate([mu, np.log(np.diag(L)), L[np.tril_indices(d, -1)]])


def _factors(U, d):
    """(mu [H, d], L [H, d, d]) of rows of u."""
    U = np.atleast_2d(np.asarray(U, dtype=np.float64))
    if U.shape[1] != d + _tri(d):
        raise ValueError("u has {:d} values for {:d} columns".format(d + _tri(d), d))
    L = np.zeros((U.shape[0], d, d))
    i = np.arange(d)
    L[:, i, i] = np.exp(U[:, d:2 * d])
    il = np.tril_indices(d, -1)
    L[:, il[0], il[1]] = U[:, 2 * d:]
    return U[:, :d].copy(), L


def unpack(u, d):
    """(mu, Sigma) of u (or of rows of u); Sigma = L L^T."""
    single = np.ndim(u) == 1
    mu, L = _factors(u, d)
    cov = np.einsum("hik,hjk->hij", L, L)
    return (mu[0], cov[0]) if single else (mu, cov)


class PopulationFit(object):
    """The hyper-chain of ``Population.sample``: ``chain`` [nwalkers, nsteps, len(u)] of u = (mu, ln L_ii,
    off-diagonals of L) and ``lnprob`` [nwalkers, nsteps] (ln L + ln prior); ``acceptance_fraction`` [nwalkers];
    ``integrated_time`` per dimension of u (of the walkers' mean; NaN when the chain is too short to tell);
    ``ess_low``: the share of (kept candidate, source) pairs whose importance-sampling ess is below 5 -- where it is not
    small the per-source chains are too short for populations this narrow, and the numbers here are not to be trusted."""

    def __init__(self, columns, d, chain, lnprob, acceptance_fraction, integrated_time, ess_low):
        self.columns, self.d = list(columns), int(d)
        self.chain, self.lnprob = chain, lnprob
        self.acceptance_fraction = acceptance_fraction
        self.integrated_time = integrated_time
        self.ess_low = float(ess_low)
        self._mu, self._cov = unpack(chain.reshape(-1, chain.shape[-1]), self.d)

    @staticmethod
    def _cen(v, percentile):
        lo, hi = 50.0 - 0.5 * percentile, 50.0 + 0.5 * percentile
        m = v.mean(axis=0)
        return np.stack([m, np.percentile(v, hi, axis=0) - m, m - np.percentile(v, lo, axis=0)], axis=-1)

    def mu_cen(self, percentile=68.3):
        """[d, 3]: [mean, upper - mean, mean - lower] of each population mean."""
        return self._cen(self._mu, percentile)

    def sigma_cen(self, percentile=68.3):
        """[d, 3] of each population standard deviation sqrt(Sigma_ii)."""
        return self._cen(np.sqrt(np.einsum("hii->hi", self._cov)), percentile)

    def corr_cen(self, percentile=68.3):
        """[d, d, 3] of the population correlations."""
        sig = np.sqrt(np.einsum("hii->hi", self._cov))
        return self._cen(self._cov / (sig[:, :, None] * sig[:, None, :]), percentile)

    @property
    def best(self):
        """(mu, Sigma, lnprob) of the kept step of largest lnprob."""
        k = int(np.argmax(self.lnprob))
        mu, cov = unpack(self.chain.reshape(-1, self.chain.shape[-1])[k], self.d)
        return mu, cov, float(self.lnprob.ravel()[k])
