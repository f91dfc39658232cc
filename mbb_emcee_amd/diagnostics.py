"""Chain convergence diagnostics computed where the chain is (mbb_diag.hip.h): integrated autocorrelation time
with Sokal's automatic window, effective sample size, split R-hat across walkers.

What the reference's fit driver prints after a fit is ``sampler.acor`` (mbb_fit.py:548-561); here the same
number, and what emcee's users expect beside it, comes per source and per parameter of a catalogue fit without
the chain leaving the device.
"""
import ctypes as C

import numpy as np

from . import _analysis, _native

__all__ = ["chain_diagnostics", "ChainDiagnostics"]

METHODS = {"mean": _native.DIAG_MEAN, "walkers": _native.DIAG_WALKERS}
PARAM_NAMES = ("T", "beta", "lambda0", "alpha", "fnorm")


class _Request(_analysis.Window):
    """What one native diagnostics call is asked for (mbb_diag_spec); everything is checked here, before the
    device is touched."""

    def __init__(self, burn=0, c=5.0, tol=50.0, method="mean", nacf=0):
        if method not in METHODS:
            raise ValueError("method must be 'mean' or 'walkers'")
        self.method = method
        self.burn, self.nacf = int(burn), int(nacf)
        self.c, self.tol = float(c), float(tol)
        if self.burn < 0:
            raise ValueError("burn must not be negative")
        if not (self.c > 0.0 and np.isfinite(self.c)):
            raise ValueError("c must be positive")
        if not (self.tol >= 0.0 and np.isfinite(self.tol)):
            raise ValueError("tol must not be negative")
        if self.nacf < 0:
            raise ValueError("nacf must not be negative")

    def check_steps(self, nsteps):
        n = _analysis.Window.check_steps(self, nsteps)        # (no thin: every step from burn on)
        if n > _native.DIAG_MAX_STEPS:
            raise ValueError("more than %d kept steps per series: raise burn" % _native.DIAG_MAX_STEPS)
        if self.nacf > n:
            raise ValueError("nacf must be at most the number of kept steps")
        return n

    def spec(self):
        return _native.DiagSpec(self.burn, METHODS[self.method], self.nacf, self.c, self.tol)


class _Raw(object):
    """The arrays of one native diagnostics call (mbb_diag_out), nsrc leading."""

    def __init__(self, nsrc, nacf):
        self.tau = np.empty((nsrc, 5)); self.ess = np.empty((nsrc, 5)); self.rhat = np.empty((nsrc, 5))
        self.window = np.empty((nsrc, 5), dtype=np.int32)
        self.status = np.empty((nsrc, 5), dtype=np.int32)
        self.acf = np.empty((nsrc, 5, nacf)) if nacf else None

    def out(self):
        return _analysis.bind_out(_native.DiagOut, vars(self))          # (acf: None, and a null field, when not asked for)


class ChainDiagnostics(object):
    """Convergence of a chain, per parameter (a leading source axis for a multi-source chain):

    tau : integrated autocorrelation time in steps, and ``window`` the lag M it was summed to;
    ess : effective sample size, nwalkers * nsteps_used / tau;
    rhat : split R-hat across walkers;
    status : bits SHORT (fewer than 8 steps), CONSTANT (a fixed parameter), HAS_NAN, UNRELIABLE (the chain is
        shorter than tol * tau, emcee's warning);
    converged : tau is known and the chain is at least tol * tau long (status 0);
    acf : the first ``nacf`` values of the autocorrelation function, or None."""

    SHORT, CONSTANT, HAS_NAN, UNRELIABLE = (_native.DIAG_SHORT, _native.DIAG_CONSTANT, _native.DIAG_HAS_NAN,
                                            _native.DIAG_UNRELIABLE)

    def __init__(self, request, raw, multi, nwalkers, nsteps_used):
        pick = (lambda a: a) if multi else (lambda a: a[0])
        self.method, self.burn, self.c, self.tol = request.method, request.burn, request.c, request.tol
        self.tau, self.ess, self.rhat = pick(raw.tau), pick(raw.ess), pick(raw.rhat)
        self.window, self.status = pick(raw.window), pick(raw.status)
        self.acf = None if raw.acf is None else pick(raw.acf)
        self.converged = self.status == 0
        self.nwalkers, self.nsteps_used = int(nwalkers), int(nsteps_used)
        self._multi = multi

    def arrays(self):
        """The results as a dict of arrays, keys ``convergence_*`` (what run_mbb_emcee --convergence saves)."""
        return dict(convergence_tau=self.tau, convergence_window=self.window, convergence_ess=self.ess,
                    convergence_rhat=self.rhat, convergence_status=self.status, convergence_converged=self.converged)

    def __str__(self):
        """One line per parameter; the first source of a multi-source result."""
        first = (lambda a: a[0]) if self._multi else (lambda a: a)
        tau, ess, rhat, win, st = (first(a) for a in (self.tau, self.ess, self.rhat, self.window, self.status))
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(self.tau.shape[0]))
        lines.append("Convergence over {:d} steps of {:d} walkers (method '{:s}')".format(
            self.nsteps_used, self.nwalkers, self.method))
        for i, name in enumerate(PARAM_NAMES):
            notes = [txt for bit, txt in ((self.SHORT, "too short"), (self.CONSTANT, "fixed"),
                                          (self.HAS_NAN, "holds a NaN"),
                                          (self.UNRELIABLE, "chain shorter than {:g} tau".format(self.tol)))
                     if st[i] & bit]
            lines.append("  {:8s} tau: {:8.2f} (window {:d})  ESS: {:10.1f}  R-hat: {:7.4f}{:s}".format(
                name, tau[i], int(win[i]), ess[i], rhat[i], "  [" + "; ".join(notes) + "]" if notes else ""))
        return "\n".join(lines)


def chain_diagnostics(like, chain, burn=0, c=5.0, tol=50.0, method="mean", nacf=0):
    """Convergence diagnostics of a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) over the steps
    ``chain[:, burn:]``, computed on ``like``'s device.

    method : "mean", the autocorrelation time of the ensemble-mean series (what
        ``DeviceEnsembleSampler.get_autocorr_time`` gives), or "walkers", every walker's own autocorrelation
        function averaged over walkers and windowed once (emcee 3's estimator, of lower variance on short, wide
        chains);
    c : Sokal's window factor; tol : the chain is flagged UNRELIABLE below tol * tau steps;
    nacf : how many values of the autocorrelation function to return."""
    req = _Request(burn, c, tol, method, nacf)
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    n = req.check_steps(nsteps)
    ctx = _native.analysis_context(like, model=False)
    raw = _Raw(nsrc, req.nacf)
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_diagnostics(ctx.h, _native._d(c4), nsrc, nw, nsteps, C.byref(spec),
                                                    C.byref(out)), ctx)
    return ChainDiagnostics(req, raw, multi, nw, n)
