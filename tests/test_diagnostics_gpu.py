"""Chain diagnostics on the GPU (csrc/mbb_diag.hip.h through mbb_chain_diagnostics / mbb_sampler_diagnostics and
mbb_emcee_amd/diagnostics.py) against the longdouble direct sums of tests/_diag_ref.py.

Bounds, derived, not measured (n kept steps, nw walkers, M the window, eps = 2^-52):
  * rho_k, k <= max(M, nacf - 1):  |rho_dev - rho_ref| <= 16 (log2(n nw) + 2) eps (1 + mean|x| / sigma).  A tree sum of n
    products errs by (log2 n + 2) eps c_0 at most (Cauchy-Schwarz); an error delta in the mean moves c_k by
    2 |delta| sqrt(n c_0) at most; 16 leaves 4x over both terms and over the division.  sigma is the standard deviation
    of the series that is autocorrelated: the ensemble-mean series for "mean", the worst walker for "walkers".
  * tau: 2 (M + 1) times the rho bound;  M: exactly the reference's (tests/test_diagnostics_cpu.py holds every chain
    here to a margin of 1e-3 in the window decision);  ESS: the tau bound, relative;
  * R-hat: relative error at most the rho bound with sigma = sqrt(W);  status bits: exact.
Every check goes through rec_allclose in units of its own bound, so that the observed maxima land in the parity report.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import rec_allclose
import _diag_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


@pytest.fixture(scope="module")
def like(mbb):
    return mbb.likelihood()


def _check(got, refs, label):
    """A ChainDiagnostics against the references of its sources."""
    multi = got.tau.ndim == 2
    for s, ref in enumerate(refs):
        pick = (lambda a: a[s]) if multi else (lambda a: a)
        tau, ess, rhat, win, st = (pick(a) for a in (got.tau, got.ess, got.rhat, got.window, got.status))
        acf = None if got.acf is None else pick(got.acf)
        assert np.array_equal(st, ref["status"]), (label, s, st, ref["status"])
        assert np.array_equal(win, ref["window"]), (label, s, win, ref["window"])
        assert np.array_equal(pick(got.converged), ref["status"] == 0)
        for p in range(5):
            known = not ref["status"][p] & (R.SHORT | R.CONSTANT | R.HAS_NAN)
            if known:
                rb, tb = ref["rho_bound"][p], ref["tau_bound"][p]
                print("    %s src %d par %d: M %d  tau err %.3g (bound %.3g)" % (label, s, p, win[p],
                                                                                  abs(tau[p] - ref["tau"][p]), tb))
                rec_allclose((tau[p] - ref["tau"][p]) / tb, 0.0, rtol=0, atol=1, kind="diag tau [its bound]")
                rel = tb / abs(ref["tau"][p])
                rec_allclose((ess[p] / ref["ess"][p] - 1.0) / (rel / (1.0 - rel)), 0.0, rtol=0, atol=1,
                             kind="diag ESS [its bound]")
                if acf is not None:
                    want = np.asarray(ref["rho"][p][:acf.shape[-1]], dtype=np.float64)
                    print("      rho err %.3g (bound %.3g)" % (np.abs(acf[p] - want).max(), rb))
                    rec_allclose((acf[p] - want) / rb, 0.0, rtol=0, atol=1, kind="diag rho [its bound]")
                    assert acf[p][0] == 1.0
            else:
                assert np.isnan(tau[p]) and np.isnan(ess[p])
                assert acf is None or np.all(np.isnan(acf[p]))
            if np.isfinite(ref["rhat"][p]):
                rec_allclose((rhat[p] / ref["rhat"][p] - 1.0) / ref["rhat_rbound"][p], 0.0, rtol=0, atol=1,
                             kind="diag R-hat [its bound]")
            else:
                assert np.isnan(rhat[p]), (label, p, rhat[p])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_chain_diagnostics_vs_direct_sums(mbb, like, name):
    """1. Every synthetic case of tests/_diag_ref.py, as a host array: n = 7 and 8, sizes that are no multiple of the
    thread count or the lag block, the seam chains (M the last lag of a lag block and the first of the next), the
    ramp (late exit, flagged), walker counts 1, 7, 10, 34 and 250, three sources, burn with n odd, a constant column,
    one constant walker, a NaN inside and outside the window, nacf beyond M, the longest series."""
    ch, kw = R.case_chain(name), R.CASES[name][1]
    got = mbb.chain_diagnostics(like, ch, **kw)
    assert (got.acf is None) == (kw.get("nacf", 0) == 0)
    assert got.nwalkers == ch.shape[-3] and got.nsteps_used == ch.shape[-2] - kw.get("burn", 0)
    _check(got, R.case_ref(name), name)
    again = mbb.chain_diagnostics(like, ch, **kw)
    for f in ("tau", "ess", "rhat", "window", "status"):
        assert np.array_equal(getattr(got, f), getattr(again, f), equal_nan=True), f       # the same bits every time
    assert str(got).count("tau:") == 5


def test_sources_do_not_leak(mbb, like):
    """2. A source of a multi-source chain gets bitwise what it gets alone."""
    ch = R.case_chain("nsrc3")
    for method in ("mean", "walkers"):
        all3 = mbb.chain_diagnostics(like, ch, method=method, nacf=32)
        assert all3.tau.shape == (3, 5) and all3.acf.shape == (3, 5, 32)
        for s in range(3):
            one = mbb.chain_diagnostics(like, ch[s], method=method, nacf=32)
            for f in ("tau", "ess", "rhat", "window", "status", "acf"):
                assert np.array_equal(getattr(all3, f)[s], getattr(one, f)), (method, s, f)


def test_native_argument_errors(mbb, like):
    """3. Bad arguments at the C-ABI: the argument error, with mbb_last_error set; a series longer than the limit is
    one of them, not a wrong answer."""
    from mbb_emcee_amd import _native, diagnostics
    ctx = like.context
    chain = np.ascontiguousarray(R.case_chain("n257"))
    raw = diagnostics._Raw(1, 4)
    out = raw.out()

    def call(spec, nsteps=257, o=out, ch=chain, nw=7):
        return ctx.lib.mbb_chain_diagnostics(ctx.h, _native._d(ch), 1, nw, nsteps, C.byref(spec), C.byref(o))
    assert call(_native.DiagSpec(0, 0, 4, 5.0, 50.0)) == 0
    for spec, msg in ((_native.DiagSpec(257, 0, 0, 5.0, 50.0), "burn"), (_native.DiagSpec(-1, 0, 0, 5.0, 50.0), "burn"),
                      (_native.DiagSpec(0, 2, 0, 5.0, 50.0), "method"), (_native.DiagSpec(0, 0, 258, 5.0, 50.0), "nacf"),
                      (_native.DiagSpec(0, 0, -1, 5.0, 50.0), "nacf"), (_native.DiagSpec(0, 0, 0, 0.0, 50.0), "c must"),
                      (_native.DiagSpec(0, 0, 0, 5.0, -1.0), "tol")):
        assert call(spec) == -2
        assert msg in ctx.lib.mbb_last_error().decode()
    other = diagnostics._Raw(1, 0)
    null = other.out()
    null.tau = None
    assert call(_native.DiagSpec(0, 0, 0, 5.0, 50.0), o=null) == -2
    long_chain = np.zeros((1, _native.DIAG_MAX_STEPS + 1, 5))
    assert call(_native.DiagSpec(0, 0, 0, 5.0, 50.0), nsteps=_native.DIAG_MAX_STEPS + 1, ch=long_chain, nw=1,
                o=other.out()) == -2
    assert "16384" in ctx.lib.mbb_last_error().decode()
    assert call(_native.DiagSpec(1, 0, 0, 5.0, 50.0), nsteps=_native.DIAG_MAX_STEPS + 1, ch=long_chain, nw=1,
                o=other.out()) == 0
    assert np.all(other.status == _native.DIAG_CONSTANT) and np.all(np.isnan(other.tau))
    # nacf > 0 with a null acf: the curve is simply not returned
    noacf = diagnostics._Raw(1, 0)
    assert call(_native.DiagSpec(0, 0, 4, 5.0, 50.0), o=noacf.out()) == 0
    assert np.array_equal(noacf.tau, raw.tau)


# ---------------------------------------------------------------- through the sampler
NW, NSTEPS = 34, 64


def _sampler_case(mbb, g_lnl, multi):
    """The golden 8-band photometry, one source or three."""
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rng = np.random.RandomState(11)
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    if multi:
        ns = 3
        truths = np.column_stack([rng.uniform(8, 20, ns), rng.uniform(1.2, 2.4, ns), rng.uniform(300, 900, ns),
                                  rng.uniform(2, 4.5, ns), rng.uniform(10, 80, ns)])
        flux = one.model_flux(truths)
        like = mbb.likelihood(response=True)
        like.set_phot_multi(bands, flux, 0.1 * flux + 1.0)
        p0 = truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, NW, 5)))
    else:
        truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
        flux = one.model_flux(truth)[0]
        like = mbb.likelihood(response=True)
        like.set_phot(bands, flux, 0.1 * flux + 1.0)
        p0 = truth * (1.0 + 0.02 * rng.normal(size=(NW, 5)))
    return like, p0


def _same_bits(a, b):
    if (a.acf is None) != (b.acf is None) or (a.acf is not None and not np.array_equal(a.acf, b.acf, equal_nan=True)):
        return False
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True)
               for f in ("tau", "ess", "rhat", "window", "status", "converged"))


@pytest.mark.parametrize("multi", [False, True])
def test_sampler_convergence_equals_diagnostics_of_stored_chain(mbb, g_lnl, multi):
    """4. A real run, 34 walkers x 64 steps: convergence() on the resident chain is bitwise chain_diagnostics of the
    chain the run returned; a run that stores nothing and summarises gives the same bits; twice the same call, the same
    bits; single-source, the "mean" tau is get_autocorr_time() to the tau bound."""
    like, p0 = _sampler_case(mbb, g_lnl, multi)
    a = mbb.DeviceEnsembleSampler(NW, 5, like, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.convergence_ is None
    for method in ("mean", "walkers"):
        kw = dict(burn=5, nacf=8, method=method)
        res = a.convergence(**kw)
        host = mbb.chain_diagnostics(like, a.chain, **kw)
        assert _same_bits(res, host) and _same_bits(res, a.convergence(**kw))
        assert res.tau.shape == ((3, 5) if multi else (5,)) and res.nsteps_used == NSTEPS - 5 and res.nwalkers == NW
        c4 = a.chain if multi else a.chain[None]
        refs = tuple(R.diagnostics_ref(c, **kw) for c in c4)
        for ref in refs:
            assert np.all(ref["margin"] >= 1e-3), ref["margin"]             # (a condition on the seed, as on the CPU)
        _check(res, refs, "sampler %s" % method)
        b = mbb.DeviceEnsembleSampler(NW, 5, like, seed=77)
        b.run_mcmc(p0, NSTEPS, storechain=False, summary=True, convergence=kw)
        assert b.chain.shape[-2] == 0 and b.summary is not None
        assert _same_bits(b.convergence_, res)
    if not multi:
        res, ref = a.convergence(), R.diagnostics_ref(a.chain)
        assert np.all(ref["margin"] >= 1e-3)
        rec_allclose((res.tau - a.get_autocorr_time()) / ref["tau_bound"], 0.0, rtol=0, atol=1,
                     kind="diag tau against get_autocorr_time [its bound]")
    # the refusals
    held = b.convergence_
    b.run_mcmc(None, 3, storechain=False)                   # the next run: nothing of it is resident
    assert b.convergence_ is None and held is not None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.convergence()
    b.run_mcmc(None, 3, convergence=False)                  # ... and this one overwrites the chain: three steps now
    assert b.convergence_ is None and b.convergence().nsteps_used == 3
    with pytest.raises(ValueError, match="burn leaves no step"):
        b.convergence(burn=5)
    b.run_mcmc(None, 9, convergence=True)
    assert b.convergence_.nsteps_used == 9
    b.reset()
    assert b.convergence_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.convergence()
    with pytest.raises(ValueError, match="needs summary= too"):
        b.run_mcmc(p0, 8, storechain=False, convergence=True)


def test_native_sampler_diagnostics_needs_a_resident_chain(mbb, g_lnl):
    """5. mbb_sampler_diagnostics on a sampler that has run nothing: MBB_ERR_STATE."""
    from mbb_emcee_amd import _native, diagnostics
    like, p0 = _sampler_case(mbb, g_lnl, False)
    s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=5)
    ctx, h = s._handle()
    raw = diagnostics._Raw(1, 0)
    spec, out = _native.DiagSpec(0, 0, 0, 5.0, 50.0), raw.out()
    assert ctx.lib.mbb_sampler_diagnostics(ctx.h, h, C.byref(spec), C.byref(out)) == -3
    assert "resident" in ctx.lib.mbb_last_error().decode()
    s.run_mcmc(p0, 8, storechain=False)
    assert ctx.lib.mbb_sampler_diagnostics(ctx.h, h, C.byref(spec), C.byref(out)) == -3
    s.run_mcmc(None, 8)
    assert ctx.lib.mbb_sampler_diagnostics(ctx.h, h, C.byref(spec), C.byref(out)) == 0
    assert ctx.lib.mbb_sampler_diagnostics(ctx.h, h, None, C.byref(out)) == -2


def test_fitter_and_cli_convergence(mbb, g_lnl, tmp_path, capsys):
    """6. mbb_fitter.run(..., convergence=True) and the CLI's --convergence end to end: the diagnostics are those of the
    chain the fit returns; without the flag nothing new is printed or written."""
    from mbb_emcee_amd import run_mbb_emcee
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    flux = one.model_flux(truth)[0]
    fit = mbb.mbb_fitter(nwalkers=NW, response=True, seed=3)
    fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    fit.run(20, NSTEPS, p0, convergence=dict(method="walkers"))
    d = fit.convergence
    assert d is not None and d.method == "walkers" and fit.summary is None
    assert _same_bits(d, mbb.chain_diagnostics(fit.like, fit.sampler.chain, method="walkers"))
    assert np.all(np.isfinite(d.tau)) and np.all(d.status == d.UNRELIABLE)      # 64 steps are fewer than 50 tau
    fit.run(20, 16, p0)
    assert fit.convergence is None                                       # the default leaves none
    capsys.readouterr()
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", str(NW), "-b", "20", "-N", str(NSTEPS), "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--convergence"]) == 0
    text = capsys.readouterr().out
    assert "Convergence over %d steps of %d walkers" % (NSTEPS, NW) in text and text.count("R-hat:") == 5
    got = np.load(out)
    keys_with = set(got.files)
    new = {"convergence_tau", "convergence_window", "convergence_ess", "convergence_rhat", "convergence_status",
           "convergence_converged"}
    assert new <= keys_with
    ref = R.diagnostics_ref(got["chain"])
    assert np.all(ref["margin"] >= 1e-3)
    assert np.array_equal(got["convergence_window"], ref["window"]) and got["convergence_tau"].shape == (5,)
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == ""
    assert keys_with - set(np.load(out).files) == new
