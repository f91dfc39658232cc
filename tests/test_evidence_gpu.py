"""GPU side of the evidence tests: the kernels of csrc/mbb_evidence.hip.h through ``evidence.chain_evidence``, the sampler,
the fitter and the CLI, against the fixture tests/golden/evidence.npz (exact ln Z of three cases), the longdouble reference
of tests/_evidence_ref.py and the package's own ``like()``.

Shapes are the smallest at which the kernels can still go wrong: 8 walkers x 64 steps (two 32-step halves: 256 posterior
samples, one workgroup's width), 7 walkers x 65 kept steps (nothing a multiple of the wave or the workgroup), windows of 2
and 3 kept steps, and one call of 3 x 100 000 draws whose slab seam (2^18 rows) falls inside a source."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity_record
import _evidence_ref as ER

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = 2.0 ** -53
TOL = 1e-10


@pytest.fixture(scope="module")
def g_ev():
    return np.load(os.path.join(GOLDEN, "evidence.npz"))


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


_LIKE = {}


def like_of(g_ev, case, scale=1.0, lowlim_T=None):
    key = (case, scale, lowlim_T)
    if key not in _LIKE:
        _LIKE[key] = ER.device_like(g_ev, case, scale, lowlim_T)
    return _LIKE[key]


def gauss_chain(g_ev, like, nw, nsteps, seed, free=(0, 4), nsrc=None, scale=1.0, spread=1.0):
    """A synthetic chain of independent Gaussian draws about the posterior of case (b) (T, fnorm), the other columns at
    THETA0, with lnprob from like(): [nw, nsteps, 5], [nw, nsteps]"""
    rng = np.random.RandomState(seed)
    chain = np.empty((nw, nsteps, 5)); chain[:] = ER.THETA0
    chain[..., 4] = scale * ER.THETA0[4]
    if 0 in free:
        chain[..., 0] = g_ev["b/mean"][0] + spread * g_ev["b/sigma"][0] * rng.normal(size=(nw, nsteps))
    if 4 in free:
        chain[..., 4] = scale * (g_ev["b/mean"][1] + spread * g_ev["b/sigma"][1] * rng.normal(size=(nw, nsteps)))
    return chain, like(chain.reshape(-1, 5)).reshape(nw, nsteps)


def replay(ev, lnprob, burn=0, thin=1, src=None, kind="case"):
    """Test 2: the longdouble reference iteration on the device's own prop_lnprob, prop_lnq, post_lnq and the chain's
    lnprob, stopped at 1e-15; |d lnz| <= tol / (1 - c) + 1e-12 with c the contraction the replay itself observes."""
    pick = (lambda a: a) if src is None else (lambda a: a[src])
    _, post = ER.window(lnprob.shape[-1], burn, thin)
    l1 = lnprob[:, post].reshape(-1) - pick(ev.posterior_lnq).astype(LD)
    with np.errstate(invalid="ignore"):
        l2 = pick(ev.proposal_lnprob).astype(LD) - pick(ev.proposal_lnq).astype(LD)
    r = ER.ref_bridge(l1, l2, neff=float(np.atleast_1d(ev.neff)[src or 0]))
    bound = TOL / (1 - r["contraction"]) + 1e-12
    dz, de = abs(float(pick(ev.lnz)) - r["lnz"]), abs(float(pick(ev.lnz_err)) - r["err"]) / r["err"]
    print("%s replay: d lnz %.2e (bound %.2e, contraction %.3f), d err %.2e relative, %d device / %d reference iterations"
          % (kind, dz, bound, r["contraction"], de, int(pick(ev.niter)), r["niter"]))
    parity_record("evidence replay |d lnz|", dz, bound)
    parity_record("evidence replay error estimate, relative", de, 1e-8)
    assert r["contraction"] < 1 and dz <= bound
    # the error estimate: sums of at most 1e5 terms of one sign and a two-pass variance, at rho within tol of the fixed point
    assert de <= 1e-8
    return r


# ---------------------------------------------------------------- 1. the exact 1-D case, 2. its replay
def test_exact_gaussian_case(mbb, g_ev):
    like = like_of(g_ev, "a")
    rng = np.random.RandomState(1)
    chain = np.empty((8, 64, 5)); chain[:] = ER.THETA0
    chain[..., 4] = float(g_ev["a/mean"]) + float(g_ev["a/sigma"]) * rng.normal(size=(8, 64))
    lp = like(chain.reshape(-1, 5)).reshape(8, 64)
    ev = mbb.chain_evidence(like, chain, lp, n2=256, fixed=ER.FIXED["a"], neff=None, keep=True)
    exact = float(g_ev["a/lnz"])
    print("case (a): lnz %.5f +- %.5f, exact %.5f (%.2f errors), %d iterations, status %s"
          % (ev.lnz, ev.lnz_err, exact, abs(ev.lnz - exact) / ev.lnz_err, ev.niter, ev.status_names()))
    assert abs(ev.lnz - exact) <= 5 * ev.lnz_err and ev.lnz_err <= 0.05
    assert ev.status == ER.CONVERGED | (0b01111 << ER.HELD_SHIFT) and ev.n1 == 256 and ev.n2 == 256 and ev.n_inside == 256
    assert np.all(ev.proposal[:, :4] == ER.THETA0[:4])                  # held parameters: their value bit for bit
    assert np.isnan(ev.proposal_cov[:4]).all() and np.isnan(ev.proposal_cov[:, :4]).all() and ev.proposal_cov[4, 4] > 0
    assert np.array_equal(ev.proposal_mean[:4], ER.THETA0[:4])
    replay(ev, lp, kind="case (a)")
    # declared or not, a constant column is held: the same bits
    ev2 = mbb.chain_evidence(like, chain, lp, n2=256, neff=None)
    assert ev2.lnz == ev.lnz and ev2.lnz_err == ev.lnz_err and ev2.status == ev.status


# ---------------------------------------------------------------- 3. case (b) through the device sampler; 4. case (c)
_RUN = {}


def sampler_run(mbb, g_ev, case):
    if case not in _RUN:
        like = like_of(g_ev, case)
        s = mbb.DeviceEnsembleSampler(32, 5, like, seed=17)
        rng = np.random.RandomState(4)
        p0 = np.empty((32, 5)); p0[:] = ER.THETA0
        p0[:, [0, 4]] = g_ev["b/mean"] + 0.5 * g_ev["b/sigma"] * np.abs(rng.normal(size=(32, 2)))
        s.run_mcmc(p0, 600, evidence=dict(burn=200, neff="auto", keep=True, fixed=ER.FIXED[case]))
        _RUN[case] = (like, s)
    return _RUN[case]


@pytest.mark.parametrize("case", ["b", "c"])
def test_cases_through_the_device_sampler(mbb, g_ev, case):
    like, s = sampler_run(mbb, g_ev, case)
    ev = s.evidence_
    truth = float(g_ev[case + "/lnz"])
    print("case (%s): lnz %.4f +- %.4f, truth %.4f (%.2f errors), neff %.0f of %d, %d of %d draws inside, %d iterations"
          % (case, ev.lnz, ev.lnz_err, truth, abs(ev.lnz - truth) / ev.lnz_err, ev.neff, ev.n1, ev.n_inside, ev.n2, ev.niter))
    assert ev.status & ER.CONVERGED and abs(ev.lnz - truth) <= 5 * ev.lnz_err and ev.lnz_err <= 0.1
    assert ev.n1 == 32 * 200 and ev.n2 == 32 * 200 and 1 <= ev.neff <= ev.n1
    assert list(ev.held) == [False, True, True, True, False]
    replay(ev, s.lnprobability, burn=200, kind="case (%s)" % case)
    inside = ev.proposal[:, 0] >= like.lowlim(0)
    assert ev.n_inside == inside.sum() and np.all(np.isneginf(ev.proposal_lnprob[~inside]))
    assert np.all(np.isfinite(ev.proposal_lnprob[inside]))
    if case == "c":
        assert 0 < (~inside).sum() < ev.n2
    else:
        assert inside.all()
    # the resident chain and the brought-back chain: the same bits
    host = mbb.chain_evidence(like, s.chain, s.lnprobability, burn=200, neff=ev.neff, seed=s.seed, keep=True,
                              fixed=ER.FIXED[case])
    for k, v in host.arrays().items():
        assert np.array_equal(v, ev.arrays()[k], equal_nan=True), k
    assert np.array_equal(host.proposal, ev.proposal) and np.array_equal(host.posterior_lnq, ev.posterior_lnq)
    auto = mbb.chain_evidence(like, s.chain, s.lnprobability, burn=200, seed=s.seed, fixed=ER.FIXED[case])
    assert abs(auto.neff - ev.neff) <= 1e-9 * ev.neff


# ---------------------------------------------------------------- 5. the proposal rows
def test_proposal_rows(mbb, g_ev):
    like = like_of(g_ev, "b")
    chain, lp = gauss_chain(g_ev, like, 8, 64, seed=5)
    seed, first = 0x1234567890abcdef, 3
    ev = mbb.chain_evidence(like, chain, lp, n2=48, neff=None, keep=True, seed=seed, first_source=first)
    free = [0, 4]
    mu, cov = ev.proposal_mean, ev.proposal_cov
    Lf = ER.chol(cov, free)
    L5 = np.zeros((5, 5), dtype=LD)
    L5[np.ix_(free, free)] = Lf
    ref, zs = ER.draws(seed, first, 48, mu, L5, free, ER.THETA0)
    assert np.all(ev.proposal[:, [1, 2, 3]] == ER.THETA0[[1, 2, 3]])
    worst = 0.0
    for i in free:
        bound = ER.PPND_MEASURED_ABS * np.abs(L5[i]).sum() + 4 * np.spacing(np.abs(ref[:, i].astype(np.float64)))
        err = np.abs(ev.proposal[:, i].astype(LD) - ref[:, i]).astype(np.float64)
        worst = max(worst, float((err / bound).max()))
        parity_record("evidence proposal row / bound", float((err / bound).max()), 1.0)
        assert np.all(err <= bound), (i, err.max(), bound.min())
    print("proposal rows: worst error %.3f of the bound; |z| up to %.2f" % (worst, float(np.abs(zs[:, free]).max())))
    # lnprob of the rows: like()'s, bit for bit
    assert np.array_equal(ev.proposal_lnprob, like(ev.proposal))
    # lnq at the draws and at the posterior samples against longdouble, from the reported mean and covariance
    _, post = ER.window(64)
    for name, got, rows in (("prop_lnq", ev.proposal_lnq, ev.proposal), ("post_lnq", ev.posterior_lnq, chain[:, post].reshape(-1, 5))):
        want = ER.lnq(rows, mu, Lf, free)
        f64 = ER.lnq(rows, mu, ER.chol(cov, free, np.float64), free, np.float64)
        margin = np.maximum(16 * np.abs(f64 - want).astype(np.float64), 1e-13 * np.maximum(1.0, np.abs(f64)))
        err = np.abs(got - want).astype(np.float64)
        print("%s: worst %.2e, %.3f of its margin" % (name, err.max(), (err / margin).max()))
        parity_record("evidence %s / margin" % name, float((err / margin).max()), 1.0)
        assert np.all(err <= margin)


# ---------------------------------------------------------------- 6. the proposal moments
@pytest.mark.parametrize("nsteps,burn,thin", [(65, 0, 1), (140, 10, 2), (2, 0, 1), (3, 0, 1), (40, 37, 1), (9, 0, 4)])
def test_proposal_moments(mbb, g_ev, nsteps, burn, thin):
    like = like_of(g_ev, "b")
    chain, lp = gauss_chain(g_ev, like, 7, nsteps, seed=nsteps)
    ev = mbb.chain_evidence(like, chain, lp, n2=8, neff=None, burn=burn, thin=thin, keep=True)
    fit, post = ER.window(nsteps, burn, thin)
    assert ev.n1 == 7 * len(post) and ev.posterior_lnq.shape == (7 * len(post),)
    mu, cov = ER.moments(chain, burn, thin)
    mu64, cov64 = ER.moments64(chain, burn, thin)
    free = [0, 4]
    m_margin = np.maximum(16 * np.abs(mu64 - mu).astype(np.float64), 1e-13 * np.maximum(1.0, np.abs(mu64)))
    err = np.abs(ev.proposal_mean[free] - mu[free]).astype(np.float64)
    parity_record("evidence proposal mean / margin", float((err / m_margin[free]).max()), 1.0)
    assert np.all(err <= m_margin[free])
    assert np.array_equal(ev.proposal_mean[[1, 2, 3]], ER.THETA0[[1, 2, 3]])
    if len(fit) * 7 < 2:
        return
    sd = np.sqrt(np.diag(cov64)[free])
    c_margin = np.maximum(16 * np.abs(cov64 - cov).astype(np.float64)[np.ix_(free, free)], 1e-13 * np.outer(sd, sd))
    cerr = np.abs(ev.proposal_cov[np.ix_(free, free)] - cov[np.ix_(free, free)]).astype(np.float64)
    print("moments over %d fit samples: mean %.2e, covariance %.3f of its margin" % (7 * len(fit), err.max(), (cerr / c_margin).max()))
    parity_record("evidence proposal covariance / margin", float((cerr / c_margin).max()), 1.0)
    assert np.all(cerr <= c_margin)
    assert np.array_equal(ev.proposal_cov, ev.proposal_cov.T, equal_nan=True)
    # lnq at the posterior samples is of THIS window's cells
    want = ER.lnq(chain[:, post].reshape(-1, 5), ev.proposal_mean, ER.chol(ev.proposal_cov, free), free)
    assert np.all(np.abs(ev.posterior_lnq - want) <= 1e-9 * np.maximum(1.0, np.abs(want.astype(np.float64))))


# ---------------------------------------------------------------- 7. sources of different scales, the slab seam
def _three_sources(mbb, g_ev):
    scales = (1.0, 10.0, 0.1)
    multi = mbb.likelihood(response=False, opthin=True, noalpha=True, device=0)
    multi.set_phot_multi(ER.WAVES, np.array([s * g_ev["flux"] for s in scales]), np.array([s * g_ev["unc"] for s in scales]))
    ones = [like_of(g_ev, "b", s) for s in scales]
    chains, lps = zip(*[gauss_chain(g_ev, ones[i], 8, 64, seed=20 + i, scale=s) for i, s in enumerate(scales)])
    return multi, ones, np.array(chains), np.array(lps)


def _same(a, b, src):
    for k, v in a.arrays().items():
        w = b.arrays()[k]
        if np.ndim(v) == 0 or k.endswith("improper"):
            continue
        assert np.array_equal(v[src], w, equal_nan=True), (k, src)
    for name in ("proposal", "proposal_lnprob", "proposal_lnq", "posterior_lnq"):
        assert np.array_equal(getattr(a, name)[src], getattr(b, name), equal_nan=True), (name, src)


def test_three_sources_and_the_slab_seam(mbb, g_ev):
    multi, ones, chains, lps = _three_sources(mbb, g_ev)
    neff = np.array([200.0, 100.0, 256.0])
    big = mbb.chain_evidence(multi, chains, lps, n2=100000, neff=neff, seed=9, keep=True)
    assert big.lnz.shape == (3,) and np.all(big.status & ER.CONVERGED) and np.all(np.isfinite(big.lnz))
    # the data scaled by s: fnorm scales, T does not; Z scales by s, its chi-square term is unchanged
    assert abs(big.lnz[1] - big.lnz[0] - np.log(10.0)) < 0.1 and abs(big.lnz[2] - big.lnz[0] + np.log(10.0)) < 0.1
    # a smaller call after a larger one: its draws are the first of the larger call's, bit for bit
    small = mbb.chain_evidence(multi, chains, lps, n2=1000, neff=neff, seed=9, keep=True)
    assert np.array_equal(small.proposal, big.proposal[:, :1000])
    assert np.array_equal(small.proposal_lnprob, big.proposal_lnprob[:, :1000])
    assert np.array_equal(small.proposal_lnq, big.proposal_lnq[:, :1000])
    assert np.array_equal(small.posterior_lnq, big.posterior_lnq)
    # across the seam the rows are still like()'s
    seam = (1 << 18) // 3
    rows = big.proposal[:, seam - 2:seam + 2]
    assert np.array_equal(big.proposal_lnprob[:, seam - 2:seam + 2], multi(rows.reshape(-1, 5)).reshape(3, 4))
    for g in range(3):
        alone = mbb.chain_evidence(ones[g], chains[g], lps[g], n2=1000, neff=neff[g], seed=9, keep=True, first_source=g)
        _same(small, alone, g)
        replay(small, lps[g], src=g, kind="source %d" % g)
    alone = mbb.chain_evidence(ones[1], chains[1], lps[1], n2=100000, neff=neff[1], seed=9, keep=True, first_source=1)
    _same(big, alone, 1)


# ---------------------------------------------------------------- 8. held parameters and the status bits
def _thick_like(mbb, g_ev):
    if "thick" not in _LIKE:
        like = mbb.likelihood(response=False, opthin=False, noalpha=False, device=0)
        waves = np.array([70.0, 100.0, 160.0, 250.0, 350.0, 500.0, 850.0])
        one = mbb.likelihood(response=False, opthin=False, noalpha=False, device=0)
        one.set_phot(waves, np.ones(7), np.ones(7))
        flux = one.model_flux(ER.THETA0)[0]
        like.set_phot(waves, flux, 0.05 * flux + 0.5)
        _LIKE["thick"] = like
    return _LIKE["thick"]


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5])
def test_one_to_five_free_parameters(mbb, g_ev, d):
    like = _thick_like(mbb, g_ev)
    rng = np.random.RandomState(30 + d)
    order = [4, 0, 1, 2, 3][:d]
    chain = np.empty((8, 64, 5)); chain[:] = ER.THETA0
    for k in order:
        chain[..., k] = ER.THETA0[k] * (1 + 0.01 * rng.normal(size=(8, 64)))
    lp = like(chain.reshape(-1, 5)).reshape(8, 64)
    ev = mbb.chain_evidence(like, chain, lp, n2=512, neff=None, keep=True)
    assert list(ev.held) == [k not in order for k in range(5)]
    assert ev.status & (ER.CONVERGED | ER.MAXITER) and np.isfinite(ev.lnz) and ev.lnz_err > 0
    fin = np.isfinite(ev.proposal_cov)
    assert np.array_equal(fin, np.outer(~ev.held, ~ev.held))
    assert np.array_equal(ev.proposal_lnprob, like(ev.proposal))
    replay(ev, lp, kind="%d free" % d)
    # declared fixed: the same result and the same held bits
    ev2 = mbb.chain_evidence(like, chain, lp, n2=512, neff=None, fixed=[k not in order for k in range(5)])
    assert ev2.lnz == ev.lnz and ev2.lnz_err == ev.lnz_err and ev2.status == ev.status


def test_status_bits(mbb, g_ev):
    like = like_of(g_ev, "b")
    chain, lp = gauss_chain(g_ev, like, 8, 64, seed=40)
    # all held
    const = np.empty((8, 64, 5)); const[:] = ER.THETA0
    lpc = like(const.reshape(-1, 5)).reshape(8, 64)
    lpc[0, 3] = -7.25
    ev = mbb.chain_evidence(like, const, lpc, n2=16, neff=None, burn=3)
    assert ev.status == ER.ALL_HELD | (31 << ER.HELD_SHIFT) and ev.lnz == -7.25 and ev.lnz_err == 0.0 and ev.niter == 0
    ev = mbb.chain_evidence(like, chain, lp, n2=16, neff=None, fixed=[1, 1, 1, 1, 1])
    assert ev.status & ER.ALL_HELD and ev.lnz == lp[0, 0]
    # two identical columns
    twin = chain.copy(); twin[..., 1] = twin[..., 0]
    ev = mbb.chain_evidence(like, twin, lp, n2=16, neff=None)
    assert ev.status & ER.COV_SINGULAR and not ev.status & (ER.CONVERGED | ER.MAXITER)
    assert np.isnan(ev.lnz) and np.isnan(ev.lnz_err) and ev.niter == 0
    # cells of the window without a finite lnprob
    holes = lp.copy()
    holes[0, 40], holes[3, 63], holes[7, 32], holes[2, 5] = np.nan, -np.inf, np.inf, np.nan      # (the last: in the fit half)
    ev = mbb.chain_evidence(like, chain, holes, n2=256, neff=None, keep=True)
    assert ev.status & ER.POST_LEFT_OUT and ev.n1 == np.isfinite(holes[:, 32:]).sum() == 253 and np.isfinite(ev.lnz)
    full = mbb.chain_evidence(like, chain, lp, n2=256, neff=None)
    assert not full.status & ER.POST_LEFT_OUT and full.n1 == 256 and abs(full.lnz - ev.lnz) < 0.05
    replay(ev, holes, kind="holes")
    # a proposal entirely below a limit
    walled = like_of(g_ev, "b", 1.0, 100.0)
    ev = mbb.chain_evidence(walled, chain, lp, n2=64, neff=None, keep=True)
    assert ev.status & ER.NO_OVERLAP and ev.n_inside == 0 and np.isnan(ev.lnz) and np.all(np.isneginf(ev.proposal_lnprob))
    # the iteration limit
    ev = mbb.chain_evidence(like, chain, lp, n2=256, neff=None, maxiter=1, tol=0.0)
    assert ev.status & ER.MAXITER and not ev.status & ER.CONVERGED and ev.niter == 1 and np.isfinite(ev.lnz)


# ---------------------------------------------------------------- 9. the resident chain: sampler, fitter, CLI; the C-ABI
def test_other_analyses_are_unchanged(mbb, g_ev):
    like = like_of(g_ev, "b")
    rng = np.random.RandomState(6)
    p0 = np.empty((16, 5)); p0[:] = ER.THETA0
    p0[:, [0, 4]] = g_ev["b/mean"] + 0.5 * g_ev["b/sigma"] * rng.normal(size=(16, 2))
    kw = dict(summary=True, convergence=True, marginals=True, predict=[250.0], draws=10, goodness=True)
    runs = []
    for extra in ({}, dict(evidence=dict(n2=300, neff=None))):
        s = mbb.DeviceEnsembleSampler(16, 5, like, seed=23)
        s.run_mcmc(p0, 48, **kw, **extra)
        runs.append(s)
    a, b = runs
    assert a.evidence_ is None and b.evidence_ is not None and np.isfinite(b.evidence_.lnz)
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.lnprobability, b.lnprobability)
    for name in ("summary", "convergence_", "marginals_", "predictions_", "draws_", "goodness_"):
        x, y = getattr(a, name).arrays(), getattr(b, name).arrays()
        assert set(x) == set(y)
        for k in x:
            u, v = np.asarray(x[k]), np.asarray(y[k])
            assert np.array_equal(u, v, equal_nan=u.dtype.kind in "fc"), (name, k)
    host = mbb.chain_evidence(like, b.chain, b.lnprobability, n2=300, neff=None, seed=b.seed)
    for k, v in host.arrays().items():
        assert np.array_equal(v, b.evidence_.arrays()[k], equal_nan=True), k
    # on demand, later, with another window
    later = b.evidence(burn=8, thin=2, n2=100, neff=50.0)
    host = mbb.chain_evidence(like, b.chain, b.lnprobability, burn=8, thin=2, n2=100, neff=50.0, seed=b.seed)
    assert later.lnz == host.lnz and later.lnz_err == host.lnz_err and later.neff == 50.0
    b.reset()
    assert b.evidence_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.evidence()


def test_fitter_and_cli_evidence(mbb, g_ev, tmp_path, capsys):
    from mbb_emcee_amd import run_mbb_emcee
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for w, f, u in zip(ER.WAVES, g_ev["flux"], g_ev["unc"]):
            fh.write("%.1f %.10g %.10g\n" % (w, f, u))
    fit = mbb.mbb_fitter(nwalkers=16, photfile=str(pf), opthin=True, noalpha=True, seed=3)
    fit.fix_param("beta")
    p0 = fit.generate_initial_values(ER.THETA0, np.array([0.2, 0.0, 0.0, 0.0, 1.5]))
    fit.run(20, 64, p0, evidence=True)
    ev = fit.evidence
    assert ev is not None and list(ev.held) == [False, True, True, True, False] and ev.status & ER.CONVERGED
    host = mbb.chain_evidence(fit.like, fit.sampler.chain, fit.sampler.lnprobability, neff=ev.neff, seed=fit.sampler.seed,
                              fixed=[0, 1, 0, 0, 0])
    assert host.lnz == ev.lnz and host.lnz_err == ev.lnz_err
    fit.run(20, 16, p0)
    assert fit.evidence is None
    capsys.readouterr()
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-n", "16", "-b", "20", "-N", "64", "--opthin", "--noalpha", "--fixBeta", "--initT", "12",
            "--initBeta", "1.8", "--seed", "5"]
    p = run_mbb_emcee.build_parser()
    if not hasattr(p.parse_args(args), "opthin"):
        pytest.fail("the CLI's switches changed")
    assert run_mbb_emcee.main(args + ["--evidence", "200"]) == 0
    text = capsys.readouterr().out
    assert "ln Z:" in text and "proposal draws: 200" in text
    got = np.load(out)
    assert {"evidence_lnz", "evidence_lnz_err", "evidence_status", "evidence_neff", "evidence_n2"} <= set(got.files)
    assert got["evidence_n2"] == 200 and np.isfinite(got["evidence_lnz"])
    like = mbb.likelihood(str(pf), opthin=True, noalpha=True)
    want = mbb.chain_evidence(like, got["chain"], got["lnprobability"], n2=200, neff=float(got["evidence_neff"]), seed=5,
                              fixed=[0, 1, 0, 0, 0])
    for k, v in want.arrays().items():
        assert np.array_equal(got[k], v, equal_nan=True), k
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == "" and not any(k.startswith("evidence_") for k in np.load(out).files)


def test_c_abi_refusals(mbb, g_ev):
    from mbb_emcee_amd import _native, evidence
    like = like_of(g_ev, "b")
    chain, lp = gauss_chain(g_ev, like, 8, 16, seed=50)
    ctx = _native.analysis_context(like)
    c4 = np.ascontiguousarray(chain[None])

    def call(edit=None, lnprob=lp, nsteps=16, out_edit=None, ctx=ctx):
        req = evidence._Request(like, 32)
        req.set_neff(None, 1)
        spec = req.spec()
        raw = evidence._Raw(1, 64, 32, False)
        out = raw.out()
        keep = []
        if edit:
            keep.append(edit(spec))
        if out_edit:
            out_edit(out)
        rc = ctx.lib.mbb_chain_evidence(ctx.h, _native._d(c4), None if lnprob is None else _native._d(lnprob), 1, 8, nsteps,
                                        C.byref(spec), C.byref(out))
        return rc, ctx.lib.mbb_last_error().decode(), raw

    rc, _, raw = call()
    assert rc == 0 and np.isfinite(raw.lnz[0])

    def setter(**kw):
        def edit(spec):
            hold = []
            for k, v in kw.items():
                if k == "neff":
                    v = np.array([v], dtype=np.float64)
                    hold.append(v)
                    spec.neff = _native._d(v)
                else:
                    setattr(spec, k, v)
            return hold
        return edit
    for kw, msg in ((dict(burn=15), "two kept steps"), (dict(thin=16), "two kept steps"), (dict(burn=16), "bad burn"),
                    (dict(thin=0), "bad burn"), (dict(n2=-1), "proposal draws"), (dict(n2=(1 << 22) + 1), "proposal draws"),
                    (dict(tol=-1.0), "tol must be"), (dict(tol=float("nan")), "tol must be"), (dict(tol=float("inf")), "tol must be"),
                    (dict(maxiter=0), "iterations"), (dict(maxiter=100001), "iterations"), (dict(neff=0.0), "neff must be"),
                    (dict(neff=float("nan")), "neff must be"), (dict(neff=float("inf")), "neff must be"),
                    (dict(neff=-3.0), "neff must be"), (dict(first_source=-1), "first_source")):
        rc, err, _ = call(setter(**kw))
        assert rc == -2 and msg in err, (kw, rc, err)
    assert call(lnprob=None)[0] == -2
    assert call(nsteps=0)[0] == -2

    def no_lnz(out):
        out.lnz = None
    assert call(out_edit=no_lnz)[0] == -2
    assert ctx.lib.mbb_chain_evidence(ctx.h, _native._d(c4), _native._d(lp), 1, 8, 16, None, None) == -2
    # a chain of two sources against... one set of data serves both; three against a context of two is refused
    multi = mbb.likelihood(response=False, opthin=True, noalpha=True, device=0)
    multi.set_phot_multi(ER.WAVES, np.array([g_ev["flux"]] * 2), np.array([g_ev["unc"]] * 2))
    mctx = _native.analysis_context(multi)
    rc, err, _ = call(ctx=mctx)
    assert rc == -2 and "sources" in err
    # neither bands nor data
    bare = _native.Context(0)
    rc, err, _ = call(ctx=bare)
    assert rc == -3 and "bands not set" in err
    bare.close()
    # no resident chain
    s = mbb.DeviceEnsembleSampler(16, 5, like, seed=1)
    sctx, h = s._handle()
    req = evidence._Request(like, 32)
    spec, out = req.spec(), evidence._Raw(1, 64, 32, False).out()
    assert sctx.lib.mbb_sampler_evidence(sctx.h, h, C.byref(spec), C.byref(out)) == -3
    assert "no chain of this sampler is resident" in sctx.lib.mbb_last_error().decode()
    assert sctx.lib.mbb_sampler_evidence(sctx.h, h, None, C.byref(out)) == -2
