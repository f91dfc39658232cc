"""Chain summaries on the GPU (csrc/mbb_summary.hip.h through mbb_chain_summary / mbb_sampler_run_summary and
mbb_emcee_amd/results.py) against the reference's own mbb_results (tests/golden/summary.npz) and against numpy.

Tolerances, and where they come from:
  * percentiles, one-sided limits, min, max of a PARAMETER column: the order statistics are selected exactly and the
    interpolation is one multiply-add, so 4 ulp of the larger bracketing value;
  * means: a fixed-order tree sum and numpy's pairwise sum each err by about log2(n) eps mean|x|: 64 eps mean|x|
    (n <= 2^20 here);
  * derived columns: an order statistic moves by no more than the largest per-entry perturbation, so the relative
    tolerances test_postprocess_vs_reference_results holds the per-entry values to against the same fixture
    (peak wavelength 1e-10, L_IR 5e-7, dust mass 1e-13), relative to the column's largest magnitude;
  * n_used, best-fit index: exact; best-fit parameters and lnprob: the bits of the chain that went in.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, rec_allclose
import _summary_ref as SR

pytestmark = pytest.mark.gpu

EPS = SR.EPS
VARIANTS = [("thin_walpha", True, False), ("thick_walpha", False, False),
            ("thick_noalpha", False, True), ("thin_noalpha", True, True)]
DERIVED_RTOL = {"peaklambda": 1e-10, "lir": 5e-7, "dustmass": 1e-13}     # test_postprocess_vs_reference_results


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


@pytest.fixture(scope="module")
def g_sum():
    return np.load(os.path.join(GOLDEN, "summary.npz"))


def _check_column(got_mean, got_pct, got_min, got_max, col, qs, kind):
    """One unclipped or already-clipped column `col` (1-d, what numpy is given) against numpy."""
    srt = np.sort(col)
    scale = np.abs(col).mean()
    print("    %s: n %d mean err %.3g eps mean|x|" % (kind, col.size, abs(got_mean - col.mean()) / (EPS * scale) if scale else 0))
    rec_allclose((got_mean - col.mean()) / (EPS * scale if scale > 0 else 1.0), 0.0, rtol=0, atol=64,
                 kind="summary mean [eps mean|x|]")
    want = np.percentile(col, qs)
    for k, q in enumerate(qs):
        lo, hi = SR.bracket(srt, q)
        rec_allclose(SR.ulps_off(got_pct[k], want[k], lo, hi), 0.0, rtol=0, atol=4, kind="summary percentile [ulp]")
    assert got_min == col.min() and got_max == col.max()


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_summary_vs_reference_results(mbb, g_res, g_sum, name, opthin, noalpha):
    """1. mbb_chain_summary on each chain of results.npz against what the reference's mbb_results returned for it."""
    from mbb_emcee_amd import results
    k = name + "/"
    chain, lnp = g_res[k + "chain"], g_res[k + "lnprobability"]
    z, dl = float(g_res["redshift"]), float(g_res["lumdist_mpc"])
    like = mbb.likelihood(response=True, opthin=opthin, noalpha=noalpha)
    like.set_phot([str(b) for b in g_res["bands"]], g_res[k + "data_flux"], 0.1 * g_res[k + "data_flux"] + 1.0)
    cen, lim = [float(p) for p in g_sum["cen_percentiles"]], [float(p) for p in g_sum["lim_percentiles"]]
    s = results.chain_summary(like, chain, lnp, percentile=cen, derived=("peaklambda", "lir", "dustmass"), redshift=z,
                              lumdist_mpc=dl, peak_model="reference")
    assert np.array_equal(s.n_used, [512] * 8) and np.all(s.status == 0)
    qs, pct = s.percentiles
    for i in range(5):
        col = chain[:, :, i].flatten()
        _check_column(s.mean[i], pct[i], s.min[i], s.max[i], col, qs, "%s par %d" % (name, i))
        srt, scale = np.sort(col), np.abs(col).mean()
        for j, p in enumerate(cen):
            # par_cen = [mean, upper - mean, mean - lower] against the reference's: the percentile's 4 ulp, the mean's
            # 64 eps mean|x|, and half an ulp each for the two subtractions (the reference's and this one's)
            got, want = s.par_cen(i, percentile=p), g_sum[k + "par_cen"][i, j]
            rec_allclose((got[0] - want[0]) / (EPS * scale), 0.0, rtol=0, atol=64, kind="summary mean [eps mean|x|]")
            for c, q in ((1, 100 - 0.5 * (100 - p)), (2, 0.5 * (100 - p))):
                lo, hi = SR.bracket(srt, q)
                bound = 4 * np.spacing(max(abs(lo), abs(hi))) + 64 * EPS * scale + EPS * abs(want[c])
                rec_allclose((got[c] - want[c]) / bound, 0.0, rtol=0, atol=1, kind="par_cen half-width [its bound]")
        for j, p in enumerate(lim):
            for fn, q, key in ((s.par_lowlim, 100 - p, "par_lowlim"), (s.par_uplim, p, "par_uplim")):
                lo, hi = SR.bracket(srt, q)
                rec_allclose(SR.ulps_off(fn(i, percentile=p), g_sum[k + key][i, j], lo, hi), 0.0, rtol=0, atol=4,
                             kind="summary percentile [ulp]")
    # the clipped interval
    par = int(g_sum[k + "clip_param"])
    lo, hi = [None if np.isnan(b) else float(b) for b in g_sum[k + "clip_bounds"]]
    sc = results.chain_summary(like, chain, lnp, clip={par: (lo, hi)})
    assert sc.n_used[par] == int(g_sum[k + "clip_n_used"])
    col = chain[:, :, par].flatten()
    col = col[(col >= (-np.inf if lo is None else lo)) & (col <= (np.inf if hi is None else hi))]
    _check_column(sc.mean[par], sc.percentiles[1][par], sc.min[par], sc.max[par], col, sc.percentiles[0], name + " clipped")
    got, want = sc.par_cen(par, lowlim=lo, uplim=hi), g_sum[k + "clip_par_cen"]
    assert np.allclose(got, want, rtol=0, atol=64 * EPS * np.abs(col).mean() + 8 * np.spacing(np.abs(col).max()))
    assert np.array_equal(s.par_cen(par, lowlim=lo, uplim=hi), got)          # on demand from the kept chain: the same
    # derived columns
    for nm, fn, src in (("peaklambda", s.peaklambda_cen, "peaklambda"), ("lir", s.lir_cen, "lir"),
                        ("dustmass", s.dustmass_cen, "dustmass")):
        want, top = g_sum[k + nm + "_cen"], np.abs(g_res[k + src]).max()
        got = fn()
        print("    %s %s_cen: max err / column max %.3g (bound %g)" % (name, nm, np.abs(got - want).max() / top, DERIVED_RTOL[nm]))
        # (the fixture holds [mean, upper - mean, mean - lower]: mean, upper and lower are compared)
        got3 = np.array([got[0], got[0] + got[1], got[0] - got[2]])
        want3 = np.array([want[0], want[0] + want[1], want[0] - want[2]])
        rec_allclose((got3 - want3) / top, 0.0, rtol=0, atol=DERIVED_RTOL[nm], kind="summary %s [column max]" % nm)
    # best fit
    pars, val, idx = s.best_fit
    assert tuple(idx) == tuple(g_sum[k + "best_fit_index"])
    assert np.array_equal(pars, chain[idx]) and val == lnp[idx] and s.best_fit_chisq == -2.0 * lnp[idx]
    assert np.array_equal(pars, g_sum[k + "best_fit_params"])
    rec_allclose(val, float(g_sum[k + "best_fit_lnprob"]), rtol=1e-13, kind="best-fit lnprob as stored")
    sed = s.best_fit_sed(np.array([100.0, 500.0]))
    assert sed.shape == (2,) and np.all(sed > 0)
    text = str(s)
    assert "ChiSquare of best fit point" in text and "L_IR(8.0 to 1000.0um)" in text and "Lambda peak" in text


def test_summary_tie_rule(mbb, g_sum):
    """The best sample at three places of the chain: the first in [walker][step] order is returned, as the reference's."""
    from mbb_emcee_amd import results
    chain, lnp = g_sum["tiecase/chain"], g_sum["tiecase/lnprobability"]
    s = results.chain_summary(mbb.likelihood(), chain, lnp)
    pars, val, idx = s.best_fit
    assert tuple(idx) == tuple(g_sum["tiecase/best_fit_index"]) and np.array_equal(pars, g_sum["tiecase/best_fit_params"])
    assert val == float(g_sum["tiecase/best_fit_lnprob"])


def _mean_err(got, want, scale):
    """|got - want| in units of eps mean|x|.  Where the values are subnormal the format's own spacing, 2^-1074, is the
    floor of any rounding (each of the two means is the rounded quotient of a sum): two spacings are taken off first."""
    tiny = 2 * 4.9406564584124654e-324
    excess = np.maximum(np.abs(np.asarray(got) - np.asarray(want)) - tiny, 0.0)
    unit = EPS * np.asarray(scale)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(excess == 0, 0.0, excess / unit)


def _random_chain(nsrc, nw, nsteps, seed):
    """A chain with rejected-move repeats whose columns hold: positive values; +-0.0 and negatives; denormals; one value;
    large negative values.  lnprob repeats with the moves, so its maximum is tied."""
    rng = np.random.RandomState(seed)
    R = nsrc * nw
    chain = np.empty((R, nsteps, 5))
    lnp = np.empty((R, nsteps))

    def draw():
        x = np.empty((R, 5))
        x[:, 0] = rng.normal(14.0, 2.5, R)
        x[:, 1] = np.round(rng.normal(0.0, 1.0, R), 1) * rng.choice([1.0, -1.0], R)       # many +0.0 and -0.0
        x[:, 2] = rng.randint(-50, 1000, R) * 4.9406564584124654e-324 * 2.0 ** rng.randint(0, 40, R)
        x[:, 3] = 3.7
        x[:, 4] = -1e6 * rng.rand(R) ** 3
        return x, -0.5 * rng.chisquare(5, R)
    chain[:, 0], lnp[:, 0] = draw()
    for t in range(1, nsteps):
        x, l = draw()
        move = rng.rand(R) < 0.4
        chain[:, t] = np.where(move[:, None], x, chain[:, t - 1])
        lnp[:, t] = np.where(move, l, lnp[:, t - 1])
    return chain.reshape(nsrc, nw, nsteps, 5), lnp.reshape(nsrc, nw, nsteps)


@pytest.mark.parametrize("nsrc,nw,nsteps", [(1, 250, 250), (1, 64, 5000), (37, 50, 101), (1000, 250, 16)])
@pytest.mark.parametrize("burn,thin", [(0, 1), (7, 3)])
def test_summary_vs_numpy(mbb, nsrc, nw, nsteps, burn, thin):
    """2. Against numpy at sizes that matter: one workgroup per column and columns split over workgroups, a window,
    three intervals at once, clipping on and off, awkward values."""
    from mbb_emcee_amd import results
    chain, lnp = _random_chain(nsrc, nw, nsteps, seed=nsrc + nsteps + burn)
    like = mbb.likelihood()
    cen = (68.3, 95.4, 99.7)
    c0 = chain[..., 0]
    clip = {0: (float(np.percentile(c0, 20)), float(np.percentile(c0, 90))), 4: (None, -1e3)}
    plain = results.chain_summary(like, chain, lnp, percentile=cen, burn=burn, thin=thin, keep=False)
    clipped = results.chain_summary(like, chain, lnp, percentile=cen, burn=burn, thin=thin, clip=clip, keep=False)
    win = chain[:, :, burn::thin, :]
    wl = lnp[:, :, burn::thin]
    n = win.shape[1] * win.shape[2]
    flat = win.reshape(nsrc, n, 5)
    qs = plain.percentiles[0]
    assert len(qs) == 6 and clipped.percentiles[0] == qs
    mean, pct, mn, mx, nu = plain.mean, plain.percentiles[1], plain.min, plain.max, plain.n_used
    assert np.all(nu[:, :5] == n) and np.all(nu[:, 5:] == 0)
    srt = np.sort(flat, axis=1)
    # (numpy's mean of a contiguous 1-d array -- what _parcen_internal is given -- sums pairwise; a reduction along the
    # middle axis of `flat` would add the rows one after another and be off by thousands of eps itself)
    cols = np.ascontiguousarray(np.moveaxis(flat, 1, -1))        # [nsrc, 5, n]
    want_mean = np.array([[cols[g, i].mean() for i in range(5)] for g in range(nsrc)])
    scale = np.abs(flat).mean(axis=1)
    err = _mean_err(mean[:, :5], want_mean, scale)
    print("    mean: worst %.3g eps mean|x| (bound 64)" % err.max())
    rec_allclose(err, 0.0, rtol=0, atol=64, kind="summary mean [eps mean|x|]")
    want = np.percentile(flat, qs, axis=1)                       # [q, nsrc, 5]
    worst = 0.0
    for k, q in enumerate(qs):
        lo, hi = SR.bracket(np.moveaxis(srt, 1, -1), q)
        u = SR.ulps_off(pct[:, :5, k], want[k], lo, hi)
        worst = max(worst, u.max())
        rec_allclose(u, 0.0, rtol=0, atol=4, kind="summary percentile [ulp]")
    print("    percentiles: worst %.3g ulp of the bracketing value (bound 4)" % worst)
    assert np.array_equal(mn[:, :5], flat.min(axis=1)) and np.array_equal(mx[:, :5], flat.max(axis=1))
    # covariance against numpy.cov.  Both sum n products about a mean; a sum of n terms in any order errs by at most
    # n eps sum|terms| and by about sqrt(n) eps of it in practice -- the tree here has depth n / 2048 + 14, numpy's dot
    # is blocked -- and sum|dx dy| <= (n - 1) sqrt(C_xx C_yy) (Cauchy-Schwarz).  A mean off by d (64 eps mean|x| at most,
    # see above) changes the sum by n d_x d_y, second order.  Bound: 512 eps sqrt(C_xx C_yy) + 2 (64 eps)^2 mean|x| mean|y|.
    cov = plain.covariance                 # (a 4-d chain: every result has the source axis, one source or many)
    worst = 0.0
    for g in range(nsrc):
        c = np.cov(cols[g])                                     # (contiguous rows: numpy's means are pairwise sums)
        d = np.sqrt(np.diag(c))
        bound = 512 * EPS * np.outer(d, d) + 2 * (64 * EPS) ** 2 * np.outer(scale[g], scale[g]) + 1e-300
        worst = max(worst, (np.abs(cov[g] - c) / bound).max())
    print("    covariance: worst %.3g of its bound" % worst)
    rec_allclose(worst, 0.0, rtol=0, atol=1, kind="summary covariance [its bound]")
    # best fit: the first maximum in [walker][step] order of the window
    bp, bv, bi = plain.best_fit
    for g in range(nsrc):
        w, t = np.unravel_index(wl[g].argmax(), wl[g].shape)
        assert (bi[g][0], bi[g][1]) == (w, burn + t * thin)
        assert np.array_equal(bp[g], win[g, w, t]) and bv[g] == wl[g, w, t]
    # clipped columns 0 (both bounds) and 4 (upper only); the others are as before, bit for bit
    cm, cp, cn = clipped.mean, clipped.percentiles[1], clipped.n_used
    assert np.array_equal(cm[:, 1:4], mean[:, 1:4]) and np.array_equal(cp[:, 1:4], pct[:, 1:4])
    for g in range(0, nsrc, max(1, nsrc // 40)):
        for col, (lo, hi) in clip.items():
            x = flat[g, :, col]
            x = x[(x >= (-np.inf if lo is None else lo)) & (x <= (np.inf if hi is None else hi))]
            assert cn[g, col] == x.size and 0 < x.size < n
            s_ = np.abs(x).mean()
            rec_allclose((cm[g, col] - x.mean()) / (EPS * s_), 0.0, rtol=0, atol=64, kind="summary mean [eps mean|x|]")
            xs, w_ = np.sort(x), np.percentile(x, qs)
            for k, q in enumerate(qs):
                rec_allclose(SR.ulps_off(cp[g, col, k], w_[k], *SR.bracket(xs, q)), 0.0, rtol=0, atol=4,
                             kind="summary percentile [ulp]")


def test_summary_nan_and_empty_columns(mbb):
    """A column holding a NaN gives NaN mean and percentiles, as numpy's; a clip that removes everything sets the status
    and raises the reference's message instead of faulting."""
    from mbb_emcee_amd import results, _native
    chain, lnp = _random_chain(2, 20, 30, seed=3)
    chain[1, 3, 4, 1] = np.nan
    like = mbb.likelihood()
    s = results.chain_summary(like, chain, lnp)
    assert np.isnan(s.mean[1, 1]) and np.all(np.isnan(s.percentiles[1][1, 1])) and s.status[1, 1] == _native.SUM_HAS_NAN
    assert np.all(np.isfinite(s.mean[0, :5])) and np.all(np.isfinite(s.percentiles[1][0, :5])) and s.status[0, 1] == 0
    assert np.all(np.isnan(s.par_cen("beta")[1])) and np.all(np.isfinite(s.par_cen("beta")[0]))
    e = results.chain_summary(like, chain, lnp, clip={"T": (1e9, None)})
    assert np.all(e.n_used[:, 0] == 0) and np.all(e.status[:, 0] == _native.SUM_EMPTY) and np.all(np.isnan(e.mean[:, 0]))
    with pytest.raises(Exception, match="No elements survive lower/upper limit clipping"):
        e.par_cen("T", lowlim=1e9)
    with pytest.raises(Exception, match="No elements survive lower/upper limit clipping"):
        s.par_cen("T", lowlim=1e9)                            # on demand
    # a clip drops the NaN before mean and percentiles, as _parcen_internal's comparison does
    c = results.chain_summary(like, chain, lnp, clip={"beta": (-1e9, None)})
    assert c.n_used[1, 1] == 20 * 30 - 1 and np.isfinite(c.mean[1, 1])


def _raw_equal(a, b):
    ra, rb = a._raw, b._raw
    return all(np.array_equal(getattr(ra, f), getattr(rb, f), equal_nan=True)
               for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best", "best_index"))


def _sampler_case(mbb, g_lnl, multi):
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rng = np.random.RandomState(11)
    if multi:
        ns, nw = 5, 40
        truths = np.column_stack([rng.uniform(8, 20, ns), rng.uniform(1.2, 2.4, ns), rng.uniform(300, 900, ns),
                                  rng.uniform(2, 4.5, ns), rng.uniform(10, 80, ns)])
        one = mbb.likelihood(response=True)
        one.set_phot(bands, np.ones(8), np.ones(8))
        flux = one.model_flux(truths)
        like = mbb.likelihood(response=True)
        like.set_phot_multi(bands, flux, 0.1 * flux + 1.0)
        p0 = truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, nw, 5)))
    else:
        nw = 64
        truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
        like = mbb.likelihood(response=True)
        like.set_phot(bands, np.ones(8), np.ones(8))
        flux = like.model_flux(truth)[0]
        like.set_phot(bands, flux, 0.1 * flux + 1.0)
        p0 = truth * (1.0 + 0.02 * rng.normal(size=(nw, 5)))
    return like, nw, p0


@pytest.mark.parametrize("multi", [False, True])
def test_sampler_summary_equals_summary_of_stored_chain(mbb, g_lnl, multi):
    """3. The same seed run twice from the same state: with a stored chain, and with storechain=False, summary=...
    The summaries are bitwise equal, and so are the final ensemble and the acceptance counts; summary= together with
    storechain=True returns bitwise the chain it returns without; run to run the summary is bitwise reproducible."""
    from mbb_emcee_amd import results
    like, nw, p0 = _sampler_case(mbb, g_lnl, multi)
    N = 60
    kw = dict(percentile=(68.3, 95.4), burn=5, thin=2, derived=("peaklambda", "lir", "dustmass"), redshift=2.3,
              lumdist_mpc=18700.0)
    a = mbb.DeviceEnsembleSampler(nw, 5, like, seed=77)
    pa, la, _ = a.run_mcmc(p0, N)
    assert a.summary is None
    ref = results.chain_summary(like, a.chain, a.lnprobability, **kw)
    outs = []
    for rep in range(2):
        b = mbb.DeviceEnsembleSampler(nw, 5, like, seed=77)
        pb, lb, _ = b.run_mcmc(p0, N, storechain=False, summary=kw)
        assert b.chain.shape[-2] == 0                                  # no chain came back
        assert np.array_equal(pa, pb) and np.array_equal(la, lb) and np.array_equal(a.naccepted, b.naccepted)
        assert _raw_equal(b.summary, ref)
        outs.append(b)
    assert _raw_equal(outs[0].summary, outs[1].summary)
    b = outs[1]
    # more from the chain that is still on the device: the same as from the stored chain
    assert np.array_equal(b.summary.par_cen("T", percentile=99.7), ref.par_cen("T", percentile=99.7))
    assert np.array_equal(b.summary.par_uplim("beta", percentile=95), ref.par_uplim("beta", percentile=95))
    assert np.all(np.isfinite(b.summary.lir_cen())) and np.all(b.summary.status[..., :8] == 0)
    held = b.summary
    b.run_mcmc(None, 3)                                                 # the next run overwrites that chain
    assert b.summary is None
    with pytest.raises(RuntimeError, match="chain was not kept"):
        held.par_cen("T", percentile=50.0)
    c = mbb.DeviceEnsembleSampler(nw, 5, like, seed=77)
    c.run_mcmc(p0, N, summary=kw)
    assert np.array_equal(c.chain, a.chain) and np.array_equal(c.lnprobability, a.lnprobability)
    assert _raw_equal(c.summary, ref)
    c.reset()
    assert c.summary is None


def test_fitter_and_cli_summary_cfg2(mbb, g_lnl, tmp_path, capsys):
    """4. mbb_fitter.run(..., summary=True) and the CLI's --summary end to end on the 8-band response-integrated
    configuration: the summary is that of the chain the fit returns."""
    from mbb_emcee_amd import results, run_mbb_emcee
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    like = mbb.likelihood(response=True)
    like.set_phot(bands, np.ones(8), np.ones(8))
    flux = like.model_flux(truth)[0]
    fit = mbb.mbb_fitter(nwalkers=250, response=True, seed=3)
    fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    fit.run(50, 100, p0, summary=True)
    s = fit.summary
    assert s is not None and fit.sampler.chain.shape == (250, 100, 5)
    ref = results.chain_summary(fit.like, fit.sampler.chain, fit.sampler.lnprobability)
    assert _raw_equal(s, ref)
    cen = s.par_cen("T")
    assert abs(cen[0] - 12.0) < 3.0 and cen[1] > 0 and cen[2] > 0
    fit.run(50, 20, p0)
    assert fit.summary is None                                           # the default leaves no summary
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", "250", "-b", "50", "-N", "100", "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--summary", "--get_peaklambda"]) == 0
    text = capsys.readouterr().out
    assert "ChiSquare of best fit point" in text and "Lambda peak" in text
    d = np.load(out)
    flat = d["chain"].reshape(-1, 5)
    want = np.ascontiguousarray(flat.T).mean(axis=1)                 # (rows contiguous: numpy sums them pairwise)
    rec_allclose((d["summary_mean"][:5] - want) / (EPS * np.abs(flat).mean(axis=0)), 0.0, rtol=0, atol=64,
                 kind="summary mean [eps mean|x|]")
    assert np.array_equal(d["summary_best_fit"], d["chain"][tuple(d["summary_best_fit_index"])])
    assert d["summary_percentiles"].shape == (8, 4) and np.all(np.isfinite(d["summary_percentiles"][:6]))
    keys_with = set(d.files)
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == ""
    assert keys_with - set(np.load(out).files) == {k for k in keys_with if k.startswith("summary_")} | {"peaklambda"}


def test_summary_kernels_use_no_scratch():
    """5. Build hygiene: the compiler's resource remarks for the summary kernels show no scratch and no spilled
    vector registers (tools/kernel_resources.py reads the same remarks; its table is profiles/r07/kernel_resources.txt)."""
    import re
    table = open(os.path.join(ROOT, "profiles", "r07", "kernel_resources.txt")).read()
    rows = [ln.split() for ln in table.splitlines() if re.search(r"k_sum_", ln)]
    names = {r[0] for r in rows}
    for k in ("k_sum_stats", "k_sum_begin", "k_sum_hist", "k_sum_pick", "k_sum_cov", "k_sum_finish", "k_sum_take",
              "k_sum_lir", "k_sum_dustmass"):
        assert any(k in n for n in names), k
    for r in rows:
        vspill, scratch = int(r[-3]), int(r[-2])
        assert vspill == 0 and scratch == 0, r
