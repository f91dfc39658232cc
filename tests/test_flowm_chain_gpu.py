"""Sampler form 7 (k_flowm) held bitwise to the plain launch train on the paths its record-to-decision chain takes
through LDS: quadrature waves that carry two or more units (their descriptors and tail slots come from LDS), records
read by the accept-test waves ahead of the quadrature's end, rows whose status is not OK, the covariance path, upper
limits and Gaussian priors (the penalties posted behind the record), and runs so short that the pipeline never fills.
Needs an MI355X: `pytest -m gpu`.

A protocol that gives up is silently redone as a launch train and would pass every bitwise check while being slow:
every case also asserts that the run was form 7's and that no fall-back was counted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN = {"lookahead_sampler": 0, "flow_sampler": 0}
# (test_gpu_parity._sampler_forms' options for the two forms; "flow_min_steps" 1 so that a run of a single step, which
# by default takes the launch train, is form 7's too)
FORM7 = {"lookahead_sampler": 1, "flow_sampler": 1, "merged_flow_sampler": 1, "resident_sampler": 1, "flow_min_steps": 1}
CENTRE = [12.0, 1.8, 600.0, 3.0, 40.0]
STEPS = (1, 2, 3, 5, 40)          # pipeline fill, fewer half-steps than record buffers, fewer than the lag, a filled pipeline


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _cfg2(mbb, g_lnl):
    like = mbb.likelihood(response=True)
    like.set_phot([str(b) for b in g_lnl["cfg2/bands"]], g_lnl["cfg2/thick_walpha/flux"], g_lnl["cfg2/thick_walpha/unc"])
    return like


def _cfg4_cov(mbb, g_lnl):
    """The 12-band set with its covariance matrix: more units than quadrature waves (second and third units, tails of
    several bands packed into shared chunks on units that are not a wave's first), more than 8 bands."""
    like = mbb.likelihood(response=True)
    k = "cfg4/thick_walpha"
    like.set_phot([str(b) for b in g_lnl["cfg4/bands"]], g_lnl[k + "/flux"], g_lnl[k + "/unc"])
    like.set_cov(g_lnl[k + "/cov"])
    return like


def _lowlim(mbb, g_lnl):
    """Lower limits right under the ensemble: many proposals fall below them (status below-limit, lnL = -inf)."""
    like = _cfg2(mbb, g_lnl)
    like.set_lowlim("T", 11.9); like.set_lowlim("beta", 1.75)
    return like


def _priors(mbb, g_lnl):
    """Upper limits and Gaussian priors on parameters and on the peak wavelength (its root solve in the constructor)."""
    like = _cfg2(mbb, g_lnl)
    like.set_uplim("T", 14.0); like.set_uplim("beta", 2.2); like.set_uplim("peaklam", 260.0)
    like.set_gaussian_prior("beta", 1.9, 0.2); like.set_gaussian_prior("peaklam", 240.0, 15.0)
    like.set_gaussian_prior("alpha", 3.2, 0.5)
    return like


# (name, likelihood, walkers, relative spread of the start, seed)
CASES = {"cfg4_covariance": (_cfg4_cov, 60, 0.02, 41),
         "below_lower_limits": (_lowlim, 64, 0.02, 42),
         "uplims_and_priors_with_peak": (_priors, 60, 0.03, 43),
         "cfg2_250_walkers": (_cfg2, 250, 0.02, 44)}


def _run(mbb, like, opts, nw, p0, seed, nsteps):
    ctx = like.context
    for o, v in opts.items():
        ctx.set_option(o, v)
    fallbacks = ctx.info("flow_fallbacks")
    s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=seed)
    pos, lnp, _ = s.run_mcmc(p0, nsteps)
    form = ctx.info("last_kernel_form")
    pos2, lnp2, _ = s.run_mcmc(None, 3)               # (the sampler's next launch: the other set of completion counters)
    form2 = ctx.info("last_kernel_form")
    grew = ctx.info("flow_fallbacks") - fallbacks
    return (pos, lnp, pos2, lnp2, s.chain.copy(), s.lnprobability.copy(), s.naccepted.copy()), (form, form2), grew


@pytest.mark.parametrize("nsteps", STEPS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_form7_equals_the_launch_train(mbb, g_lnl, case, nsteps):
    make, nw, spread, seed = CASES[case]
    p0 = np.array(CENTRE) * (1.0 + spread * np.random.RandomState(seed).normal(size=(nw, 5)))
    ref, forms, _ = _run(mbb, make(mbb, g_lnl), PLAIN, nw, p0, seed, nsteps)
    assert forms == (1, 1)
    got, forms, grew = _run(mbb, make(mbb, g_lnl), FORM7, nw, p0, seed, nsteps)
    assert forms == (7, 7) and grew == 0, (forms, grew)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y, equal_nan=True), (case, nsteps)
    assert ref[4].shape == (nw, nsteps + 3, 5)
    if case == "below_lower_limits" and nsteps == 40:
        assert 0.0 < ref[6].mean() / 43 < 0.6             # many proposals fell below the limits
    if case != "below_lower_limits":
        assert np.isfinite(ref[1]).all()


def test_form7_rows_with_non_finite_parameters(mbb, g_lnl):
    """Rows whose status is not OK, with the record read ahead of the quadrature's end: walkers started below the lower
    limits, two of them at fnorm = -1.7e308 and T = 1000.  Their own proposals x + z (c - x) have fnorm below its limit,
    -inf for z > 1.06: a parameter that is not finite, lnL = -inf.  A proposal made through them, c + z (x - c), has
    fnorm below its limit for z < 1 and T = 1000 - 988 z below its limit for z > 1.0001 (in between it would be a valid
    row with fnorm ~ 1e304, which no draw of this seed makes).  None is ever accepted; the chain is the train's."""
    nw, seed, far = 64, 45, [3, 40]
    p0 = np.array(CENTRE) * (1.0 + 0.02 * np.random.RandomState(seed).normal(size=(nw, 5)))
    p0[far, 4] = -1.7e308; p0[far, 0] = 1000.0
    p0[7, 0] = 11.0; p0[50, 1] = 1.0                      # (below the limits, in range)
    out = []
    for opts in (PLAIN, FORM7):
        out.append(_run(mbb, _lowlim(mbb, g_lnl), opts, nw, p0, seed, 40))
    (ref, _, _), (got, forms, grew) = out
    assert forms == (7, 7) and grew == 0, (forms, grew)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.isneginf(ref[3][far]).all() and np.array_equal(ref[2][far], p0[far])       # (they never moved)
    assert np.isfinite(np.delete(ref[3], far + [7, 50])).all() and ref[6].sum() > 0
