"""Sampler form 7 (k_flowm) held bitwise to the plain launch train (form 1) on band sets that stress how the quadrature's
units are dealt to its waves: fewer units than quadrature waves, exactly as many, many more (units of one chunk), a layout
whose leftovers share tail units that are some waves' second unit, and the 12-band set with its covariance matrix; runs
of 1, 2, 5 and 40 steps.  Every case states the shape it is there for as an assertion on the layout the library made
(units, quadrature waves), so that a change of the layout cannot quietly turn it into another case.  Needs an MI355X:
`pytest -m gpu`.

A protocol that gives up is redone as a launch train (with a RuntimeWarning) and would pass every bitwise check: every
case also asserts that both launches were form 7's, that no fall-back was counted and that no RuntimeWarning was raised."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN = {"lookahead_sampler": 0, "flow_sampler": 0}
FORM7 = {"lookahead_sampler": 1, "flow_sampler": 1, "merged_flow_sampler": 1, "resident_sampler": 1, "flow_min_steps": 1}
CENTRE = [12.0, 1.8, 600.0, 3.0, 40.0]
STEPS = (1, 2, 5, 40)
SERVICE_WAVES = 5                  # three constructor waves and two accept-test waves: the others are the quadrature's


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _cfg2_subset(mbb, g_lnl, names):
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    idx = [bands.index(n) for n in names]
    like = mbb.likelihood(response=True)
    like.set_phot(names, g_lnl["cfg2/thick_walpha/flux"][idx], g_lnl["cfg2/thick_walpha/unc"][idx])
    return like


def _few(mbb, g_lnl):
    """four bands of two or three chunks each, three leftovers in one tail unit: five units, for which the launch is made
    with eight quadrature waves (the workgroup is sized in steps of four waves)"""
    return _cfg2_subset(mbb, g_lnl, ["PACS_160um", "SPIRE_250um", "SPIRE_350um", "SPIRE_500um"])


def _exactly(mbb, g_lnl):
    """six bands: nine units of full chunks and six leftover rows in two tail units, eleven units for eleven waves"""
    return _cfg2_subset(mbb, g_lnl, ["PACS_70um", "PACS_160um", "SPIRE_350um", "SPIRE_500um", "SCUBA2_850um", "Bolocam_1.1mm"])


def _tails(mbb, g_lnl):
    """the bench's eight bands: thirteen units, the last two of them tail units -- two waves' second unit"""
    return _cfg2_subset(mbb, g_lnl, [str(b) for b in g_lnl["cfg2/bands"]])


def _many(mbb, g_lnl):
    """the same bands in units of one chunk: three units and more per wave"""
    like = _tails(mbb, g_lnl)
    like.context.set_option("seg_chunks", 1)
    like._dirty = True                                     # (a layout option acts when the bands are next set)
    return like


def _cov(mbb, g_lnl):
    """the 12-band set with its covariance matrix: more units than waves, more than 8 bands"""
    like = mbb.likelihood(response=True)
    k = "cfg4/thick_walpha"
    like.set_phot([str(b) for b in g_lnl["cfg4/bands"]], g_lnl[k + "/flux"], g_lnl[k + "/unc"])
    like.set_cov(g_lnl[k + "/cov"])
    return like


# name -> (likelihood, walkers, seed, what the layout must look like: units against quadrature waves)
CASES = {"fewer_units_than_waves": (_few, 60, 51, lambda nun, nq: nun < nq),
         "as_many_units_as_waves": (_exactly, 60, 52, lambda nun, nq: nun == nq),
         "tail_units_as_second_units": (_tails, 64, 53, lambda nun, nq: nq < nun <= 2 * nq),
         "many_more_units_than_waves": (_many, 60, 54, lambda nun, nq: nun >= 3 * nq),
         "covariance_set": (_cov, 60, 55, lambda nun, nq: nun > nq)}


def _run(mbb, like, opts, nw, p0, seed, nsteps):
    ctx = like.context
    for o, v in opts.items():
        ctx.set_option(o, v)
    fallbacks = ctx.info("flow_fallbacks")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=seed)
        pos, lnp, _ = s.run_mcmc(p0, nsteps)
        form, threads, nun = ctx.info("last_kernel_form"), ctx.info("last_threads"), ctx.info("nunit")
        pos2, lnp2, _ = s.run_mcmc(None, 3)           # (the sampler's next launch: control words and counters start anew)
        form2 = ctx.info("last_kernel_form")
    grew = ctx.info("flow_fallbacks") - fallbacks
    out = (pos, lnp, pos2, lnp2, s.chain.copy(), s.lnprobability.copy(), s.naccepted.copy())
    return out, (form, form2), grew, (int(nun), int(threads) // 64 - SERVICE_WAVES)


@pytest.mark.parametrize("nsteps", STEPS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_form7_equals_the_launch_train_whatever_the_deal_of_units(mbb, g_lnl, case, nsteps):
    make, nw, seed, shape = CASES[case]
    p0 = np.array(CENTRE) * (1.0 + 0.02 * np.random.RandomState(seed).normal(size=(nw, 5)))
    ref, forms, _, _ = _run(mbb, make(mbb, g_lnl), PLAIN, nw, p0, seed, nsteps)
    assert forms == (1, 1)
    got, forms, grew, (nun, nq) = _run(mbb, make(mbb, g_lnl), FORM7, nw, p0, seed, nsteps)
    assert forms == (7, 7) and grew == 0, (forms, grew)
    assert shape(nun, nq), (case, nun, nq)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y, equal_nan=True), (case, nsteps)
    assert ref[4].shape == (nw, nsteps + 3, 5) and np.isfinite(ref[1]).all()
