"""Sampler form 7 (k_flowm) held bitwise to the plain launch train (form 1) where the arbitration between its waves can
go wrong: which wave of a SIMD gets the issue slots (priorities by how soon the chain needs a wave's result, the
constructor of the earlier half-step ahead of the later one's) and what the accept-test wave works out before its
partner's decision arrives.  None of that can give wrong numbers: a mistake starves a wave until a bounded wait gives up
(error 9) and the run is silently redone as a launch train, which passes every bitwise check.  So every case also asserts
that both launches were form 7's, that no fall-back was counted and that no RuntimeWarning was raised.
Needs an MI355X: `pytest -m gpu`.

Shapes: runs of 1, 2, 3, 4, 7 and 40 steps (a constructor wave with no proposal at all; the first proposals, whose look at
the hand-over word of half-step j - 1 has j = 0 or meets a record buffer not yet used once -- there are four --; steady
state), ensembles of 4 walkers (two possible partners per draw: the longest dependency chains) and of 64, the bench's eight
bands (a workgroup of 16 waves, the spread placement of the roles) and a four-band set that gets fewer than 16 waves (the
other role branch); an ensemble whose start scatters rows below a lower limit and to non-finite values (constructors of
near-zero length: a later proposal is through before an earlier one); upper limits and Gaussian priors with the
peak-wavelength terms (the penalties behind the hand-over, and the hook behind the constructor's prologue); the 12-band
covariance set."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PLAIN = {"lookahead_sampler": 0, "flow_sampler": 0}
FORM7 = {"lookahead_sampler": 1, "flow_sampler": 1, "merged_flow_sampler": 1, "resident_sampler": 1, "flow_min_steps": 1}
CENTRE = [12.0, 1.8, 600.0, 3.0, 40.0]
STEPS = (1, 2, 3, 4, 7, 40)
FOUR_BANDS = ["PACS_160um", "SPIRE_250um", "SPIRE_350um", "SPIRE_500um"]      # (test_flowm_dealing_gpu._few)


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _sampler(mbb, nw, like, seed):
    """The device sampler for any even number of walkers: the library takes two and more, the Python class keeps emcee's
    rule of at least twice the dimension, which an ensemble of four does not meet."""
    if nw >= 10:
        return mbb.DeviceEnsembleSampler(nw, 5, like, seed=seed)

    class Small(mbb.DeviceEnsembleSampler):
        def __init__(self):                                 # (DeviceEnsembleSampler.__init__ without that rule)
            self.k, self.dim, self.a = int(nw), 5, 2.0
            self.lnprobfn = like
            self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
            self._h = None
            self._ctx = None
            self._ns = 1
            self.reset()
    return Small()


def _cfg2(mbb, g_lnl, names=None):
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    names = bands if names is None else names
    idx = [bands.index(n) for n in names]
    like = mbb.likelihood(response=True)
    like.set_phot(names, g_lnl["cfg2/thick_walpha/flux"][idx], g_lnl["cfg2/thick_walpha/unc"][idx])
    return like


def _eight(mbb, g_lnl):
    return _cfg2(mbb, g_lnl)


def _four(mbb, g_lnl):
    return _cfg2(mbb, g_lnl, FOUR_BANDS)


def _lowlim(mbb, g_lnl):
    like = _cfg2(mbb, g_lnl)
    like.set_lowlim("T", 11.9); like.set_lowlim("beta", 1.75)
    return like


def _priors(mbb, g_lnl):
    like = _cfg2(mbb, g_lnl)
    like.set_uplim("T", 14.0); like.set_uplim("beta", 2.2); like.set_uplim("peaklam", 260.0)
    like.set_gaussian_prior("beta", 1.9, 0.2); like.set_gaussian_prior("peaklam", 240.0, 15.0)
    like.set_gaussian_prior("alpha", 3.2, 0.5)
    return like


def _cov(mbb, g_lnl):
    like = mbb.likelihood(response=True)
    k = "cfg4/thick_walpha"
    like.set_phot([str(b) for b in g_lnl["cfg4/bands"]], g_lnl[k + "/flux"], g_lnl[k + "/unc"])
    like.set_cov(g_lnl[k + "/cov"])
    return like


def _run(mbb, like, opts, nw, p0, seed, nsteps):
    ctx = like.context
    for o, v in opts.items():
        ctx.set_option(o, v)
    fallbacks = ctx.info("flow_fallbacks")
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        s = _sampler(mbb, nw, like, seed)
        pos, lnp, _ = s.run_mcmc(p0, nsteps)
        form, threads = ctx.info("last_kernel_form"), int(ctx.info("last_threads"))
        pos2, lnp2, _ = s.run_mcmc(None, 3)           # (the sampler's next launch: control words and counters start anew)
        form2 = ctx.info("last_kernel_form")
    grew = ctx.info("flow_fallbacks") - fallbacks
    out = (pos, lnp, pos2, lnp2, s.chain.copy(), s.lnprobability.copy(), s.naccepted.copy())
    return out, (form, form2), grew, threads


def _held_to_the_train(mbb, g_lnl, make, nw, p0, seed, nsteps):
    ref, forms, _, _ = _run(mbb, make(mbb, g_lnl), PLAIN, nw, p0, seed, nsteps)
    assert forms == (1, 1)
    got, forms, grew, threads = _run(mbb, make(mbb, g_lnl), FORM7, nw, p0, seed, nsteps)
    assert forms == (7, 7) and grew == 0, (forms, grew)
    for x, y in zip(ref, got):
        assert np.array_equal(x, y, equal_nan=True), (nw, nsteps)
    assert ref[4].shape == (nw, nsteps + 3, 5)
    return ref, threads


def _start(nw, seed, spread=0.02):
    return np.array(CENTRE) * (1.0 + spread * np.random.RandomState(seed).normal(size=(nw, 5)))


@pytest.mark.parametrize("nsteps", STEPS)
@pytest.mark.parametrize("nw", (4, 64))
@pytest.mark.parametrize("bands", ("eight_bands_16_waves", "four_bands_fewer_waves"))
def test_form7_equals_the_launch_train_under_arbitration(mbb, g_lnl, bands, nw, nsteps):
    seed = 61 + nw
    ref, threads = _held_to_the_train(mbb, g_lnl, _eight if bands.startswith("eight") else _four, nw, _start(nw, seed), seed, nsteps)
    # (the role branch the case is there for: the spread placement of a 16-wave workgroup, or "the last five")
    assert threads == 1024 if bands.startswith("eight") else 0 < threads < 1024, (bands, threads)
    assert np.isfinite(ref[1]).all()


def test_form7_constructors_of_near_zero_length(mbb, g_lnl):
    """Rows below a lower limit and rows with values that are not finite (test_flowm_chain_gpu's ensemble): their
    constructor ends at the gate, so the proposal of a later half-step is through before an earlier one's -- the later
    wave, one level down while the earlier record is not handed over, must come through all the same."""
    nw, seed, far = 64, 45, [3, 40]
    p0 = _start(nw, seed)
    p0[far, 4] = -1.7e308; p0[far, 0] = 1000.0
    p0[7, 0] = 11.0; p0[50, 1] = 1.0                      # (below the limits, in range)
    ref, threads = _held_to_the_train(mbb, g_lnl, _lowlim, nw, p0, seed, 40)
    assert threads == 1024
    assert np.isneginf(ref[3][far]).all() and np.array_equal(ref[2][far], p0[far])       # (they never moved)
    assert np.isfinite(np.delete(ref[3], far + [7, 50])).all() and ref[6].sum() > 0


def test_form7_penalties_behind_the_hand_over(mbb, g_lnl):
    """Upper limits and Gaussian priors on parameters and on the peak wavelength: the penalties' path behind the
    hand-over and the peak's root solve behind the constructor's prologue."""
    nw, seed = 60, 43
    ref, threads = _held_to_the_train(mbb, g_lnl, _priors, nw, _start(nw, seed, 0.03), seed, 40)
    assert threads == 1024 and np.isfinite(ref[1]).all()


def test_form7_covariance_set(mbb, g_lnl):
    nw, seed = 60, 55
    ref, _ = _held_to_the_train(mbb, g_lnl, _cov, nw, _start(nw, seed), seed, 5)
    assert np.isfinite(ref[1]).all()
