"""Predicted fluxes without a GPU: spec parsing and its refusals, the sample lists a spec reaches the library as, the
request's validation, ``predflux_cen`` / ``sed_band`` arithmetic on a hand-made raw result, the on-demand and
``drop_chain`` rules, the sampler's ``predict=`` keyword rules on a faked device, and the numpy restatement of the
analysis (tests/_predict_ref.py) against the columns the reference itself made (tests/golden/results.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, golden_bands
import _predict_ref as PR
from mbb_emcee_amd.results import _pval          # (_parcen_internal's two percentiles in its own arithmetic)

VARIANTS = [("thin_walpha", True, False), ("thick_walpha", False, False),
            ("thick_noalpha", False, True), ("thin_noalpha", True, True)]


@pytest.fixture(scope="module")
def wheel():
    import mbb_emcee_amd
    return mbb_emcee_amd.likelihood(response=True)._responsewheel


class _Like(object):
    """Stands where a likelihood would: it has a filter wheel, and touching the device is an error."""
    data_read = True
    response_integrate = True
    opthin = noalpha = False
    wavenorm = 500.0

    def __init__(self, wheel=None):
        self._responsewheel = wheel
        self.response_integrate = wheel is not None

    def _sync_device(self):
        raise AssertionError("the device was touched")

    context = property(_sync_device)


# ---------------------------------------------------------------- specs
def test_spec_parsing_and_refusals(wheel):
    """A wavelength, a band name, a list mixing both; postprocess.predict_flux's refusals with its messages."""
    from mbb_emcee_amd import predict
    like = _Like(wheel)
    assert predict.parse_specs(like, 450.0) == ([450.0], True)
    assert predict.parse_specs(like, 450) == ([450.0], True)
    assert predict.parse_specs(like, "SCUBA2_450um") == (["SCUBA2_450um"], True)
    keys, single = predict.parse_specs(like, ["SPIRE_250um", 70, np.float64(1100.0), "SCUBA2_450um"])
    assert keys == ["SPIRE_250um", 70.0, 1100.0, "SCUBA2_450um"] and not single
    assert all(isinstance(k, (str, float)) for k in keys)
    with pytest.raises(ValueError, match="Do not have response function matching NoSuchBand_1um"):
        predict.parse_specs(like, ["SPIRE_250um", "NoSuchBand_1um"])
    for bad in (-3.0, 0.0, float("nan")):
        with pytest.raises(ValueError, match="Invalid wavelength"):
            predict.parse_specs(like, [70.0, bad])
    with pytest.raises(Exception, match="Asked for response integration, but no response functions"):
        predict.parse_specs(_Like(None), "SPIRE_250um")
    assert predict.parse_specs(_Like(None), [70.0, 1100.0]) == ([70.0, 1100.0], False)      # wavelengths need no wheel
    with pytest.raises(ValueError, match="given twice"):
        predict.parse_specs(like, [70.0, 70])
    with pytest.raises(ValueError, match="no prediction spec"):
        predict.parse_specs(like, [])
    for bad in (True, False, np.bool_(True)):                     # (float(True) would be a wavelength of 1 um)
        with pytest.raises(ValueError, match="not (True|False)"):
            predict.parse_specs(like, bad)
        with pytest.raises(ValueError, match="not (True|False)"):
            predict.parse_specs(like, [70.0, bad])


def test_sample_lists_are_the_responses_own(wheel):
    """A passband reaches the library as response.quadrature() -- weight sedmult * normfac --, a wavelength as the single
    frequency um_to_GHz / lambda with weight 1; any band of the wheel, in a fit or not."""
    from mbb_emcee_amd import predict
    from mbb_emcee_amd.modified_blackbody import um_to_GHz
    like = _Like(wheel)
    keys = ["SPIRE_250um", 70.0, "SCUBA2_450um", 1100.0, "GISMO_2mm"]
    off, freq, weight = predict.sample_lists(like, keys)
    assert off.dtype == np.int32 and off[0] == 0 and len(off) == len(keys) + 1 and off[-1] == freq.size == weight.size
    for i, k in enumerate(keys):
        f, w = freq[off[i]:off[i + 1]], weight[off[i]:off[i + 1]]
        if isinstance(k, str):
            r = wheel[k]
            qf, qw = r.quadrature()
            assert np.array_equal(f, qf) and np.array_equal(w, qw) and f.size > 1
            assert np.array_equal(w, r._sedmult * r._normfac) and np.array_equal(f, r._freq)
        else:
            assert f.size == 1 and f[0] == um_to_GHz / k and w[0] == 1.0
    # sample counts below 64 and not multiples of 64 exist among the real bands (the kernel's lane loop)
    counts = np.diff(off)
    assert counts[4] < 64 and counts[0] % 64 and counts[2] > 1024
    # a delta-function band is one sample of weight 1
    import mbb_emcee_amd
    w2 = mbb_emcee_amd.likelihood(response=True)._responsewheel
    w2.add_special("Line_delta_450um")
    off, freq, weight = predict.sample_lists(_Like(w2), ["Line_delta_450um"])
    assert list(off) == [0, 1] and weight[0] == 1.0 and abs(freq[0] - um_to_GHz / 450.0) < 1e-9 * freq[0]


def test_request_validation(wheel):
    from mbb_emcee_amd import predict, _native
    like = _Like(wheel)
    R = predict._Request
    with pytest.raises(ValueError, match="1 to 8 percentiles"):
        R(like, 70.0, [])
    with pytest.raises(ValueError, match="1 to 8 percentiles"):
        R(like, 70.0, list(np.linspace(1, 99, 9)))
    with pytest.raises(ValueError, match="Invalid percentile"):
        R(like, 70.0, [50.0, 100.5])
    with pytest.raises(ValueError, match="burn must be"):
        R(like, 70.0, [50.0], burn=-1)
    with pytest.raises(ValueError, match="burn must be"):
        R(like, 70.0, [50.0], thin=0)
    with pytest.raises(ValueError, match="wavenorm must be positive"):
        R(like, 70.0, [50.0], wavenorm=0.0)
    with pytest.raises(ValueError, match="was not asked for"):
        R(like, [70.0, "SPIRE_250um"], [50.0], clip={"SPIRE_350um": (0.0, None)})
    with pytest.raises(ValueError, match="at most %d specs" % _native.PRED_MAX_SPECS):
        R(like, list(np.linspace(20.0, 2000.0, _native.PRED_MAX_SPECS + 1)), [50.0])
    assert _native.PRED_MAX_SAMPLES // 1108 < _native.PRED_MAX_SPECS
    assert R(like, ["SCUBA2_450um"], [50.0]).freq.size == 1108          # (the largest band of the wheel)
    w2 = type(wheel)()
    w2._responses = dict(wheel._responses)
    for i in range(_native.PRED_MAX_SAMPLES // 1108 + 1):
        w2._responses["copy%d" % i] = wheel["SCUBA2_450um"]
    with pytest.raises(ValueError, match="at most %d quadrature samples" % _native.PRED_MAX_SAMPLES):
        R(_Like(w2), ["copy%d" % i for i in range(_native.PRED_MAX_SAMPLES // 1108 + 1)], [50.0])
    # 64 wavelengths and the eight bands of a fit go in one call
    bands = ["PACS_70um", "PACS_100um", "PACS_160um", "SPIRE_250um", "SPIRE_350um", "SPIRE_500um", "SCUBA2_850um",
             "Bolocam_1.1mm"]
    r = R(like, bands + list(np.geomspace(20.0, 2000.0, 64)), [15.85, 84.15], burn=3, thin=2,
          clip={"SPIRE_250um": (1.0, None), 20.0: (None, 5.0)}, wavenorm=350.0)
    assert len(r.keys) == 72 and r.freq.size <= _native.PRED_MAX_SAMPLES
    with pytest.raises(ValueError, match="burn leaves no step"):
        r.check_steps(3)
    assert r.check_steps(10) == 4
    s = r.spec()
    assert (s.nspec, s.npct, s.burn, s.thin, s.wavenorm) == (72, 2, 3, 2, 350.0) and list(s.pct[:2]) == [15.85, 84.15]
    assert [s.sample_off[i] for i in range(73)] == list(r.sample_off) and s.freq[0] == r.freq[0]
    assert s.has_lo[3] == 1 and s.lo[3] == 1.0 and s.has_hi[3] == 0 and s.has_hi[8] == 1 and s.hi[8] == 5.0 and s.has_lo[8] == 0
    assert sum(s.has_lo[i] + s.has_hi[i] for i in range(72)) == 2
    plain = R(like, 70.0, [50.0]).spec()
    assert not plain.has_lo and not plain.lo and plain.wavenorm == 0.0        # no clip: null pointers; the context's wavenorm
    one = r.only(3, [2.5, 97.5], None, 9.0)
    assert one.keys == ["SPIRE_250um"] and list(one.sample_off) == [0, 189] and one.clip == {0: (None, 9.0)}
    assert np.array_equal(one.freq, wheel["SPIRE_250um"].quadrature()[0]) and (one.burn, one.thin, one.wavenorm) == (3, 2, 350.0)


def test_chain_predictions_validates_before_the_device(wheel):
    from mbb_emcee_amd import predict
    like = _Like(wheel)
    chain = np.ones((4, 6, 5))
    with pytest.raises(ValueError, match="chain must be"):
        predict.chain_predictions(like, np.ones((4, 6, 4)), 70.0)
    with pytest.raises(ValueError, match="Do not have response function"):
        predict.chain_predictions(like, chain, "Nope")
    with pytest.raises(ValueError, match="burn leaves no step"):
        predict.chain_predictions(like, chain, 70.0, burn=6)
    with pytest.raises(ValueError, match="Invalid percentile"):
        predict.chain_predictions(like, chain, 70.0, percentile=101.0)
    with pytest.raises(AssertionError, match="the device was touched"):
        predict.chain_predictions(like, chain, [70.0, "SPIRE_250um"], burn=5)


# ---------------------------------------------------------------- the result object
def _made(wheel, keys, mean, pct, qs, status=None, multi=False, again=None, clip=None):
    from mbb_emcee_amd import predict
    req = predict._Request(_Like(wheel), keys, qs, clip=clip)
    nsrc = mean.shape[0]
    raw = predict._Raw(nsrc, len(req.keys), len(qs))
    raw.mean[:], raw.pct[:] = mean, pct
    raw.min[:], raw.max[:], raw.n_used[:] = pct.min(axis=-1), pct.max(axis=-1), 100
    if status is not None:
        raw.status[:] = status
    return predict.ChainPredictions(req, raw, multi, again, 68.3, 10, 10)


def test_predflux_cen_and_sed_band_arithmetic(wheel):
    qs = list(_pval(68.3)) + list(_pval(95.4))
    keys = [1100.0, "SPIRE_250um", 70.0, 450.0]
    mean = np.array([[5.0, 40.0, 9.0, 20.0], [6.0, 41.0, 10.0, 21.0]])
    pct = mean[..., None] + np.array([-1.0, 2.0, -3.0, 5.0])
    p = _made(wheel, keys, mean, pct, qs, multi=True)
    assert p.specs == keys
    got = p.predflux_cen("SPIRE_250um")
    assert got.shape == (2, 3) and np.array_equal(got, [[40.0, 2.0, 1.0], [41.0, 2.0, 1.0]])
    assert np.array_equal(p.predflux_cen(450, percentile=95.4), [[20.0, 5.0, 3.0], [21.0, 5.0, 3.0]])
    waves, lower, mid, upper = p.sed_band()
    assert np.array_equal(waves, [70.0, 450.0, 1100.0])
    assert np.array_equal(mid, [[9.0, 20.0, 5.0], [10.0, 21.0, 6.0]])
    assert np.array_equal(lower, mid - 1.0) and np.array_equal(upper, mid + 2.0)
    lower2, upper2 = p.sed_band(95.4)[1], p.sed_band(95.4)[3]
    assert np.array_equal(lower2, mid - 3.0) and np.array_equal(upper2, mid + 5.0)
    one = _made(wheel, keys, mean[:1], pct[:1], qs)
    assert one.predflux_cen(70.0).shape == (3,) and np.array_equal(one.predflux_cen(70.0), [9.0, 2.0, 1.0])
    assert one.sed_band()[2].shape == (3,) and one.mean.shape == (4,) and one.percentiles[1].shape == (4, 4)
    assert one.percentiles[0] == qs and np.array_equal(one.n_used, [100] * 4)
    arr = one.arrays()
    assert sorted(arr) == sorted("predict_" + k for k in ("specs", "n_used", "mean", "min", "max", "q", "percentiles", "status"))
    assert list(arr["predict_specs"]) == ["1100.0", "SPIRE_250um", "70.0", "450.0"] and np.array_equal(arr["predict_q"], qs)
    assert "Predicted flux SPIRE_250um: 40.00 +2.00 -1.00 [mJy]" in str(one) and "Predicted flux 70.0um" in str(one)
    with pytest.raises(ValueError, match="was not asked for"):
        one.predflux_cen("SPIRE_350um")
    with pytest.raises(ValueError, match="Invalid percentile"):
        one.predflux_cen(70.0, percentile=120.0)
    with pytest.raises(ValueError, match="no wavelength spec"):
        _made(wheel, ["SPIRE_250um"], mean[:1, :1], pct[:1, :1], qs).sed_band()


def test_predflux_cen_raising_rules(wheel):
    """ChainSummary._cen's: nothing survives -> the reference's exception; a failing SED row inside the window raises
    as postprocess raises it; a NaN gives NaN and does not raise; any source's status counts."""
    from mbb_emcee_amd import _native
    qs = list(_pval(68.3))
    keys = [70.0, "SPIRE_250um"]
    mean = np.array([[9.0, 40.0], [10.0, 41.0]])
    pct = mean[..., None] + np.array([-1.0, 2.0])
    st = np.zeros((2, 2), dtype=np.int32)
    st[1, 0] = _native.SUM_EMPTY
    p = _made(wheel, keys, mean, pct, qs, status=st, multi=True)
    with pytest.raises(Exception, match="No elements survive lower/upper limit clipping"):
        p.predflux_cen(70.0)
    assert p.predflux_cen("SPIRE_250um").shape == (2, 3)
    for code, msg in ((_native.ROW_BAD_ALPHA, "alpha must be positive"), (_native.ROW_BAD_BETA, "beta must be non-negative"),
                      (_native.ROW_NOCONV, "couldn't find")):
        st = np.zeros((2, 2), dtype=np.int32)
        st[0, 1] = _native.SUM_HAS_NAN | (1 << (_native.SUM_ROW_SHIFT + code))
        p = _made(wheel, keys, mean, pct, qs, status=st, multi=True)
        with pytest.raises(ValueError, match=msg):
            p.predflux_cen("SPIRE_250um")
        assert np.array_equal(p.predflux_cen(70.0)[:, 0], [9.0, 10.0])
    st = np.zeros((1, 2), dtype=np.int32)
    st[0, 0] = _native.SUM_HAS_NAN | (1 << (_native.SUM_ROW_SHIFT + _native.ROW_NONFINITE))
    m2, p2 = mean[:1].copy(), pct[:1].copy()
    m2[0, 0], p2[0, 0] = np.nan, np.nan
    got = _made(wheel, keys, m2, p2, qs, status=st).predflux_cen(70.0)
    assert got.shape == (3,) and np.all(np.isnan(got))


def test_on_demand_and_drop_chain_rules(wheel):
    """Percentiles or clip bounds that were not prepared come from the kept chain -- one call for that spec alone, then
    cached --; without the chain the same RuntimeError as a summary's."""
    from mbb_emcee_amd import predict
    qs = list(_pval(68.3))
    keys = [70.0, "SPIRE_250um"]
    mean = np.array([[9.0, 40.0]])
    pct = mean[..., None] + np.array([-1.0, 2.0])
    calls = []

    def again(req):
        calls.append(req)
        raw = predict._Raw(1, 1, len(req.qs))
        raw.mean[:] = 100.0
        raw.pct[:] = 100.0 + np.arange(len(req.qs)) * 10.0 - 5.0
        return raw
    p = _made(wheel, keys, mean, pct, qs, again=again)
    assert np.array_equal(p.predflux_cen(70.0), [9.0, 2.0, 1.0]) and not calls            # prepared: no call
    got = p.predflux_cen("SPIRE_250um", percentile=95.4)
    assert np.array_equal(got, [100.0, 5.0, 5.0]) and len(calls) == 1
    r = calls[0]
    assert r.keys == ["SPIRE_250um"] and r.clip == {} and r.qs == list(_pval(95.4)) and r.sample_off[-1] == 189
    p.predflux_cen("SPIRE_250um", percentile=95.4)
    assert len(calls) == 1                                                                  # cached
    p.predflux_cen(70.0, lowlim=1.0)
    assert len(calls) == 2 and calls[1].keys == [70.0] and calls[1].clip == {0: (1.0, None)} and calls[1].qs == qs
    # a clip that was prepared is served from the prepared result, any other is not
    pc = _made(wheel, keys, mean, pct, qs, again=again, clip={70.0: (1.0, None)})
    del calls[:]
    assert np.array_equal(pc.predflux_cen(70.0, lowlim=1.0), [9.0, 2.0, 1.0]) and not calls
    pc.predflux_cen(70.0)
    assert len(calls) == 1 and calls[0].clip == {}
    p.drop_chain()
    assert np.array_equal(p.predflux_cen("SPIRE_250um", percentile=95.4), got)               # still cached
    with pytest.raises(RuntimeError, match="the chain was not kept"):
        p.predflux_cen("SPIRE_250um", percentile=99.0)
    with pytest.raises(RuntimeError, match="the chain was not kept"):
        _made(wheel, keys, mean, pct, qs).predflux_cen(70.0, uplim=3.0)


# ---------------------------------------------------------------- the sampler's keyword
def _bare_sampler(wheel):
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary = 10, 5, _Like(wheel), None, None

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_predict_keyword_rules(wheel):
    """storechain=False without summary= keeps no chain on the device: predict= says so before anything runs; so do bad
    specs and keywords, and predictions() of a sampler that has no chain; burn and thin default to the summary's."""
    s = _bare_sampler(wheel)
    p0 = np.zeros((10, 5))
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(p0, 16, storechain=False, predict=[70.0, "SPIRE_250um"])
    with pytest.raises(ValueError, match="Do not have response function"):
        s.run_mcmc(p0, 16, predict="Nope")
    with pytest.raises(ValueError, match="Invalid wavelength"):
        s.run_mcmc(p0, 16, predict=dict(specs=[-1.0]))
    with pytest.raises(ValueError, match="predict= needs specs"):
        s.run_mcmc(p0, 16, predict=dict(burn=2))
    with pytest.raises(ValueError, match="not True"):              # (the other analyses' True has no meaning here)
        s.run_mcmc(p0, 16, predict=True)
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(p0, 16, predict=dict(specs=70.0, burn=16))
    with pytest.raises(ValueError, match="burn leaves no step"):          # burn taken from the summary's keywords
        s.run_mcmc(p0, 16, summary=dict(burn=16), predict=70.0)
    with pytest.raises(TypeError, match="unexpected keyword"):
        s.run_mcmc(p0, 16, predict=dict(specs=70.0, nbins=2))
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, summary=dict(burn=15), predict=dict(specs=[70.0, "SCUBA2_450um"], percentile=95.4))
    assert s.predictions_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.predictions(70.0)
    s._resident = 16
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.predictions(70.0, burn=16)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.predictions(70.0, burn=15)


class _Held(object):
    dropped = False

    def drop_chain(self):
        self.dropped = True


def test_predictions_attribute_is_reset(wheel):
    """reset() and the start of the next run -- run_mcmc or sample() -- put predictions_ back to None, and the result
    that was there can no longer go back to the chain."""
    s = _bare_sampler(wheel)
    s._open = None
    held = s.predictions_ = _Held()
    s.reset()
    assert s.predictions_ is None and held.dropped and s.marginals_ is None
    held = s.predictions_ = _Held()
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(np.zeros((10, 5)), 4)
    assert s.predictions_ is None and held.dropped
    s.predictions_ = _Held()
    with pytest.raises(AssertionError, match="the device was touched"):
        next(s.sample(np.zeros((10, 5)), iterations=4))
    assert s.predictions_ is None


def test_results_handed_out_are_invalidated_with_the_chain(wheel):
    """Every result predictions() hands out can go back to the resident chain; the start of the next run -- run_mcmc or
    sample() -- and reset() take that away from ALL of them, not from predictions_ alone: what a result was not made
    with is the RuntimeError afterwards, never a number from another chain.  A result nobody holds is forgotten."""
    import gc
    from mbb_emcee_amd import predict
    qs = list(_pval(68.3))

    def sampler():
        s = _bare_sampler(wheel)
        s._open, calls = None, []
        s.reset()                                                     # (an empty chain and no state, as after __init__)
        s._resident = 16

        def again(req):
            calls.append(req)
            raw = predict._Raw(1, len(req.keys), len(req.qs))
            raw.mean[:], raw.pct[:] = 10.0, 10.0 + np.arange(len(req.qs))
            return raw
        s._predict_again = again
        return s, calls

    for end in ("run_mcmc", "sample", "reset"):
        s, calls = sampler()
        p, q = s.predictions([70.0, "SPIRE_250um"]), s.predictions(450.0, burn=3)
        lost = s.predictions(70.0, keep=False)
        assert len(calls) == 3 and len(s._handed_predictions) == 2
        assert np.array_equal(p.predflux_cen(70.0, percentile=95.4), [10.0, 1.0, 0.0]) and len(calls) == 4      # on demand
        del lost
        gc.collect()
        tmp = s.predictions(1100.0)
        assert len(s._handed_predictions) == 3
        del tmp
        gc.collect()
        assert len(s._handed_predictions) == 2                        # (held weakly)
        if end == "reset":
            s.reset()
        else:
            with pytest.raises(AssertionError, match="the device was touched"):
                if end == "run_mcmc":
                    s.run_mcmc(np.zeros((10, 5)), 4)
                else:
                    next(s.sample(np.zeros((10, 5)), iterations=4))
        s._resident = 9                                               # another chain is resident now
        assert np.array_equal(p.predflux_cen(70.0), [10.0, 1.0, 0.0])                 # what it was made with: still there
        assert np.array_equal(p.predflux_cen(70.0, percentile=95.4), [10.0, 1.0, 0.0])    # ... and what it had cached
        for ask in (lambda: p.predflux_cen(70.0, percentile=90.0), lambda: p.predflux_cen("SPIRE_250um", uplim=3.0),
                    lambda: p.sed_band(90.0), lambda: q.predflux_cen(450.0, lowlim=1.0)):
            with pytest.raises(RuntimeError, match="the chain was not kept"):
                ask()
        assert len(calls) == 5 and p.nsteps_used == 16 and q.nsteps_used == 13
        fresh = s.predictions(70.0)                                   # a result of the new chain works as ever
        fresh.predflux_cen(70.0, percentile=90.0)
        assert len(calls) == 7 and fresh.nsteps_used == 9


def test_sharded_run_is_not_predicted_from(wheel):
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.lnprobfn = _Like(wheel)
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded"):
        s.run_mcmc(np.zeros((10, 5)), 4, predict=70.0)


def test_fitter_and_cli_know_predict():
    import mbb_emcee_amd
    from mbb_emcee_amd import mbb_fitter, run_mbb_emcee
    assert mbb_emcee_amd.chain_predictions is mbb_emcee_amd.predict.chain_predictions
    assert "ChainPredictions" in mbb_emcee_amd.__all__ and "chain_predictions" in mbb_emcee_amd.__all__
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="predict= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), predict=[70.0])
    assert fit.predictions is None
    a = run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz"])
    assert a.predict is None
    a = run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz", "--predict", "70,SCUBA2_450um, 1.1e3"])
    assert run_mbb_emcee.parse_predict(a.predict) == [70.0, "SCUBA2_450um", 1100.0]
    with pytest.raises(ValueError, match="empty spec"):
        run_mbb_emcee.parse_predict("70,,80")


def test_predict_entries_are_declared_and_bound():
    from mbb_emcee_amd import _native
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_predict", "mbb_sampler_predict"):
        assert name in hdr and name in _native.SIGNATURES
    assert [f[0] for f in _native.PredictSpec._fields_] == ["nspec", "npct", "burn", "thin", "sample_off", "freq", "weight",
                                                            "pct", "wavenorm", "has_lo", "has_hi", "lo", "hi"]
    assert [f[0] for f in _native.PredictOut._fields_] == ["n_used", "mean", "min", "max", "pct", "status"]
    assert C.sizeof(_native.PredictSpec) == 144 and C.sizeof(_native.PredictOut) == 48
    for macro, value in (("MBB_PRED_MAX_SPECS", _native.PRED_MAX_SPECS), ("MBB_PRED_MAX_SAMPLES", _native.PRED_MAX_SAMPLES)):
        assert "#define %s %d" % (macro, value) in hdr
    assert _native.PRED_MAX_SPECS >= 64 + 8
    src = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_predict.hip.h")).read()
    assert "kMaxSpecs = %d" % _native.PRED_MAX_SPECS in src and "kMaxSamples = %d" % _native.PRED_MAX_SAMPLES in src
    assert "mbb_predict.hip.h" in open(os.path.join(ROOT, "mbb_emcee_amd", "build.py")).read()
    # the summary's layout is what it was
    assert _native.SUMMARY_COLS == 8 and "#define MBB_SUMMARY_COLS 8" in hdr
    assert "constexpr int kCols = 8;" in open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_chain_view.hip.h")).read()


# ---------------------------------------------------------------- the numpy reference against the reference's own columns
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_reference_columns_vs_golden(oracle, g_res, g_pb, wheel, name, opthin, noalpha):
    """tests/_predict_ref.py's column (oracle SED x samples) against results.npz's reference-made predict/* columns at
    1e-12, from the reference-made passband tables and from the package's own sample lists; then numpy's statistics of
    that column are what _parcen_internal makes of the fixture's."""
    from mbb_emcee_amd import predict
    k = name + "/"
    chain = g_res[k + "chain"]
    like = _Like(wheel)
    for b in [str(b) for b in g_res["pred_bands"]]:
        want = g_res[k + "predict/" + b]
        got = PR.column(oracle, chain, PR.band_samples(*golden_bands(g_pb, [b])[0]), opthin, noalpha)
        assert np.abs(got / want - 1.0).max() < 1e-12, (b, np.abs(got / want - 1.0).max())
        off, f, w = predict.sample_lists(like, [b])
        own = PR.column(oracle, chain, (f, w), opthin, noalpha)
        assert np.abs(own / want - 1.0).max() < 1e-12, (b, np.abs(own / want - 1.0).max())
    for wv in [float(w) for w in g_res["pred_waves"]]:
        want = g_res[k + "predict/%g" % wv]
        off, f, w = predict.sample_lists(like, [wv])
        assert np.array_equal(f, PR.wave_samples(wv)[0]) and np.array_equal(w, PR.wave_samples(wv)[1])
        got = PR.column(oracle, chain, (f, w), opthin, noalpha)
        assert np.abs(got / want - 1.0).max() < 1e-12, (wv, np.abs(got / want - 1.0).max())
        col = PR.windowed_column(got)
        cen = PR.predflux_cen(col, 68.3)
        ref = PR.predflux_cen(PR.windowed_column(want), 68.3)
        assert np.allclose(cen, ref, rtol=0, atol=4e-12 * np.abs(want).max())
        st = PR.stats(col, [15.85, 84.15])
        assert st["n"] == 512 and st["mean"] == cen[0] and st["pct"][1] - st["mean"] == cen[1]
