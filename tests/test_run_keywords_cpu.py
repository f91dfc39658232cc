"""The analysis keywords of ``DeviceEnsembleSampler.run_mcmc`` -- predict, loo, goodness, evidence, marginals, draws,
convergence and summary -- held to one set of rules on a sampler whose device is faked: what a run with
storechain=False needs, which of the summary's keywords a request inherits, which keywords it refuses, what a sharded
run says, and which refusal comes first when two apply.  The messages below are written out as run_mcmc has always
given them; none is built by the code under test.
"""
import numpy as np
import pytest

ANALYSES = ("predict", "loo", "goodness", "evidence", "marginals", "draws", "convergence")
KEYWORDS = ANALYSES + ("summary",)

# the smallest value that asks for the analysis
ASK = {"predict": 70.0, "loo": True, "goodness": True, "evidence": True, "marginals": True, "draws": 4,
       "convergence": True, "summary": True}

STORECHAIN = {k: k + "= with storechain=False needs summary= too: a run that neither stores nor summarises its chain "
              "keeps none on the device" for k in ANALYSES}

SHARDED = {
    "convergence": "a sharded sampler run cannot be diagnosed on the device: a rank holds only its own walkers' chain",
    "marginals": "a sharded sampler run cannot be binned on the device: a rank holds only its own walkers' chain",
    "predict": "a sharded sampler run cannot be predicted from on the device: a rank holds only its own walkers' chain",
    "loo": "a sharded sampler run cannot be cross-validated on the device: a rank holds only its own walkers' chain",
    "goodness": "a sharded sampler run cannot be tested for goodness of fit on the device: a rank holds only its own "
                "walkers' chain",
    "evidence": "a sharded sampler run cannot be bridged to an evidence on the device: a rank holds only its own "
                "walkers' chain",
    "draws": "a sharded sampler run cannot be drawn from on the device: a rank holds only its own walkers' chain",
    "summary": "a sharded sampler run cannot be summarised on the device: a rank holds only its own walkers' chain",
}
# the order in which a sharded run's refusals are tried
SHARDED_ORDER = ("convergence", "marginals", "predict", "loo", "goodness", "evidence", "draws", "summary")

# an unknown keyword: the four analyses with a list of their own name it, the others leave it to the call
UNKNOWN = {"predict": "predict= got unexpected keyword(s) ['bogus']", "loo": "loo= got unexpected keyword(s) ['bogus']",
           "goodness": "goodness= got unexpected keyword(s) ['bogus']",
           "evidence": "evidence= got unexpected keyword(s) ['bogus']",
           "marginals": "unexpected keyword argument 'bogus'", "draws": "unexpected keyword argument 'bogus'",
           "convergence": "unexpected keyword argument 'bogus'", "summary": "unexpected keyword argument 'bogus'"}

TOUCHED = "the device was touched"


class _Like(object):
    """Stands where a likelihood would: it has data, limits and priors, and touching the device is an error."""
    data_read = True
    nsources = 1
    opthin = noalpha = False
    wavenorm = 500.0
    response_integrate = False

    def __init__(self):
        self._ndata = 3
        self._flux = np.array([10.0, 20.0, 30.0])
        self.data_flux_unc = np.array([1.0, 2.0, 4.0])
        self._lowlim = np.array([1, 0.1, 1, 0.1, 1e-3])
        self._has_uplim = [False, True, False, True, False, False]
        self._uplim = np.array([np.inf, 20.0, np.inf, 20.0, np.inf, np.inf])
        self._has_gprior = [False] * 6
        self._gprior_mean, self._gprior_sigma = np.zeros(6), np.ones(6)

    def _sync_device(self):
        raise AssertionError(TOUCHED)

    context = property(_sync_device)


class _Ctx(object):
    """A context of ``nranks`` ranks whose library is not there."""
    xchg_barrier = None

    def __init__(self, nranks):
        self.nranks = nranks

    def info(self, name):
        return self.nranks if name == "nranks" else 0

    @property
    def lib(self):
        raise AssertionError(TOUCHED)


def _bare_sampler(nranks=None):
    """A sampler without a device: _handle raises, or with ``nranks`` hands out a stand-in context."""
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary, s.seed, s._last = 10, 5, _Like(), None, None, 5, None

    def handle():
        if nranks is None:
            raise AssertionError(TOUCHED)
        return _Ctx(nranks), None
    s._handle = handle
    return s


def _as_dict(key, **more):
    """The keyword's value as a dict with ``more`` in it."""
    base = {"predict": dict(specs=70.0), "draws": dict(n=4)}.get(key, {})
    return dict(base, **more)


P0 = np.zeros((10, 5))


@pytest.mark.parametrize("key", KEYWORDS)
def test_storechain_false_needs_summary(key):
    s = _bare_sampler()
    if key == "summary":
        # a summary is what keeps the chain of such a run on the device: nothing is refused, the device is next
        with pytest.raises(AssertionError, match=TOUCHED):
            s.run_mcmc(P0, 16, storechain=False, summary=True)
        return
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, storechain=False, **{key: ASK[key]})
    assert str(e.value) == STORECHAIN[key]
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, storechain=False, summary=False, **{key: ASK[key]})
    assert str(e.value) == STORECHAIN[key]
    with pytest.raises(AssertionError, match=TOUCHED):                    # with a summary the run itself is next
        s.run_mcmc(P0, 16, storechain=False, summary=True, **{key: ASK[key]})
    for off in (None, False):                                             # (neither asks for the analysis)
        with pytest.raises(AssertionError, match=TOUCHED):
            s.run_mcmc(P0, 16, storechain=False, **{key: off})


@pytest.mark.parametrize("key", KEYWORDS)
def test_burn_of_the_summary_is_inherited(key):
    if key == "summary":
        # the summary's own request is made once the context is known
        s = _bare_sampler(nranks=1)
        with pytest.raises(ValueError) as e:
            s.run_mcmc(P0, 16, summary=dict(burn=16))
        assert str(e.value) == "burn leaves no step of the chain"
        return
    s = _bare_sampler()
    with pytest.raises(ValueError) as e:                                  # the request's own burn
        s.run_mcmc(P0, 16, **{key: _as_dict(key, burn=16)})
    assert str(e.value) == "burn leaves no step of the chain"
    if key == "convergence":
        # a diagnosis has its own burn and takes nothing from the summary's keywords
        with pytest.raises(AssertionError, match=TOUCHED):
            s.run_mcmc(P0, 16, summary=dict(burn=16), convergence=True)
        return
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, summary=dict(burn=16), **{key: ASK[key]})
    assert str(e.value) == "burn leaves no step of the chain"
    with pytest.raises(AssertionError, match=TOUCHED):                    # the request's own keyword wins
        s.run_mcmc(P0, 16, summary=dict(burn=16), **{key: _as_dict(key, burn=14)})   # (an evidence needs two kept steps)
    with pytest.raises(AssertionError, match=TOUCHED):                    # summary=True has nothing to hand on
        s.run_mcmc(P0, 16, summary=True, **{key: ASK[key]})


@pytest.mark.parametrize("key", KEYWORDS)
def test_unknown_keyword_is_refused(key):
    s = _bare_sampler(nranks=1 if key == "summary" else None)
    with pytest.raises(TypeError) as e:
        s.run_mcmc(P0, 16, **{key: _as_dict(key, bogus=1)})
    if key in ("predict", "loo", "goodness", "evidence"):
        assert str(e.value) == UNKNOWN[key]
    else:
        assert UNKNOWN[key] in str(e.value)


def test_refusals_of_a_keyword_of_their_own():
    s = _bare_sampler()
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, predict=dict(burn=2))
    assert str(e.value) == "predict= needs specs: wavelengths in um and / or passband names"
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, evidence=dict(neff="some"))
    assert str(e.value) == "neff must be 'auto', None, a number or one number per source"


@pytest.mark.parametrize("key", KEYWORDS)
def test_sharded_run_is_refused_with_the_analysis_verb(key):
    s = _bare_sampler(nranks=2)
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, **{key: ASK[key]})
    assert str(e.value) == SHARDED[key]
    # the one-hop exchange shards a run too, whatever the communicator says
    s = _bare_sampler(nranks=1)
    ctx = _Ctx(1)
    ctx.xchg_barrier = lambda: None
    s._handle = lambda: (ctx, None)
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, **{key: ASK[key]})
    assert str(e.value) == SHARDED[key]


@pytest.mark.parametrize("a,b", [(a, b) for i, a in enumerate(KEYWORDS) for b in KEYWORDS[i + 1:]])
def test_first_sharded_refusal_of_two(a, b):
    s = _bare_sampler(nranks=2)
    first = min((a, b), key=SHARDED_ORDER.index)
    with pytest.raises(ValueError) as e:
        s.run_mcmc(P0, 16, **{a: ASK[a], b: ASK[b]})
    assert str(e.value) == SHARDED[first]


def test_request_refusals_come_in_their_order():
    """Two requests that are both refused before the device: the one tried first speaks -- predict, loo, goodness,
    evidence, marginals, draws, convergence."""
    s = _bare_sampler()
    for i, a in enumerate(ANALYSES):
        for b in ANALYSES[i + 1:]:
            with pytest.raises(ValueError) as e:
                s.run_mcmc(P0, 16, storechain=False, **{a: ASK[a], b: _as_dict(b, burn=16)})
            assert str(e.value) == STORECHAIN[a]
            with pytest.raises(ValueError) as e:
                s.run_mcmc(P0, 16, storechain=False, **{a: _as_dict(a, burn=16), b: ASK[b]})
            assert str(e.value) == STORECHAIN[a]


def test_results_are_cleared_before_anything_is_checked():
    s = _bare_sampler()
    names = ("convergence_", "marginals_", "predictions_", "draws_", "goodness_", "evidence_", "loo_")
    for n in names:
        setattr(s, n, None if n == "predictions_" else "held")
    with pytest.raises(ValueError):
        s.run_mcmc(P0, 16, storechain=False, loo=True)
    assert all(getattr(s, n) is None for n in names)
