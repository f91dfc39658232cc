"""The population hyper-likelihood on the GPU (csrc/mbb_population.hip.h and mbb_popsteps.hip.h through
mbb_*_population_build / mbb_population_eval and mbb_emcee_amd/population.py) against tests/_population_ref.py.

Tolerances, and where they come from:
  * lnl_src, ess, mean, cov (and the totals lnl): against the longdouble restatement, by _population_ref.distance
    (|a - b| / max(1, |b|)), within 64 x the largest distance of the float64 restatement from the longdouble one over
    this file's accuracy cases, computed here on the CPU from the restatement alone (the loo tests' recipe: the factor
    covers the device's lane-, wave- and split-ordered merges, a reciprocal in the place of a division, and an exp / log
    within 2 ulp that is not correctly rounded); the bound is asserted < 1e-9;
  * n_used, n_left_out, status, n_src_used, cand_status and everything said to be "the same bits": exact.
The chains are made in numpy; the likelihood needs no photometry: a population reads its limits and priors alone.
Sizes: the evaluation kernel's workgroup is 256 entries wide (waves of 64), a split seam lies at 8192 entries, its
candidate tile is 8 (4 with moments, 2 with moments from d = 4 on)."""
import ctypes as C

import numpy as np
import pytest

from conftest import parity_record
import _population_ref as PR

pytestmark = pytest.mark.gpu

LD = PR.LD
TILE = 8
KEYS = PR.FLOATS + ("lnl",)


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _like(mbb, walls=True):
    """A likelihood without photometry; with an upper limit on T inside the chains' range and a Gaussian prior on beta."""
    like = mbb.likelihood()
    if walls:
        like.set_uplim("T", 27.0)
        like.set_gaussian_prior("beta", 1.8, 0.5)
    return like


def _chain(seed, nsrc, nw, nsteps, scales=None):
    rng = np.random.RandomState(seed)
    cen = np.column_stack([rng.uniform(20, 30, nsrc), rng.uniform(1.2, 2.4, nsrc), rng.uniform(150, 300, nsrc),
                           rng.uniform(2, 4, nsrc), rng.uniform(5, 50, nsrc)])
    wid = np.array([3.0, 0.3, 20.0, 0.4, 0.2])
    c = cen[:, None, None, :] + wid * rng.standard_normal((nsrc, nw, nsteps, 5))
    c[..., 4] = cen[:, None, None, 4] * np.exp(wid[4] * rng.standard_normal((nsrc, nw, nsteps)))
    c[..., 0] = np.maximum(c[..., 0], 2.0); c[..., 1] = np.maximum(c[..., 1], 0.2)
    if scales is not None:
        c[..., 4] *= np.asarray(scales)[:, None, None]
    return np.ascontiguousarray(c)


def _cands(seed, xb, H):
    """H candidates about the pooled entries: the pooled mean shifted, the pooled covariance scaled and turned."""
    rng = np.random.RandomState(seed)
    x = np.concatenate([np.asarray(x[b > -np.inf], dtype=np.float64) for x, b in xb])
    d = x.shape[1]
    mean, sd = x.mean(axis=0), x.std(axis=0) + 1e-3
    out = []
    for _ in range(H):
        A = np.eye(d) + 0.3 * np.tril(rng.standard_normal((d, d)), -1)
        L = (A * sd[:, None]) * rng.uniform(0.6, 2.5)
        out.append((mean + sd * rng.uniform(-1, 1, d), L))
    return out


def _entries(like, chain4, cols, tr, burn, thin, dt):
    prior = PR.like_prior(like)
    return [PR.entries(PR.window(c, burn, thin), cols, tr, prior, dt) for c in chain4]


def _device(pop, cands, moments=True):
    mu = np.array([c[0] for c in cands]); L = np.array([c[1] for c in cands])
    return pop.evaluate(mu, chol=L, moments=moments)


def _as_ref(ev, nsrc):
    """A PopulationEval of a multi-source build as _population_ref.evaluate's dict."""
    return dict(lnl=ev.lnl, lnl_src=ev.lnl_source, ess=ev.ess, mean=ev.mean, cov=ev.covariance)


NAMES = {"T": 0, "beta": 1, "lambda0": 2, "alpha": 3, "fnorm": 4}
# label: (nsrc, nw, nsteps, burn, thin, columns, transforms, H)
CASES = {
    "n 1": (1, 1, 1, 0, 1, ("T",), (None,), 1),
    "n 63 burned and thinned": (3, 7, 27, 2, 3, ("T", "beta"), (None, None), 2),
    "n 64": (3, 8, 8, 0, 1, ("T", "beta", "fnorm"), ("log10", None, "log10"), TILE - 1),
    "n 65 d 5": (1, 5, 13, 0, 1, ("T", "beta", "lambda0", "alpha", "fnorm"), ("log10", None, None, None, "log10"), TILE),
    "n 5 one kept step": (3, 5, 10, 9, 1, ("beta", "T"), (None, "log10"), 2),
    "n 255": (3, 15, 17, 0, 1, ("beta", "T"), (None, "log10"), TILE + 1),
    "n 256": (1, 16, 16, 0, 1, ("fnorm",), ("log10",), TILE),
    "n 257": (3, 1, 257, 0, 1, ("alpha", "T", "beta"), (None, None, None), 2),
    "n 8193 beyond the split seam": (3, 3, 2731, 0, 1, ("T", "beta"), (None, None), TILE + 1),
    "n 8193 d 5": (1, 3, 2731, 0, 1, ("fnorm", "alpha", "lambda0", "beta", "T"), ("log10", None, "log10", None, None), 1),
    "256 sources": (256, 8, 8, 0, 1, ("T", "beta"), (None, None), 2),
}


@pytest.fixture(scope="module")
def cases(mbb):
    """Every accuracy case once: the device's tables, the two restatements, and the build's outputs."""
    out = {}
    for k, (label, (nsrc, nw, nsteps, burn, thin, names, tr, H)) in enumerate(CASES.items()):
        like = _like(mbb)
        chain = _chain(100 + k, nsrc, nw, nsteps)
        cols = [NAMES[n] for n in names]
        trn = [PR.LOG10 if t == "log10" else PR.IDENTITY for t in tr]
        xb64 = _entries(like, chain, cols, trn, burn, thin, np.float64)
        xbld = _entries(like, chain, cols, trn, burn, thin, LD)
        cands = _cands(200 + k, xb64, H)
        pop = mbb.chain_population(like, chain, names, tr, burn, thin)
        dev = _device(pop, cands)
        plain = _device(pop, cands, moments=False)
        out[label] = dict(pop=pop, dev=dev, plain=plain, ref=PR.evaluate(xbld, cands, LD), f64=PR.evaluate(xb64, cands, np.float64),
                          xb=xbld, chain=chain, like=like, cands=cands, n=nw * len(range(burn, nsteps, thin)))
        pop.close()
    return out


@pytest.fixture(scope="module")
def bound(cases):
    """64 x the largest distance of the float64 restatement from the longdouble one over every case of this file."""
    spread = max(PR.distance(c["f64"], c["ref"], KEYS) for c in cases.values())
    print("    float64 restatement vs longdouble over %d cases: %.3g; bound %.3g" % (len(cases), spread, 64.0 * spread))
    parity_record("population float64 restatement vs longdouble", spread, 1e-9 / 64.0)
    assert 0.0 < 64.0 * spread < 1e-9
    return 64.0 * spread


@pytest.mark.parametrize("label", list(CASES))
def test_against_longdouble(cases, bound, label):
    c = cases[label]
    nsrc = CASES[label][0]
    pop, dev, ref = c["pop"], c["dev"], c["ref"]
    assert pop.n_used.shape == (nsrc,) and pop.d == len(CASES[label][5])
    used = np.array([int((b > -np.inf).sum()) for _, b in c["xb"]])
    assert np.array_equal(pop.n_used, used) and np.array_equal(pop.n_left_out, c["n"] - used)
    assert np.array_equal(pop.status, np.where(used == 0, 1, 0) | np.where(used < c["n"], 2, 0))
    assert np.all(used == c["n"]) and pop.nsteps_used * pop.nwalkers == c["n"]
    assert np.array_equal(dev.n_sources_used, ref["n_src_used"]) and not dev.status.any()
    # entries on both sides of T's wall, where T is a column
    if "T" in CASES[label][5] and c["n"] > 60:
        T = c["chain"][..., 0]
        assert (T > 27.0).any() and (T < 27.0).any()
    d = PR.distance(_as_ref(dev, nsrc), ref, KEYS)
    print("    %s: device vs longdouble %.3g (bound %.3g)" % (label, d, bound))
    parity_record("population tables vs longdouble [max(1, |x|)]", d, bound)
    assert d <= bound
    # without moments: the tables of another tile size, held the same way
    p = c["plain"]
    assert p.mean is None and p.covariance is None
    d = PR.distance(dict(lnl=p.lnl, lnl_src=p.lnl_source, ess=p.ess), ref, ("lnl", "lnl_src", "ess"))
    parity_record("population tables vs longdouble [max(1, |x|)]", d, bound)
    assert d <= bound
    assert np.all(np.isfinite(dev.lnl)) and np.all(dev.ess >= 1.0 - 1e-12) and np.all(dev.ess <= c["n"] * (1 + 1e-12))


def _bits(a, b, fields=("lnl", "lnl_source", "ess", "mean", "covariance", "status", "n_sources_used")):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if x is None and y is None:
            continue
        if not np.array_equal(x, y, equal_nan=True):
            return f
    return True


def _pick(ev, h):
    """Candidate h of a PopulationEval as arrays with a leading axis of one."""
    class One(object):
        pass
    o = One()
    for f in ("lnl", "lnl_source", "ess", "mean", "covariance", "status", "n_sources_used"):
        v = getattr(ev, f)
        setattr(o, f, None if v is None else v[h:h + 1])
    return o


@pytest.mark.parametrize("moments", [False, True])
def test_candidates_bit_for_bit(mbb, moments):
    """Every candidate of a call of tile + 3 equals the call with that candidate alone, and in another position."""
    like = _like(mbb)
    chain = _chain(7, 3, 4, 75)                                   # n = 300: two lanes' strides, a ragged last one
    names, tr = ("T", "beta", "fnorm"), ("log10", None, "log10")
    pop = mbb.chain_population(like, chain, names, tr)
    H = TILE + 3
    cands = _cands(8, _entries(like, chain, [0, 1, 4], [1, 0, 1], 0, 1, np.float64), H)
    whole = _device(pop, cands, moments)
    assert np.all(np.isfinite(whole.lnl))
    for h in range(H):
        assert _bits(_device(pop, [cands[h]], moments), _pick(whole, h)) is True, h
    order = list(np.random.RandomState(1).permutation(H))
    turned = _device(pop, [cands[h] for h in order], moments)
    for k, h in enumerate(order):
        assert _bits(_pick(turned, k), _pick(whole, h)) is True, (k, h)
    twice = _device(pop, [cands[3], cands[0], cands[3]], moments)
    assert _bits(_pick(twice, 0), _pick(twice, 2)) is True and _bits(_pick(twice, 0), _pick(whole, 3)) is True


def test_sources_bit_for_bit_and_a_smaller_build_after_a_larger(mbb):
    """Every source of a three-source build (scales 1, 1e-3, 1e4 on fnorm) equals its own one-source build; a smaller
    build and call after a larger one in the same context gives what it gave before."""
    like = _like(mbb)
    chain = _chain(9, 3, 6, 50, scales=(1.0, 1e-3, 1e4))
    names, tr = ("T", "fnorm"), (None, "log10")
    cands = _cands(10, _entries(like, chain[:1], [0, 4], [0, 1], 5, 2, np.float64), 5)
    three = _device(mbb.chain_population(like, chain, names, tr, 5, 2), cands)
    ones = []
    for s in range(3):
        pop = mbb.chain_population(like, chain[s], names, tr, 5, 2)
        assert pop.n_used.shape == () and pop.n_used == 6 * 23
        one = _device(pop, cands)
        ones.append(one)
        assert one.lnl_source.shape == (5,) and one.mean.shape == (5, 2) and one.covariance.shape == (5, 2, 2)
        for f in ("lnl_source", "ess", "mean", "covariance"):
            assert np.array_equal(getattr(one, f), getattr(three, f)[:, s], equal_nan=True), (s, f)
        assert np.array_equal(one.lnl, one.lnl_source)
    # the total is the sum in source order
    assert np.array_equal(three.lnl, (ones[0].lnl + ones[1].lnl) + ones[2].lnl)
    # a larger build (more sources, more entries, more columns, more candidates), then the small one again
    big = _chain(11, 5, 3, 2800)
    bp = mbb.chain_population(like, big, ("T", "beta", "lambda0", "alpha", "fnorm"))
    _device(bp, _cands(12, _entries(like, big, [0, 1, 2, 3, 4], [0] * 5, 0, 1, np.float64), 70))
    small = mbb.chain_population(like, chain[2], names, tr, 5, 2)
    assert small.serial > bp.serial
    assert _bits(_device(small, cands), ones[2]) is True
    with pytest.raises(RuntimeError, match="a later build replaced it"):
        bp.lnlike(np.zeros(5), cov=np.eye(5))
    small.close()
    with pytest.raises(RuntimeError, match="closed"):
        small.lnlike(cands[0][0], chol=cands[0][1])


def test_planted_cells(mbb, bound):
    """NaN, +-inf and theta <= 0 under log10 at the ends of the entries, of a wave, of the workgroup and of a split; a
    source of NaN rows only; the counts exact, the tables against the restatement."""
    like = _like(mbb)
    chain = _chain(13, 3, 1, 8193)
    spots = [0, 1, 62, 63, 64, 65, 254, 255, 256, 257, 4095, 4096, 4097, 8190, 8191, 8192]
    bad = [np.nan, np.inf, -np.inf, 0.0, -3.0]
    for k, j in enumerate(spots):
        chain[0, 0, j, (0, 4)[k % 2]] = bad[k % 5]                # T (identity) or fnorm (log10)
    chain[0, 0, 300, 1] = np.nan                                  # (beta is not a column: the entry is used)
    chain[1] = np.nan
    names, tr = ("T", "fnorm"), (None, "log10")
    pop = mbb.chain_population(like, chain, names, tr)
    xb = _entries(like, chain, [0, 4], [0, 1], 0, 1, LD)
    # (T = 0 and T = -3 are finite identity values: used)
    left0 = sum(1 for k, j in enumerate(spots) if not (k % 2 == 0 and bad[k % 5] in (0.0, -3.0)))
    assert np.array_equal(pop.n_left_out, [left0, 8193, 0]) and np.array_equal(pop.n_used, [8193 - left0, 0, 8193])
    assert np.array_equal(pop.n_used, [int((b > -np.inf).sum()) for _, b in xb])
    assert np.array_equal(pop.status, [pop.HAS_NAN, pop.EMPTY | pop.HAS_NAN, 0])
    cands = _cands(14, _entries(like, chain[2:], [0, 4], [0, 1], 0, 1, np.float64), 3)
    dev, ref = _device(pop, cands), PR.evaluate(xb, cands, LD)
    assert np.all(np.isnan(dev.lnl_source[:, 1])) and np.all(np.isnan(dev.ess[:, 1])) and np.all(np.isnan(dev.mean[:, 1]))
    assert np.array_equal(dev.n_sources_used, [2, 2, 2]) and np.array_equal(dev.status, [dev.HAS_EMPTY] * 3)
    assert np.array_equal(dev.lnl, dev.lnl_source[:, 0] + dev.lnl_source[:, 2])
    d = PR.distance(_as_ref(dev, 3), ref, KEYS)
    parity_record("population tables vs longdouble [max(1, |x|)]", d, bound)
    assert d <= bound
    # the source without planted cells is what it is alone
    alone = _device(mbb.chain_population(like, chain[2], names, tr), cands)
    assert np.array_equal(alone.lnl_source, dev.lnl_source[:, 2]) and np.array_equal(alone.covariance, dev.covariance[:, 2])


def test_far_and_bad_candidates(mbb):
    """A candidate 1e4 sigma from every entry: -inf and the underflow bit; bad candidates (NaN, L_ii = 0, L_ii < 0): NaN
    and the bad bit; their neighbours in the call are untouched."""
    like = _like(mbb)
    chain = _chain(15, 3, 4, 40)
    pop = mbb.chain_population(like, chain, ("T", "beta"))
    good = _cands(16, _entries(like, chain, [0, 1], [0, 0], 0, 1, np.float64), 4)
    ref = _device(pop, good)
    mu, L = good[0]
    sig = np.sqrt(np.sum(L * L, axis=1))
    far = (mu + 1e4 * sig * np.array([1.0, 0.0]), L)
    nanmu = (np.array([np.nan, mu[1]]), L)
    Lz, Ln, Li = L.copy(), L.copy(), L.copy()
    Lz[1, 1], Ln[0, 0], Li[1, 0] = 0.0, -L[0, 0], np.inf
    mix = [good[0], far, good[1], nanmu, (mu, Lz), good[2], (mu, Ln), (mu, Li), good[3]]
    dev = _device(pop, mix)
    for k, h in ((0, 0), (2, 1), (5, 2), (8, 3)):
        assert _bits(_pick(dev, k), _pick(ref, h)) is True, k
    assert dev.lnl[1] == -np.inf and np.all(dev.lnl_source[1] == -np.inf) and dev.status[1] == dev.UNDERFLOW
    assert np.all(np.isnan(dev.ess[1])) and np.all(np.isnan(dev.mean[1])) and dev.n_sources_used[1] == 3
    for k in (3, 4, 6, 7):
        assert dev.status[k] == dev.BAD and np.isnan(dev.lnl[k]) and np.all(np.isnan(dev.lnl_source[k])), k
        assert np.all(np.isnan(dev.ess[k])) and np.all(np.isnan(dev.covariance[k])) and dev.n_sources_used[k] == 0
    # a covariance that is not positive definite is a bad candidate, not an exception
    ev = pop.evaluate(np.array([mu, mu]), cov=np.array([L @ L.T, -np.eye(2)]))
    assert ev.status[1] == ev.BAD and np.isnan(ev.lnl[1]) and ev.lnl[0] == ref.lnl[0]
    assert np.all(ev.mass_below[0] >= 0) and np.all(ev.mass_below[0] < 0.5) and np.all(np.isnan(ev.mass_below[1]))
    # source_means: the interim prior divided out, no population imposed
    sm = pop.source_means()
    xb = _entries(like, chain, [0, 1], [0, 0], 0, 1, LD)
    for s, (x, b) in enumerate(xb):
        w = np.exp(b - b.max())
        assert np.allclose(sm[s], np.asarray((w[:, None] * x).sum(axis=0) / w.sum(), dtype=np.float64), rtol=1e-9)


# ---------------------------------------------------------------- through the stack
NW, NSTEPS = 34, 40


def _sampler_case(mbb, g_lnl):
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rng = np.random.RandomState(11)
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    ns = 3
    truths = np.column_stack([rng.uniform(8, 20, ns), rng.uniform(1.2, 2.4, ns), rng.uniform(300, 900, ns),
                              rng.uniform(2, 4.5, ns), rng.uniform(10, 80, ns)])
    flux = one.model_flux(truths)
    lk = mbb.likelihood(response=True)
    lk.set_phot_multi(bands, flux, 0.1 * flux + 1.0)
    lk.set_gaussian_prior("beta", 1.8, 0.4)
    p0 = truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, NW, 5)))
    return lk, p0, bands


CANDS = (np.array([[14.0, 1.8], [12.0, 2.0], [1.2, 1.5]]), np.array([[[4.0, 0.0], [0.1, 0.4]]] * 2 + [[[0.2, 0.0], [0.0, 0.3]]]))


def test_resident_chain(mbb, g_lnl):
    """sampler.population(), run_mcmc(storechain=False, summary=, population=) equal chain_population of the chain a
    storechain=True run of the same seed brings back, bit for bit; the run's other analyses are what they are without."""
    lk, p0, bands = _sampler_case(mbb, g_lnl)
    a = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.population_ is None
    kw = dict(columns=("T", "beta"), burn=5, thin=2)
    host = mbb.chain_population(lk, a.chain, **kw).evaluate(CANDS[0][:2], chol=CANDS[1][:2], moments=True)
    pop = a.population(**kw)
    assert pop.nsteps_used == 18 and pop.nwalkers == NW and np.array_equal(pop.n_used, [NW * 18] * 3)
    assert _bits(pop.evaluate(CANDS[0][:2], chol=CANDS[1][:2], moments=True), host) is True
    logs = a.population(columns=("T", "beta"), transform=("log10", None), burn=5, thin=2)
    assert _bits(logs.evaluate(CANDS[0][2:], chol=CANDS[1][2:], moments=True),
                 mbb.chain_population(lk, a.chain, ("T", "beta"), ("log10", None), 5, 2).evaluate(
                     CANDS[0][2:], chol=CANDS[1][2:], moments=True)) is True
    skw = dict(burn=5, thin=2, percentile=(68.3, 95.4))
    others = dict(summary=dict(skw), convergence=True, marginals=dict(bins=24, bins2d=6), predict=[bands[3], 70.0], draws=9,
                  goodness=True, evidence=dict(n2=256), loo=True)
    b = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b.run_mcmc(p0, NSTEPS, storechain=False, population=dict(columns=("T", "beta")), **others)
    assert b.chain.shape[-2] == 0 and b.population_.burn == 5 and b.population_.thin == 2     # (the summary's window)
    assert _bits(b.population_.evaluate(CANDS[0][:2], chol=CANDS[1][:2], moments=True), host) is True
    c = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    c.run_mcmc(p0, NSTEPS, storechain=False, **others)
    assert c.population_ is None
    import _summary_ref as SR
    assert SR.raw_equal(b.summary, c.summary)
    for f in ("tau", "ess", "rhat", "window", "status"):
        assert np.array_equal(getattr(b.convergence_, f), getattr(c.convergence_, f), equal_nan=True), f
    for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "status"):
        assert np.array_equal(getattr(b.marginals_._raw, f), getattr(c.marginals_._raw, f), equal_nan=True), f
    for f in ("n_used", "mean", "min", "max", "pct", "status"):
        assert np.array_equal(getattr(b.predictions_._raw, f), getattr(c.predictions_._raw, f), equal_nan=True), f
    for name in ("draws_", "goodness_", "evidence_", "loo_"):
        for k, v in getattr(c, name).arrays().items():
            assert np.array_equal(getattr(b, name).arrays()[k], v, equal_nan=True), (name, k)
    # the analyses after an evaluation, and the block after them
    assert np.array_equal(b.goodness(burn=5, thin=2).chisq_mean, c.goodness(burn=5, thin=2).chisq_mean)
    assert _bits(b.population_.evaluate(CANDS[0][:2], chol=CANDS[1][:2], moments=True), host) is True
    b.run_mcmc(None, 3, storechain=False)
    assert b.population_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.population()
    b.reset()
    assert b.population_ is None


def test_fitter_population(mbb, g_lnl):
    """mbb_fitter.run(..., population=...) and mbb_fitter.population(): the block is of the chain the fit returns."""
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    flux = one.model_flux(truth)[0]
    fit = mbb.mbb_fitter(nwalkers=NW, response=True, seed=3)
    fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    fit.run(20, NSTEPS, p0, population=True)
    mu, L = CANDS[0][0], CANDS[1][0]
    assert fit.population_ is not None and fit.population_.columns == ["T", "beta"]
    want = mbb.chain_population(fit.like, fit.sampler.chain).evaluate(mu, chol=L, moments=True)
    assert np.ndim(want.lnl) == 0 and want.mean.shape == (2,)
    assert _bits(fit.sampler.population().evaluate(mu, chol=L, moments=True), want) is True
    fit.run(20, 16, p0, population=dict(columns=("T",), burn=2), summary=True)
    got = fit.population_.evaluate(mu[:1], chol=L[:1, :1])
    assert _bits(got, mbb.chain_population(fit.like, fit.sampler.chain, ("T",), burn=2).evaluate(mu[:1], chol=L[:1, :1])) is True
    assert _bits(fit.population(columns=("T",), burn=2).evaluate(mu[:1], chol=L[:1, :1]), got) is True
    fit.run(20, 16, p0)
    assert fit.population_ is None


def test_sample(mbb):
    """Population.sample, 8 walkers x 40 steps over (mu, ln sigma) of T on 8 sources: every stored lnprob is the bits of
    lnlike at that position plus the prior (0 inside the default region); the chain is reproducible by seed."""
    like = _like(mbb, walls=False)
    chain = _chain(17, 8, 4, 64)
    pop = mbb.chain_population(like, chain, ("T",))
    fit = pop.sample(nsteps=40, nwalkers=8, nburn=10, seed=5)
    assert fit.chain.shape == (8, 40, 2) and fit.lnprob.shape == (8, 40) and np.all(np.isfinite(fit.lnprob))
    mu, cov = pop.unpack(fit.chain.reshape(-1, 2))
    assert np.array_equal(pop.lnlike(mu, cov), fit.lnprob.ravel())
    L = np.exp(fit.chain.reshape(-1, 2)[:, 1]).reshape(-1, 1, 1)
    assert np.array_equal(pop.lnlike(mu, chol=L), fit.lnprob.ravel())
    assert 0.0 <= fit.ess_low <= 1.0 and fit.acceptance_fraction.shape == (8,) and fit.acceptance_fraction.mean() > 0.1
    lo, hi, s = pop.default_bounds()
    assert np.all(mu >= lo) and np.all(mu <= hi) and np.all(np.sqrt(cov[:, 0, 0]) >= s / 100) and np.all(np.sqrt(cov[:, 0, 0]) <= 100 * s)
    again = pop.sample(nsteps=40, nwalkers=8, nburn=10, seed=5)
    assert np.array_equal(again.chain, fit.chain) and np.array_equal(again.lnprob, fit.lnprob) and again.ess_low == fit.ess_low
    other = pop.sample(nsteps=40, nwalkers=8, nburn=10, seed=6)
    assert not np.array_equal(other.chain, fit.chain)
    # the sampler moved towards where the sources are
    sm = pop.source_means()[:, 0]
    assert abs(fit.mu_cen()[0, 0] - sm.mean()) < 3 * sm.std() and fit.best[2] == fit.lnprob.max()


# ---------------------------------------------------------------- refusals of the C-ABI
def test_native_refusals_leave_the_context_usable(mbb, g_lnl):
    from mbb_emcee_amd import _native, population as P
    like = _like(mbb)
    chain = _chain(19, 2, 4, 16)
    ctx = _native.analysis_context(like)
    hy = np.ascontiguousarray(np.array([[25.0, 1.8, 3.0, 0.05, 0.3]]))

    def build(nsrc=2, nw=4, nsteps=16, edit=None, drop=None, chain_ptr=True, spec_ptr=True, out_ptr=True, h=True):
        req = P._Request(like, ("T", "beta"), burn=2, thin=3)
        spec, raw = req.spec(), P._BuildRaw(2)
        out = raw.out()
        if edit:
            edit(spec)
        if drop:
            setattr(out, drop, None)
        rc = ctx.lib.mbb_chain_population_build(ctx.h if h else None, _native._d(chain) if chain_ptr else None, nsrc, nw, nsteps,
                                                C.byref(spec) if spec_ptr else None, C.byref(out) if out_ptr else None)
        return rc, raw

    def evaluate(serial, H=1, hyper=True, moments=0, drop=None, out_ptr=True):
        arrays = dict(lnl=np.full(max(H, 1), np.nan), n_src_used=np.zeros(max(H, 1), dtype=np.int32),
                      cand_status=np.zeros(max(H, 1), dtype=np.int32), mean=np.zeros((1, 2, 2)), cov=np.zeros((1, 2, 2, 2)))
        if drop:
            arrays.pop(drop)
        out = P._analysis.bind_out(_native.PopulationEvalOut, arrays)
        rc = ctx.lib.mbb_population_eval(ctx.h, serial, _native._d(hy) if hyper else None, H, moments,
                                         C.byref(out) if out_ptr else None)
        return rc, arrays["lnl"] if "lnl" in arrays else None

    rc, first = build()
    assert rc == 0 and np.array_equal(first.n_used, [20, 20])
    rc, want = evaluate(int(first.serial[0]))
    assert rc == 0 and np.isfinite(want[0])
    state = {"serial": int(first.serial[0])}

    def good():
        rc, lnl = evaluate(state["serial"])
        assert rc == 0 and lnl[0] == want[0]

    def msg():
        return ctx.lib.mbb_last_error().decode()

    def sets(**kw):
        def edit(spec):
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(spec, k)[v[0]] = v[1]
                else:
                    setattr(spec, k, v)
        return edit
    # refused builds leave the block and its serial alone
    for kw, text in [(dict(nsteps=0), "empty chain"), (dict(nw=0), "empty chain"), (dict(nsrc=0), "empty chain"),
                     (dict(edit=sets(burn=16)), "burn"), (dict(edit=sets(burn=-1)), "burn"), (dict(edit=sets(thin=0)), "burn"),
                     (dict(edit=sets(d=0)), "1 to 5 columns"), (dict(edit=sets(d=6)), "1 to 5 columns"),
                     (dict(edit=sets(col=(1, 0))), "given twice"), (dict(edit=sets(col=(1, 5))), "unknown population column"),
                     (dict(edit=sets(col=(0, -1))), "unknown population column"),
                     (dict(edit=sets(transform=(1, 2))), "unknown population transform"),
                     (dict(drop="n_used"), "null"), (dict(drop="n_left_out"), "null"), (dict(drop="status"), "null"),
                     (dict(drop="serial"), "null"), (dict(spec_ptr=False), "null"), (dict(out_ptr=False), "null"),
                     (dict(chain_ptr=False), "bad arguments")]:
        rc, _ = build(**kw)
        assert rc == -2 and text in msg(), (kw, rc, msg())
        good()
    assert build(h=False)[0] == -2
    good()
    for kw, text in [(dict(H=0), "1 to MBB_POP_MAX_CAND"), (dict(H=1025), "1 to MBB_POP_MAX_CAND"), (dict(hyper=False), "null"),
                     (dict(out_ptr=False), "null"), (dict(drop="lnl"), "null"), (dict(drop="n_src_used"), "null"),
                     (dict(drop="cand_status"), "null"), (dict(moments=1, drop="mean"), "null"), (dict(moments=1, drop="cov"), "null")]:
        rc, _ = evaluate(state["serial"], **kw)
        assert rc == -2 and text in msg(), (kw, rc, msg())
        good()
    # a serial that is not the current block's
    for serial in (state["serial"] + 1, state["serial"] - 1, 0, -1):
        rc, _ = evaluate(serial)
        assert rc == -3 and "no population block of this serial" in msg()
        good()
    rc, second = build()
    assert rc == 0 and int(second.serial[0]) == state["serial"] + 1
    assert evaluate(state["serial"])[0] == -3
    state["serial"] = int(second.serial[0])
    good()
    assert ctx.lib.mbb_population_drop(ctx.h) == 0
    assert evaluate(state["serial"])[0] == -3 and ctx.lib.mbb_population_drop(ctx.h) == 0 and ctx.lib.mbb_population_drop(None) == -2
    rc, third = build()
    assert rc == 0 and int(third.serial[0]) == state["serial"] + 1
    state["serial"] = int(third.serial[0])
    good()
    # the sampler call: nothing resident, then a run
    lk, p0, _ = _sampler_case(mbb, g_lnl)
    sm = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=5)
    sctx, h = sm._handle()
    req = P._Request(lk, ("T",))
    spec, raw = req.spec(), P._BuildRaw(3)
    out = raw.out()
    assert sctx.lib.mbb_sampler_population_build(sctx.h, h, C.byref(spec), C.byref(out)) == -3
    assert "resident" in sctx.lib.mbb_last_error().decode()
    sm.run_mcmc(p0, 8)
    assert sctx.lib.mbb_sampler_population_build(sctx.h, h, C.byref(spec), C.byref(out)) == 0 and np.array_equal(raw.n_used, [NW * 8] * 3)
    assert sctx.lib.mbb_sampler_population_build(sctx.h, h, None, C.byref(out)) == -2
    assert sctx.lib.mbb_sampler_population_build(sctx.h, h, C.byref(spec), None) == -2
    assert sctx.lib.mbb_sampler_population_build(sctx.h, None, C.byref(spec), C.byref(out)) == -2
    assert sctx.lib.mbb_sampler_population_build(None, h, C.byref(spec), C.byref(out)) == -2
    spec.d = 7
    assert sctx.lib.mbb_sampler_population_build(sctx.h, h, C.byref(spec), C.byref(out)) == -2
    spec.d = 1
    again = P._BuildRaw(3)
    assert sctx.lib.mbb_sampler_population_build(sctx.h, h, C.byref(spec), C.byref(again.out())) == 0
    assert int(again.serial[0]) == int(raw.serial[0]) + 1 and np.array_equal(again.n_used, raw.n_used)
