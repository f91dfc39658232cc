"""Binned marginals on the GPU (csrc/mbb_marginals.hip.h through mbb_chain_marginals / mbb_sampler_marginals and
mbb_emcee_amd/marginals.py) against the numpy restatement of their definition in tests/_marginals_ref.py, which
tests/test_marginals_cpu.py holds to numpy.histogram / numpy.histogram2d.

Everything is held EXACTLY: counts, n_used / n_below / n_above / n_nonfinite and status with array_equal, edges bit
for bit against numpy.linspace's formula.  The one bound is on the derived columns (peak wavelength, L_IR, dust mass),
whose values the device is known to give to 1e-13 of postprocess's and mostly bitwise: there the test first asserts, on
postprocess's values alone, that no sample lies within 1e-9 bin widths of an interior edge (a condition on the seed,
not a tolerance: no sample is excluded), then requires exact counts; with automatic ranges the edges are held to
rtol 1e-13.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT
import _marginals_ref as MR
import _summary_ref as SR

pytestmark = pytest.mark.gpu

PARAM_PAIRS = [(a, b) for a in range(5) for b in range(a + 1, 5)]
_CACHE = {}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


@pytest.fixture(scope="module")
def like(mbb):
    return mbb.likelihood()


def _chain(key, make):
    """A chain made once and shared, read-only."""
    if key not in _CACHE:
        _CACHE[key] = make()
        _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _c4(chain):
    return chain if chain.ndim == 4 else chain[None]


# ---------------------------------------------------------------- held exactly: the five parameter columns
@pytest.mark.parametrize("bins", [1, 64])
def test_fewer_samples_than_a_workgroup_has_threads(mbb, like, bins):
    """1. One source, 7 walkers x 37 steps: 259 samples, and with burn 30 only 49 -- fewer than a workgroup's 256
    threads."""
    chain = _chain("small", lambda: MR.random_chain(1, 7, 37, seed=1)[0])
    for burn in (0, 30):
        got = mbb.chain_marginals(like, chain, bins=bins, bins2d=7, burn=burn)
        assert got.n_used.shape == (8,) and got.hist1d("T")[0].shape == (bins,) and got.hist2d("T", "beta")[0].shape == (7, 7)
        assert np.all(got.n_used[:5] == 7 * (37 - burn)) and got.nsteps_used == 37 - burn and got.nwalkers == 7
        MR.check(got, chain[None], bins, 7, PARAM_PAIRS, burn=burn, multi=False, label="small burn %d" % burn)
    assert str(got).count("range:") == 5


def test_several_splits_no_divisor(mbb, like):
    """2. 33 walkers x 1000 steps with burn=7, thin=3: 10923 samples per column in three splits of 3641, no multiple of
    256; and the unthinned window, 33000 samples in nine splits of 3667 of which the last is short."""
    chain = _chain("splits", lambda: MR.random_chain(1, 33, 1000, seed=2)[0])
    assert 33 * 331 == 10923 and -(-10923 // 4096) == 3 and 3641 % 256 != 0
    assert -(-33000 // 4096) == 9 and 33000 % 9 != 0 and -(-33000 // 9) % 256 != 0
    got = mbb.chain_marginals(like, chain, bins=63, bins2d=7, burn=7, thin=3)
    MR.check(got, chain[None], 63, 7, PARAM_PAIRS, burn=7, thin=3, multi=False, label="splits")
    again = mbb.chain_marginals(like, chain, bins=63, bins2d=7, burn=7, thin=3)
    for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below", "n_above", "n_nonfinite", "status"):
        assert np.array_equal(getattr(got._raw, f), getattr(again._raw, f), equal_nan=True), f   # the same bits every time
    got = mbb.chain_marginals(like, chain, bins=64, range={"T": (20.0, 30.0)})
    MR.check(got, chain[None], 64, ranges={0: (20.0, 30.0)}, multi=False, label="splits, unthinned")


RANGES = {0: (17.0, 33.0), 1: (1.25, 2.375), 2: (250.0, 750.3), 3: (2.0, 4.0), 4: (19.7, 41.1)}


def _planted_chain():
    """Random samples, then in the window (burn 5, thin 2) of every column: every edge of the 64-bin and of the 7-bin
    table on, just under and just over it (first and last included), samples far below and above the range, NaN and
    both infinities; outside the window (odd steps, steps before burn) NaN, infinities and out-of-range values that
    must not count."""
    rng = np.random.RandomState(3)
    chain = MR.random_chain(1, 24, 205, seed=3)[0]
    burn, thin = 5, 2
    kept = np.arange(burn, 205, thin)
    for slot, (lo, hi) in RANGES.items():
        vals = np.concatenate((MR.edge_values(MR.edges(lo, hi, 64)), MR.edge_values(MR.edges(lo, hi, 7)),
                               [lo - 3.0 * (hi - lo), hi + 2.0 * (hi - lo), lo - 1e-9, np.nan, np.inf, -np.inf]))
        cells = rng.choice(24 * kept.size, vals.size, replace=False)
        chain[cells // kept.size, kept[cells % kept.size], slot] = vals
        # outside the window
        out_steps = np.array([0, 1, 4, 6, 8, 204])
        for k, v in enumerate((np.nan, np.inf, -np.inf, lo - 100.0 * (hi - lo), hi + 100.0 * (hi - lo), np.nan)):
            chain[(3 * k + slot) % 24, out_steps[k], slot] = v
    return chain


def test_planted_edge_samples_and_non_finite_cells(mbb, like):
    """3. Samples on, just under and just over every edge with a given range; out-of-range samples on both sides; NaN
    and +-inf cells inside and outside the window -- only those inside count.  The 2-d tables see samples inside one
    column's range and outside the other's."""
    chain = _chain("planted", _planted_chain)
    burn, thin = 5, 2
    names = {MR.NAMES[k]: v for k, v in RANGES.items()}
    got = mbb.chain_marginals(like, chain, bins=64, bins2d=7, burn=burn, thin=thin, range=names)
    MR.check(got, chain[None], 64, 7, PARAM_PAIRS, ranges=RANGES, burn=burn, thin=thin, multi=False, label="planted")
    assert np.all(got.n_nonfinite[:5] == 3) and np.all(got.status[:5] == got.NONFINITE)
    assert np.all(got.n_below[:5] >= 3) and np.all(got.n_above[:5] >= 2)
    assert np.all(got.n_used[:5] + got.n_below[:5] + got.n_above[:5] + got.n_nonfinite[:5] == 24 * 100)
    x, y = MR.column(chain[None], 0, 0, burn, thin), MR.column(chain[None], 0, 1, burn, thin)
    px, py = MR.place(x, MR.edges(*RANGES[0], 7)), MR.place(y, MR.edges(*RANGES[1], 7))
    assert ((px >= 0) & (py < 0)).sum() >= 5 and ((px < 0) & (py >= 0)).sum() >= 5
    assert got.hist2d("T", "beta")[0].sum() == ((px >= 0) & (py >= 0)).sum()
    # the same chain with automatic ranges: the planted extremes are the range
    got = mbb.chain_marginals(like, chain, bins=64, bins2d=7, burn=burn, thin=thin)
    MR.check(got, chain[None], 64, 7, PARAM_PAIRS, burn=burn, thin=thin, multi=False, label="planted, automatic")
    assert np.all(got.n_below[:5] == 0) and np.all(got.n_above[:5] == 0)


@pytest.mark.parametrize("bins", [64, 7])
def test_fixed_parameter(mbb, like, bins):
    """4. A fixed parameter sends every sample -- every lane of every wave -- to one bin: the +-0.5 range; with an
    even number of bins the value sits exactly on an edge."""
    def make():
        chain = MR.random_chain(1, 20, 130, seed=4)[0]
        chain[..., 3] = 2.0
        chain[..., 2] = 500.0
        return chain
    chain = _chain("fixed", make)
    got = mbb.chain_marginals(like, chain, bins=bins, bins2d=8, pairs=[("alpha", "lambda0"), ("T", "alpha")])
    MR.check(got, chain[None], bins, 8, [(2, 3), (0, 3)], multi=False, label="fixed")
    counts, e = got.hist1d("alpha")
    assert (e[0], e[-1]) == (1.5, 2.5) and counts.max() == 20 * 130 and np.count_nonzero(counts) == 1
    if bins % 2 == 0:
        assert e[bins // 2] == 2.0 and counts[bins // 2] == 2600
    i = int(np.argmax(counts))
    assert got.mode("alpha") == 0.5 * (e[i] + e[i + 1])
    H = got.hist2d("lambda0", "alpha")[0]
    assert H[4, 4] == 2600 and H.sum() == 2600 and np.array_equal(got.levels("lambda0", "alpha"), [2600, 2600])


def test_three_sources_of_different_scales(mbb, like):
    """5. Automatic ranges are per source, a given range is shared; every source gets bit for bit what it gets alone."""
    chain = _chain("nsrc3", lambda: MR.random_chain(3, 12, 90, seed=5, scale=[1.0, 1e-3, 250.0]))
    kw = dict(bins=33, bins2d=9, burn=3, thin=2, range={"beta": (0.0, 4.0)})
    got = mbb.chain_marginals(like, chain, **kw)
    assert got.n_used.shape == (3, 8) and got.hist1d("T")[1].shape == (3, 34) and got.hist2d("T", "beta")[0].shape == (3, 9, 9)
    MR.check(got, chain, 33, 9, PARAM_PAIRS, ranges={1: (0.0, 4.0)}, burn=3, thin=2, label="nsrc3")
    e = got.hist1d("T")[1]
    assert e[1, -1] < e[0, 0] < e[0, -1] < e[2, 0]                        # (the sources' own ranges)
    assert np.all(got.hist1d("beta")[1][:, 0] == 0.0) and got.n_below[1, 1] == 0 and got.n_above[2, 1] > 0
    for s in range(3):
        one = mbb.chain_marginals(like, chain[s], **kw)
        for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below", "n_above", "n_nonfinite", "status"):
            assert np.array_equal(getattr(got._raw, f)[s], getattr(one._raw, f)[0], equal_nan=True), (s, f)
    assert np.array_equal(got.levels("T", "beta")[1], MR.levels_direct(got.hist2d("T", "beta")[0][1], (0.683, 0.954)))
    pdf, edges = got.pdf1d("fnorm")
    for s in range(3):
        x = MR.column(chain, s, 4, 3, 2)
        assert np.array_equal(pdf[s], np.histogram(x, bins=33, density=True)[0])


def test_largest_tables_and_a_transposed_pair(mbb, like):
    """6. 4096 bins; 100 x 100 bins with all ten parameter pairs; a pair given in the transposed order."""
    chain = _chain("large", lambda: MR.random_chain(2, 20, 200, seed=6, scale=[1.0, 3.0]))
    got = mbb.chain_marginals(like, chain, bins=4096, bins2d=100)
    assert len(got.pairs) == 10
    MR.check(got, chain, 4096, 100, PARAM_PAIRS, label="largest")
    one = mbb.chain_marginals(like, chain, bins=4096, bins2d=100, pairs=[("beta", "T")], range={"T": (24.0, 26.0)})
    assert one.pairs == [("T", "beta")]
    MR.check(one, chain, 4096, 100, [(0, 1)], ranges={0: (24.0, 26.0)}, label="transposed")
    H, xe, ye = one.hist2d("beta", "T")
    W, wx, wy = one.hist2d("T", "beta")
    assert np.array_equal(H, np.swapaxes(W, -1, -2)) and np.array_equal(xe, wy) and np.array_equal(ye, wx)
    for s in range(2):
        x, y = MR.column(chain, s, 0), MR.column(chain, s, 1)
        want, _, _ = np.histogram2d(y, x, bins=100, range=[MR.auto_range(y), (24.0, 26.0)])
        assert np.array_equal(H[s], want.astype(np.int64))


def test_no_stale_counts_after_a_larger_call(mbb, like):
    """7. A larger call on the same context (more sources, bins, pairs and splits), then a smaller one."""
    big = _chain("large", lambda: MR.random_chain(2, 20, 200, seed=6, scale=[1.0, 3.0]))
    mbb.chain_marginals(like, big, bins=4096, bins2d=100)
    small = _chain("small", lambda: MR.random_chain(1, 7, 37, seed=1)[0])
    got = mbb.chain_marginals(like, small, bins=5, bins2d=3, pairs=[("T", "fnorm")], burn=2)
    MR.check(got, small[None], 5, 3, [(0, 4)], burn=2, multi=False, label="after a larger call")
    mid = _chain("splits", lambda: MR.random_chain(1, 33, 1000, seed=2)[0])
    mbb.chain_marginals(like, mid, bins=64, bins2d=16)
    got = mbb.chain_marginals(like, mid, bins=17, bins2d=4, burn=900)
    MR.check(got, mid[None], 17, 4, PARAM_PAIRS, burn=900, multi=False, label="after more splits")


# ---------------------------------------------------------------- derived columns
Z, DL = 2.3, 18700.0
DERIVED = ("peaklambda", "lir", "dustmass")
WAVE = np.array([100.0, 250.0, 500.0, 850.0])
MODELS = {"thin_noalpha": (True, True), "thin_walpha": (True, False), "thick_noalpha": (False, True),
          "thick_walpha": (False, False)}
CHUNK = SR.chunk_rows(ROOT)
MARGIN = 1e-9                                                            # bin widths about an interior edge


def _model_like(mbb, model):
    if ("like", model) not in _CACHE:
        opthin, noalpha = MODELS[model]
        lk = mbb.likelihood(response=False, opthin=opthin, noalpha=noalpha)
        lk.set_phot(WAVE, np.full(4, 10.0), np.full(4, 2.0))
        _CACHE["like", model] = lk
    return _CACHE["like", model]


def _entries(lk, chain, z=Z):
    """postprocess's per-entry values of a chain [nsrc, nw, nsteps, 5]: {slot: [nsrc, nw, nsteps]}."""
    from mbb_emcee_amd import postprocess as pp
    return {5: pp.peak_wavelength(lk, chain), 6: pp.lir(lk, chain, z, DL), 7: pp.dustmass(lk, chain, z, DL)}


def _clear_of_edges(x, e, outer=False):
    """The precondition: no sample within MARGIN bin widths of an interior edge (outer: of any edge -- a given range,
    whose ends are not samples)."""
    inner = e if outer else e[1:-1]
    if inner.size == 0:
        return True
    i = np.clip(np.searchsorted(inner, x), 0, inner.size - 1)
    d = np.minimum(np.abs(x - inner[i]), np.abs(x - inner[np.maximum(i - 1, 0)]))
    return bool(np.all(d > MARGIN * (e[1] - e[0])))


def _derived_case(mbb, model, chain, bins, bins2d, burn, thin, label):
    lk = _model_like(mbb, model)
    extra = _entries(lk, chain)
    nsrc = chain.shape[0]
    pairs = [(0, 5), (1, 6), (5, 7), (6, 7)]
    names = [(MR.NAMES[a], MR.NAMES[b]) for a, b in pairs]
    # given ranges, from the central 90 % of postprocess's values over all sources
    ranges = {}
    for slot in (5, 6, 7):
        lo, hi = np.percentile(extra[slot][:, :, burn::thin], [5.0, 95.0])
        ranges[slot] = (float(lo), float(hi))
    for rng, tag in ((ranges, "given"), ({}, "automatic")):
        for slot in (5, 6, 7):
            for s in range(nsrc):
                x = MR.column(chain, s, slot, burn, thin, extra)
                for nb in (bins, bins2d):
                    lo, hi = rng.get(slot) or MR.auto_range(x)
                    assert _clear_of_edges(x, MR.edges(lo, hi, nb), outer=bool(rng)), (label, tag, slot, s, nb,
                                                                                       "choose another seed")
        got = mbb.chain_marginals(lk, chain, bins=bins, bins2d=bins2d, pairs=names, burn=burn, thin=thin, derived=DERIVED,
                                  redshift=Z, lumdist_mpc=DL, range={MR.NAMES[k]: v for k, v in rng.items()})
        MR.check(got, chain, bins, bins2d, pairs, ranges=rng, burn=burn, thin=thin, extra=extra, multi=True,
                 label="%s %s" % (label, tag), derived_edge_rtol=0.0 if rng else 1e-13)
        assert np.all(got.status == 0)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_derived_columns_per_model(mbb, model):
    """Peak wavelength, L_IR and dust mass as columns, 2 sources x 16 walkers x 64 steps per model variant: counts
    exactly those of postprocess's values, with given ranges and with automatic ones, 1-d and in pairs with parameters
    and with each other."""
    chain = _chain("derived", lambda: SR.distinct_chain(2, 16, 64, seed=8)[0])
    _derived_case(mbb, model, chain, 32, 6, 4, 3, model)


def test_derived_columns_across_the_chunk_seam(mbb):
    """The derived columns are filled kSumChunkRows chain rows at a time: a chain whose cells cross that seam."""
    nsrc, nw, nsteps, burn, thin = SR.seam_shapes(CHUNK)["windows"][1]
    assert nsrc * nw * nsteps > CHUNK >= nw * (nsteps - 1)
    chain = _chain("seam", lambda: SR.distinct_chain(nsrc, nw, nsteps, seed=9)[0])
    _derived_case(mbb, "thick_walpha", chain, 64, 5, burn, thin, "seam")


def test_a_source_of_unknown_redshift(mbb):
    """A source with NaN redshift: its L_IR and dust mass have no finite sample (EMPTY and NONFINITE, every sample
    counted as not finite, NaN edges, as the summary reports HAS_NAN there); its parameter and peak-wavelength
    columns, and the other source, are unaffected."""
    lk = _model_like(mbb, "thick_walpha")
    chain = _chain("derived", lambda: SR.distinct_chain(2, 16, 64, seed=8)[0])
    extra = _entries(lk, chain)
    for slot in (6, 7):
        extra[slot] = extra[slot].copy()
        extra[slot][1] = np.nan
    got = mbb.chain_marginals(lk, chain, bins=32, bins2d=6, pairs=[("T", "lir"), ("lir", "dustmass"), ("T", "beta")],
                              derived=DERIVED, redshift=np.array([Z, np.nan]), lumdist_mpc=DL)
    for slot in (5, 6, 7):
        x = MR.column(chain, 0, slot, extra=extra)
        assert _clear_of_edges(x, MR.edges(*MR.auto_range(x), 32)) and _clear_of_edges(x, MR.edges(*MR.auto_range(x), 6))
    MR.check(got, chain, 32, 6, [(0, 6), (6, 7), (0, 1)], extra=extra, multi=True, label="unknown redshift",
             derived_edge_rtol=1e-13)
    assert np.all(got.status[1, 6:] == (got.EMPTY | got.NONFINITE)) and np.all(got.n_nonfinite[1, 6:] == 16 * 64)
    assert np.all(got.status[0] == 0) and np.all(got.status[1, :6] == 0)
    assert np.all(np.isnan(got.hist1d("lir")[1][1])) and got.hist2d("lir", "dustmass")[0][1].sum() == 0
    assert "no finite sample" not in str(got)                             # (the first source)


SUMMARY_FIELDS = ("n_used", "mean", "min", "max", "pct", "status", "cov", "best", "best_index")
MARGINALS_FIELDS = ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below", "n_above", "n_nonfinite", "status")


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def test_summary_and_marginals_share_the_derived_column_state(mbb):
    """The derived columns, their per-source constants and their row-status words are one state of the context, used
    by the summary and by the marginals.  Four calls in turn on ONE context -- a summary with per-source redshifts
    (source 1's unknown), marginals with L_IR alone and one redshift, the summary again, marginals with all three
    columns and the per-source arrays: every array of every result, status words included, has the bits of the same
    call made on a context of its own."""
    chain, lnprob = SR.distinct_chain(3, 8, 40, seed=12)
    zs, dls = np.array([Z, np.nan, 0.9]), np.array([DL, 9000.0, 6000.0])
    win = dict(burn=4, thin=3)

    def fresh():
        opthin, noalpha = MODELS["thick_walpha"]
        lk = mbb.likelihood(response=False, opthin=opthin, noalpha=noalpha)
        lk.set_phot(WAVE, np.full(4, 10.0), np.full(4, 2.0))
        return lk

    def summary(lk):
        return mbb.chain_summary(lk, chain, lnprob, derived=DERIVED, redshift=zs, lumdist_mpc=dls, keep=False, **win)

    calls = [
        (summary, SUMMARY_FIELDS),
        (lambda lk: mbb.chain_marginals(lk, chain, bins=16, bins2d=8, pairs="all", derived=("lir",), redshift=Z,
                                        lumdist_mpc=DL, **win), MARGINALS_FIELDS),
        (summary, SUMMARY_FIELDS),
        (lambda lk: mbb.chain_marginals(lk, chain, bins=16, bins2d=8, pairs="all", derived=DERIVED, redshift=zs,
                                        lumdist_mpc=dls, **win), MARGINALS_FIELDS),
    ]
    shared = fresh()
    for k, (call, fields) in enumerate(calls):
        got, want = call(shared), call(fresh())
        for f in fields:
            a, b = getattr(got._raw, f), getattr(want._raw, f)
            assert a.dtype == b.dtype and a.shape == b.shape and a.size > 0, (k, f)
            assert np.array_equal(_bits(a), _bits(b)), (k, f)
    # (the calls did what they were asked: source 1's L_IR and dust mass are unknown to both analyses)
    assert np.all(got.status[1, 6:] == (got.EMPTY | got.NONFINITE)) and np.all(got.status[0] == 0)


# ---------------------------------------------------------------- through the layers
NW, NSTEPS = 34, 64
RAW_FIELDS = ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below", "n_above", "n_nonfinite", "status")


def _same_bits(a, b):
    return all(np.array_equal(getattr(a._raw, f), getattr(b._raw, f), equal_nan=True) for f in RAW_FIELDS)


def _sampler_case(mbb, g_lnl, multi):
    """The golden 8-band photometry, one source or three (tests/test_diagnostics_gpu.py's)."""
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rng = np.random.RandomState(11)
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    if multi:
        ns = 3
        truths = np.column_stack([rng.uniform(8, 20, ns), rng.uniform(1.2, 2.4, ns), rng.uniform(300, 900, ns),
                                  rng.uniform(2, 4.5, ns), rng.uniform(10, 80, ns)])
        flux = one.model_flux(truths)
        lk = mbb.likelihood(response=True)
        lk.set_phot_multi(bands, flux, 0.1 * flux + 1.0)
        p0 = truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, NW, 5)))
    else:
        truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
        flux = one.model_flux(truth)[0]
        lk = mbb.likelihood(response=True)
        lk.set_phot(bands, flux, 0.1 * flux + 1.0)
        p0 = truth * (1.0 + 0.02 * rng.normal(size=(NW, 5)))
    return lk, p0


@pytest.mark.parametrize("multi", [False, True])
def test_sampler_marginals_equal_those_of_the_stored_chain(mbb, g_lnl, multi):
    """A real run, 34 walkers x 64 steps: marginals() on the resident chain is bitwise chain_marginals of the chain the
    run returned, and numpy's; a run that stores nothing and summarises gives the same bits, its keywords defaulting to
    the summary's; the refusals."""
    lk, p0 = _sampler_case(mbb, g_lnl, multi)
    a = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.marginals_ is None
    kw = dict(bins=24, bins2d=6, burn=5, thin=2, derived=("peaklambda",))
    res = a.marginals(**kw)
    host = mbb.chain_marginals(lk, a.chain, **kw)
    assert _same_bits(res, host) and _same_bits(res, a.marginals(**kw))
    assert res.n_used.shape == ((3, 8) if multi else (8,)) and res.nsteps_used == 30 and res.nwalkers == NW
    c4 = _c4(a.chain)
    for s in range(c4.shape[0]):
        for slot in range(5):
            x = MR.column(c4, s, slot, 5, 2)
            counts, edges = res.hist1d(slot)
            counts, edges = (counts[s], edges[s]) if multi else (counts, edges)
            want, we = np.histogram(x, bins=24)
            assert np.array_equal(counts, want) and np.array_equal(edges.view(np.int64), we.view(np.int64))
    b = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b.run_mcmc(p0, NSTEPS, storechain=False, summary=dict(burn=5, thin=2, derived=("peaklambda",)),
               marginals=dict(bins=24, bins2d=6))
    assert b.chain.shape[-2] == 0 and b.summary is not None
    assert _same_bits(b.marginals_, res) and b.marginals_.burn == 5 and b.marginals_.thin == 2
    held = b.marginals_
    b.run_mcmc(None, 3, storechain=False)                   # the next run: nothing of it is resident
    assert b.marginals_ is None and held is not None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.marginals()
    b.run_mcmc(None, 9, marginals=True)
    assert b.marginals_.nsteps_used == 9 and b.marginals_.bins == 64
    with pytest.raises(ValueError, match="burn leaves no step"):
        b.marginals(burn=9)
    for pos, lnp, _ in b.sample(None, iterations=2):
        assert b.marginals_ is None
    b.reset()
    assert b.marginals_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.marginals()
    with pytest.raises(ValueError, match="needs summary= too"):
        b.run_mcmc(p0, 8, storechain=False, marginals=True)


def _spec(nbins=8, nbins2=0, pairs=(), ranges=None, burn=0, thin=1, derived=0):
    from mbb_emcee_amd import _native
    s = _native.MarginalsSpec()
    s.nbins, s.nbins2, s.npairs = nbins, nbins2, len(pairs)
    for i, (a, b) in enumerate(pairs[:_native.MARG_MAX_PAIRS]):
        s.pairs[i][0], s.pairs[i][1] = a, b
    for slot, (lo, hi) in (ranges or {}).items():
        s.has_range[slot], s.lo[slot], s.hi[slot] = 1, lo, hi
    s._summary = _native.SummarySpec()
    s._summary.npct, s._summary.burn, s._summary.thin, s._summary.derived = 1, burn, thin, derived
    s._summary.kappa, s._summary.kappa_wave, s._summary.lir_wavemin, s._summary.lir_wavemax = 2.64, 125.0, 8.0, 1000.0
    s.summary = C.pointer(s._summary)
    return s


def test_native_refusals_leave_the_context_usable(mbb, like, g_lnl):
    """The C-ABI's MBB_ERR_ARG refusals, each before anything is uploaded and each followed by a good call that gives
    the right answer; mbb_sampler_marginals' MBB_ERR_STATE without a resident chain."""
    from mbb_emcee_amd import _native, marginals
    ctx = like.context
    chain = np.ascontiguousarray(_chain("small", lambda: MR.random_chain(1, 7, 37, seed=1)[0]))
    ref = mbb.chain_marginals(like, chain, bins=8, bins2d=3)

    def call(spec, raw=None, nsteps=37, edit=None):
        raw = raw or marginals._Raw(1, max(spec.nbins, 1), max(spec.nbins2, 0), max(spec.npairs, 0))
        out = raw.out()
        if edit:
            edit(out)
        return ctx.lib.mbb_chain_marginals(ctx.h, _native._d(chain), 1, 7, nsteps, C.byref(spec), C.byref(out)), raw

    def good():
        rc, raw = call(_spec(8, 3, PARAM_PAIRS))
        assert rc == 0
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(raw, f), getattr(ref._raw, f), equal_nan=True), f

    good()
    inf, nan = float("inf"), float("nan")
    bad = [(_spec(0), "nbins"), (_spec(4097), "nbins"), (_spec(8, -1), "nbins2"), (_spec(8, 101), "nbins2"),
           (_spec(8, 3, [(0, 1)] * 29), "pairs"), (_spec(8, 0, [(0, 1)]), "pairs need"),
           (_spec(8, 3, [(1, 0)]), "a < b"), (_spec(8, 3, [(2, 2)]), "a < b"), (_spec(8, 3, [(0, 6)]), "absent"),
           (_spec(8, 3, [(0, 8)]), "absent"), (_spec(8, 3, [(-1, 2)]), "absent"),
           (_spec(8, ranges={0: (1.0, 1.0)}), "range"), (_spec(8, ranges={1: (2.0, 1.0)}), "range"),
           (_spec(8, ranges={2: (0.0, inf)}), "range"), (_spec(8, ranges={3: (nan, 1.0)}), "range"),
           (_spec(8, ranges={4: (-1e308, 1e308)}), "range"),
           (_spec(8, burn=37), "burn"), (_spec(8, burn=-1), "burn"), (_spec(8, thin=0), "burn"),
           (_spec(8, derived=8), "derived"), (_spec(8, derived=_native.SUM_LIR), "redshift")]
    for spec, msg in bad:
        rc, _ = call(spec)
        assert rc == -2 and msg in ctx.lib.mbb_last_error().decode(), (msg, rc, ctx.lib.mbb_last_error())
        good()

    def drop(field):
        def edit(o):
            setattr(o, field, None)
        return edit
    for field in ("counts1", "edges1", "n_used", "n_below", "n_above", "n_nonfinite", "status"):
        assert call(_spec(8), edit=drop(field))[0] == -2
    assert call(_spec(8, 3, [(0, 1)]), edit=drop("counts2"))[0] == -2 and call(_spec(8, 3), edit=drop("edges2"))[0] == -2
    no_summary = _spec(8)
    no_summary.summary = None
    assert call(no_summary)[0] == -2
    assert call(_spec(8, 0), edit=drop("counts2"))[0] == 0                 # not needed without 2-d tables
    good()
    # the sampler call
    lk, p0 = _sampler_case(mbb, g_lnl, False)
    s = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=5)
    sctx, h = s._handle()
    raw = marginals._Raw(1, 8, 0, 0)
    spec, out = _spec(8), raw.out()
    assert sctx.lib.mbb_sampler_marginals(sctx.h, h, C.byref(spec), C.byref(out)) == -3
    assert "resident" in sctx.lib.mbb_last_error().decode()
    s.run_mcmc(p0, 8, storechain=False)
    assert sctx.lib.mbb_sampler_marginals(sctx.h, h, C.byref(spec), C.byref(out)) == -3
    s.run_mcmc(None, 8)
    assert sctx.lib.mbb_sampler_marginals(sctx.h, h, C.byref(spec), C.byref(out)) == 0
    assert np.all(raw.n_used[0, :5] == NW * 8)
    assert sctx.lib.mbb_sampler_marginals(sctx.h, h, None, C.byref(out)) == -2
    bad_spec = _spec(0)
    assert sctx.lib.mbb_sampler_marginals(sctx.h, h, C.byref(bad_spec), C.byref(out)) == -2
    assert sctx.lib.mbb_sampler_marginals(sctx.h, h, C.byref(spec), C.byref(out)) == 0
    assert _same_bits(s.marginals(bins=8), mbb.chain_marginals(lk, s.chain, bins=8))


def test_fitter_and_cli_marginals(mbb, g_lnl, tmp_path, capsys):
    """mbb_fitter.run(..., marginals=True) and the CLI's --marginals / --marginals2d end to end: the tables are those of
    the chain the fit returns; without the flag nothing new is printed or written."""
    from mbb_emcee_amd import run_mbb_emcee
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    flux = one.model_flux(truth)[0]
    fit = mbb.mbb_fitter(nwalkers=NW, response=True, seed=3)
    fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    fit.run(20, NSTEPS, p0, marginals=True)
    m = fit.marginals
    assert m is not None and m.bins == 64 and fit.summary is None and fit.convergence is None
    assert _same_bits(m, mbb.chain_marginals(fit.like, fit.sampler.chain))
    MR.check(m, fit.sampler.chain[None], 64, multi=False, label="fitter")
    fit.run(20, 16, p0, marginals=dict(bins=12, bins2d=5), summary=True)
    assert _same_bits(fit.marginals, mbb.chain_marginals(fit.like, fit.sampler.chain, bins=12, bins2d=5))
    fit.run(20, 16, p0)
    assert fit.marginals is None                                         # the default leaves none
    capsys.readouterr()
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", str(NW), "-b", "20", "-N", str(NSTEPS), "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--marginals", "20", "--marginals2d", "6"]) == 0
    text = capsys.readouterr().out
    assert "Marginals over %d steps of %d walkers, 20 bins, 10 pairs of 6 x 6" % (NSTEPS, NW) in text
    assert text.count("range:") == 5
    got = np.load(out)
    keys_with = set(got.files)
    new = {"marginals_counts1", "marginals_edges1", "marginals_counts2", "marginals_edges2", "marginals_pairs",
           "marginals_n_used", "marginals_n_below", "marginals_n_above", "marginals_n_nonfinite", "marginals_status",
           "marginals_columns"}
    assert new <= keys_with
    chain = got["chain"]
    assert got["marginals_counts1"].shape == (8, 20) and got["marginals_counts2"].shape == (10, 6, 6)
    for slot in range(5):
        want, we = np.histogram(chain[:, :, slot].ravel(), bins=20)
        assert np.array_equal(got["marginals_counts1"][slot], want)
        assert np.array_equal(got["marginals_edges1"][slot].view(np.int64), we.view(np.int64))
    for k, (a, b) in enumerate(got["marginals_pairs"]):
        x, y = chain[:, :, a].ravel(), chain[:, :, b].ravel()
        want = np.histogram2d(x, y, bins=6)[0]
        assert np.array_equal(got["marginals_counts2"][k], want.astype(np.int64)), (a, b)
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == ""
    assert keys_with - set(np.load(out).files) == new
