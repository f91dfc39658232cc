"""Posterior draws on the device (csrc/mbb_draws.hip.h, draws_run in csrc/mbb_hip.hip) against tests/_draws_ref.py --
its own Philox, (u N) >> 64 in Python integers, the window as a list of steps -- and, for the derived values of the
drawn rows, against mbb_emcee_amd.postprocess at tests/test_summary_derived_gpu.py's own per-entry bounds (relative
1e-13; a dust mass beyond that is decided by 50 digits) and bit for bit against the summary of the same cell.

The shapes are where the kernels can go wrong: fewer draws than a wave, 63 / 64 / 65, more draws than cells, one-step
and one-kept-step windows, populations of 2^32 - 1 and steps of 2^31 - 1, a compact block that crosses the seam of the
chunks the derived columns are filled by."""
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT, parity_record, rec_allclose
import _draws_ref as DR
import _summary_ref as SR
from mbb_emcee_amd import draws as _draws_module              # noqa: F401

pytestmark = pytest.mark.gpu

Z, DL = 2.3, 18700.0
DERIVED = ("peaklambda", "lir", "dustmass")
ENTRY_RTOL = 1e-13
WAVE = np.array([100.0, 250.0, 500.0, 850.0])
MODELS = {"thick_walpha": (False, False, {}),
          "thin_noalpha": (True, True, dict(kappa=1.5, kappa_wave=250.0, lir_range=(1000.0, 40.0)))}
RAW_FIELDS = ("rows", "lnprob", "index", "status")
_CACHE = {}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _new_like(mbb, model="thick_walpha"):
    opthin, noalpha, _ = MODELS[model]
    like = mbb.likelihood(response=False, opthin=opthin, noalpha=noalpha)
    like.set_phot(WAVE, np.full(4, 10.0), np.full(4, 2.0))
    return like


def _like(mbb, model="thick_walpha"):
    if ("like", model) not in _CACHE:
        _CACHE["like", model] = _new_like(mbb, model)
    return _CACHE["like", model]


def _planted():
    if "planted" not in _CACHE:
        chain, lnp = DR.planted_chain(3, 7, 5, scale=[1.0, 1e-3, 250.0])
        chain.setflags(write=False)
        lnp.setflags(write=False)
        _CACHE["planted"] = (chain, lnp)
    return _CACHE["planted"]


def _same_bits(a, b):
    """Two ChainDraws hold the same bits (NaNs at the same places)."""
    if set(a._raw.derived) != set(b._raw.derived):
        return False
    return (all(np.array_equal(getattr(a._raw, f), getattr(b._raw, f), equal_nan=True) for f in RAW_FIELDS) and
            all(np.array_equal(DR.bits(a._raw.derived[d]), DR.bits(b._raw.derived[d])) for d in a._raw.derived))


def _check_against_reference(d, chain, lnp, nw, nsteps, burn, thin, n, how, seed, what):
    """index, params and lnprob of a [nsrc, ...] result are the reference's exactly, and every row is the chain's cell
    at its index bit for bit."""
    nsrc = chain.shape[0]
    idx = DR.indices(nsrc, nw, nsteps, burn, thin, n, how, seed)
    got_idx, rows, l = d._raw.index, d._raw.rows, d._raw.lnprob
    assert got_idx.dtype == np.int32 and got_idx.shape == (nsrc, n, 2), what
    assert np.array_equal(got_idx, idx), (what, np.argwhere(got_idx != idx)[:4])
    want_rows, want_l = DR.gather(chain, lnp, idx)
    assert np.array_equal(DR.bits(rows), DR.bits(want_rows)), what
    assert np.array_equal(DR.bits(l), DR.bits(want_l)) if lnp is not None else np.all(np.isnan(l)), what
    src = np.arange(nsrc)[:, None]
    assert np.array_equal(DR.bits(rows), DR.bits(chain[src, got_idx[..., 0], got_idx[..., 1]])), what
    assert np.all(d._raw.status[:, :5] == 0) and np.all(d._raw.status[:, 5:] == d.ABSENT), (what, d._raw.status)


# ---------------------------------------------------------------- 1. picks and gathers
def _planted_single():
    """One source, chain [3, 7, 5]: 3 walkers of 7 steps."""
    if "single" not in _CACHE:
        chain, lnp = DR.planted_chain(1, 3, 7)
        chain.setflags(write=False)
        lnp.setflags(write=False)
        _CACHE["single"] = (chain, lnp)
    return _CACHE["single"]


@pytest.mark.parametrize("how", ["random", "even"])
@pytest.mark.parametrize("window", [(0, 1), (2, 3), (6, 1), (0, 100)])
def test_picks_and_gathers_of_a_planted_chain(mbb, window, how):
    """A chain [3, 7, 5] whose every cell encodes its own walker and step (and so does its lnprob): n = 1, 2, 63, 64,
    65 and 1000 draws -- more than the window has cells -- from the whole chain, a thinned window (two kept steps), a
    window of one step and a window of one kept step."""
    chain, lnp = _planted_single()
    assert chain[0].shape == (3, 7, 5)
    burn, thin = window
    nkept = len(range(burn, 7, thin))
    like = _like(mbb)
    for n in (1, 2, 63, 64, 65, 1000):
        d = mbb.chain_draws(like, chain[0], lnp[0], n=n, how=how, seed=11 + n, burn=burn, thin=thin)
        assert d.params.shape == (n, 5) and d.lnprob.shape == (n,) and d.index.shape == (n, 2) and d.status.shape == (8,)
        assert d.nsteps_used == nkept and d.nwalkers == 3
        _check_against_reference(d, chain, lnp, 3, 7, burn, thin, n, how, 11 + n, (window, how, n))
        if how == "even" and n <= 3 * nkept:
            assert len(set(map(tuple, d.index))) == n                     # no repeats
        if n == 1000:
            assert len(set(map(tuple, d.index))) == 3 * nkept             # every cell of the window, none outside
    nolnp = mbb.chain_draws(like, chain[0], None, n=65, how=how, seed=76, burn=burn, thin=thin)
    _check_against_reference(nolnp, chain, None, 3, 7, burn, thin, 65, how, 76, (window, how, "no lnprob"))
    assert np.array_equal(nolnp.index, mbb.chain_draws(like, chain[0], lnp[0], n=65, how=how, seed=76, burn=burn,
                                                       thin=thin).index)


# ---------------------------------------------------------------- 2. several sources
def test_several_sources(mbb):
    """Three sources of different scales: the picks differ between the sources and are the reference's; one source's
    data placed as source 0, 1 and 2 is drawn with that place's stream (the source is a word of the counter), so a
    source drawn alone is drawn as source 0."""
    chain, lnp = _planted()
    like = _like(mbb)
    n = 200
    d = mbb.chain_draws(like, chain, lnp, n=n, seed=5, burn=1)
    idx = DR.indices(3, 7, 5, 1, 1, n, "random", 5)
    assert np.array_equal(d.index, idx)
    assert not np.array_equal(idx[0], idx[1]) and not np.array_equal(idx[1], idx[2]) and not np.array_equal(idx[0], idx[2])
    for place in range(3):
        rolled, rl = np.roll(chain, place, axis=0), np.roll(lnp, place, axis=0)      # source 0's data at `place`
        r = mbb.chain_draws(like, rolled, rl, n=n, seed=5, burn=1)
        assert np.array_equal(r.index, idx)                                           # the picks are the place's
        assert np.array_equal(DR.bits(r.params[place]), DR.bits(chain[0][idx[place, :, 0], idx[place, :, 1]]))
        assert np.array_equal(r.lnprob[place], lnp[0][idx[place, :, 0], idx[place, :, 1]])
    alone = mbb.chain_draws(like, chain[2], lnp[2], n=n, seed=5, burn=1)
    assert alone.params.shape == (n, 5) and np.array_equal(alone.index, idx[0])
    assert np.array_equal(DR.bits(alone.params), DR.bits(chain[2][idx[0, :, 0], idx[0, :, 1]]))


# ---------------------------------------------------------------- 3. the pick at large populations
@pytest.mark.parametrize("shape", [(65535, 65537), (1, 2 ** 31 - 1)])
def test_draw_indices_at_large_populations(mbb, shape):
    """N = 2^32 - 1 cells (the cap) and steps up to 2^31 - 2: where a 32-bit or a signed slip in the high multiply or
    in the step arithmetic shows.  Exact against Python integers."""
    nw, nsteps = shape
    like = _like(mbb)
    for how in ("random", "even"):
        got = mbb.draw_indices(nw, nsteps, 4096, how=how, seed=2 ** 64 - 59, nsources=2, like=like)
        want = DR.indices(2, nw, nsteps, 0, 1, 4096, how, 2 ** 64 - 59)
        assert got.dtype == np.int32 and np.array_equal(got, want), (how, np.argwhere(got != want)[:4])
        assert got[..., 0].max() < nw and got[..., 1].max() < nsteps and got.min() >= 0
        assert got[..., 1].max() > nsteps - nsteps // 64 or nw > 1
    got = mbb.draw_indices(nw, nsteps, 100, seed=7, burn=nsteps // 2 + 1, thin=3, like=like)
    assert got.shape == (100, 2)
    assert np.array_equal(got, DR.indices(1, nw, nsteps, nsteps // 2 + 1, 3, 100, "random", 7)[0])
    # the picks of chain_draws are these
    chain, lnp = _planted()
    d = mbb.chain_draws(like, chain, lnp, n=33, seed=8, burn=1, thin=2)
    assert np.array_equal(d.index, mbb.draw_indices(7, 5, 33, seed=8, burn=1, thin=2, nsources=3, like=like))


# ---------------------------------------------------------------- 4. derived columns
def _kw(model, **more):
    kw = dict(derived=DERIVED, redshift=Z, lumdist_mpc=DL)
    kw.update(MODELS[model][2])
    kw.update(more)
    return kw


def _entries(mbb, model, rows, peak_model="fit"):
    """postprocess's per-entry values of plain rows [..., 5]."""
    from mbb_emcee_amd import postprocess as pp
    like, extra = _like(mbb, model), MODELS[model][2]
    rng = extra.get("lir_range", (8.0, 1000.0))
    return {"peaklambda": pp.peak_wavelength(like, rows, model=peak_model),
            "lir": pp.lir(like, rows, Z, DL, rng[0], rng[1]),
            "dustmass": pp.dustmass(like, rows, Z, DL, extra.get("kappa", 2.64), extra.get("kappa_wave", 125.0))}


def _check_entries(mbb, model, rows, got, what, peak_model="fit"):
    """tests/test_summary_derived_gpu.py's per-entry bounds: peak wavelength and L_IR relative 1e-13 of postprocess;
    dust mass relative 1e-13, a row beyond it decided by 50 digits."""
    ref = _entries(mbb, model, rows, peak_model)
    for nm in ("peaklambda", "lir"):
        print("    %s %s: %d of %d entries not bitwise equal" % (what, nm, int((DR.bits(got[nm]) != DR.bits(ref[nm])).sum()),
                                                               np.size(ref[nm])))
        rec_allclose(got[nm], ref[nm], rtol=ENTRY_RTOL, kind="draws %s vs postprocess" % nm)
    rows2, g, host = rows.reshape(-1, 5), np.ravel(got["dustmass"]), np.ravel(ref["dustmass"])
    rel = np.abs(g - host) / np.abs(host)
    parity_record("draws dustmass vs postprocess (rel)", rel.max(), ENTRY_RTOL)
    print("    %s dustmass: max rel %.3g over %d entries, %d not bitwise equal" % (what, rel.max(), g.size,
                                                                                 int((DR.bits(g) != DR.bits(host)).sum())))
    extra = MODELS[model][2]
    for i in np.flatnonzero(~(rel <= ENTRY_RTOL)):
        truth = SR.dustmass_mp(rows2[i], MODELS[model][0], 500.0, Z, DL, extra.get("kappa", 2.64), extra.get("kappa_wave", 125.0))
        dev = abs(g[i] - truth) / abs(truth)
        parity_record("draws dustmass vs 50 digits (rel)", dev, ENTRY_RTOL)
        assert dev <= ENTRY_RTOL, (what, rows2[i], g[i], host[i], truth)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_derived_values_of_the_drawn_rows(mbb, model):
    """2 sources x 16 walkers x 64 steps, 300 random draws of a thinned window: the derived values are postprocess's of
    the drawn rows, per entry; and the rows are the chain's."""
    chain, lnp = SR.distinct_chain(2, 16, 64, seed=31)
    like = _like(mbb, model)
    for peak_model in (("fit",) if model == "thick_walpha" else ("fit", "reference")):
        d = mbb.chain_draws(like, chain, lnp, n=300, seed=41, burn=5, thin=2, peak_model=peak_model, **_kw(model))
        idx = DR.indices(2, 16, 64, 5, 2, 300, "random", 41)
        assert np.array_equal(d.index, idx)
        rows = d.params
        assert np.array_equal(DR.bits(rows), DR.bits(DR.gather(chain, lnp, idx)[0]))
        assert np.all(d.status == 0), d.status
        got = {"peaklambda": d.peaklambda, "lir": d.lir, "dustmass": d.dustmass}
        assert all(np.all(np.isfinite(v)) and v.shape == (2, 300) for v in got.values())
        _check_entries(mbb, model, rows, got, "%s %s" % (model, peak_model), peak_model)
        t = d.choice(getpeaklambda=True, getlir=True, getdustmass=True)
        assert np.array_equal(t[0], rows) and np.array_equal(t[1], got["peaklambda"]) and np.array_equal(t[3], got["dustmass"])
        # flux(): postprocess.predict_flux on the drawn rows
        from mbb_emcee_amd import postprocess as pp
        assert np.array_equal(d.flux(250.0), pp.predict_flux(like, rows, 250.0)) and d.flux([100.0, 850.0]).shape == (2, 300, 2)
    some = mbb.chain_draws(like, chain, lnp, n=5, derived=("peaklambda",))
    assert np.all(some.status[:, 6:] == some.ABSENT) and np.all(some.status[:, :6] == 0)
    with pytest.raises(Exception, match="LIR not computed"):
        some.lir


@pytest.mark.parametrize("model", sorted(MODELS))
def test_one_cell_window_is_the_summary_of_that_cell(mbb, model):
    """nw = 1, burn = k, thin >= nsteps: the window is the cell (s, 0, k).  Every draw is that cell, and its three
    derived values are bit for bit chain_summary's min of the same window; a cell whose row fails in the SED
    constructor (alpha = -1 in the model that uses alpha) carries NaN and the summary's row-status bit."""
    from mbb_emcee_amd import results, _native
    chain, lnp = SR.distinct_chain(2, 1, 12, seed=37)
    bad_k = 7 if model == "thick_walpha" else None
    if bad_k is not None:
        chain[1, 0, bad_k, 3] = -1.0
    like = _like(mbb, model)
    for k in (0, 6, 7, 11):
        for how in ("random", "even"):
            d = mbb.chain_draws(like, chain, lnp, n=3, how=how, seed=k, burn=k, thin=12, **_kw(model))
            s = results.chain_summary(like, chain, lnp, burn=k, thin=12, keep=False, **_kw(model))
            assert np.all(s.n_used == 1) and np.all(d.index == [0, k])
            for i in range(3):
                assert np.array_equal(DR.bits(d.params[:, i]), DR.bits(chain[:, 0, k])), (k, how, i)
                for c, nm in enumerate(DERIVED):
                    got, want = getattr(d, nm)[:, i], s.min[:, 5 + c]
                    # (bit for bit; where the cell's row failed, NaN on both sides)
                    assert np.array_equal(np.isnan(got), np.isnan(want)), (k, how, i, nm)
                    fin = ~np.isnan(want)
                    assert np.array_equal(DR.bits(got[fin]), DR.bits(want[fin])), (k, how, i, nm)
            row_bits = s.status[:, 5:] & ~(_native.SUM_HAS_NAN | _native.SUM_EMPTY)
            assert np.array_equal(d.status[:, 5:], row_bits), (k, d.status, s.status)
            assert np.all(d.status[:, :5] == 0)
            if k == bad_k:
                bit = 1 << (_native.SUM_ROW_SHIFT + _native.ROW_BAD_ALPHA)
                assert np.all(np.isnan(d.peaklambda[1])) and np.all(np.isnan(d.lir[1])) and np.all(np.isfinite(d.dustmass[1]))
                assert d.status[1, 5] == bit and d.status[1, 6] == bit and d.status[1, 7] == 0 and np.all(d.status[0] == 0)
                assert np.all(np.isfinite(d.peaklambda[0]))
            else:
                assert np.all(d.status == 0) and np.all(np.isfinite(d.lir))


# ---------------------------------------------------------------- 5. the chunk seam of the compact block
def test_compact_block_across_the_chunk_seam(mbb):
    """chain [5, 4, 8, 5] with n = 52 500: the compact block has 262 500 rows, so the second chunk of the derived fill
    begins inside the last source.  With one redshift per source (one of them unknown) every source's derived draws are
    bit for bit those of the same source drawn alone with its own redshift; the unknown source's L_IR and dust mass
    are NaN, its peak wavelength is not.  (how="even": the picks do not depend on the source's place.)"""
    chunk = SR.chunk_rows(ROOT)
    n = 52500
    assert chunk == 1 << 18 and 4 * n < chunk < 5 * n
    chain, lnp = SR.distinct_chain(5, 4, 8, seed=43)
    like = _like(mbb)
    z = np.array([0.5, np.nan, 1.5, 2.3, 4.0])
    dl = np.array([2900.0, 7000.0, 11000.0, 18700.0, 36000.0])
    d = mbb.chain_draws(like, chain, lnp, n=n, how="even", derived=DERIVED, redshift=z, lumdist_mpc=dl)
    assert d.lir.shape == (5, n) and np.all(d.status == 0), d.status
    for s in range(5):
        known = not np.isnan(z[s])
        one = mbb.chain_draws(like, chain[s], lnp[s], n=n, how="even", derived=DERIVED if known else ("peaklambda",),
                              redshift=z[s] if known else None, lumdist_mpc=dl[s] if known else None)
        assert np.array_equal(one.index, d.index[s]) and np.array_equal(DR.bits(one.params), DR.bits(d.params[s]))
        assert np.array_equal(DR.bits(one.peaklambda), DR.bits(d.peaklambda[s])) and np.all(np.isfinite(d.peaklambda[s]))
        if known:
            assert np.array_equal(DR.bits(one.lir), DR.bits(d.lir[s])) and np.all(np.isfinite(d.lir[s]))
            assert np.array_equal(DR.bits(one.dustmass), DR.bits(d.dustmass[s])) and np.all(np.isfinite(d.dustmass[s]))
        else:
            assert np.all(np.isnan(d.lir[s])) and np.all(np.isnan(d.dustmass[s]))
    # every cell repeated n / 32 times, in order: the values on both sides of the seam are those of their cells
    idx = d.index[4]
    flat = idx[:, 0] * 8 + idx[:, 1]
    assert np.array_equal(flat, (np.arange(n, dtype=np.int64) * 32) // n)
    first = np.searchsorted(flat, np.arange(32))
    for nm in DERIVED:
        v = getattr(d, nm)[4]
        assert np.array_equal(DR.bits(v), DR.bits(v[first][flat])), nm


# ---------------------------------------------------------------- 6. stale buffers
def test_no_stale_rows_after_a_larger_call(mbb):
    """n = 8 after n = 1000 on the same context returns what it returns on a fresh context."""
    chain, lnp = SR.distinct_chain(3, 6, 9, seed=47)
    used, fresh = _new_like(mbb), _new_like(mbb)
    assert used.context is not fresh.context
    kw = dict(seed=9, burn=1, thin=2, derived=DERIVED, redshift=Z, lumdist_mpc=DL)
    big = mbb.chain_draws(used, chain * 3.0, lnp - 5.0, n=1000, **kw)
    assert big.params.shape == (3, 1000, 5)
    for how in ("random", "even"):
        a = mbb.chain_draws(used, chain, lnp, n=8, how=how, **kw)
        b = mbb.chain_draws(fresh, chain, lnp, n=8, how=how, **kw)
        assert _same_bits(a, b) and np.all(np.isfinite(a.dustmass))
        assert np.array_equal(DR.bits(a._raw.rows), DR.bits(DR.gather(chain, lnp, a._raw.index)[0]))


# ---------------------------------------------------------------- 7. through the sampler
NW, NSTEPS = 16, 20


def _sampler_case(mbb, g_lnl, multi):
    """The golden 8-band photometry, one source or three (tests/test_marginals_gpu.py's)."""
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


def _c4(a, multi):
    return a if multi else a[None]


def _raw_arrays_equal(a, b):
    """Every array of two results (of their _raw blocks, where they keep one) holds the same bits."""
    fa, fb = vars(getattr(a, "_raw", a)), vars(getattr(b, "_raw", b))
    names = [k for k, v in fa.items() if isinstance(v, np.ndarray)]
    assert names and set(names) == set(k for k, v in fb.items() if isinstance(v, np.ndarray))
    return all(np.array_equal(fa[k], fb[k], equal_nan=True) for k in names)


@pytest.mark.parametrize("multi", [False, True])
def test_sampler_draws(mbb, g_lnl, multi):
    """A seeded run of 20 steps, 16 walkers, one source and three: draws() of the resident chain are the stored
    chain's cells at their index; a run that stores nothing, summarises and draws gives the same draws; adding draws=
    changes no bit of the run's other analyses; reset() forgets."""
    lk, p0 = _sampler_case(mbb, g_lnl, multi)
    ns = 3 if multi else 1
    a = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.draws_ is None
    d = a.draws(50)
    assert d.seed == 77 and d.params.shape == ((3, 50, 5) if multi else (50, 5))
    c4, l3 = _c4(a.chain, multi), _c4(a.lnprobability, multi)
    idx = d._raw.index
    assert np.array_equal(idx, DR.indices(ns, NW, NSTEPS, 0, 1, 50, "random", 77))
    src = np.arange(ns)[:, None]
    assert np.array_equal(DR.bits(d._raw.rows), DR.bits(c4[src, idx[..., 0], idx[..., 1]]))
    assert np.array_equal(DR.bits(d._raw.lnprob), DR.bits(l3[src, idx[..., 0], idx[..., 1]]))
    assert _same_bits(d, mbb.chain_draws(lk, a.chain, a.lnprobability, n=50, seed=77)) and _same_bits(d, a.draws(50))
    kw = dict(n=50, burn=3, thin=2, derived=("peaklambda",))
    win = a.draws(**kw)
    assert _same_bits(win, mbb.chain_draws(lk, a.chain, a.lnprobability, seed=77, **kw)) and win.nsteps_used == 9
    assert np.all(np.isfinite(win.peaklambda)) and not _same_bits(win, a.draws(seed=78, **kw))
    b = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b.run_mcmc(p0, NSTEPS, storechain=False, summary=True, draws=50)
    assert b.chain.shape[-2] == 0 and _same_bits(b.draws_, d)
    b2 = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b2.run_mcmc(p0, NSTEPS, storechain=False, summary=dict(burn=3, thin=2, derived=("peaklambda",)), draws=50)
    assert _same_bits(b2.draws_, win)                                   # (the keywords default to the summary's)
    # the other analyses of a run do not notice draws=
    extra = dict(summary=dict(derived=("peaklambda",)), convergence=True, marginals=dict(bins=16), predict=[250.0])
    c = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    c.run_mcmc(p0, NSTEPS, storechain=False, **extra)
    e = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    e.run_mcmc(p0, NSTEPS, storechain=False, draws=dict(n=50, derived=("peaklambda",)), **extra)
    assert c.draws_ is None and e.draws_ is not None and np.array_equal(e.draws_.index, d.index)
    for name in ("summary", "convergence_", "marginals_", "predictions_"):
        assert _raw_arrays_equal(getattr(c, name), getattr(e, name)), name
    # the next run and reset() forget
    held = e.draws_
    e.run_mcmc(None, 3, storechain=False)
    assert e.draws_ is None and held is not None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        e.draws(5)
    e.run_mcmc(None, 9, draws=4)
    assert e.draws_.nsteps_used == 9 and e.draws_.n == 4
    e.reset()
    assert e.draws_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        e.draws(5)
    with pytest.raises(ValueError, match="needs summary= too"):
        e.run_mcmc(p0, 8, storechain=False, draws=5)


def test_fitter_and_cli_draws(mbb, g_lnl, tmp_path, capsys):
    """mbb_fitter.run(..., draws=...) and the CLI's --draws end to end: the draws are those of the direct call on the
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
    fit.run(10, NSTEPS, p0, draws=40)
    d = fit.draws
    assert d is not None and d.n == 40 and fit.summary is None
    assert _same_bits(d, mbb.chain_draws(fit.like, fit.sampler.chain, fit.sampler.lnprobability, n=40, seed=fit.sampler.seed))
    fit.run(10, NSTEPS, p0, draws=dict(n=7, how="even", derived=("peaklambda",)), summary=True)
    assert _same_bits(fit.draws, mbb.chain_draws(fit.like, fit.sampler.chain, fit.sampler.lnprobability, n=7, how="even",
                                                 seed=fit.sampler.seed, derived=("peaklambda",)))
    fit.run(10, 8, p0)
    assert fit.draws is None                                             # the default leaves none
    capsys.readouterr()
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", str(NW), "-b", "10", "-N", str(NSTEPS), "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--draws", "30", "--get_peaklambda"]) == 0
    text = capsys.readouterr().out
    assert "30 random draws from %d steps of %d walkers (seed 5)" % (NSTEPS, NW) in text and text.count("mean:") == 6
    got = np.load(out)
    with_keys = set(got.files)
    new = {"draws_params", "draws_lnprob", "draws_index", "draws_status", "draws_peaklambda"}
    assert new <= with_keys
    like = mbb.likelihood(response=True)
    like.set_phot(bands, flux, 0.1 * flux + 1.0)
    direct = mbb.chain_draws(like, got["chain"], got["lnprobability"], n=30, seed=5, derived=("peaklambda",))
    for k, v in direct.arrays().items():
        assert np.array_equal(got[k], v, equal_nan=True), k
    assert run_mbb_emcee.main(args + ["--get_peaklambda"]) == 0
    assert capsys.readouterr().out == ""
    assert with_keys - set(np.load(out).files) == new


# ---------------------------------------------------------------- 8. refusals
def _spec(n=8, how=0, seed=1, burn=0, thin=1, derived=0):
    from mbb_emcee_amd import _native
    s = _native.DrawsSpec()
    s.n, s.how, s.seed = n, how, seed
    s._summary = _native.SummarySpec()
    s._summary.npct, s._summary.burn, s._summary.thin, s._summary.derived = 1, burn, thin, derived
    s._summary.kappa, s._summary.kappa_wave, s._summary.lir_wavemin, s._summary.lir_wavemax = 2.64, 125.0, 8.0, 1000.0
    s.summary = C.pointer(s._summary)
    return s


def test_native_refusals_leave_the_context_usable(mbb, g_lnl):
    """The C-ABI's MBB_ERR_ARG refusals, each followed by a good call that gives the right answer (a refused call has
    allocated, uploaded and launched nothing: the sizes it names could not be); mbb_sampler_draws' MBB_ERR_STATE
    without a resident chain."""
    from mbb_emcee_amd import _native, draws
    like = _like(mbb)
    ctx = like.context
    chain, lnp = [np.ascontiguousarray(a) for a in _planted()]
    ref = mbb.chain_draws(like, chain, lnp, n=8, seed=1)

    def call(spec, nsrc=3, nsteps=5, edit=None, n_out=8, chain_p=True, derived=()):
        raw = draws._Raw(3, n_out, derived)
        out = raw.out()
        if edit:
            edit(out)
        return ctx.lib.mbb_chain_draws(ctx.h, _native._d(chain) if chain_p else None, _native._d(lnp), nsrc, 7, nsteps,
                                       C.byref(spec) if spec is not None else None, C.byref(out)), raw

    def good():
        rc, raw = call(_spec())
        assert rc == 0
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(raw, f), getattr(ref._raw, f), equal_nan=True), f

    good()
    big = _native.DRAWS_MAX
    bad = [(_spec(0), {}, "at least one draw"), (_spec(-5), {}, "at least one draw"),
           (_spec(big + 1), {}, "2^24 draws per source"),
           (_spec(big), dict(nsrc=128), "2^31 - 1 draws per call"),
           (_spec(how=2), {}, "unknown how"), (_spec(how=-1), {}, "unknown how"),
           (_spec(burn=5), {}, "burn"), (_spec(burn=-1), {}, "burn"), (_spec(thin=0), {}, "burn"),
           (_spec(derived=8), {}, "derived"), (_spec(derived=_native.SUM_LIR), dict(derived=("lir",)), "redshift"),
           (_spec(), dict(nsrc=0), "empty chain"), (_spec(), dict(nsteps=0), "empty chain")]
    for spec, kw, msg in bad:
        rc, _ = call(spec, **kw)
        assert rc == -2 and msg in ctx.lib.mbb_last_error().decode(), (msg, rc, ctx.lib.mbb_last_error())
        good()

    def drop(field):
        def edit(o):
            setattr(o, field, None)
        return edit
    for field in ("rows", "lnprob", "index", "status"):
        assert call(_spec(), edit=drop(field))[0] == -2
    assert call(_spec(derived=_native.SUM_PEAK))[0] == -2                   # asked for, nowhere to put it
    assert call(_spec(derived=_native.SUM_PEAK), derived=("peaklambda",))[0] == 0
    no_summary = _spec()
    no_summary.summary = None
    assert call(no_summary)[0] == -2 and call(None)[0] == -2 and call(_spec(), chain_p=False)[0] == -2
    good()
    # the picks alone
    index = np.zeros((3, 8, 2), dtype=np.int32)

    def picks(nsrc=3, nw=7, nsteps=5, burn=0, thin=1, n=8, how=0, ptr=True):
        return ctx.lib.mbb_draw_indices(ctx.h, nsrc, nw, nsteps, burn, thin, n, how, 1, _native._i(index) if ptr else None)
    assert picks() == 0 and np.array_equal(index, ref._raw.index)
    for kw, msg in ((dict(n=0), "at least one"), (dict(n=big + 1), "2^24"), (dict(n=big, nsrc=128), "2^31 - 1"),
                    (dict(how=7), "unknown how"), (dict(burn=5), "burn"), (dict(thin=0), "burn"), (dict(nw=0), "empty"),
                    (dict(nw=65536, nsteps=65536), "2^32 samples"), (dict(ptr=False), "null")):
        assert picks(**kw) == -2 and msg in ctx.lib.mbb_last_error().decode(), (kw, ctx.lib.mbb_last_error())
    assert picks() == 0 and np.array_equal(index, ref._raw.index)
    # the sampler call
    lk, p0 = _sampler_case(mbb, g_lnl, False)
    s = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=5)
    sctx, h = s._handle()
    raw = draws._Raw(1, 8)
    spec, out = _spec(seed=5), raw.out()
    assert sctx.lib.mbb_sampler_draws(sctx.h, h, C.byref(spec), C.byref(out)) == -3
    assert "resident" in sctx.lib.mbb_last_error().decode()
    s.run_mcmc(p0, 8, storechain=False)
    assert sctx.lib.mbb_sampler_draws(sctx.h, h, C.byref(spec), C.byref(out)) == -3
    s.run_mcmc(None, 8)
    assert sctx.lib.mbb_sampler_draws(sctx.h, h, C.byref(spec), C.byref(out)) == 0
    assert sctx.lib.mbb_sampler_draws(sctx.h, h, None, C.byref(out)) == -2
    bad_spec = _spec(0)
    assert sctx.lib.mbb_sampler_draws(sctx.h, h, C.byref(bad_spec), C.byref(out)) == -2
    assert sctx.lib.mbb_sampler_draws(sctx.h, h, C.byref(spec), C.byref(out)) == 0
    assert np.array_equal(raw.rows, s.draws(8)._raw.rows)
    assert _same_bits(s.draws(8), mbb.chain_draws(lk, s.chain, s.lnprobability, n=8, seed=5))


def test_sharded_refusal_is_the_python_rule():
    """A sharded run is refused by the sampler's rule before anything runs (no extra ranks are started here)."""
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    class Like(object):
        data_read = True

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.lnprobfn, s.seed = Like(), 5
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded sampler run cannot be drawn from"):
        s.run_mcmc(np.zeros((10, 5)), 4, draws=3)
