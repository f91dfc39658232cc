"""A redshift and a luminosity distance per source in a chain summary: mbb_summary_spec's src_redshift /
src_lumdist_mpc, the table of per-source constants summary_fill_derived forms (csrc/mbb_hip.hip) and the kernels that
look a row's source up in it (k_sed_integrate_src in csrc/mbb_kernels.hip.h, k_sum_lir_src / k_sum_dustmass_src in
csrc/mbb_summary.hip.h).

Two references:
  A. the scalar path of the same build, one source at a time: chain_summary(like, chain[s], lnprob[s], redshift=z[s],
     lumdist_mpc=d[s], ...) is source s of the per-source call in every raw field, bit for bit.  Exact while
     nsrc * columns < 1024 (from there on summary_run takes one split per column and the tree order of the sums
     changes); every shape here stays under it, and keeps the number of splits the same in both calls.
  B. postprocess.lir / postprocess.dustmass with scalars, source by source, on plain rows (pinned to the reference's
     results.py by test_postprocess_vs_reference_results; they share no source arithmetic with the summary).

Bounds: those of tests/test_summary_derived_gpu.py's docstring, no other.  Per entry 1e-13 relative (a dust-mass row
beyond it is decided by the 50-digit SR.dustmass_mp); means 64 eps mean|x| plus the per-entry bound; percentiles 4 ulp
of the larger bracketing value plus the per-entry bound.

Redshifts are distinct per source, 0.5 + 0.37 s; the distances are unrelated to them.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import parity_record, rec_allclose
import _summary_ref as SR
import test_summary_derived_gpu as D

pytestmark = pytest.mark.gpu

MODELS, SHAPES, DERIVED, ENTRY_RTOL = D.MODELS, D.SHAPES, D.DERIVED, D.ENTRY_RTOL
SMALL = (5, 3, 41, 7, 3)                                    # sources, walkers, steps, burn, thin: 12 kept steps


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _z(nsrc):
    return 0.5 + 0.37 * np.arange(nsrc)


def _d(nsrc):
    """Distances [Mpc] that do not follow the redshifts: a fixed scramble over 40 Mpc .. 40 Gpc."""
    return 40.0 * 1000.0 ** (((np.arange(nsrc) * 7 + 3) % 11) / 10.0) * (1.0 + 0.01 * np.arange(nsrc))


def _kw(model, z, d, **more):
    kw = dict(derived=DERIVED, redshift=z, lumdist_mpc=d)
    kw.update(MODELS[model][2])
    kw.update(more)
    return kw


def _small():
    return D._cached(("distinct", "sources-small"), lambda: SR.distinct_chain(*SMALL[:3], seed=31))


def _source_equals(multi, s, one, fields=SR.RAW_FIELDS):
    """Source s of a multi-source summary holds the bits of a single-source summary."""
    return all(np.array_equal(getattr(multi._raw, f)[s], getattr(one._raw, f)[0], equal_nan=True) for f in fields)


def _entries(mbb, model, rows, z, d):
    """Reference B for the plain rows [n, 5] of one source: postprocess with that source's scalars."""
    from mbb_emcee_amd import postprocess as pp
    like, extra = D._like(mbb, model), MODELS[model][2]
    rng = extra.get("lir_range", (8.0, 1000.0))
    return {"lir": pp.lir(like, rows, float(z), float(d), rng[0], rng[1]),
            "dustmass": pp.dustmass(like, rows, float(z), float(d), extra.get("kappa", 2.64), extra.get("kappa_wave", 125.0))}


def _check_cell(mbb, model, row, z, d, got_lir, got_dust, what):
    """One chain row's L_IR and dust mass against reference B at the per-entry bound."""
    ref = _entries(mbb, model, row[None], z, d)
    rec_allclose(got_lir, ref["lir"][0], rtol=ENTRY_RTOL, kind="per-source summary cell lir vs postprocess")
    rel = abs(got_dust - ref["dustmass"][0]) / abs(ref["dustmass"][0])
    parity_record("per-source summary cell dustmass vs postprocess (rel)", rel, ENTRY_RTOL)
    if not rel <= ENTRY_RTOL:
        extra = MODELS[model][2]
        truth = SR.dustmass_mp(row, MODELS[model][0], 500.0, z, d, extra.get("kappa", 2.64), extra.get("kappa_wave", 125.0))
        dev = abs(got_dust - truth) / abs(truth)
        print("    %s: device %.3g, host %.3g of the 50-digit value" % (what, dev, abs(ref["dustmass"][0] - truth) / abs(truth)))
        parity_record("per-source summary cell dustmass vs 50 digits (rel)", dev, ENTRY_RTOL)
        assert dev <= ENTRY_RTOL, (what, row, got_dust, ref["dustmass"][0], truth)


# ---------------------------------------------------------------- 1. small, both references
@pytest.mark.parametrize("model", sorted(MODELS))
def test_small_chain_against_both_references(mbb, model):
    from mbb_emcee_amd import results
    nsrc, nw, nsteps, burn, thin = SMALL
    chain, lnp = _small()
    like, z, d = D._like(mbb, model), _z(nsrc), _d(nsrc)
    assert len(set(z)) == nsrc and len(set(d)) == nsrc
    s = results.chain_summary(like, chain, lnp, burn=burn, thin=thin, keep=False, **_kw(model, z, d))
    assert np.all(s.status == 0) and np.all(s.n_used == nw * 12), (s.status, s.n_used)
    qs = s.percentiles[0]
    win = SR.windowed(chain, burn, thin)
    for g in range(nsrc):
        one = results.chain_summary(like, chain[g], lnp[g], burn=burn, thin=thin, keep=False, **_kw(model, z[g], d[g]))
        assert _source_equals(s, g, one), g                              # A
        ent = _entries(mbb, model, win[g], z[g], d[g])                   # B
        for slot, nm in ((6, "lir"), (7, "dustmass")):
            D._check_column(s, g, slot, ent[nm], qs, ENTRY_RTOL, nm)
    # the redshifts matter: with source 0's for everyone the other sources' columns move by far more than any bound
    flat = results.chain_summary(like, chain, lnp, burn=burn, thin=thin, keep=False, **_kw(model, z[0], d[0]))
    assert np.all(np.abs(flat.mean[1:, 6:] / s.mean[1:, 6:] - 1.0) > 1e-3)
    assert np.array_equal(flat.mean[0], s.mean[0]) and np.array_equal(flat.mean[:, :6], s.mean[:, :6])


# ---------------------------------------------------------------- 2. the chunk seam inside the last source
@pytest.mark.parametrize("model", sorted(MODELS))
def test_second_chunk_begins_inside_the_last_source(mbb, model):
    """262500 rows: the second chunk of 2^18 begins inside source 2 and holds nothing else, so a lookup that forgets
    the chunk's offset takes source 0's redshift there."""
    from mbb_emcee_amd import results
    shape = SHAPES["windows"][0]
    nsrc, nw, nsteps, burn, thin = shape
    assert 2 * nw * nsteps < D.CHUNK < nsrc * nw * nsteps
    chain, lnp, _, _ = D._sentinel_case(shape)
    like, z, d = D._like(mbb, model), _z(nsrc), _d(nsrc)
    kw = dict(percentile=(68.3, 95.4), burn=burn, thin=thin, keep=False)
    s = results.chain_summary(like, chain, lnp, **_kw(model, z, d, **kw))
    assert np.all(s.status == 0)
    for g in range(nsrc):
        one = results.chain_summary(like, chain[g], lnp[g], **_kw(model, z[g], d[g], **kw))
        assert _source_equals(s, g, one), g
    wrong = results.chain_summary(like, chain[2], lnp[2], **_kw(model, z[0], d[0], **kw))
    assert not _source_equals(s, 2, wrong, fields=("mean",))              # (the test can see that mistake)


# ---------------------------------------------------------------- 3. one cell per source across the seam
@pytest.mark.parametrize("model", sorted(MODELS))
def test_one_cell_per_source_across_the_seam(mbb, model):
    """burn=b, thin=nsteps summarises the cell (s, 0, b) of each of 64 sources, each with its own redshift and
    distance; b = 3843 / 3844 / 3845 are the cells of source 63 on either side of the chunk seam."""
    from mbb_emcee_amd import results
    (nsrc, nw, nsteps), steps = SHAPES["cells"]
    chain, lnp = D._cached(("distinct", "cells"), lambda: SR.distinct_chain(nsrc, nw, nsteps, seed=17 + nsteps % 7))
    like, z, d = D._like(mbb, model), _z(nsrc), _d(nsrc)
    assert len(set(z)) == nsrc
    for b in steps:
        s = results.chain_summary(like, chain, lnp, burn=b, thin=nsteps, keep=False, **_kw(model, z, d))
        assert np.all(s.n_used == 1) and np.all(s.status == 0), (b, s.status)
        mean = s.mean
        assert np.array_equal(D._bits(mean[:, :5]), D._bits(chain[:, 0, b, :])), b
        for g in range(nsrc):
            _check_cell(mbb, model, chain[g, 0, b], z[g], d[g], mean[g, 6], mean[g, 7], "b=%d source %d" % (b, g))


# ---------------------------------------------------------------- 4. unknown sources
@pytest.mark.parametrize("which, src", [("redshift", 1), ("lumdist_mpc", 3)])
@pytest.mark.parametrize("model", sorted(MODELS))
def test_unknown_source_is_nan_and_nothing_else_moves(mbb, model, which, src):
    from mbb_emcee_amd import results, _native
    nsrc, nw, nsteps, burn, thin = SMALL
    chain, lnp = _small()
    like, z, d = D._like(mbb, model), _z(nsrc), _d(nsrc)
    kw = dict(burn=burn, thin=thin, keep=True)
    known = results.chain_summary(like, chain, lnp, **_kw(model, z, d, **kw))
    (z if which == "redshift" else d)[src] = np.nan
    s = results.chain_summary(like, chain, lnp, **_kw(model, z, d, **kw))
    assert np.all(s.status[src, 6:] == _native.SUM_HAS_NAN), s.status
    assert np.all(np.isnan(s.mean[src, 6:])) and np.all(np.isnan(s.percentiles[1][src, 6:]))
    assert np.all(s.n_used == nw * 12)
    others = [g for g in range(nsrc) if g != src]
    for f in ("n_used", "mean", "min", "max", "pct", "status"):
        a, b = getattr(s._raw, f), getattr(known._raw, f)
        assert np.array_equal(a[others], b[others]), f
        assert np.array_equal(a[src, :6], b[src, :6]), f
    assert SR.raw_equal(s, known, fields=("cov", "best", "best_index"))
    for fn, ref in ((s.lir_cen, known.lir_cen), (s.dustmass_cen, known.dustmass_cen)):
        for args in ((), (95.4,)):                                       # (95.4: not prepared, from the kept chain)
            got, want = fn(*args), ref(*args)
            assert got.shape == (nsrc, 3) and np.all(np.isnan(got[src]))
            assert np.array_equal(got[others], want[others]) and np.all(np.isfinite(got[others]))
    assert np.array_equal(s.peaklambda_cen(), known.peaklambda_cen())
    got = s.lir_cen(lowlim=0.0)                                          # a clip empties the unknown source's column
    assert np.all(np.isnan(got[src])) and np.array_equal(got[others], known.lir_cen(lowlim=0.0)[others])


# ---------------------------------------------------------------- 5. scalar broadcast, single source
@pytest.mark.parametrize("model", sorted(MODELS))
def test_scalar_broadcast_and_single_source(mbb, model):
    from mbb_emcee_amd import results
    nsrc, nw, nsteps, burn, thin = SMALL
    chain, lnp = _small()
    like, d = D._like(mbb, model), _d(nsrc)
    kw = dict(burn=burn, thin=thin, keep=False)
    a = results.chain_summary(like, chain, lnp, **_kw(model, 1.7, d, **kw))
    b = results.chain_summary(like, chain, lnp, **_kw(model, np.full(nsrc, 1.7), d, **kw))
    c = results.chain_summary(like, chain, lnp, **_kw(model, np.full(nsrc, 1.7), 950.0, **kw))
    e = results.chain_summary(like, chain, lnp, **_kw(model, 1.7, 950.0, **kw))          # the scalar path
    assert SR.raw_equal(a, b) and SR.raw_equal(c, e) and not SR.raw_equal(a, c, fields=("mean",))
    assert np.array_equal(a.arrays()["summary_redshift"], np.full(nsrc, 1.7))
    assert np.array_equal(e.arrays()["summary_lumdist_mpc"], np.full(nsrc, 950.0))
    one = results.chain_summary(like, chain[2], lnp[2], **_kw(model, np.array([1.7]), np.array([950.0]), **kw))
    ref = results.chain_summary(like, chain[2], lnp[2], **_kw(model, 1.7, 950.0, **kw))
    assert one.mean.shape == (8,) and SR.raw_equal(one, ref) and _source_equals(e, 2, ref)
    assert one.arrays()["summary_redshift"].shape == () and np.all(np.isfinite(one.mean))


# ---------------------------------------------------------------- 6. the resident chain of a catalogue run
def _catalogue(mbb, model, ns=3, nw=16):
    opthin, noalpha, _ = MODELS[model]
    rng = np.random.RandomState(29)
    truths = np.column_stack([rng.uniform(15, 40, ns), rng.uniform(1.2, 2.2, ns), rng.uniform(200, 700, ns),
                              rng.uniform(2, 4, ns), rng.uniform(10, 80, ns)])
    one = mbb.likelihood(response=False, opthin=opthin, noalpha=noalpha)
    one.set_phot(D.WAVE, np.ones(4), np.ones(4))
    flux = one.model_flux(truths)
    p0 = truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, nw, 5)))
    return flux, 0.1 * flux + 1.0, p0


@pytest.mark.parametrize("model", sorted(MODELS))
def test_resident_chain_of_a_catalogue_run(mbb, model):
    from mbb_emcee_amd import results
    opthin, noalpha, _ = MODELS[model]
    ns, nw, nsteps = 3, 16, 40
    flux, unc, p0 = _catalogue(mbb, model, ns, nw)
    z, d = _z(ns), _d(ns)
    kw = _kw(model, z, d, burn=5)
    like = mbb.likelihood(response=False, opthin=opthin, noalpha=noalpha)
    like.set_phot_multi(D.WAVE, flux, unc)
    sampler = mbb.DeviceEnsembleSampler(nw, 5, like, seed=41)
    bad = z.copy()
    bad[1] = -2.0
    with pytest.raises(ValueError, match="source 1"):                    # refused before the run
        sampler.run_mcmc(p0, nsteps, summary=dict(kw, redshift=bad))
    assert sampler.iterations == 0 and sampler.summary is None
    sampler.run_mcmc(p0, nsteps, storechain=True, summary=kw)
    assert sampler.chain.shape == (ns, nw, nsteps, 5)
    ref = results.chain_summary(like, sampler.chain, sampler.lnprobability, **kw)
    assert SR.raw_equal(sampler.summary, ref)
    assert np.all(ref.status == 0) and np.all(np.isfinite(ref.mean)) and np.all(ref.n_used == nw * 35)
    got = sampler.summary.lir_cen(95.4)                                  # not prepared: the zero-step re-summary
    assert got.shape == (ns, 3) and np.all(np.isfinite(got)) and np.array_equal(got, ref.lir_cen(95.4))
    assert np.array_equal(sampler.summary.dustmass_cen(95.4), ref.dustmass_cen(95.4))
    for g in range(ns):                                                  # ... with each source's own values
        one = results.chain_summary(D._like(mbb, model), sampler.chain[g], sampler.lnprobability[g],
                                    **_kw(model, z[g], d[g], burn=5))
        assert np.array_equal(got[g], one.lir_cen(95.4)), g
    # the same through the fitter
    fit = mbb.mbb_fitter(nwalkers=nw, response=False, opthin=opthin, noalpha=noalpha, seed=43)
    fit.like.set_phot_multi(D.WAVE, flux, unc)
    fit.run(5, nsteps, p0, summary=kw)
    fref = results.chain_summary(fit.like, fit.sampler.chain, fit.sampler.lnprobability, **kw)
    assert fit.summary is not None and SR.raw_equal(fit.summary, fref)
    assert np.array_equal(fit.summary.lir_cen(95.4), fref.lir_cen(95.4))
    assert np.array_equal(fit.summary.arrays()["summary_redshift"], z)


# ---------------------------------------------------------------- 7. validation through the C-ABI
def test_bad_entries_and_half_given_arrays_are_refused(mbb):
    from mbb_emcee_amd import results, _native
    model = "thick_walpha"
    nsrc, nw, nsteps, burn, thin = SMALL
    chain, lnp = _small()
    like, z, d = D._like(mbb, model), _z(nsrc), _d(nsrc)
    before = results.chain_summary(like, chain, lnp, keep=False, **_kw(model, 2.3, 18700.0))
    for arr, which, src, val in ((z, "redshift", 2, -1.5), (d, "lumdist_mpc", 0, 0.0), (z, "redshift", 4, np.inf),
                                 (d, "lumdist_mpc", 3, -np.inf), (z, "redshift", 1, -1.0)):
        bad = arr.copy()
        bad[src] = val
        with pytest.raises(ValueError, match="source %d" % src):
            results.chain_summary(like, chain, lnp, keep=False, **_kw(model, **{"z": z, "d": d, which: bad}))
    both = d.copy()                                                      # the first offending source is named
    both[[1, 4]] = 0.0
    with pytest.raises(ValueError, match="source 1"):
        results.chain_summary(like, chain, lnp, keep=False, **_kw(model, z, both))
    # not looked at when neither L_IR nor dust mass is asked for
    results.chain_summary(like, chain, lnp, keep=False, derived=("peaklambda",), redshift=z, lumdist_mpc=both)
    # a spec with one of the two pointers only
    req = results._Request([15.85, 84.15], derived=DERIVED, redshift=z, lumdist_mpc=d, nsources=nsrc)
    ctx = like._sync_device()
    for drop in ("src_redshift", "src_lumdist_mpc"):
        raw = results._Raw(nsrc, 2)
        spec, out = req.spec(), raw.out()
        setattr(spec, drop, None)
        rc = ctx.lib.mbb_chain_summary(ctx.h, _native._d(chain), _native._d(lnp), nsrc, nw, nsteps, C.byref(spec), C.byref(out))
        assert rc == -2 and b"both or neither" in ctx.lib.mbb_last_error()
    after = results.chain_summary(like, chain, lnp, keep=False, **_kw(model, 2.3, 18700.0))
    assert SR.raw_equal(before, after) and np.all(after.status == 0) and np.all(np.isfinite(after.mean))
