"""Predicted fluxes on the GPU (csrc/mbb_predict.hip.h through mbb_chain_predict / mbb_sampler_predict and
mbb_emcee_amd/predict.py) against ``postprocess.predict_flux`` and numpy, and against the columns the reference's own
``mbb_results._predict_flux`` made (tests/golden/results.npz, predict/*).

Tolerances, and where they come from:
  * per entry: a wavelength's value is f_nu itself, bit for bit what ``postprocess.predict_flux`` gets from
    mbb_sed_eval_batch; f_nu and band fluxes are held to the reference's columns at relative 1e-12.  The
    device's band sum (lane-strided partial sums and a fixed tree) and the likelihood kernel's, which
    ``postprocess.predict_flux`` uses, order the same samples differently: relative 1e-12 between them as well;
  * statistics of a column whose entries are known bit for bit (a wavelength's ``postprocess.predict_flux`` column, or
    the device's own per-entry column read back through a 1 x 1 window per entry): the mean within 64 eps mean|x| of
    numpy's, percentiles within 4 ulp of numpy's inside the bracket of their two order statistics, min and max exact,
    ``predflux_cen`` half-widths within test_summary_gpu.py's bound for ``par_cen`` half-widths;
  * statistics against a column known to relative 1e-12 only (``postprocess.predict_flux``'s band columns, the
    fixture's columns): a mean or an order statistic moves by no more than the largest per-entry difference, so the
    bound above plus 1e-12 of the column's largest magnitude (2e-12 for a half-width, a difference of two such).  The
    whole difference, nothing taken off, is what is compared and recorded there, in units of the column's largest
    magnitude and under kinds of its own ("... vs a 1e-12 column");
  * counts, status bits and everything said to be "the same bits": exact.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, rec_allclose
import _predict_ref as PR
import _summary_ref as SR

pytestmark = pytest.mark.gpu

EPS = SR.EPS
VARIANTS = [("thin_walpha", True, False), ("thick_walpha", False, False),
            ("thick_noalpha", False, True), ("thin_noalpha", True, True)]
SPECS = [70.0, 1100.0, "SPIRE_250um", "SCUBA2_450um"]           # (SCUBA2_450um is in no fit of this suite)
RAW_FIELDS = ("n_used", "mean", "min", "max", "pct", "status")
NW, NSTEPS = 34, 64
_CACHE = {}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _like(mbb, opthin=False, noalpha=False):
    key = ("like", opthin, noalpha)
    if key not in _CACHE:
        _CACHE[key] = mbb.likelihood(response=True, opthin=opthin, noalpha=noalpha)
    return _CACHE[key]


def _name(spec):
    return spec if isinstance(spec, str) else "%g" % spec


def _entries(mbb, like, chain, specs):
    """The device's own per-entry values [rows, nspec]: every chain row as a source of one walker and one step, whose
    mean is the cell's value.  Made once per (model, specs) -- the chain is that model's fixture chain -- and shared."""
    key = ("entries", like.opthin, like.noalpha, tuple(specs))
    if key in _CACHE:
        return _CACHE[key]
    rows = np.ascontiguousarray(chain).reshape(-1, 1, 1, 5)
    p = mbb.chain_predictions(like, rows, specs, keep=False)
    assert np.all(p.n_used == 1) and np.all(p.status == 0)
    qs, pct = p.percentiles
    for k in range(len(qs)):                                        # one sample: every percentile, min and max are it
        assert np.array_equal(pct[..., k], p.mean)
    assert np.array_equal(p.min, p.mean) and np.array_equal(p.max, p.mean)
    _CACHE[key] = p.mean
    _CACHE[key].setflags(write=False)
    return _CACHE[key]


def _same_bits(a, b, cols_a=None, cols_b=None):
    """Two ChainPredictions hold the same bits (NaNs at the same places), in the given spec columns."""
    for f in RAW_FIELDS:
        x, y = getattr(a._raw, f), getattr(b._raw, f)
        x = x if cols_a is None else x[:, cols_a]
        y = y if cols_b is None else y[:, cols_b]
        if not np.array_equal(x, y, equal_nan=True):
            return False
    return True


def _check_stats(p, i, col, qs, exact, label, lo=None, hi=None):
    """Spec i of a single-source result against numpy on the 1-d column `col` (what _parcen_internal is given).  `exact`:
    the column is the device's bit for bit; else it is known to relative 1e-12."""
    ref = PR.stats(col, qs, lo, hi)
    top = np.abs(col).max()
    assert p.n_used[i] == ref["n"], (label, p.n_used[i], ref["n"])
    got_pct = p.percentiles[1][i]
    if exact:
        err = abs(p.mean[i] - ref["mean"]) / (EPS * ref["scale"])
        print("    %s: n %d mean err %.3g eps mean|x|" % (label, ref["n"], err))
        rec_allclose(err, 0.0, rtol=0, atol=64, kind="predict mean [eps mean|x|]")
        for k, q in enumerate(qs):
            a, b = SR.bracket(ref["sorted"], q)
            rec_allclose(SR.ulps_off(got_pct[k], ref["pct"][k], a, b), 0.0, rtol=0, atol=4, kind="predict percentile [ulp]")
        assert p.min[i] == ref["min"] and p.max[i] == ref["max"], label
        return ref
    # the column is known to 1e-12 of its largest magnitude: that, and the exact column's bound, in those units
    err = abs(p.mean[i] - ref["mean"]) / top
    print("    %s: n %d mean off %.3g of the column's max" % (label, ref["n"], err))
    rec_allclose(err, 0.0, rtol=0, atol=1e-12 + 64 * EPS * ref["scale"] / top, kind="predict mean vs a 1e-12 column [column max]")
    for k, q in enumerate(qs):
        a, b = SR.bracket(ref["sorted"], q)
        rec_allclose(abs(got_pct[k] - ref["pct"][k]) / top, 0.0, rtol=0, atol=1e-12 + 4 * np.spacing(max(abs(a), abs(b))) / top,
                     kind="predict percentile vs a 1e-12 column [column max]")
    rec_allclose([abs(p.min[i] - ref["min"]) / top, abs(p.max[i] - ref["max"]) / top], 0.0, rtol=0, atol=1e-12,
                 kind="predict min, max vs a 1e-12 column [column max]")
    return ref


def _check_cen(got, col, percentile, exact, label, lo=None, hi=None):
    """[mean, upper - mean, mean - lower] against _parcen_internal's formula on `col`: test_summary_gpu.py's bound for
    par_cen half-widths, plus the per-entry term where the column is known to 1e-12 only."""
    want, _ = SR.parcen(col, percentile, lo, hi)
    x = np.asarray(col)
    if lo is not None:
        x = x[x >= lo]
    if hi is not None:
        x = x[x <= hi]
    srt, scale, top = np.sort(x), np.abs(x).mean(), np.abs(x).max()
    if exact:
        rec_allclose(abs(got[0] - want[0]) / (EPS * scale), 0.0, rtol=0, atol=64, kind="predict mean [eps mean|x|]")
    else:
        rec_allclose(abs(got[0] - want[0]) / top, 0.0, rtol=0, atol=1e-12 + 64 * EPS * scale / top,
                     kind="predict mean vs a 1e-12 column [column max]")
    for c, q in ((1, 100 - 0.5 * (100 - percentile)), (2, 0.5 * (100 - percentile))):
        a, b = SR.bracket(srt, q)
        bound = 4 * np.spacing(max(abs(a), abs(b))) + 64 * EPS * scale + EPS * abs(want[c])
        off = abs(got[c] - want[c])
        if exact:
            print("    %s half-width %d: off %.3g of its bound" % (label, c, off / bound))
            rec_allclose(off / bound, 0.0, rtol=0, atol=1, kind="predflux_cen half-width [its bound]")
        else:
            print("    %s half-width %d: off %.3g of the column's max" % (label, c, off / top))
            rec_allclose(off / top, 0.0, rtol=0, atol=2e-12 + bound / top,
                         kind="predflux_cen half-width vs a 1e-12 column [column max]")


# ---------------------------------------------------------------- 1. per entry
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_per_entry_values(mbb, g_res, name, opthin, noalpha):
    """1. The fixture chain (32 x 16) as 512 sources of 1 walker x 1 step: the mean is the cell's value.  Wavelengths:
    bit for bit postprocess.predict_flux, <= 1e-12 from the fixture; bands (one of them in no fit): <= 1e-12 from both."""
    from mbb_emcee_amd import postprocess as pp
    like = _like(mbb, opthin, noalpha)
    chain = g_res[name + "/chain"]
    got = _entries(mbb, like, chain, SPECS).reshape(32, 16, len(SPECS))
    host = pp.predict_flux(like, chain, SPECS)
    for i, s in enumerate(SPECS):
        fixture = g_res[name + "/predict/" + _name(s)]
        if isinstance(s, str):
            rec_allclose(got[..., i], host[..., i], rtol=1e-12, kind="predicted band flux vs predict_flux")
        else:
            assert np.array_equal(got[..., i], host[..., i]), (name, s)
        rec_allclose(got[..., i], fixture, rtol=1e-12, kind="predicted flux vs the reference's")
    # a multi-source predflux_cen has a leading source axis; one sample: both half-widths are zero
    p = mbb.chain_predictions(like, chain.reshape(512, 1, 1, 5), [1100.0])
    cen = p.predflux_cen(1100.0)
    assert cen.shape == (512, 3) and np.array_equal(cen[:, 0], got[..., 1].reshape(-1)) and np.all(cen[:, 1:] == 0)


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS[:2])
def test_per_entry_values_at_another_wavenorm(mbb, g_res, name, opthin, noalpha):
    """1b. The spec's own normalisation wavelength (Q18: the fit's unless given), 850 um where the context's is 500:
    per entry against postprocess.predict_flux at that wavenorm -- wavelengths bit for bit, a band to 1e-12 --, the
    flux at 850 um is then fnorm itself, and the numbers are not those of the context's wavenorm."""
    from mbb_emcee_amd import postprocess as pp
    like = _like(mbb, opthin, noalpha)
    assert like.wavenorm == 500.0
    chain = g_res[name + "/chain"]
    specs = [70.0, 850.0, "SPIRE_250um", "SCUBA2_450um"]
    rows = np.ascontiguousarray(chain).reshape(-1, 1, 1, 5)
    p = mbb.chain_predictions(like, rows, specs, wavenorm=850.0, keep=False)
    assert np.all(p.n_used == 1) and np.all(p.status == 0)
    got = p.mean.reshape(32, 16, len(specs))
    host = pp.predict_flux(like, chain, specs, wavenorm=850.0)
    for i, s in enumerate(specs):
        if isinstance(s, str):
            rec_allclose(got[..., i], host[..., i], rtol=1e-12, kind="predicted band flux vs predict_flux")
        else:
            assert np.array_equal(got[..., i], host[..., i]), (name, s)
    rec_allclose(got[..., 1], chain[..., 4], rtol=1e-13, kind="f_nu(wavenorm) = fnorm")
    own = mbb.chain_predictions(like, rows, specs, keep=False).mean.reshape(32, 16, len(specs))
    assert np.all(np.abs(own / got - 1.0) > 1e-3)                     # (the context's 500 um gives other numbers)
    same = mbb.chain_predictions(like, rows, specs, wavenorm=500.0, keep=False).mean.reshape(32, 16, len(specs))
    assert np.array_equal(same, own)                                   # ... and 500 given is 500 taken from the context
    # on demand, a result goes back to the chain with the wavenorm it was made with
    one = mbb.chain_predictions(like, chain, specs, wavenorm=850.0)
    ref = mbb.chain_predictions(like, chain, specs, percentile=95.4, wavenorm=850.0, keep=False)
    assert np.array_equal(one.predflux_cen("SPIRE_250um", percentile=95.4), ref.predflux_cen("SPIRE_250um", percentile=95.4))


# ---------------------------------------------------------------- 2. statistics
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_statistics_of_one_source(mbb, g_res, name, opthin, noalpha):
    """2. The same chain as one source of 32 walkers x 16 steps: n_used, mean, min, max, percentiles and predflux_cen
    against numpy on postprocess.predict_flux's column and on the device's own per-entry column, and against
    _parcen_internal's formula on the fixture's column."""
    from mbb_emcee_amd import postprocess as pp
    like = _like(mbb, opthin, noalpha)
    chain = g_res[name + "/chain"]
    own = _entries(mbb, like, chain, SPECS).reshape(32, 16, len(SPECS))
    host = pp.predict_flux(like, chain, SPECS)
    p = mbb.chain_predictions(like, chain, SPECS, percentile=(68.3, 95.4), percentiles=(50.0, 0.0, 100.0))
    qs = p.percentiles[0]
    assert len(qs) == 7 and p.mean.shape == (4,) and p.percentiles[1].shape == (4, 7) and np.all(p.status == 0)
    assert p.nwalkers == 32 and p.nsteps_used == 16 and p.specs == SPECS
    for i, s in enumerate(SPECS):
        band = isinstance(s, str)
        _check_stats(p, i, PR.windowed_column(own[..., i]), qs, True, "%s %s own column" % (name, _name(s)))
        _check_stats(p, i, PR.windowed_column(host[..., i]), qs, not band, "%s %s predict_flux" % (name, _name(s)))
        fixture = PR.windowed_column(g_res[name + "/predict/" + _name(s)])
        for pc in (68.3, 95.4):
            got = p.predflux_cen(s, percentile=pc)
            assert got.shape == (3,)
            _check_cen(got, PR.windowed_column(own[..., i]), pc, True, "%s %s %g own" % (name, _name(s), pc))
            _check_cen(got, PR.windowed_column(host[..., i]), pc, not band, "%s %s %g predict_flux" % (name, _name(s), pc))
            _check_cen(got, fixture, pc, False, "%s %s %g fixture" % (name, _name(s), pc))
    waves, lower, mid, upper = p.sed_band()
    assert np.array_equal(waves, [70.0, 1100.0]) and np.array_equal(mid, p.mean[:2])
    c = p.predflux_cen(70.0)
    assert lower[0] == c[0] - c[2] and upper[0] == c[0] + c[1]
    assert "Predicted flux SCUBA2_450um" in str(p) and set(p.arrays()) >= {"predict_mean", "predict_specs"}
    # the same bits on every call
    assert _same_bits(p, mbb.chain_predictions(like, chain, SPECS, percentile=(68.3, 95.4), percentiles=(50.0, 0.0, 100.0)))


# ---------------------------------------------------------------- 3. grouping
def test_results_do_not_depend_on_the_grouping(mbb, g_res):
    """3. nspec = 1, 3, 4 and 7 of the same specs in different orders: every spec's outputs are bit for bit those of
    the spec alone (columns are made three at a time; a spec meets other neighbours, other places in its group and
    other staging of the sample lists in every call)."""
    like = _like(mbb)
    chain = g_res["thick_walpha/chain"]
    seven = [70.0, "SPIRE_250um", 1100.0, "SCUBA2_450um", 250.0, "GISMO_2mm", 450.0]
    kw = dict(percentile=(68.3, 95.4), burn=3, thin=2, keep=False)
    alone = {_name(s): mbb.chain_predictions(like, chain, [s], **kw) for s in seven}
    for s in seven:
        assert alone[_name(s)].n_used[0] == 32 * 7 and alone[_name(s)].status[0] == 0
    orders = [[seven[5], seven[0], seven[3]], [seven[3], seven[1], seven[6], seven[5]], seven, seven[::-1],
              [seven[i] for i in (2, 5, 1, 6, 3, 0, 4)]]
    for specs in orders:
        p = mbb.chain_predictions(like, chain, specs, **kw)
        for i, s in enumerate(specs):
            assert _same_bits(p, alone[_name(s)], [i], [0]), (specs, s)
    # ... and a multi-source call gives each source what it gets alone
    c3 = np.ascontiguousarray(chain.reshape(2, 16, 16, 5))
    p = mbb.chain_predictions(like, c3, seven[:4], **kw)
    for s in range(2):
        q = mbb.chain_predictions(like, c3[s], seven[:4], **kw)
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(p._raw, f)[s], getattr(q._raw, f)[0]), (s, f)


# ---------------------------------------------------------------- 4. chunk seam
def test_chunk_seam(mbb):
    """4. One source of 2^18 + 3 rows (the fill takes kSumChunkRows = 2^18 rows at a time) with burn leaving the last
    five steps, two before the seam and three after it: with five samples the percentiles 0, 25, 50, 75, 100 ARE the
    five cells, and the five rows' fluxes rise with the step.  Then the whole chain: min, max and mean of both chunks."""
    from mbb_emcee_amd import postprocess as pp
    chunk = SR.chunk_rows(ROOT)
    assert chunk == 1 << 18
    n = chunk + 3
    rng = np.random.RandomState(18)
    chain = (SR.BOX_LO + (SR.BOX_HI - SR.BOX_LO) * rng.rand(n, 5)).reshape(1, n, 5)
    last = np.arange(n - 5, n)
    chain[0, last] = [25.0, 1.8, 500.0, 3.0, 30.0]
    chain[0, last, 4] = 100.0 * 2.0 ** np.arange(5)                 # fnorm: the flux doubles from step to step
    like = _like(mbb)
    specs = [433.0, "SPIRE_250um"]
    p = mbb.chain_predictions(like, chain, specs, percentile=(50.0, 100.0), percentiles=(50.0,), burn=n - 5, keep=False)
    assert p.percentiles[0] == [25.0, 75.0, 0.0, 100.0, 50.0] and np.all(p.n_used == 5) and np.all(p.status == 0)
    cells = p.percentiles[1][:, [2, 0, 4, 1, 3]]                    # [spec, step]
    want = pp.predict_flux(like, chain[0, last], specs)              # [step, spec]
    assert np.all(np.diff(want, axis=0) > 0)
    assert np.array_equal(cells[0], want[:, 0]), (cells[0], want[:, 0])
    rec_allclose(cells[1], want[:, 1], rtol=1e-12, kind="predicted band flux vs predict_flux")
    assert np.array_equal(p.min, cells[:, 0]) and np.array_equal(p.max, cells[:, 4])
    # every row of both chunks: the wavelength column is predict_flux's bit for bit
    full = mbb.chain_predictions(like, chain, [433.0], percentile=68.3, keep=False)
    col = pp.predict_flux(like, chain[0], 433.0)
    _check_stats(full, 0, col, full.percentiles[0], True, "seam, all rows")
    thin = mbb.chain_predictions(like, chain, [433.0], percentile=68.3, burn=chunk - 4, thin=3, keep=False)
    _check_stats(thin, 0, col[chunk - 4::3], thin.percentiles[0], True, "seam, thinned across it")


# ---------------------------------------------------------------- 5. windows
def _window_chain():
    rng = np.random.RandomState(5)
    return SR.BOX_LO + (SR.BOX_HI - SR.BOX_LO) * rng.rand(3, 5, 40, 5)


def test_windows_and_failing_rows(mbb):
    """5. Three sources with burn and thin; a row with a failing alpha outside the window -- no status bit, no raise,
    the numbers of the chain without it --, then inside: the row-status bit on that source (every spec of it) and on no
    other, NaN statistics there, and predflux_cen raises as postprocess.predict_flux does.  A NaN-T cell gives HAS_NAN
    and a NaN mean without a raise."""
    from mbb_emcee_amd import postprocess as pp, _native
    like = _like(mbb)
    burn, thin = 7, 3
    specs = [70.0, "SPIRE_250um", 1100.0, "SCUBA2_450um"]
    kw = dict(burn=burn, thin=thin, keep=False)
    good = _window_chain()
    base = mbb.chain_predictions(like, good, specs, **kw)
    assert np.all(base.status == 0) and np.all(base.n_used == 5 * 11) and base.mean.shape == (3, 4)
    host = pp.predict_flux(like, good, specs)
    for s in range(3):
        one = mbb.chain_predictions(like, good[s], specs, **kw)
        for i, sp in enumerate(specs):
            _check_stats(one, i, PR.windowed_column(host[s, ..., i], burn, thin), one.percentiles[0], not isinstance(sp, str),
                         "window source %d %s" % (s, _name(sp)))
            assert one.mean[i] == base.mean[s, i]
    out = good.copy()
    out[1, 2, 8, 3] = -1.0                                          # step 8 is not kept: 7, 10, 13, ...
    p = mbb.chain_predictions(like, out, specs, **kw)
    assert _same_bits(p, base)
    assert p.predflux_cen(70.0).shape == (3, 3)
    ins = good.copy()
    ins[1, 2, 10, 3] = -1.0
    p = mbb.chain_predictions(like, ins, specs, **kw)
    bit = 1 << (_native.SUM_ROW_SHIFT + _native.ROW_BAD_ALPHA)
    assert np.all(p.status[1] == (bit | _native.SUM_HAS_NAN)) and np.all(p.status[[0, 2]] == 0)
    assert np.all(np.isnan(p.mean[1])) and np.all(np.isnan(p.percentiles[1][1])) and np.all(p.n_used[1] == 55)
    assert np.array_equal(p.mean[[0, 2]], base.mean[[0, 2]])
    with pytest.raises(ValueError, match="alpha must be positive"):
        pp.predict_flux(like, ins, 70.0)
    for sp in specs:
        with pytest.raises(ValueError, match="alpha must be positive"):
            p.predflux_cen(sp)
    nan = good.copy()
    nan[2, 0, 13, 0] = np.nan
    p = mbb.chain_predictions(like, nan, specs, **kw)
    assert np.all(p.status[2] & _native.SUM_HAS_NAN) and np.all(p.status[:2] == 0)
    assert not np.any(p.status[2] & _native.SUM_EMPTY)
    cen = p.predflux_cen("SPIRE_250um")
    assert np.all(np.isnan(cen[2])) and np.array_equal(cen[:2, 0], base.mean[:2, 1])
    assert np.all(np.isnan(pp.predict_flux(like, nan, 70.0)[2, 0, 13]))


# ---------------------------------------------------------------- 6. clip
def test_clip_per_spec(mbb, g_res):
    """6. A clip per spec against numpy; a clip that empties one spec sets EMPTY there and nowhere else and raises the
    reference's exception; the on-demand clip from the kept chain equals the prepared one bit for bit."""
    from mbb_emcee_amd import postprocess as pp, _native
    like = _like(mbb)
    chain = g_res["thick_walpha/chain"]
    own = _entries(mbb, like, chain, SPECS).reshape(32, 16, len(SPECS))
    bounds = {}
    for i, s in enumerate(SPECS):
        srt = np.sort(own[..., i].reshape(-1))
        lo, gap = SR.clip_midpoint(srt, srt[100])
        hi, gap2 = SR.clip_midpoint(srt, srt[430])
        assert min(gap, gap2) > 1e-6 and lo < hi
        bounds[s] = (lo, hi)
    clip = {70.0: bounds[70.0], 1100.0: (None, bounds[1100.0][1]), "SPIRE_250um": (bounds["SPIRE_250um"][0], None)}
    p = mbb.chain_predictions(like, chain, SPECS, percentile=(68.3, 95.4), clip=clip)
    plain = mbb.chain_predictions(like, chain, SPECS, percentile=(68.3, 95.4))
    qs = p.percentiles[0]
    for i, s in enumerate(SPECS):
        lo, hi = clip.get(s, (None, None))
        ref = _check_stats(p, i, PR.windowed_column(own[..., i]), qs, True, "clip %s" % _name(s), lo, hi)
        assert (ref["n"] < 512) == (s in clip)
        got = p.predflux_cen(s, lowlim=lo, uplim=hi)
        _check_cen(got, PR.windowed_column(own[..., i]), 68.3, True, "clip %s" % _name(s), lo, hi)
        # on demand, from the chain the unclipped result kept: one call for this spec alone
        assert np.array_equal(plain.predflux_cen(s, lowlim=lo, uplim=hi), got)
        assert np.array_equal(plain.predflux_cen(s, percentile=95.4, lowlim=lo, uplim=hi),
                              p.predflux_cen(s, percentile=95.4, lowlim=lo, uplim=hi))
    assert _same_bits(p, plain, [3], [3])                                   # the spec without a clip: untouched
    gone = mbb.chain_predictions(like, chain, SPECS, clip={"SPIRE_250um": (1e30, None)})
    assert gone.status[2] == _native.SUM_EMPTY and gone.n_used[2] == 0 and np.isnan(gone.mean[2])
    assert np.all(gone.status[[0, 1, 3]] == 0)
    for f in ("n_used", "mean", "min", "max", "status"):
        assert np.array_equal(getattr(gone._raw, f)[:, [0, 1, 3]], getattr(plain._raw, f)[:, [0, 1, 3]])
    with pytest.raises(Exception, match="No elements survive lower/upper limit clipping"):
        gone.predflux_cen("SPIRE_250um", lowlim=1e30)
    with pytest.raises(Exception, match="No elements survive lower/upper limit clipping"):
        plain.predflux_cen(70.0, uplim=-1.0)                                 # on demand
    assert gone.predflux_cen(70.0).shape == (3,)
    dropped = mbb.chain_predictions(like, chain, SPECS, keep=False)
    with pytest.raises(RuntimeError, match="the chain was not kept"):
        dropped.predflux_cen(70.0, uplim=1.0)


# ---------------------------------------------------------------- 7. sizes
def _native_call(like, chain4, off, freq, weight, qs=(50.0,), burn=0, thin=1, clip=None, wavenorm=0.0, edit=None, nsteps=None):
    """mbb_chain_predict with sample lists of the test's own making; returns (rc, raw)."""
    from mbb_emcee_amd import _native, predict
    ctx = _native.analysis_context(like)
    nsrc, nw, ns = chain4.shape[:3]
    nspec = len(off) - 1
    raw = predict._Raw(nsrc, max(nspec, 1), max(len(qs), 1))
    s = _native.PredictSpec()
    s.nspec, s.npct, s.burn, s.thin, s.wavenorm = nspec, len(qs), burn, thin, wavenorm
    for i, q in enumerate(qs[:8]):
        s.pct[i] = q
    keep = [np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(freq, dtype=np.float64),
            np.ascontiguousarray(weight, dtype=np.float64)]
    s.sample_off, s.freq, s.weight = _native._i(keep[0]), _native._d(keep[1]), _native._d(keep[2])
    if clip is not None:
        keep += [np.ascontiguousarray(a, dtype=t) for a, t in zip(clip, (np.int32, np.int32, np.float64, np.float64))]
        s.has_lo, s.has_hi, s.lo, s.hi = _native._i(keep[3]), _native._i(keep[4]), _native._d(keep[5]), _native._d(keep[6])
    out = raw.out()
    if edit:
        edit(s, out)
    rc = ctx.lib.mbb_chain_predict(ctx.h, _native._d(chain4), nsrc, nw, ns if nsteps is None else nsteps,
                                   C.byref(s), C.byref(out))
    return rc, raw, ctx


def _synthetic_lists(counts, seed):
    """Sample lists of the given lengths: frequencies over the far infrared in GHz, positive weights summing to 1."""
    rng = np.random.RandomState(seed)
    off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    freq = np.concatenate([np.sort(rng.uniform(150.0, 6000.0, c)) for c in counts])
    weight = np.concatenate([(lambda w: w / w.sum())(rng.uniform(0.5, 1.5, c)) for c in counts])
    return off, freq, weight


def _list_reference(like, rows, off, freq, weight):
    """sum_i f_nu(freq_i) weight_i per row and spec from mbb_sed_eval_batch's values, summed by numpy."""
    f, st = like.context.sed_eval(rows, like.opthin, like.noalpha, like.wavenorm, freq)
    assert np.all(st == 0)
    return np.stack([(f[:, off[i]:off[i + 1]] * weight[off[i]:off[i + 1]]).sum(axis=1) for i in range(len(off) - 1)], axis=1)


def test_sizes(mbb, g_res):
    """7. One and three samples per column; a band of fewer than 64 samples (GISMO_2mm, 53), bands whose counts are no
    multiple of 64, a delta-function band; the maximum number of specs; the maximum total of samples, with the sample
    lists of a group at the LDS limit exactly (staged), one beyond it (read from global memory: the same bits), and far
    beyond it."""
    from mbb_emcee_amd import postprocess as pp, _native
    from mbb_emcee_amd.modified_blackbody import um_to_GHz
    like = mbb.likelihood(response=True)
    like._responsewheel.add_special("Line_delta_450um")
    chain = g_res["thick_walpha/chain"]
    specs = ["GISMO_2mm", "SPIRE_250um", "Line_delta_450um", 450.0, "PACS_70um"]
    assert [like._responsewheel[s].quadrature()[0].size for s in specs if isinstance(s, str)] == [53, 189, 1, 370]
    for shape in ((1, 1), (3, 1), (1, 3)):
        sub = np.ascontiguousarray(chain[:shape[0], :shape[1]])
        p = mbb.chain_predictions(like, sub, specs, percentile=(68.3,), percentiles=(50.0,), keep=False)
        host = pp.predict_flux(like, sub, ["GISMO_2mm", "SPIRE_250um", 450.0, 450.0, "PACS_70um"])
        n = shape[0] * shape[1]
        assert np.all(p.n_used == n) and np.all(p.status == 0)
        for i, s in enumerate(specs):
            col = host[..., i].reshape(-1)
            if i in (2, 3):                                              # the delta band IS the wavelength
                assert np.array_equal(np.sort(col)[[0, -1]], [p.min[i], p.max[i]]) and p.percentiles[1][i, 2] == np.median(col)
            else:
                rec_allclose([p.min[i], p.max[i], p.percentiles[1][i, 2]], [col.min(), col.max(), np.median(col)],
                             rtol=1e-12, kind="predicted band flux vs predict_flux")
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(p._raw, f)[:, 2], getattr(p._raw, f)[:, 3]), f
    # the maximum number of specs, all wavelengths
    waves = list(np.geomspace(20.0, 2000.0, _native.PRED_MAX_SPECS))
    p = mbb.chain_predictions(like, chain, waves, keep=False)
    host = pp.predict_flux(like, chain, waves)
    for i in (0, 1, 2, 3, 63, 125, 126, 127):
        _check_stats(p, i, PR.windowed_column(host[..., i]), p.percentiles[0], True, "128 specs, %d" % i)
    assert np.array_equal(p.max, host.reshape(512, -1).max(axis=0)) and np.array_equal(p.min, host.reshape(512, -1).min(axis=0))
    assert np.array_equal(p.sed_band()[0], waves)
    # sample lists of the test's own making through the C-ABI: 32 rows, every row a source
    rows = np.ascontiguousarray(chain[:2].reshape(32, 1, 1, 5))
    lds = 2560                                                          # kLdsSamples
    src = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_predict.hip.h")).read()
    assert "constexpr int kLdsSamples = %d;" % lds in src
    fits = _synthetic_lists([853, 853, 854], 7)
    assert fits[0][-1] == lds
    rc, staged, _ = _native_call(like, rows, *fits)
    assert rc == 0 and np.all(staged.n_used == 1) and np.all(staged.status == 0)
    rec_allclose(staged.mean, _list_reference(like, rows.reshape(32, 5), *fits), rtol=1e-12, kind="predicted list flux")
    off2 = np.array([0, 853, 1706, 2560, 2561], dtype=np.int32)          # the same three, and a fourth: no change
    f2, w2 = np.append(fits[1], 1234.5), np.append(fits[2], 1.0)
    rc, four, _ = _native_call(like, rows, off2, f2, w2)
    assert rc == 0 and np.array_equal(four.mean[:, :3], staged.mean)
    single = like.context.sed_eval(rows.reshape(32, 5), like.opthin, like.noalpha, like.wavenorm, np.array([1234.5]))[0][:, 0]
    assert np.array_equal(four.mean[:, 3], single)                       # one sample of weight 1: f_nu itself
    # one sample more in the group: 2561, past the limit -- the lists are read from global memory
    off3 = np.array([0, 853, 1706, 2561], dtype=np.int32)
    f3 = np.concatenate((fits[1], [fits[1][-1] + 1.0]))
    w3 = np.concatenate((fits[2], [0.25]))
    rc, beyond, _ = _native_call(like, rows, off3, f3, w3)
    assert rc == 0 and np.array_equal(beyond.mean[:, :2], staged.mean[:, :2])          # the same bits either way
    rec_allclose(beyond.mean, _list_reference(like, rows.reshape(32, 5), off3, f3, w3), rtol=1e-12, kind="predicted list flux")
    # the maximum total: 32 specs of 1024 samples -- ten groups of 3072 (global) and one of 2048 (staged)
    assert _native.PRED_MAX_SAMPLES == 32 * 1024
    big = _synthetic_lists([1024] * 32, 8)
    rc, mx, _ = _native_call(like, rows, *big)
    assert rc == 0 and np.all(mx.status == 0)
    rec_allclose(mx.mean, _list_reference(like, rows.reshape(32, 5), *big), rtol=1e-12, kind="predicted list flux")
    rc, alone, _ = _native_call(like, rows, big[0][:2], big[1][:1024], big[2][:1024])    # spec 0 alone: staged
    assert rc == 0 and np.array_equal(alone.mean[:, 0], mx.mean[:, 0])


# ---------------------------------------------------------------- 8. stale buffers
def test_stale_buffers(mbb, g_res):
    """8. A larger call (more specs, more samples, more percentiles, a longer chain of more sources) followed by a smaller
    one gives what the smaller gives alone, bit for bit."""
    like = mbb.likelihood(response=True)
    chain = g_res["thick_walpha/chain"]
    small = np.ascontiguousarray(chain[:3, :5])
    kw = dict(percentile=68.3, burn=1, keep=False)
    first = mbb.chain_predictions(like, small, [1100.0, "GISMO_2mm"], **kw)
    rng = np.random.RandomState(8)
    large = SR.BOX_LO + (SR.BOX_HI - SR.BOX_LO) * rng.rand(5, 16, 300, 5)
    large[3, 2, 100, 3] = -1.0                                              # (its status bits must not stay behind)
    big = mbb.chain_predictions(like, large, [70.0, "SPIRE_250um", 1100.0, "SCUBA2_450um", 250.0, "GISMO_2mm", 450.0],
                                percentile=(68.3, 95.4, 99.7), keep=False)
    assert big.mean.shape == (5, 7) and np.all(big.status[3] != 0)
    again = mbb.chain_predictions(like, small, [1100.0, "GISMO_2mm"], **kw)
    assert _same_bits(first, again)
    fresh = mbb.chain_predictions(mbb.likelihood(response=True), small, [1100.0, "GISMO_2mm"], **kw)
    assert _same_bits(first, fresh)


# ---------------------------------------------------------------- 9. resident
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
    return lk, p0, bands


@pytest.mark.parametrize("multi", [False, True])
def test_resident_chain(mbb, g_lnl, multi):
    """9. run_mcmc(storechain=False, summary=..., predict=...) equals chain_predictions on the chain a storechain=True
    run of the same seed brings back, bit for bit; predictions() afterwards gives the same; and the summary, the
    diagnostics and the marginals of that run are bit for bit what they are without predict= -- also a percentile asked
    of the summary after the prediction ran (the derived-column block is shared)."""
    lk, p0, bands = _sampler_case(mbb, g_lnl, multi)
    specs = [bands[3], 70.0, "SCUBA2_450um", 1100.0, bands[0]]
    a = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.predictions_ is None
    host = mbb.chain_predictions(lk, a.chain, specs, percentile=(68.3, 95.4), burn=5, thin=2)
    res = a.predictions(specs, percentile=(68.3, 95.4), burn=5, thin=2)
    assert _same_bits(res, host) and res.nsteps_used == 30 and res.nwalkers == NW
    assert res.mean.shape == ((3, 5) if multi else (5,)) and np.all(res.status == 0) and np.all(res.n_used == NW * 30)
    skw = dict(burn=5, thin=2, derived=("peaklambda",), percentile=(68.3, 95.4))
    mkw = dict(bins=24, bins2d=6)
    b = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b.run_mcmc(p0, NSTEPS, storechain=False, summary=dict(skw), convergence=True, marginals=dict(mkw),
               predict=dict(specs=specs, percentile=(68.3, 95.4)))
    assert b.chain.shape[-2] == 0 and b.predictions_.burn == 5 and b.predictions_.thin == 2       # the summary's window
    assert _same_bits(b.predictions_, host)
    assert _same_bits(b.predictions(specs, percentile=(68.3, 95.4), burn=5, thin=2), host)
    # on demand from the resident chain: another interval, a clip
    assert np.array_equal(b.predictions_.predflux_cen("SCUBA2_450um", percentile=90.0),
                          host.predflux_cen("SCUBA2_450um", percentile=90.0))
    lim = float(np.max(host.mean[..., 1]))          # (every source keeps the samples below its own mean at least)
    assert np.array_equal(b.predictions_.predflux_cen(70.0, uplim=lim), host.predflux_cen(70.0, uplim=lim))
    c = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    c.run_mcmc(p0, NSTEPS, storechain=False, summary=dict(skw), convergence=True, marginals=dict(mkw))
    assert c.predictions_ is None
    assert SR.raw_equal(b.summary, c.summary)
    for f in ("tau", "ess", "rhat", "window", "status"):
        assert np.array_equal(getattr(b.convergence_, f), getattr(c.convergence_, f), equal_nan=True), f
    for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below", "n_above", "n_nonfinite", "status"):
        assert np.array_equal(getattr(b.marginals_._raw, f), getattr(c.marginals_._raw, f), equal_nan=True), f
    # after the prediction has used the derived-column block: the summary's own on-demand columns, the diagnostics and
    # the marginals from the resident chain
    b.predictions(specs, burn=5, thin=2)
    assert np.array_equal(b.summary.peaklambda_cen(90.0), c.summary.peaklambda_cen(90.0))
    assert np.array_equal(b.summary.par_cen(0, 90.0, lowlim=1.0), c.summary.par_cen(0, 90.0, lowlim=1.0))
    assert np.array_equal(b.convergence(burn=5).tau, c.convergence(burn=5).tau)
    mb, mc = b.marginals(derived=("peaklambda",), **mkw), c.marginals(derived=("peaklambda",), **mkw)
    for f in ("counts1", "edges1", "counts2", "status"):
        assert np.array_equal(getattr(mb._raw, f), getattr(mc._raw, f), equal_nan=True), f
    held, handed = b.predictions_, b.predictions(specs, burn=5, thin=2)
    before = handed.predflux_cen(70.0)
    b.run_mcmc(None, 3, storechain=False)                   # the next run: nothing of it is resident
    assert b.predictions_ is None
    with pytest.raises(RuntimeError, match="the chain was not kept"):
        held.predflux_cen(70.0, percentile=12.0)
    # a result predictions() handed out goes with the chain as well -- also when the next run leaves another chain
    # resident, which must never answer for the old one
    with pytest.raises(RuntimeError, match="the chain was not kept"):
        handed.predflux_cen(70.0, percentile=12.0)
    a_handed = a.predictions(specs, burn=5, thin=2)
    a.run_mcmc(None, 40)                                     # (a chain of another length is resident now)
    for ask in (lambda: a_handed.predflux_cen(70.0, percentile=95.4), lambda: a_handed.predflux_cen(70.0, uplim=lim),
                lambda: a_handed.sed_band(90.0)):
        with pytest.raises(RuntimeError, match="the chain was not kept"):
            ask()
    assert np.array_equal(a_handed.predflux_cen(70.0), before) and a_handed.nsteps_used == 30      # what it was made with
    assert a.predictions(specs, burn=5, thin=2).nsteps_used == 18
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.predictions(70.0)
    b.run_mcmc(None, 9, predict=[450.0])
    assert b.predictions_.nsteps_used == 9 and b.predictions_.specs == [450.0]
    b.reset()
    assert b.predictions_ is None


def test_fitter_and_cli_predictions(mbb, g_lnl, tmp_path, capsys):
    """mbb_fitter.run(..., predict=...) and the CLI's --predict end to end: the numbers are those of the chain the fit
    returns; without the flag nothing new is printed or written."""
    from mbb_emcee_amd import run_mbb_emcee
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    flux = one.model_flux(truth)[0]
    fit = mbb.mbb_fitter(nwalkers=NW, response=True, seed=3)
    fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    specs = [70.0, "SCUBA2_450um", 1100.0]
    fit.run(20, NSTEPS, p0, predict=specs)
    assert fit.predictions is not None and fit.summary is None and fit.marginals is None
    assert _same_bits(fit.predictions, mbb.chain_predictions(fit.like, fit.sampler.chain, specs))
    fit.run(20, 16, p0, predict=dict(specs=specs, burn=2), summary=True, marginals=True)
    assert _same_bits(fit.predictions, mbb.chain_predictions(fit.like, fit.sampler.chain, specs, burn=2))
    fit.run(20, 16, p0)
    assert fit.predictions is None                                       # the default leaves none
    capsys.readouterr()
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", str(NW), "-b", "20", "-N", str(NSTEPS), "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--predict", "70,SCUBA2_450um,1100"]) == 0
    text = capsys.readouterr().out
    assert text.count("Predicted flux") == 3 and "Predicted flux SCUBA2_450um:" in text
    got = np.load(out)
    new = {"predict_specs", "predict_n_used", "predict_mean", "predict_min", "predict_max", "predict_q",
           "predict_percentiles", "predict_status"}
    assert new <= set(got.files)
    like = mbb.likelihood(response=True)
    want = mbb.chain_predictions(like, got["chain"], specs)
    assert np.array_equal(got["predict_mean"], want.mean) and np.array_equal(got["predict_percentiles"], want.percentiles[1])
    assert list(got["predict_specs"]) == ["70.0", "SCUBA2_450um", "1100.0"] and np.all(got["predict_n_used"] == NW * NSTEPS)
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == "" and not new & set(np.load(out).files)


# ---------------------------------------------------------------- 10. refusals
def test_native_refusals_leave_the_context_usable(mbb, g_res, g_lnl):
    """10. The C-ABI's MBB_ERR_ARG refusals, each before anything is allocated or uploaded and each followed by a good
    call that gives the right answer; mbb_sampler_predict's MBB_ERR_STATE without a resident chain."""
    from mbb_emcee_amd import _native, predict
    like = mbb.likelihood(response=True)
    chain = np.ascontiguousarray(g_res["thick_walpha/chain"][None, :7, :])          # 1 x 7 x 16
    ok = _synthetic_lists([5, 1, 70], 3)
    rc, ref, ctx = _native_call(like, chain, *ok, qs=(16.0, 84.0), burn=2)
    assert rc == 0 and np.all(ref.n_used == 7 * 14)

    def good():
        rc, raw, _ = _native_call(like, chain, *ok, qs=(16.0, 84.0), burn=2)
        assert rc == 0
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(raw, f), getattr(ref, f), equal_nan=True), f

    def lists(arr, i, v):
        """The good lists with one frequency ("f") or weight ("w") replaced."""
        off, f, w = _synthetic_lists([5, 1, 70], 3)
        (f if arr == "f" else w)[i] = v
        return off, f, w

    inf, nan = float("inf"), float("nan")
    bad = [(dict(lists=([0], [1.0], [1.0])), "specs per"),                                   # nspec 0
           (dict(lists=_synthetic_lists([1] * (_native.PRED_MAX_SPECS + 1), 1)), "specs per"),
           (dict(lists=(np.array([0, 5, 5, 76]),) + ok[1:]), "no samples"),
           (dict(lists=(np.array([0, 5, 4, 76]),) + ok[1:]), "no samples"),
           (dict(lists=(np.array([1, 5, 6, 76]),) + ok[1:]), "start at 0"),
           (dict(lists=_synthetic_lists([1024] * 32 + [1], 2)), "samples in a prediction"),
           (dict(lists=lists("f", 3, 0.0)), "frequency"), (dict(lists=lists("f", 75, -5.0)), "frequency"),
           (dict(lists=lists("f", 0, inf)), "frequency"), (dict(lists=lists("f", 6, nan)), "frequency"),
           (dict(lists=lists("w", 2, inf)), "weight"), (dict(lists=lists("w", 75, nan)), "weight"),
           (dict(qs=()), "percentiles per"), (dict(qs=tuple(range(9))), "percentiles per"),
           (dict(qs=(50.0, 100.5)), "[0, 100]"), (dict(qs=(-1.0,)), "[0, 100]"), (dict(qs=(nan,)), "[0, 100]"),
           (dict(burn=16), "burn"), (dict(burn=-1), "burn"), (dict(thin=0), "burn"),
           (dict(wavenorm=-500.0), "wavenorm"), (dict(wavenorm=nan), "wavenorm"),
           (dict(nsteps=0), "empty chain")]
    for kw, msg in bad:
        kw = dict(kw)
        ls = kw.pop("lists", ok)
        kw.setdefault("qs", (16.0, 84.0))
        kw.setdefault("burn", 2)
        rc, _, _ = _native_call(like, chain, *ls, **kw)
        assert rc == -2 and msg in ctx.lib.mbb_last_error().decode(), (msg, rc, ctx.lib.mbb_last_error())
        good()
    # more than 2^32 - 1 samples per column: refused from the shape alone, before the (far too short) chain is read
    s = _native.PredictSpec()
    s.nspec, s.npct, s.burn, s.thin = 1, 1, 0, 1
    s.pct[0] = 50.0
    keep = [np.array([0, 1], dtype=np.int32), np.array([600.0]), np.ones(1)]
    s.sample_off, s.freq, s.weight = _native._i(keep[0]), _native._d(keep[1]), _native._d(keep[2])
    raw = predict._Raw(1, 1, 1)
    out = raw.out()
    assert ctx.lib.mbb_chain_predict(ctx.h, _native._d(chain), 1, 1 << 16, 1 << 16, C.byref(s), C.byref(out)) == -2
    assert "2^32 - 1 samples per column" in ctx.lib.mbb_last_error().decode()
    good()

    def drop(field, of_spec):
        def edit(spec, out):
            setattr(spec if of_spec else out, field, None)
        return edit
    for field in ("sample_off", "freq", "weight"):
        assert _native_call(like, chain, *ok, edit=drop(field, True))[0] == -2
    for field in ("n_used", "mean", "min", "max", "pct", "status"):
        assert _native_call(like, chain, *ok, edit=drop(field, False))[0] == -2
    clip = ([1, 0, 0], [0, 0, 1], [0.0, 0.0, 0.0], [0.0, 0.0, 1e30])
    assert _native_call(like, chain, *ok, clip=clip)[0] == 0
    assert _native_call(like, chain, *ok, clip=clip, edit=drop("hi", True))[0] == -2          # all four or none
    assert "go together" in ctx.lib.mbb_last_error().decode()
    assert ctx.lib.mbb_chain_predict(ctx.h, None, 1, 7, 16, C.byref(s), C.byref(out)) == -2
    assert ctx.lib.mbb_chain_predict(ctx.h, _native._d(chain), 1, 7, 16, None, C.byref(out)) == -2
    assert ctx.lib.mbb_chain_predict(ctx.h, _native._d(chain), 1, 7, 16, C.byref(s), None) == -2
    good()
    # the sampler call
    lk, p0, _ = _sampler_case(mbb, g_lnl, False)
    sm = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=5)
    sctx, h = sm._handle()
    assert sctx.lib.mbb_sampler_predict(sctx.h, h, C.byref(s), C.byref(out)) == -3
    assert "resident" in sctx.lib.mbb_last_error().decode()
    sm.run_mcmc(p0, 8, storechain=False)
    assert sctx.lib.mbb_sampler_predict(sctx.h, h, C.byref(s), C.byref(out)) == -3
    sm.run_mcmc(None, 8)
    assert sctx.lib.mbb_sampler_predict(sctx.h, h, C.byref(s), C.byref(out)) == 0 and raw.n_used[0, 0] == NW * 8
    assert sctx.lib.mbb_sampler_predict(sctx.h, h, None, C.byref(out)) == -2
    assert sctx.lib.mbb_sampler_predict(sctx.h, h, C.byref(s), None) == -2
    assert sctx.lib.mbb_sampler_predict(sctx.h, None, C.byref(s), C.byref(out)) == -2
    s.npct = 0
    assert sctx.lib.mbb_sampler_predict(sctx.h, h, C.byref(s), C.byref(out)) == -2
    s.npct = 1
    assert sctx.lib.mbb_sampler_predict(sctx.h, h, C.byref(s), C.byref(out)) == 0
    assert _same_bits(sm.predictions(500.0), mbb.chain_predictions(lk, sm.chain, 500.0))


def test_sharded_run_is_refused_by_the_library():
    """10 (the sharded case).  Two ranks as processes on this GPU with a communicator over tests/rccl_standin/: a rank
    holds only its own walkers' chain, so mbb_sampler_predict answers MBB_ERR_STATE as mbb_sampler_diagnostics does, and
    run_mcmc(predict=) says so before anything runs (tests/_predict_rank_worker.py)."""
    import subprocess
    from _filecomm import launch
    d = os.path.join(ROOT, "tests", "rccl_standin")
    so, src = os.path.join(d, "librccl_standin.so"), os.path.join(d, "rccl_standin.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-shared", "-fPIC", "-o", so, src, "-lrt"])
    ok, text = launch(os.path.join(ROOT, "tests", "_predict_rank_worker.py"), 2, extra_env={"MBB_RCCL_LIB": so}, timeout=300.0)
    assert ok and "PREDICT_RANKS_OK 0" in text and "PREDICT_RANKS_OK 1" in text, text[-6000:]
