"""The derived columns of a chain summary (peak wavelength, L_IR, dust mass: summary_fill_derived in csrc/mbb_hip.hip,
k_sum_take / k_sum_lir / k_sum_dustmass and note_status in csrc/mbb_summary.hip.h) held per chain entry, across the
seam of the chunks they are filled by, inside and outside the burn / thin window, with clipping and with failing rows.

The independent reference: mbb_emcee_amd.postprocess (peak_wavelength, lir, dustmass -- pinned to the reference's own
results.py output by test_postprocess_vs_reference_results) on the windowed chain handed over as plain rows, then
numpy per source.  No offset, window or source arithmetic of the summary is shared with it; postprocess.dustmass is
host numpy, k_sum_dustmass the device's pow / expm1.

Bounds (all of them the suite's own, see tests/test_summary_gpu.py and test_postprocess_vs_reference_results):
  * n_used, best-fit index, the status bits: exact; a parameter column read out of one cell: the chain's bits;
  * per-entry peak wavelength and L_IR against postprocess: the same kernels with the same arguments in the same
    order, so bitwise equality is expected; relative 1e-13 is asserted and the number of entries that are not
    bitwise equal is printed;
  * per-entry dust mass: relative 1e-13; a row that exceeds it is evaluated in 50 digits (SR.dustmass_mp) and the
    device is held to 1e-13 of that;
  * means over many samples: 64 eps mean|x| plus the per-entry bound; percentiles: 4 ulp of the larger bracketing
    value plus the per-entry bound; min and max of a derived column: the per-entry bound.
"""
import numpy as np
import pytest

from conftest import ROOT, parity_record, rec_allclose
import _summary_ref as SR

pytestmark = pytest.mark.gpu

EPS = SR.EPS
Z, DL = 2.3, 18700.0
DERIVED = ("peaklambda", "lir", "dustmass")
ENTRY_RTOL = 1e-13
CHUNK = SR.chunk_rows(ROOT)
SHAPES = SR.seam_shapes(CHUNK)
WAVE = np.array([100.0, 250.0, 500.0, 850.0])                       # delta bands: the band set does not matter here
MODELS = {"thick_walpha": (False, False, {}),
          "thin_noalpha": (True, True, dict(kappa=1.5, kappa_wave=250.0, lir_range=(1000.0, 40.0)))}
_CACHE = {}


def test_chunk_length_is_the_one_the_shapes_are_for():
    """A change of kSumChunkRows must fail loudly, not silently un-test the seam."""
    assert CHUNK == 1 << 18
    assert SHAPES["cells"][0] == (64, 1, 4100) and SHAPES["windows"][0] == (3, 50, 1750, 7, 3)


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _like(mbb, model):
    """One likelihood (and so one device context, whose der buffer is reused from call to call) per model."""
    if ("like", model) not in _CACHE:
        opthin, noalpha, _ = MODELS[model]
        like = mbb.likelihood(response=False, opthin=opthin, noalpha=noalpha)
        like.set_phot(WAVE, np.full(4, 10.0), np.full(4, 2.0))
        _CACHE["like", model] = like
    return _CACHE["like", model]


def _kw(model, **more):
    kw = dict(derived=DERIVED, redshift=Z, lumdist_mpc=DL)
    kw.update(MODELS[model][2])
    kw.update(more)
    return kw


def _entries(mbb, model, rows, peak_model="fit"):
    """postprocess's per-entry values of plain rows [..., 5]: peaklambda, lir, dustmass."""
    from mbb_emcee_amd import postprocess as pp
    like, extra = _like(mbb, model), MODELS[model][2]
    rng = extra.get("lir_range", (8.0, 1000.0))
    return {"peaklambda": pp.peak_wavelength(like, rows, model=peak_model),
            "lir": pp.lir(like, rows, Z, DL, rng[0], rng[1]),
            "dustmass": pp.dustmass(like, rows, Z, DL, extra.get("kappa", 2.64), extra.get("kappa_wave", 125.0))}


def _cached(key, make):
    """A reference computed once and shared, read-only."""
    if key not in _CACHE:
        val = make()
        for a in (val.values() if isinstance(val, dict) else val if isinstance(val, tuple) else (val,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check_dust_entries(model, rows, got, host, what):
    """Per-entry dust mass: 1e-13 of the host closed form; where a row exceeds that, 50 digits decide."""
    rows, got, host = rows.reshape(-1, 5), np.ravel(got), np.ravel(host)
    rel = np.abs(got - host) / np.abs(host)
    parity_record("summary cell dustmass vs postprocess (rel)", rel.max(), ENTRY_RTOL)
    print("    %s dustmass: max rel %.3g over %d entries, %d not bitwise equal" % (what, rel.max(), got.size,
                                                                                 int((_bits(got) != _bits(host)).sum())))
    extra = MODELS[model][2]
    for i in np.flatnonzero(~(rel <= ENTRY_RTOL)):
        truth = SR.dustmass_mp(rows[i], MODELS[model][0], 500.0, Z, DL, extra.get("kappa", 2.64), extra.get("kappa_wave", 125.0))
        dev, hst = abs(got[i] - truth) / abs(truth), abs(host[i] - truth) / abs(truth)
        print("    row %s: device %.3g, host %.3g of the 50-digit value (%s is off)" % (rows[i], dev, hst,
                                                                                      "the device" if dev > hst else "the host"))
        parity_record("summary cell dustmass vs 50 digits (rel)", dev, ENTRY_RTOL)
        assert dev <= ENTRY_RTOL, (what, rows[i], got[i], host[i], truth)


def _check_entries(mbb, model, rows, got, what, peak_model="fit"):
    """got: {name: values} of the rows, against postprocess at the per-entry bounds."""
    ref = _entries(mbb, model, rows, peak_model)
    for nm in ("peaklambda", "lir"):
        print("    %s %s: %d of %d entries not bitwise equal" % (what, nm, int((_bits(got[nm]) != _bits(ref[nm])).sum()),
                                                               np.size(ref[nm])))
        rec_allclose(got[nm], ref[nm], rtol=ENTRY_RTOL, kind="summary cell %s vs postprocess" % nm)
    _check_dust_entries(model, rows, got["dustmass"], ref["dustmass"], what)


# ---------------------------------------------------------------- 1. one cell at a time, at the seam
@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("which", ["cells", "tail"])
def test_single_cells_at_the_chunk_seam(mbb, which, model):
    """burn=b, thin=nsteps summarises exactly the cell (s, 0, b) of every source: with 64 sources of one walker the
    cells b = 3843 / 3844 / 3845 of source 63 are the last row of the first chunk and the first two of the second; with
    one source of 2^18 + 1 steps the last chunk is one row.  Every column of every source is that one cell."""
    from mbb_emcee_amd import results
    (nsrc, nw, nsteps), steps = SHAPES[which]
    chain, lnp = _cached(("distinct", which), lambda: SR.distinct_chain(nsrc, nw, nsteps, seed=17 + nsteps % 7))
    like = _like(mbb, model)
    for b in steps:
        s = results.chain_summary(like, chain, lnp, burn=b, thin=nsteps, keep=False, **_kw(model))
        assert np.all(s.n_used == 1), (b, s.n_used)
        assert np.all(s.status == 0), (b, s.status)
        mean, pct = s.mean, s.percentiles[1]
        assert np.all(np.isfinite(mean))
        assert np.array_equal(_bits(s.min), _bits(mean)) and np.array_equal(_bits(s.max), _bits(mean)), b
        for k in range(pct.shape[-1]):
            assert np.array_equal(_bits(pct[..., k]), _bits(mean)), (b, k)
        cell = chain[:, 0, b, :]
        assert np.array_equal(_bits(mean[:, :5]), _bits(cell)), b
        bp, bv, bi = s.best_fit
        assert np.array_equal(bi, [[0, b]] * nsrc) and np.array_equal(_bits(bp), _bits(cell)) and np.array_equal(bv, lnp[:, 0, b])
        _check_entries(mbb, model, cell, {nm: mean[:, 5 + i] for i, nm in enumerate(DERIVED)}, "%s b=%d" % (which, b))


# ---------------------------------------------------------------- 2. windows, sources, sentinels, stale buffer
def _sentinel_case(shape):
    key = ("sentinel", shape)
    if key not in _CACHE:
        chain, lnp, inside, outside = SR.sentinel_chain(*shape, chunk=CHUNK, seed=5)
        chain.setflags(write=False)
        lnp.setflags(write=False)
        _CACHE[key] = (chain, lnp, inside, outside)
    return _CACHE[key]


def _window_entries(mbb, model, shape, peak_model):
    """The windowed chain as plain rows [nsrc, n, 5] and its per-entry reference, [nsrc, n] per derived column;
    computed once per model, shape and peak model."""
    win = _cached(("window", shape), lambda: SR.windowed(_sentinel_case(shape)[0], shape[3], shape[4]))

    def make():
        e = _entries(mbb, model, win.reshape(-1, 5), peak_model)
        return {k: np.ascontiguousarray(v.reshape(win.shape[:2])) for k, v in e.items()}
    return win, _cached(("entries", model, shape, peak_model), make)


def _check_column(got, g, slot, col, qs, entry, what, lo=None, hi=None):
    """Column `slot` of source g of a summary against numpy's statistics of the 1-d column `col` (clipped to [lo, hi]);
    `entry` is the per-entry relative bound of the column's values (0 for a parameter)."""
    ref = SR.column_reference(col, qs, lo, hi)
    assert got.n_used[g, slot] == ref["n"], (what, g, slot, got.n_used[g, slot], ref["n"])
    if entry == 0:
        assert got.min[g, slot] == ref["min"] and got.max[g, slot] == ref["max"], (what, g, slot)
    else:
        rec_allclose([got.min[g, slot], got.max[g, slot]], [ref["min"], ref["max"]], rtol=entry,
                     kind="summary derived min / max vs postprocess")
    bound = (64 * EPS + entry) * ref["scale"]
    rec_allclose((got.mean[g, slot] - ref["mean"]) / bound, 0.0, rtol=0, atol=1,
                 kind="summary column mean vs postprocess + numpy [its bound]")
    pct = got.percentiles[1]
    for k, q in enumerate(qs):
        a, b = SR.bracket(ref["sorted"], q)
        top = max(abs(a), abs(b))
        rec_allclose((pct[g, slot, k] - ref["pct"][k]) / (4 * np.spacing(top) + entry * top), 0.0, rtol=0, atol=1,
                     kind="summary column percentile vs postprocess + numpy [its bound]")


@pytest.mark.parametrize("model", sorted(MODELS))
@pytest.mark.parametrize("shape", SHAPES["windows"])
def test_windows_sources_sentinels_and_stale_buffer(mbb, shape, model):
    """Multi-source chains with a window whose chunk seam falls inside a source: every statistic of every column per
    source against postprocess + numpy.  Sentinel cells at the ends of everything (chain, chunks, windows, walkers,
    sources) hold each source's extreme derived values, their out-of-window neighbours hold values more extreme still,
    and the call before left T x 3, fnorm x 1000 in the same buffer: a cell filled at a wrong place, a cell not filled,
    or a step counted that the window drops shows in min, max or n_used."""
    from mbb_emcee_amd import results
    nsrc, nw, nsteps, burn, thin = shape
    chain, lnp, inside, outside = _sentinel_case(shape)
    like = _like(mbb, model)
    kw = _kw(model, percentile=(68.3, 95.4), burn=burn, thin=thin, keep=False)
    stale = chain.copy()
    stale[..., 0] *= 3.0
    stale[..., 4] *= 1000.0
    before = results.chain_summary(like, stale, lnp, **kw)
    nkept = len(range(burn, nsteps, thin))
    for peak_model in (("fit",) if model == "thick_walpha" else ("fit", "reference")):
        win, ent = _window_entries(mbb, model, shape, peak_model)
        s = results.chain_summary(like, chain, lnp, peak_model=peak_model, **kw)
        qs = s.percentiles[0]
        assert len(qs) == 4 and np.all(s.status == 0), s.status
        assert np.all(s.n_used == nw * nkept)
        for g in range(nsrc):
            for i in range(5):
                _check_column(s, g, i, win[g, :, i], qs, 0.0, "par")
            for i, nm in enumerate(DERIVED):
                _check_column(s, g, 5 + i, ent[nm][g], qs, ENTRY_RTOL, nm)
            # the test sees what it claims to: the extremes of the reference columns ARE this source's top sentinel,
            # the stale values and the out-of-window neighbours would win if they were read
            top = max((k, c) for c, k in inside.items() if c[0] == g)[1]
            j = top[1] * nkept + (top[2] - burn) // thin
            assert ent["peaklambda"][g].argmin() == j and ent["lir"][g].argmax() == j and ent["dustmass"][g].argmax() == j
            assert before.min[g, 5] < s.min[g, 5] and before.max[g, 6] > s.max[g, 6] and before.max[g, 7] > s.max[g, 7]
            out = [c for c in outside if c[0] == g]
            if out:
                eo = _entries(mbb, model, np.array([chain[c] for c in out]), peak_model)
                assert eo["peaklambda"].max() < s.min[g, 5] and eo["lir"].min() > s.max[g, 6] and \
                    eo["dustmass"].min() > s.max[g, 7]
        assert bool(outside) == (thin > 1)


# ---------------------------------------------------------------- 3. clip on a derived column, and on demand
def test_clip_on_derived_columns_and_on_demand(mbb):
    """clip= on lir (both sides) and dustmass (upper side), bounds at midpoints of adjacent per-entry values more than
    1e-6 apart (pooled over the sources, so no entry of any source can round across a bound), taken near the 20th and
    90th percentile of one source's column at a time: n_used exact for every source, 0 < n_used < n for that source,
    the clipped columns within the bounds, the others bit for bit those of the unclipped call; then lir_cen with those
    bounds and another percentile from the kept chain (the on-demand path) equals a fresh summary prepared with them."""
    from mbb_emcee_amd import results, _native
    model, shape = "thick_walpha", SHAPES["windows"][0]
    nsrc, nw, nsteps, burn, thin = shape
    chain, lnp, _, _ = _sentinel_case(shape)
    like = _like(mbb, model)
    win, ent = _window_entries(mbb, model, shape, "fit")
    n = win.shape[1]
    kw = _kw(model, percentile=(68.3, 95.4), burn=burn, thin=thin)
    plain = results.chain_summary(like, chain, lnp, keep=True, **kw)
    qs = plain.percentiles[0]
    pooled = {nm: np.sort(ent[nm].reshape(-1)) for nm in ("lir", "dustmass")}
    for g in range(nsrc):
        lo, gap_lo = SR.clip_midpoint(pooled["lir"], np.percentile(ent["lir"][g], 20))
        hi, gap_hi = SR.clip_midpoint(pooled["lir"], np.percentile(ent["lir"][g], 90))
        dhi, gap_d = SR.clip_midpoint(pooled["dustmass"], np.percentile(ent["dustmass"][g], 90))
        assert min(gap_lo, gap_hi, gap_d) > 1e-6 and lo < hi
        clip = {"lir": (lo, hi), "dustmass": (None, dhi)}
        c = results.chain_summary(like, chain, lnp, keep=False, clip=clip, **kw)
        assert 0 < c.n_used[g, 6] < n and 0 < c.n_used[g, 7] < n
        for h in range(nsrc):
            for slot, col, a, b in ((6, ent["lir"][h], lo, hi), (7, ent["dustmass"][h], None, dhi)):
                count = int(((col >= (-np.inf if a is None else a)) & (col <= b)).sum())
                assert c.n_used[h, slot] == count, (g, h, slot)
                if count:
                    _check_column(c, h, slot, col, qs, ENTRY_RTOL, "clipped", a, b)
                    assert c.status[h, slot] == 0
                else:
                    assert c.status[h, slot] == _native.SUM_EMPTY and np.isnan(c.mean[h, slot])
        for f in ("n_used", "mean", "min", "max", "pct", "status"):
            assert np.array_equal(getattr(c._raw, f)[:, :6], getattr(plain._raw, f)[:, :6]), f
        assert SR.raw_equal(c, plain, fields=("cov", "best", "best_index"))
        # on demand from the kept chain: 99.7 was not prepared, nor these bounds
        fresh = results.chain_summary(like, chain, lnp, keep=False, clip={"lir": (lo, hi)},
                                      **dict(kw, percentile=99.7))
        if np.any(fresh.status[:, 6] & _native.SUM_EMPTY):
            with pytest.raises(Exception, match="No elements survive"):
                plain.lir_cen(percentile=99.7, lowlim=lo, uplim=hi)
        else:
            assert np.array_equal(plain.lir_cen(percentile=99.7, lowlim=lo, uplim=hi), fresh.lir_cen(percentile=99.7, lowlim=lo, uplim=hi))
        one = results.chain_summary(like, chain[g], lnp[g], keep=True, **kw)                 # source g alone: values
        fresh1 = results.chain_summary(like, chain[g], lnp[g], keep=False, clip={"lir": (lo, hi)}, **dict(kw, percentile=99.7))
        got = one.lir_cen(percentile=99.7, lowlim=lo, uplim=hi)
        assert got.shape == (3,) and np.all(np.isfinite(got)) and np.array_equal(got, fresh1.lir_cen(percentile=99.7, lowlim=lo, uplim=hi))
        assert fresh1.n_used[6] == c.n_used[g, 6]
        key = (6, lo, hi, tuple(results._pval(99.7)))
        assert key in plain._cache                                      # (it did go through _again)
        again = plain._cache[key]
        for f in ("n_used", "mean", "min", "max", "pct", "status"):
            assert np.array_equal(getattr(again, f)[:, 6], getattr(fresh._raw, f)[:, 6], equal_nan=True), f


# ---------------------------------------------------------------- 4. row status through note_status
STATUS_SHAPE = (3, 20, 30, 5, 2)


def _status_case(mbb, cells, bad, **window):
    """The summary of the [3, 20, 30] chain with rows `cells` made bad by `bad(row)`, and the chain."""
    from mbb_emcee_amd import results
    nsrc, nw, nsteps, burn, thin = STATUS_SHAPE
    base, lnp = _cached(("distinct", "status"), lambda: SR.distinct_chain(nsrc, nw, nsteps, seed=23))
    chain = base.copy()
    for c in cells:
        bad(chain[c])
    kw = _kw("thick_walpha", burn=window.get("burn", burn), thin=window.get("thin", thin))
    return results.chain_summary(_like(mbb, "thick_walpha"), chain, lnp, **kw), chain


def _bad_alpha(row):
    row[3] = -1.0


def _nan_T(row):
    row[0] = np.nan


def _row_bit(code):
    from mbb_emcee_amd import _native
    return 1 << (_native.SUM_ROW_SHIFT + code)


def test_row_status_bad_alpha_inside_the_window(mbb):
    """(a) alpha = -1 in source 1 at a kept step: that source's peak-wavelength and L_IR columns carry the row's status
    (and the NaN the row gave), its dust mass -- which does not use alpha -- and the other sources carry nothing.
    lir_cen / peaklambda_cen raise what postprocess.lir raises for the same chain; they OR the status of all sources
    first, so the whole multi-source result raises, not source 1's part of it."""
    from mbb_emcee_amd import _native, postprocess as pp
    s, chain = _status_case(mbb, [(1, 7, 9)], _bad_alpha)
    want = _native.SUM_HAS_NAN | _row_bit(_native.ROW_BAD_ALPHA)
    st = s.status
    assert st[1, 5] == want and st[1, 6] == want, st
    st[1, 5] = st[1, 6] = 0
    assert np.all(st == 0), s.status
    assert np.isnan(s.mean[1, 5]) and np.isnan(s.mean[1, 6]) and np.all(np.isnan(s.percentiles[1][1, 5:7]))
    keep = [0, 2]
    assert np.all(np.isfinite(s.mean[keep])) and np.all(np.isfinite(s.percentiles[1][keep]))
    assert np.all(np.isfinite(s.mean[1, [0, 1, 2, 3, 4, 7]])) and np.all(s.n_used == 20 * 13)
    for fn in (s.lir_cen, s.peaklambda_cen):
        with pytest.raises(ValueError, match="alpha must be positive"):
            fn()
    assert np.all(np.isfinite(s.dustmass_cen())) and np.all(np.isfinite(s.par_cen("alpha")))
    with pytest.raises(ValueError, match="alpha must be positive"):
        pp.lir(_like(mbb, "thick_walpha"), chain, Z, DL)
    with pytest.raises(ValueError, match="alpha must be positive"):
        pp.peak_wavelength(_like(mbb, "thick_walpha"), chain)


@pytest.mark.parametrize("step", [4, 6])
def test_row_status_bad_alpha_outside_the_window(mbb, step):
    """(b) The same row in the burn-in (step 4) and at a step thin skips (step 6): no status, nothing raises, and every
    result is bit for bit that of the chain with a good row in that cell."""
    s, _ = _status_case(mbb, [(1, 7, step)], _bad_alpha)
    good, _ = _status_case(mbb, [(1, 7, step)], lambda row: row.__setitem__(3, 2.125))
    assert np.all(s.status == 0), s.status
    assert SR.raw_equal(s, good)
    for fn in (s.lir_cen, s.peaklambda_cen, s.dustmass_cen):
        assert np.all(np.isfinite(fn()))


def test_row_status_nan_temperature(mbb):
    """(c) A NaN temperature at a kept step of source 2: the non-finite row's status and the NaN flag, NaN mean and
    percentiles for that source's derived columns, no exception (a NaN in is a NaN out), the other sources untouched."""
    from mbb_emcee_amd import _native
    s, _ = _status_case(mbb, [(2, 0, 5)], _nan_T)
    clean, _ = _status_case(mbb, [], _nan_T)
    nan = _native.SUM_HAS_NAN
    st = s.status
    assert st[2, 5] == nan | _row_bit(_native.ROW_NONFINITE) and st[2, 6] == nan | _row_bit(_native.ROW_NONFINITE), st
    assert st[2, 7] == nan and st[2, 0] == nan and np.all(st[2, 1:5] == 0) and np.all(st[:2] == 0), st
    assert np.all(np.isnan(s.mean[2, 5:])) and np.all(np.isnan(s.percentiles[1][2, 5:]))
    for fn in (s.lir_cen, s.peaklambda_cen, s.dustmass_cen):
        got = fn()
        assert np.all(np.isnan(got[2])) and np.all(np.isfinite(got[:2]))
    for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best", "best_index"):
        assert np.array_equal(getattr(s._raw, f)[:2], getattr(clean._raw, f)[:2]), f
    assert np.all(clean.status == 0)


def test_row_status_at_the_ends_of_the_chain(mbb):
    """(d) The bad row in cell 0 and in the last cell of the last source: source and step rebuilt from the flat row
    index at both ends.  With burn 5, thin 2 only the last cell (step 29) is kept; with burn 0, thin 29 both are."""
    from mbb_emcee_amd import _native
    want = _native.SUM_HAS_NAN | _row_bit(_native.ROW_BAD_ALPHA)
    ends = [(0, 0, 0), (2, 19, 29)]
    s, _ = _status_case(mbb, ends, _bad_alpha)
    assert np.all(s.status[2, 5:7] == want) and s.status[2, 7] == 0 and np.all(s.status[2, :5] == 0), s.status
    assert np.all(s.status[:2] == 0), s.status
    s, _ = _status_case(mbb, ends, _bad_alpha, burn=0, thin=29)
    assert np.all(s.n_used == 40)
    assert np.all(s.status[[0, 2], 5:7] == want) and np.all(s.status[1] == 0), s.status
    assert np.all(s.status[[0, 2], 7] == 0) and np.all(s.status[:, :5] == 0), s.status
    for cell in ends:                                                   # each end alone, so neither hides the other
        s, _ = _status_case(mbb, [cell], _bad_alpha, burn=0, thin=29)
        for g in range(3):
            assert np.all(s.status[g, 5:7] == (want if g == cell[0] else 0)), (cell, s.status)


# ---------------------------------------------------------------- 5. the resident chain past the seam
def test_sampler_summary_of_a_resident_chain_past_the_seam(mbb):
    """mbb_sampler_run_summary's derived fill through a second chunk: 64 walkers, 4100 steps, run twice from the same
    state -- stored chain summarised by chain_summary, and storechain=False with summary= -- bitwise equal."""
    from mbb_emcee_amd import results
    nsrc, nw, nsteps = SHAPES["resident"]
    assert nsrc == 1 and nw * nsteps > CHUNK
    truth = np.array([25.0, 1.8, 500.0, 3.0, 40.0])
    like = mbb.likelihood(response=False)
    like.set_phot(WAVE, np.ones(4), np.ones(4))
    flux = like.model_flux(truth)[0]
    like.set_phot(WAVE, flux, 0.1 * flux + 1.0)
    p0 = truth * (1.0 + 0.02 * np.random.RandomState(11).normal(size=(nw, 5)))
    kw = dict(percentile=(68.3, 95.4), burn=100, thin=3, derived=DERIVED, redshift=Z, lumdist_mpc=DL)
    a = mbb.DeviceEnsembleSampler(nw, 5, like, seed=77)
    pa, la, _ = a.run_mcmc(p0, nsteps)
    assert a.chain.shape == (nw, nsteps, 5)
    ref = results.chain_summary(like, a.chain, a.lnprobability, **kw)
    b = mbb.DeviceEnsembleSampler(nw, 5, like, seed=77)
    pb, lb, _ = b.run_mcmc(p0, nsteps, storechain=False, summary=kw)
    assert b.chain.shape[-2] == 0
    assert np.array_equal(pa, pb) and np.array_equal(la, lb) and np.array_equal(a.naccepted, b.naccepted)
    assert np.all(ref.n_used == nw * len(range(100, nsteps, 3)))
    assert SR.raw_equal(b.summary, ref)
    assert np.all(ref.status == 0) and np.all(np.isfinite(ref.mean))
