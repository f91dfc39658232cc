"""What tests/test_domain_paths_gpu.py relies on, asserted with the oracle alone (no GPU): the GPU tests leave out
(row, band) cells whose flux is next to 0, rows the oracle cannot build and nothing else, and hold the device's
frequency integral to a reference that must itself be good everywhere.  Here:

  * the oracle builds every wide and grid row in all four models and finds its peak;
  * at least 90% of the (row, band) fluxes exceed 1e-280, so the relative check covers the bulk of each set;
  * lir_reference (scipy's quad in log nu, split at the kinks) raises no integration warning and estimates its own
    error at <= 1e-12 of the value on EVERY row, range and model;
  * the rows put the merge wavelength and lambda0 below, inside and above the integration ranges, and nu0 beyond the
    merge point (the piece the clamp of the break points empties), often enough to test each arrangement;
  * the device's fixed rule (three pieces, eight panels of 64 Gauss-Legendre nodes in log nu), restated in numpy and fed
    the oracle's f_nu, is within 1e-13 of lir_reference on all of them: the rule is adequate over the whole volume, so
    a GPU failure points at the kernel and not at the design.
"""
import numpy as np
import pytest

from conftest import VARIANTS, golden_bands
import _domain_rows as D


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_oracle_builds_every_row_and_finds_its_peak(oracle, name, opthin, noalpha):
    for rows in (D.wide_rows(), D.grid_rows()):
        for p in rows:
            peak = oracle.OracleSED(*p, opthin=opthin, noalpha=noalpha).max_wave()      # (raises on a failure)
            assert np.isfinite(peak) and peak > 0, p


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_most_band_fluxes_are_far_from_zero(oracle, g_pb, name, opthin, noalpha):
    for rows, names, flux in ((D.wide_rows(), D.WIDE_BANDS, D.WIDE_FLUX), (D.grid_rows(), D.GRID_BANDS, D.GRID_FLUX)):
        orc = oracle.OracleLikelihood(flux, D.unc_of(flux), bands=golden_bands(g_pb, names), opthin=opthin,
                                      noalpha=noalpha, lowlim=np.full(5, -np.inf), has_uplim=[0] * 6)
        model = orc(rows, return_flux=True)[1]
        assert np.all(orc.status == 0) and not np.isnan(model).any()
        big = model > D.FLUX_FLOOR
        print("    %s: %d of %d fluxes above %g, smallest %.3g" % (name, big.sum(), big.size, D.FLUX_FLOOR, model.min()))
        assert big.sum() >= 0.9 * big.size


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_lir_reference_is_good_on_every_row(oracle, name, opthin, noalpha):
    val, err = D.lir_table(oracle, opthin, noalpha)                     # (an integration warning raises there)
    assert val.shape == (120 + 225, 3) and np.all(np.isfinite(val)) and np.all(val > 0)
    rel = err / val
    print("    %s: worst error estimate %.3g of the value" % (name, rel.max()))
    assert np.all(rel <= 1e-12), np.argwhere(~(rel <= 1e-12))


def _places(w, lo, hi):
    """0, 1, 2: the wavelength lies below, inside, above [lo, hi]"""
    return 0 if w < lo else (1 if w <= hi else 2)


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_rows_put_the_break_points_everywhere(oracle, name, opthin, noalpha):
    """Counted over the every-fifth wide rows, the three ranges together."""
    wide = D.lir_rows()[0]
    merge, lam0, beyond = np.zeros(3, dtype=int), np.zeros(3, dtype=int), 0
    for p in wide:
        sed = oracle.OracleSED(*p, opthin=opthin, noalpha=noalpha)
        wm, w0 = D.breaks_um(sed, opthin, noalpha, p[2])
        for lo, hi in D.RANGES:
            if wm is not None:
                merge[_places(wm, lo, hi)] += 1
            if w0 is not None:
                lam0[_places(w0, lo, hi)] += 1
        beyond += int(wm is not None and w0 is not None and w0 < wm)
    print("    %s: merge wavelength below / inside / above %s, lambda0 %s, lambda0 < merge wavelength in %d rows"
          % (name, merge, lam0, beyond))
    if not noalpha:
        assert np.all(merge >= 5), merge
    if not opthin:
        assert np.all(lam0 >= 5), lam0
    if not noalpha and not opthin:
        assert beyond >= 20


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_the_fixed_rule_is_adequate_everywhere(oracle, name, opthin, noalpha):
    val, _ = D.lir_table(oracle, opthin, noalpha)
    rows = np.concatenate(D.lir_rows())
    worst = 0.0
    for i, p in enumerate(rows):
        sed = oracle.OracleSED(*p, opthin=opthin, noalpha=noalpha)
        for j, (lo, hi) in enumerate(D.RANGES):
            rule = D.device_rule(sed, lo, hi, opthin, noalpha, p[2])
            rel = abs(rule - val[i, j]) / val[i, j]
            assert rel <= 1e-13, (p, (lo, hi), rule, val[i, j], rel)
            worst = max(worst, rel)
    print("    %s: the rule's worst distance from the reference %.3g" % (name, worst))
