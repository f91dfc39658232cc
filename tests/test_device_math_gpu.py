"""The device's fp64 primitives (mbb_math.hip.h), the row forms, the table look-up, the SED constructor and the
per-sample f_nu of the hot loop (mbb_device.hip.h) against the TRUE values: the mpmath fixtures
tests/golden/hp_math.npz and hp_sed.npz (tests/golden/make_golden_hp.py) and, for the dense sweeps, numpy's
longdouble (held to mpmath by tests/test_device_math_cpu.py).  The functions are reached through the test-only
probe tests/_device_probe.hip, which includes the product's headers and is built with the product's device flags;
the constructor's rows also go through the product's own entry point and must match the probe bit for bit.

Needs an MI355X: `pytest -m gpu`.  Every test says how many points it checked and fails if that is not the number
the fixture holds: nothing is left out for being awkward.
"""
import os

import numpy as np
import pytest

import _hp_common as hp
from conftest import VARIANTS, parity_record

pytestmark = pytest.mark.gpu

FUNCS = ("m_exp", "m_exp_t", "m_expm1", "m_log", "m_div")
N_SED_ROWS, N_FNU_ROWS, N_FREQ = 1584, 64, 48
N_SWEEP = 4000000
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def g_math():
    return np.load(os.path.join(hp.GOLDEN, "hp_math.npz"))


@pytest.fixture(scope="module")
def g_hps():
    return np.load(os.path.join(hp.GOLDEN, "hp_sed.npz"))


@pytest.fixture(scope="module")
def probe():
    p = hp.probe_module().load()
    assert not p.is_host
    return p


@pytest.fixture(scope="module")
def ctx():
    from mbb_emcee_amd import _native
    return _native.default_context()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------ 1. primitives
@pytest.mark.parametrize("f", FUNCS)
def test_primitives_on_the_curated_points(probe, g_math, f):
    """mbb_math.hip.h's contract in ulp of the true value (mpmath, double-double), on the points where such functions
    go wrong: the ends of the range (subnormal results in subnormal spacing), the seams of both reductions, 0 and
    tiny arguments, 2^-k for expm1, both sides of sqrt(1/2) at every binade for log, the whole exponent range and
    the clamp for the division.  m_exp, m_exp_t, m_expm1, m_log <= 2 ulp, m_div <= 1.5; beyond the range exactly 0,
    inf or -1; never NaN, never below 0 (-1)."""
    worst, n = hp.check_curated(probe, g_math, f, record=parity_record)
    assert n == g_math[f + "/x"].size >= 1200


@pytest.mark.skipif(not hp.LD_OK, reason=hp.LD_REASON)
@pytest.mark.parametrize("f", FUNCS)
def test_primitives_dense_sweep(probe, f):
    """4e6 seeded points per function against longdouble, same bounds."""
    x, y, ref = hp.sweep_args(f, N_SWEEP, seed=20261016)
    got = probe.math(f, x, y)
    err = np.abs(hp.ulp_err_ld(got, ref))
    assert err.size == N_SWEEP and np.isfinite(ref.astype(np.float64)).all() and np.isfinite(err).all()
    w = err.argmax()
    print("%s: %d points, max %.3f ulp at x = %r%s: got %r, longdouble %r" % (
        f, N_SWEEP, err[w], x[w], "" if y is None else " / %r" % y[w], got[w], ref[w]))
    parity_record(f + " dense sweep (ulp)", err[w], hp.ULP_BOUND[f])
    assert err[w] <= hp.ULP_BOUND[f]


def test_exp_family_outside_the_range(probe):
    """Below -746 exactly 0 (expm1: -1), above 709.79 exactly +inf, and no NaN or negative value from any finite
    argument m_exp / m_expm1 accept (all of them) or m_exp_t accepts (|x| < 1e90, its header)."""
    rng = np.random.RandomState(5)
    n = 200000
    mag = 10.0 ** rng.uniform(-320, 89.9, n)
    x = np.concatenate([mag, -mag, -746.0 - 10.0 ** rng.uniform(-3, 89.9, n), 709.79 + 10.0 ** rng.uniform(-3, 89.9, n)])
    for f in ("m_exp", "m_exp_t", "m_expm1"):
        got = probe.math(f, x)
        assert got.size == 4 * n and not np.isnan(got).any(), (f, x[np.isnan(got)][:5])
        assert np.all(got >= (-1.0 if f == "m_expm1" else 0.0))
        lo, hi = got[2 * n:3 * n], got[3 * n:]
        assert np.all(lo == (-1.0 if f == "m_expm1" else 0.0)) and np.all(hi == np.inf), f
    big = np.concatenate([10.0 ** rng.uniform(90, 308, 1000), -10.0 ** rng.uniform(90, 308, 1000), [np.inf, -np.inf]])
    for f in ("m_exp", "m_expm1"):                      # (clamped at +-800: infinities included)
        got = probe.math(f, big)
        assert np.array_equal(got, np.where(big > 0, np.inf, -1.0 if f == "m_expm1" else 0.0)), f


def test_m_div_outside_its_domain_is_what_the_header_says(probe):
    """mbb_math.hip.h states m_div's domain -- b normal and at most 8e307 in size, the quotient finite -- and what comes
    back outside it; this holds the statement to the device.  (a) 1/b overflows (|b| < 2^-1024, subnormal): v_rcp_f64
    gives inf and the Newton step inf (2 - b inf) = -inf: NOT IEEE's +inf, but never a finite value.  (b) the quotient
    overflows: a r = inf, the residual inf - inf: NaN, never a finite value.  (c) b above 8e307, +inf included, is taken
    for 8e307 (fixture, kind 2: within 1.5 ulp of a / 8e307, so 0 only for a = 0)."""
    b = np.array([5e-324, 1e-320, 1e-312, 1e-310, 5.5e-309, -1e-310, -5e-324])
    a = np.array([1.0, 1e10, 1e-5, -3.0, 2.0, 1.0, 7.0])
    got = probe.math("m_div", a, b)
    print("m_div, 1/b overflows:", list(zip(a, b, got)))
    assert not np.isfinite(got).any()
    a = np.array([1e300, 1e308, 1e200, -1e200, 1.7e308, 3.0])
    b = np.array([1e-10, 0.5, 1e-200, 1e-200, 0.9, 1e-308])
    got = probe.math("m_div", a, b)
    print("m_div, the quotient overflows:", list(zip(a, b, got)))
    assert not np.isfinite(got).any()
    # (and the smallest normal denominators are inside the domain)
    b = np.array([2.2250738585072014e-308, 4.4501477170144028e-308, -2.2250738585072014e-308])
    got = probe.math("m_div", np.array([1.0, 1.0, 1.0]), b)
    assert np.array_equal(got, 1.0 / b)


# ------------------------------------------------------ 2. row forms = lane forms
def _row_args(islog, k, n, rng):
    if islog:
        a = np.exp(rng.uniform(-700.0, 700.0, (n, k)))
        a[::7] = 0.5 + rng.uniform(size=(a[::7].shape))
        return a
    a = -745.0 + 1455.0 * rng.uniform(size=(n, k))
    a[1::3] = rng.uniform(-40, 40, a[1::3].shape)
    a[2::3] = rng.uniform(-1, 1, a[2::3].shape)
    a[5::11] = rng.uniform(709.0, 711.0, a[5::11].shape)          # across 2^k's overflow
    return a


@pytest.mark.parametrize("block", [64, 256])
def test_row_forms_equal_lane_forms_bit_for_bit(probe, block):
    """vexp<true, M1, K> and vlog<true, K> -- row_pick, one evaluation per lane, DPP row_newbcast -- return in EVERY
    lane of the row exactly what vexp<false> / vlog<false> return for the same arguments, for every (M1, K) the
    product's sources instantiate (tests/test_device_math_cpu.py holds the probe's list to the sources).  Consecutive
    elements sit in consecutive rows, so the four rows of a wave hold different arguments; the count is not a
    multiple of four, so the last wave is ragged.  The lane form in turn is m_exp / m_expm1 / m_log of the argument,
    the functions of the ulp tests above, bit for bit."""
    insts = probe.row_instantiations()
    assert insts == hp.probe_row_instantiations_in_source() and len(insts) == 11
    rng = np.random.RandomState(31 + block)
    n = 4099
    checked = 0
    for i, (islog, m1, k) in enumerate(insts):
        args = _row_args(islog, k, n, rng)
        row, lane = probe.rows(i, args, block)
        assert row.shape == (n, 16, k) and lane.shape == (n, k)
        same = bits(row) == bits(lane)[:, None, :]
        assert same.all(), "instantiation %s, block %d: %d of %d lane values differ, first at element %r" % (
            (islog, m1, k), block, (~same).sum(), same.size, np.argwhere(~same)[0])
        for j in range(k):
            f = "m_log" if islog else ("m_expm1" if (m1 >> j) & 1 else "m_exp")
            assert np.array_equal(bits(lane[:, j]), bits(probe.math(f, args[:, j]))), (islog, m1, k, j)
        assert not np.isnan(lane).any()
        checked += same.size
    assert checked == n * 16 * sum(k for _, _, k in insts)


# -------------------------------------------------------- 3. the table look-up
@pytest.mark.skipif(not hp.LD_OK, reason=hp.LD_REASON)
@pytest.mark.parametrize("which", ["b", "c"])
def test_device_lookup_of_b_and_C(probe, which):
    """polyrow_eval ON THE DEVICE (v_cvt_i32_f64 for the row, v_fract_f64 for t, v_mul_u32_u24 for the address, seven
    fma) on the product's tables, on the points of test_poly_tables_accuracy -- random, 1e-15..1, every row edge, both
    neighbours, the table ends -- against longdouble at that test's bounds: 4 ulp (4 * 2^-53 relative), 3e-15 in row 0
    of C.  And against Horner's rule on the same table row in numpy with each fused multiply-add emulated in
    longdouble (product and sum carried to 64 bits, rounded once to double): that differs from a true fma only where
    the 64-bit value falls on a double's rounding tie, so 1 ulp is accepted there and such points must be rare
    (below 1 %); everywhere else the device is bit for bit the emulation."""
    b, c = probe.poly_tables()
    tab, xmax = (b, 48.0) if which == "b" else (c, 37.0)
    fun = (lambda v: v / np.expm1(v)) if which == "b" else (lambda v: -np.expm1(-v))
    row0 = 4 * 2.0 ** -53 if which == "b" else 3e-15
    rng = np.random.RandomState(9)
    edges = np.arange(1, int(8 * xmax)) / 8.0
    x = np.concatenate([rng.uniform(0, xmax, 20000), 10.0 ** rng.uniform(-15, 0, 4000), edges, np.nextafter(edges, 0),
                        np.nextafter(edges, 100), [xmax, 1e-300]])
    X = 8.0 * x
    got = probe.poly(which, X)
    ref = fun(x.astype(hp.LD))
    assert got.size == 24002 + 3 * edges.size and np.isfinite(ref.astype(np.float64)).all()
    err = np.abs((got.astype(hp.LD) - ref) / ref).astype(np.float64)
    row = np.floor(X).astype(np.int64)
    rest = row > 0
    print("%s: rows > 0 max rel %.3g at x = %r; row 0 max rel %.3g at x = %r" % (
        which, err[rest].max(), x[rest][err[rest].argmax()], err[~rest].max(), x[~rest][err[~rest].argmax()]))
    parity_record("device %s(x) look-up, rows > 0 (rel)" % which, err[rest].max(), 4 * 2.0 ** -53)
    parity_record("device %s(x) look-up, row 0 (rel)" % which, err[~rest].max(), row0)
    assert err[rest].max() < 4 * 2.0 ** -53 and err[~rest].max() < row0
    t = X - np.floor(X)
    p = tab[row, 7]
    for k in range(6, -1, -1):
        p = (p.astype(hp.LD) * t.astype(hp.LD) + tab[row, k].astype(hp.LD)).astype(np.float64)
    d = np.abs(got - p) / hp.ulp_of(p)
    print("%s: device against emulated Horner: %d of %d points differ, by at most %.0f ulp" % (which, (d > 0).sum(), d.size, d.max()))
    assert d.max() <= 1.0 and (d > 0).mean() < 0.01
    hostgot = hp.probe_module().load_host().poly(which, X)       # (and the host variant -- floor, an index -- is the same function)
    assert np.array_equal(bits(hostgot), bits(got))


# ------------------------------------------------------------ 4. the constructor
def _within(kind, got, true, rtol, rows):
    err = np.abs(got / true - 1.0)
    w = err.argmax() if not np.isnan(err).any() else np.flatnonzero(np.isnan(err))[0]
    print("   %-16s max rel %.3g (bound %g) at row %d: pars %r, device %r, true %r" % (kind, err[w], rtol, w, rows[w].tolist(), got[w], true[w]))
    parity_record(kind + " against the truth (rel)", err[w], rtol)
    assert np.all(err <= rtol), (kind, w, rows[w], got[w], true[w], err[w])


def _check_scalars(name, opthin, noalpha, out, st, it, g, pars):
    """every row: status 0, finite, and each scalar within its bound of the truth"""
    F = {k: out[:, i] for i, k in enumerate(("normfac", "xmerge", "kappa", "hcokt", "hokt9", "lhokt9", "lx0", "peak", "x0", "wavemerge"))}
    bad = np.flatnonzero(st != 0)
    assert bad.size == 0, "status %r at rows %r: pars %r, iters %r" % (st[bad][:5], bad[:5], pars[bad][:5], it[bad][:5])
    used = ["normfac", "hcokt", "hokt9", "lhokt9", "lx0", "peak"] + ([] if noalpha else ["xmerge", "kappa", "wavemerge"]) + ([] if opthin else ["x0"])
    for k in used:
        assert np.all(np.isfinite(F[k])), (k, pars[~np.isfinite(F[k])][:5])
    assert out.shape[0] == N_SED_ROWS
    _within(name + " normfac", F["normfac"], g[name + "/normfac"], 1e-12, pars)
    if not opthin:
        _within(name + " x0", F["x0"], g["thick/x0"], 1e-14, pars)
    _within(name + " peak", F["peak"], g[("thin" if opthin else "thick") + "/peak"], 1e-10, pars)
    if not noalpha:
        xm, kap = g[name + "/xmerge"], g[name + "/kappa"]
        d = np.abs(F["xmerge"] - xm)
        lim = 2e-12 + 4 * EPS * np.abs(xm)
        w = (d / lim).argmax()
        print("   %-16s max |d| %.3g (bound %.3g) at row %d: pars %r, device %r, true %r, iters %d" % (
            name + " xmerge", d[w], lim[w], w, pars[w].tolist(), F["xmerge"][w], xm[w], it[w]))
        parity_record(name + " xmerge against the truth (abs)", d.max(), 2e-12)
        assert np.all(d <= lim), (w, pars[w], F["xmerge"][w], xm[w], it[w])
        _within(name + " kappa", F["kappa"], kap, 2e-12, pars)
        _within(name + " normfac*kappa", F["normfac"] * F["kappa"], g[name + "/normfac"] * kap, 1e-12, pars)


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_constructor_against_the_truth(probe, ctx, g_hps, name, opthin, noalpha):
    """vlog of T and lambda0, sed_prologue, sed_peak_wave on every row of hp_sed.npz -- the suite's two parameter boxes,
    beta = 0 and 1e-8, rows whose y at the merge point sits beside each switch of h_and_dh (1e-4, 700) and of the fp32
    stage (0.02, 80), rows whose xnorm is within 1e-6 of xmerge (the switch of normfac's formula), sixteen rows at
    1 to 6 K -- in the row-of-16-lanes form and the single-lane form, in blocks of 64 and 256 threads.  Status 0 and
    finite on EVERY row; x0 1e-14, normfac 1e-12, normfac kappa 1e-12, kappa 2e-12 (their quotient),
    |d xmerge| <= 2e-12 + 4 eps |xmerge| (the stopping rule of the reference's brentq), peak wavelength 1e-10 against
    the exact root of the reference's own stationarity equation.  The two forms are bitwise equal; the product's
    mbb_sed_prologue_batch returns the single-lane form's bits, so the probe tests what ships.

    iters (the fp64 Newton evaluations of thick_merge_root, thick model with alpha only): if no row of the fixture
    takes a second one the second-iteration kappa path of sed_prologue is dead in practice (DESIGN.md says so) and
    iters == 1 is asserted, so that a change which starts to use the path is noticed; rows with iters >= 2 meet the
    same bounds either way, being rows of the same arrays."""
    pars = g_hps["pars"]
    lane, st, it = probe.prologue(pars, opthin, noalpha, row=False, block=256)
    print("%s, single-lane form:" % name)
    _check_scalars(name, opthin, noalpha, lane, st, it, g_hps, pars)
    for row, block in ((True, 64), (True, 256), (False, 64)):
        o2, st2, it2 = probe.prologue(pars, opthin, noalpha, row=row, block=block)
        same = (bits(o2) == bits(lane)) | (np.isnan(o2) & np.isnan(lane))
        assert same.all(), "%s form, block %d: differs from the single-lane form at %r" % (
            "row" if row else "lane", block, np.argwhere(~same)[:5])
        assert np.array_equal(st2, st) and np.array_equal(it2, it)
    hist = np.bincount(it, minlength=3)
    print("%s: iters histogram %r" % (name, {int(k): int(v) for k, v in enumerate(hist) if v}))
    if it.max() > 1:
        for o in np.unique(g_hps["origin"]):
            h = np.bincount(it[g_hps["origin"] == o])
            print("   rows of origin %d: iters %r" % (o, {int(k): int(v) for k, v in enumerate(h) if v}))
    parity_record(name + " constructor iters (max)", it.max(), 80)
    if opthin or noalpha:
        assert np.all(it == 0)                         # (no root find that counts)
    elif (it >= 2).sum() == 0:
        assert np.all(it == 1)
    # what ships: the product's entry point, the same bits
    out, pst = ctx.sed_prologue(pars, opthin, noalpha, 500.0, want_peak=True)
    assert np.all(pst == 0) and out.shape == (N_SED_ROWS, 6)
    for j, k in enumerate((0, 1, 2, 8, 9, 7)):
        a, b = out[:, j], lane[:, k]
        assert np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))), (name, j, np.flatnonzero(bits(a) != bits(b))[:5])


# ------------------------------------------------------------ 5. one sample
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_per_sample_fnu_against_the_truth(probe, g_hps, name, opthin, noalpha):
    """fnu_sample<.., TAB = true, SCALE = false> -- the hot loop's sample: fnu_bb_tab, fnu_wien_tab, the far branch beyond
    X = 384 -- times cq nu^2 as the fused kernels scale a band, and fnu_sample<.., false, true>, both f_nu in mJy, sample
    by sample against the truth: 64 rows (16 at 1 to 6 K) x 48 frequencies -- a log grid over 20-3000 um, the doubles on
    either side of X = 8 xmerge and X = 384, X on table-row edges and one ulp below, Y at the clamp 8 * 37 and in row 0
    of C.  Relative 1e-12 wherever the truth exceeds 1e-280 of the row's normalisation (at most 2 % of the samples do
    not); below that the device value is at most 1e-270 of it, never NaN, never negative.  Every sample is judged on
    its own, those beside a hand-over included: each side has its own formula and its own true value."""
    pars, rows, freq = g_hps["pars"], g_hps["fnu/rows"], g_hps["fnu/freq"]
    true = g_hps["fnu/" + name]
    p = pars[rows]
    tab, plain, st = probe.fnu(p, freq, opthin, noalpha)
    assert np.all(st == 0) and tab.shape == plain.shape == true.shape == (N_FNU_ROWS, N_FREQ)
    fnorm = p[:, 4][:, None]
    big = true > 1e-280 * fnorm
    assert big.sum() >= 0.98 * true.size
    hokt9 = (1e9 * 6.6260693e-34 / 1.3806505e-23) / p[:, 0][:, None]
    X = 8.0 * hokt9 * freq
    far = (X > 384.0) & (np.ones_like(big) if noalpha else np.zeros_like(big))
    near_merge = np.zeros_like(big)
    if not noalpha:
        xm = g_hps[name + "/xmerge"][rows][:, None]
        near_merge = np.abs(X / (8.0 * xm) - 1.0) < 8 * EPS
        assert near_merge.sum() >= 2 * N_FNU_ROWS - 4
    else:
        assert far.sum() >= 100
    for label, got in (("table form", tab), ("plain form", plain)):
        assert not np.isnan(got).any(), (label, p[np.isnan(got).any(axis=1)][:3], freq[np.isnan(got)][:5])
        assert np.all(got >= 0.0)
        err = np.where(big, np.abs(got / np.where(big, true, 1.0) - 1.0), 0.0)
        w = np.unravel_index(err.argmax(), err.shape)
        print("%s %s: %d samples, max rel %.3g at pars %r, nu = %r GHz (X = %.6f): device %r, true %r; beside the merge point %.3g "
              "(%d samples), far branch %.3g (%d samples); %d under the floor" % (
                  name, label, big.sum(), err[w], p[w[0]].tolist(), freq[w], X[w], got[w], true[w],
                  err[near_merge].max() if near_merge.any() else 0.0, near_merge.sum(),
                  err[far].max() if far.any() else 0.0, far.sum(), (~big).sum()))
        parity_record("per-sample f_nu, %s, against the truth (rel)" % label, err[w], 1e-12)
        assert np.all(err <= 1e-12), (name, label, p[w[0]], freq[w], got[w], true[w], err[w])
        assert np.all(got[~big] <= 1e-270 * np.broadcast_to(fnorm, got.shape)[~big])
    assert big.sum() + (~big).sum() == N_FNU_ROWS * N_FREQ
