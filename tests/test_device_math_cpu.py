"""CPU side of the high-precision tests of the device math (tests/test_device_math_gpu.py is the GPU side): the
fixtures tests/golden/hp_math.npz and hp_sed.npz are what they claim to be, numpy's longdouble is a fit dense
reference, the HOST build of mbb_math.hip.h (the probe compiled with MBB_MATH_HOST) meets the header's bounds on
the same points and through the same ulp arithmetic the GPU tests use, the CPU oracle constructs every row of the
fixture and stays within its own stopping rule of the truth, and the probe instantiates every row form the
product's sources call."""
import os

import numpy as np
import pytest

import _hp_common as hp
from conftest import VARIANTS

N_SED_ROWS = 1584          # 600 wide + 600 box + 40 + 40 (beta 0, 1e-8) + 144 + 144 (edges, switches) + 16 cold
N_FNU_ROWS, N_FREQ = 64, 48
FUNCS = ("m_exp", "m_exp_t", "m_expm1", "m_log", "m_div")


@pytest.fixture(scope="module")
def g_math():
    return np.load(os.path.join(hp.GOLDEN, "hp_math.npz"))


@pytest.fixture(scope="module")
def g_hps():
    return np.load(os.path.join(hp.GOLDEN, "hp_sed.npz"))


@pytest.fixture(scope="module")
def host():
    return hp.probe_module().load_host()


def test_fixture_is_self_consistent(g_math, g_hps):
    for f in FUNCS:
        x, hi, lo, sh, kind = (g_math[f + "/" + k] for k in ("x", "hi", "lo", "sh", "kind"))
        assert x.dtype == np.float64 and x.shape == hi.shape == lo.shape == sh.shape == kind.shape and x.size >= 1200, f
        assert not np.isnan(x).any() and not np.isnan(hi).any() and np.isfinite(lo).all()
        fin = np.isfinite(hi)
        # a normalised double-double: lo is no more than half a spacing of hi (the spacing is the subnormal one at least)
        assert np.all(np.abs(lo[fin]) <= 0.5 * hp.ulp_of(hi[fin]) * (1 + 1e-15)), f
        assert set(np.unique(sh)) <= {0, 256} and np.all((kind != 1) | (lo == 0)), f
        assert set(np.unique(kind)) <= ({0, 2} if f == "m_div" else {0, 1} if f != "m_log" else {0}), f
    # the points the issue names are there
    xe = g_math["m_exp/x"]
    for v in (-745.2, -708.4, 709.78, 0.0, 5e-324, 800.0, -800.0, 1e89, -1e89):
        assert v in xe and v in g_math["m_exp_t/x"]
    assert all(2.0 ** -k in g_math["m_expm1/x"] and -2.0 ** -k in g_math["m_expm1/x"] for k in range(1, 61))
    xl = g_math["m_log/x"]
    assert 2.2250738585072014e-308 in xl and 1.7976931348623157e308 in xl and np.all(xl >= 2.2250738585072014e-308)
    assert np.isinf(g_math["m_div/y"]).sum() >= 5 and (g_math["m_div/y"] == 8.0e307).sum() >= 20
    # the constructor's rows
    pars = g_hps["pars"]
    assert pars.shape == (N_SED_ROWS, 5) and g_hps["origin"].shape == (N_SED_ROWS,)
    assert (pars[:, 1] == 0.0).sum() >= 40 and (pars[:, 1] == 1e-8).sum() == 40
    for name, opthin, noalpha in VARIANTS:
        keys = ["normfac"] + ([] if noalpha else ["xmerge", "kappa"])
        for k in keys:
            v = g_hps[name + "/" + k]
            assert v.shape == (N_SED_ROWS,) and np.all(np.isfinite(v)) and np.all(v > 0), (name, k)
    for k in ("thick/x0", "thin/peak", "thick/peak"):
        assert g_hps[k].shape == (N_SED_ROWS,) and np.all(np.isfinite(g_hps[k])) and np.all(g_hps[k] > 0)
    rows, freq = g_hps["fnu/rows"], g_hps["fnu/freq"]
    assert rows.shape == (N_FNU_ROWS,) and freq.shape == (N_FNU_ROWS, N_FREQ) and np.all(freq > 0) and np.all(np.isfinite(freq))
    assert (pars[rows, 0] <= 6.0).sum() >= 16
    hokt9 = (1e9 * 6.6260693e-34 / 1.3806505e-23) / pars[rows, 0]
    X = 8.0 * hokt9[:, None] * freq
    assert (X > 384.0).sum() >= 100 and (X == np.round(X)).sum() >= 100       # the far branch; row edges hit exactly
    for name, _, _ in VARIANTS:
        f = g_hps["fnu/" + name]
        assert f.shape == freq.shape and np.all(np.isfinite(f)) and np.all(f >= 0)
        under = f < 1e-280 * pars[rows, 4][:, None]
        assert under.sum() <= 0.02 * f.size, (name, under.sum())


def test_fixture_rederived_with_mpmath(g_math, g_hps):
    """A sample of every array, computed again: the committed files are the generator's."""
    pytest.importorskip("mpmath")
    gen = hp.generator_module()
    mp, M = gen.mp, gen.M
    for f, fun in (("m_exp", mp.exp), ("m_exp_t", mp.exp), ("m_expm1", mp.expm1), ("m_log", mp.log)):
        x, hi, lo, sh, kind = (g_math[f + "/" + k] for k in ("x", "hi", "lo", "sh", "kind"))
        idx = [i for i in range(0, x.size, 23) if kind[i] == 0]
        assert len(idx) >= 40
        for i in idx:
            assert gen.dd(fun(M(float(x[i]))), int(sh[i])) == (hi[i], lo[i]), (f, x[i])
    a, b, hi, lo, sh, kind = (g_math["m_div/" + k] for k in ("x", "y", "hi", "lo", "sh", "kind"))
    for i in range(0, a.size, 11):
        if a[i] != 0:
            den = M(8.0e307) if kind[i] == 2 else M(float(b[i]))
            assert gen.dd(M(float(a[i])) / den, int(sh[i])) == (hi[i], lo[i]), (a[i], b[i])
    pars = g_hps["pars"]
    assert np.array_equal(gen.param_rows()[0], pars)
    rows, freq = g_hps["fnu/rows"], g_hps["fnu/freq"]
    for name, opthin, noalpha in VARIANTS:
        for i in range(5, pars.shape[0], 97):
            t = gen.Truth(pars[i], opthin, noalpha)
            assert float(t.normfac) == g_hps[name + "/normfac"][i]
            if not noalpha:
                assert float(t.xmerge) == g_hps[name + "/xmerge"][i] and float(t.kappa) == g_hps[name + "/kappa"][i]
            assert float(t.peak) == g_hps[("thin" if opthin else "thick") + "/peak"][i]
            if not opthin:
                assert float(t.x0) == g_hps["thick/x0"][i]
        for j in range(0, N_FNU_ROWS, 9):
            t = gen.Truth(pars[rows[j]], opthin, noalpha)
            for k in range(0, N_FREQ, 5):
                assert float(t.fnu(freq[j, k])) == g_hps["fnu/" + name][j, k]


@pytest.mark.skipif(not hp.LD_OK, reason=hp.LD_REASON)
def test_longdouble_is_a_fit_reference(g_math):
    """The dense sweeps take numpy's longdouble (64-bit mantissa: its own ulp is 2^-11 of a double's) for the truth.
    Here it is held to the mpmath fixture on every curated point in range: within 2^-9 = 2e-3 of a double ulp, i.e.
    four of its own -- libm's long double exp, expm1 and log are good to one or two, division is correctly rounded.
    Observed here: 5e-4, i.e. one."""
    for f, fun in (("m_exp", np.exp), ("m_expm1", np.expm1), ("m_log", np.log), ("m_div", None)):
        x, hi, lo, sh, kind = (g_math[f + "/" + k] for k in ("x", "hi", "lo", "sh", "kind"))
        ok = (kind == 0) & np.isfinite(hi) & (sh == 0)
        assert ok.sum() >= 1000, f
        xl = x[ok].astype(hp.LD)
        ref = xl / g_math["m_div/y"][ok].astype(hp.LD) if fun is None else fun(xl)
        err = np.abs(((ref - hi[ok].astype(hp.LD)) - lo[ok].astype(hp.LD)) / hp.ulp_of(hi[ok]).astype(hp.LD)).astype(np.float64)
        print("%s: longdouble against mpmath on %d points: %.2e of a double ulp" % (f, ok.sum(), err.max()))
        assert err.max() <= 2.0 ** -9, (f, err.max(), x[ok][err.argmax()])


@pytest.mark.parametrize("f", FUNCS)
def test_host_build_meets_the_header_on_the_fixture(host, g_math, f):
    """The host variant of mbb_math.hip.h (another reciprocal seed, `if`s for the saturating conversion, floor for
    the fraction) at the header's bounds on every curated point: 2 ulp, m_div 1.5; exact 0 / inf / -1 beyond."""
    _, n = hp.check_curated(host, g_math, f)
    assert n == g_math[f + "/x"].size


@pytest.mark.skipif(not hp.LD_OK, reason=hp.LD_REASON)
@pytest.mark.parametrize("f", FUNCS)
def test_host_build_dense_sweep(host, f):
    """What tools/test_math_host.cpp printed, asserted: 1e6 seeded points per function against longdouble."""
    n = 1000000
    x, y, ref = hp.sweep_args(f, n, seed=11)
    got = host.math(f, x, y)
    err = np.abs(hp.ulp_err_ld(got, ref))
    assert np.isfinite(err).all() and err.size == n
    print("%s host build: %d points, max %.3f ulp at %r" % (f, n, err.max(), x[err.argmax()]))
    assert err.max() <= hp.ULP_BOUND[f], (f, err.max(), x[err.argmax()])


def test_host_build_edges(host):
    """The retired tool's last line: infinities and NaN through exp, expm1(0), 1 / inf."""
    inf = np.inf
    assert np.array_equal(host.math("m_exp", [inf, -inf, 800.0, -800.0]), [inf, 0.0, inf, 0.0])
    assert np.array_equal(host.math("m_expm1", [710.0, -800.0, 0.0, 710.3]), [inf, -1.0, 0.0, inf])
    assert host.math("m_div", [1.0], [inf])[0] <= 1.25e-308


def test_host_poly_lookup_is_horner_on_the_table(host):
    """polyrow_eval's host variant on the product's tables equals Horner's rule with a fused multiply-add per step,
    emulated in longdouble and rounded once (an 11-bit longer product and sum: the double rounding differs from a
    true fma in rare ties only, hence 1 ulp is accepted and the count of differing points is bounded)."""
    b, c = host.poly_tables()
    rng = np.random.RandomState(9)
    for which, tab, top in (("b", b, 384.0), ("c", c, 296.0)):
        X = np.concatenate([rng.uniform(0, top, 20000), np.arange(0, top + 1), np.nextafter(np.arange(1, top + 1), 0), [top]])
        got = host.poly(which, X)
        i = np.floor(X).astype(np.int64); t = X - np.floor(X)
        p = tab[i, 7]
        for k in range(6, -1, -1):
            p = (p.astype(hp.LD) * t.astype(hp.LD) + tab[i, k].astype(hp.LD)).astype(np.float64) if hp.LD_OK else p * t + tab[i, k]
        d = np.abs(got - p) / hp.ulp_of(p)
        assert d.max() <= (1.0 if hp.LD_OK else 4.0) and (d > 0).mean() < (0.01 if hp.LD_OK else 1.0), (which, d.max(), (d > 0).mean())
    with pytest.raises(RuntimeError):
        host.poly("b", [384.5])
    with pytest.raises(RuntimeError):
        host.poly("c", [-1.0])


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_oracle_against_the_truth(oracle, g_hps, name, opthin, noalpha):
    """The CPU oracle (what every other GPU test is judged against) constructs EVERY row of the fixture and stays
    within the stopping rule of the reference's brentq (2e-12 + 4 eps |x|) in xmerge and within 1e-13 in kappa and
    normfac -- powers with exponents up to 45 of arguments up to 50 in double: (3 + alpha + beta) |log x| eps is 2e-14.
    The maxima recorded in the fixture when it was made obey the same bounds."""
    pars = g_hps["pars"]
    eps = 2.0 ** -52
    worst = np.zeros(3)
    n = 0
    for i, p in enumerate(pars):
        s = oracle.OracleSED(*p, opthin=opthin, noalpha=noalpha).s
        assert np.isfinite(s.normfac)
        worst[2] = max(worst[2], abs(s.normfac / g_hps[name + "/normfac"][i] - 1.0))
        if not noalpha:
            xm = g_hps[name + "/xmerge"][i]
            assert abs(s.xmerge - xm) <= 2e-12 + 4 * eps * xm, (p, s.xmerge, xm)
            worst[0] = max(worst[0], abs(s.xmerge - xm))
            worst[1] = max(worst[1], abs(s.kappa / g_hps[name + "/kappa"][i] - 1.0))
        n += 1
    assert n == N_SED_ROWS
    print(name, "oracle against the truth: |d xmerge| %.3g, kappa %.3g, normfac %.3g (recorded: %s)" %
          (worst[0], worst[1], worst[2], g_hps["oracle_max/" + name]))
    assert worst[1] <= 1e-13 and worst[2] <= 1e-13
    rec = g_hps["oracle_max/" + name]
    assert rec[0] <= 2e-12 and rec[1] <= 1e-13 and rec[2] <= 1e-13


def test_probe_has_every_row_instantiation_of_the_sources():
    """probe_rows runs vexp<true, M1, K> / vlog<true, K> beside the lane form for a fixed list; a call site with another
    (M1, K) added to the product's sources must be added to tests/_device_probe.hip too."""
    src = hp.source_row_instantiations()
    probe = hp.probe_row_instantiations_in_source()
    assert len(probe) == len(set(probe)) == 11
    assert {(False, 0x08, 6), (False, 0x1E, 5), (False, 0x00, 2), (False, 0x02, 2), (False, 0x01, 2), (False, 0x09, 5),
            (False, 0x01, 1), (False, 0x06, 3), (True, 0, 1), (True, 0, 2), (True, 0, 4)} <= src
    assert src == set(probe), "in the sources only: %s; in the probe only: %s" % (src - set(probe), set(probe) - src)
