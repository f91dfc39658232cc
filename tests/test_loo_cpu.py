"""CPU side of the out-of-sample-fit tests: the step logic of csrc/mbb_psis.hip.h in its HOST build (tests/_loo_host.cpp)
function by function against the longdouble restatement (tests/_loo_ref.py) and mpmath; the reference itself on a
linear-Gaussian toy whose leave-one-out predictive density is closed form; ``ChainLoo``'s arithmetic on hand-made
tables; the refusals and the ``loo=`` rules of the sampler and the fitter on a faked device.

Bounds.  ps_gpd_fit's k-hat against the longdouble reference on the same draws: the fit is a sum of M log1p terms per
grid point and a softmax over at most 94 of them; the float64 restatement of the same formulas differs from the
longdouble one by the amount measured here on the same draws (``spread``), and the host build is allowed 64 x that
(other summation order inside libm's log1p and exp is all that separates them), never more than 1e-9.
ps_norm_cdf: erfc is correctly rounded to about 1 ulp in glibc; the product by 1/2 is exact and the argument's product
by sqrt(1/2) has a relative error of 1 eps, which erfc amplifies by z^2 in the tail: (4 + 2 z^2) eps relative, plus the
spacing of the subnormal doubles, 2^-1074, which is what is left of Phi at z = -38."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _loo_ref as LR

LD = LR.LD
EPS = np.finfo(np.float64).eps
_dp = C.POINTER(C.c_double)


def _d(a):
    return a.ctypes.data_as(_dp)


class Host(object):
    def __init__(self, tmpdir):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        if not cxx:
            raise RuntimeError("no host C++ compiler")
        so = os.path.join(str(tmpdir), "libloo_host.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               os.path.join(ROOT, "tests", "_loo_host.cpp"), "-o", so])
        L = self.lib = C.CDLL(so)
        dbl = C.c_double
        L.ps_constants.argtypes = [_dp]
        L.ps_host_tail_len.argtypes = [C.c_longlong]; L.ps_host_tail_len.restype = C.c_longlong
        L.ps_host_grid_len.argtypes = [C.c_int]
        L.ps_host_gpd_fit.argtypes = [_dp, C.c_int, _dp, _dp, _dp]
        L.ps_host_gpd_quantile.argtypes = [dbl] * 3; L.ps_host_gpd_quantile.restype = dbl
        L.ps_host_smoothed.argtypes = [C.c_int, C.c_int, dbl, dbl, dbl]; L.ps_host_smoothed.restype = dbl
        L.ps_host_norm_cdf.argtypes = [dbl]; L.ps_host_norm_cdf.restype = dbl
        L.ps_host_ll.argtypes = [dbl, dbl]; L.ps_host_ll.restype = dbl
        L.ps_host_lse.argtypes = [_dp, C.c_int, C.c_int]; L.ps_host_lse.restype = dbl
        c = np.empty(3)
        L.ps_constants(_d(c))
        self.tail_max, self.grid_max, self.ln2pi = int(c[0]), int(c[1]), c[2]

    def fit(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out, th, l = np.empty(3), np.empty(self.grid_max), np.empty(self.grid_max)
        why = self.lib.ps_host_gpd_fit(_d(x), x.size, _d(out), _d(th), _d(l))
        return why, out[0], out[1], out[2], th, l


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    try:
        return Host(tmp_path_factory.mktemp("loo_host"))
    except RuntimeError as e:
        pytest.skip(str(e))


def gpd_draws(k, M, seed, sigma=1.0):
    """M draws of a generalised Pareto distribution of shape k by inverse CDF, ascending"""
    u = np.random.RandomState(seed).uniform(size=M)
    x = -sigma * np.log1p(-u) if k == 0 else sigma * np.expm1(-k * np.log1p(-u)) / k
    return np.sort(x)


# ---------------------------------------------------------------- 1. the Pareto fit
@pytest.mark.parametrize("k", [-0.3, 0.0, 0.3, 0.7, 1.5])
def test_gpd_fit_on_draws_of_known_shape(H, k):
    """k-hat of the host build against the longdouble reference on the same draws, within 64 x the float64
    restatement's distance from it; the reference alone recovers k within 0.15 at M = 750 (the prior pulls (k M + 5) /
    (M + 10) towards 0.5 by less than 0.02 there)."""
    worst = spread = 0.0
    for M, seed in ((750, 1), (750, 2), (64, 3), (65, 4), (257, 5), (5, 6), (4096, 7)):
        x = gpd_draws(k, M, seed)
        why_r, k_r, s_r, kh_r = LR.gpd_fit(x, LD)
        why_f, k_f, s_f, kh_f = LR.gpd_fit(x, np.float64)
        why, kk, sg, kh, th, l = H.fit(x)
        assert why == why_r == why_f == LR.FIT_OK
        if M == 750:
            assert abs(float(kh_r) - k) < 0.15, (k, float(kh_r))
        spread = max(spread, abs(float(LD(kh_f) - kh_r)), abs(float((LD(s_f) - s_r) / s_r)))
        worst = max(worst, abs(float(LD(kh) - kh_r)), abs(float((LD(sg) - s_r) / s_r)))
        assert kh == (kk * M + 5.0) / (M + 10.0) and H.lib.ps_host_grid_len(M) == 30 + int(np.sqrt(M))
    print("    k = %g: host build %.3g from longdouble; the float64 restatement %.3g" % (k, worst, spread))
    assert worst <= max(64 * spread, 64 * EPS) < 1e-9


def test_gpd_fallbacks(H):
    """Every fallback, one case each, host build and reference alike: M = 4 (short) and M = 5 (fitted), a constant
    tail, x* = 0 from planted ties, a non-finite k."""
    x5 = gpd_draws(0.3, 5, 11)
    for x, want in ((x5[:4], LR.FIT_SHORT), (x5, LR.FIT_OK), (np.full(40, 0.25), LR.FIT_FLAT),
                    (np.concatenate([np.zeros(6), gpd_draws(0.3, 15, 12)]), LR.FIT_FLAT),      # x* = x[5] = 0
                    (np.concatenate([gpd_draws(0.3, 30, 13), [np.inf]]), LR.FIT_FLAT)):        # 1 / x_M = 0, k = NaN
        why, kk, sg, kh, _, _ = H.fit(x)
        ref = LR.gpd_fit(x, LD)
        assert why == want == ref[0], (x.size, why, want, ref[0])
        if want == LR.FIT_OK:
            assert np.isfinite(kh) and abs(float(LD(kh) - ref[3])) < 1e-12
        else:
            assert np.isinf(kh) and kh > 0 and np.isnan(kk) and np.isnan(sg) and np.isinf(ref[3])
    # the S = 21 window with repeats that gives x* = 0 through the whole path
    ll = np.array([-1.0] * 4 + [-5.0] * 3 + [-0.5] * 14)
    lw, khat, M, why, tail = LR.psis(ll, LD)
    assert M == 5 and why == LR.FIT_FLAT and np.isinf(khat)


def test_profile_spanning_more_than_1500_does_not_overflow(H):
    """l_j spanning more than 1500: exp(l) overflows, the softmax with the maximum subtracted does not."""
    x = gpd_draws(0.3, 4096, 21) * 1e-3
    why, kk, sg, kh, th, l = H.fit(x)
    m = H.lib.ps_host_grid_len(4096)
    assert why == LR.FIT_OK and np.all(np.isfinite(l[:m]))
    assert l[:m].max() - l[:m].min() > 1500.0 and l[:m].max() > 710.0, (l[:m].min(), l[:m].max())
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(l[:m])).any()
    ref = LR.gpd_fit(x, LD)
    assert abs(float(LD(kh) - ref[3])) < 1e-10 and np.isfinite(sg)


def test_quantile_and_smoothed_tail(H):
    for khat, sigma in ((0.3, 2.0), (-0.4, 0.5), (1.2, 1e-3), (0.0, 1.5)):
        for p in (0.5 / 750, 0.25, 0.5, 1 - 0.5 / 750):
            got = H.lib.ps_host_gpd_quantile(p, khat, sigma)
            want = -LD(sigma) * np.log1p(-LD(p)) if khat == 0 else LR.gpd_quantile(LD(p), LD(khat), LD(sigma))
            assert abs(float((LD(got) - want) / want)) < 8 * EPS
    # capped at 0
    assert H.lib.ps_host_smoothed(749, 750, 1.5, 1.0, 0.5) == 0.0
    v = H.lib.ps_host_smoothed(3, 750, 0.3, 0.01, 0.5)
    want = np.log(LR.gpd_quantile((LD(4) - LD(0.5)) / 750, LD(0.3), LD(0.01)) + LD(0.5))
    assert v < 0 and abs(float(LD(v) - want)) < 8 * EPS


# ---------------------------------------------------------------- 2. Phi, the tail length, log-sum-exp, ll
def test_norm_cdf_against_mpmath(H):
    pytest.importorskip("mpmath")
    z = np.concatenate([np.linspace(-38.0, 8.5, 187), [-37.5, -30.0, -1e-300, 0.0, 1e-17, 38.0]])
    ref = LR.norm_cdf_mp(z)
    got = np.array([H.lib.ps_host_norm_cdf(v) for v in z])
    assert np.all(ref > 0) and got[-1] == 1.0 and got[z == 0.0][0] == 0.5
    err = np.abs(got.astype(LD) - ref)
    bound = (4 + 2 * z * z) * EPS * ref + LD(2.0) ** -1074            # (Phi(-38) = 2.9e-316 is a subnormal double)
    ratio = (err / bound).astype(np.float64)
    print("    Phi: worst %.3g of its bound, at z = %g" % (ratio.max(), z[np.argmax(ratio)]))
    assert np.all(ratio <= 1.0)


def test_tail_len(H):
    t = H.lib.ps_host_tail_len
    for S, M in ((0, 0), (1, 1), (5, 1), (6, 2), (20, 4), (21, 5), (225, 45), (226, 46), (455, 64), (456, 65), (7281, 256),
                 (7282, 257), (7283, 257), (1864135, 4096), (1864136, 4097)):
        assert t(S) == M == LR.tail_len(S), (S, t(S), LR.tail_len(S))
    rng = np.random.RandomState(5)
    for S in np.concatenate([np.arange(1, 3000), rng.randint(3000, 8000000, 2000), (2 * np.arange(1, 600)) ** 2]):
        assert t(int(S)) == LR.tail_len(int(S)), S
    from mbb_emcee_amd import _native
    assert H.tail_max == _native.PW_TAIL_MAX == 4096 and t(_native.PW_MAX_WINDOW) == H.tail_max < t(_native.PW_MAX_WINDOW + 1)
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    assert "#define MBB_PW_TAIL_MAX %d" % H.tail_max in hdr and "#define MBB_PW_MAX_WINDOW %d" % _native.PW_MAX_WINDOW in hdr


def test_lse_merge_in_any_grouping(H):
    rng = np.random.RandomState(9)
    for v in (rng.normal(-3, 2, 1000), rng.normal(-1e5, 300, 777), np.array([-745.0, 2.0, 709.0]), np.full(17, -1e308)):
        v = np.ascontiguousarray(v)
        want = LR._lse(v.astype(LD))
        for run in (1, 7, 256, v.size):
            got = H.lib.ps_host_lse(_d(v), v.size, run)
            assert abs(float(LD(got) - want)) <= 8 * EPS * max(1.0, abs(float(want))), (run, got, want)
    assert H.lib.ps_host_lse(_d(np.zeros(1)), 0, 1) == -np.inf


def test_ll_is_the_definition(H):
    rng = np.random.RandomState(3)
    for g, lam in zip(rng.normal(0, 3, 200) * 10.0 ** rng.randint(-3, 4, 200), 10.0 ** rng.uniform(-6, 6, 200)):
        want = (np.log(LD(lam)) - np.log(2 * np.arccos(LD(-1)))) / 2 - LD(g) ** 2 / LD(lam) / 2
        got = H.lib.ps_host_ll(g, lam)
        assert abs(float(LD(got) - want)) <= 4 * EPS * (abs(float(np.log(LD(lam)))) + 2 + float(LD(g) ** 2 / lam)), (g, lam)
    assert np.isnan(H.lib.ps_host_ll(np.nan, 1.0)) and H.lib.ps_host_ll(np.inf, 1.0) == -np.inf
    assert abs(H.ln2pi - np.log(2 * np.pi)) < 1e-15


def test_ll_constant_where_lambda_is_next_to_2_pi(H):
    """The constant of ll, log(Lambda / 2 pi) / 2, keeps its RELATIVE accuracy where it is small: _loo_ref.ll_bound
    allows 2 eps of it, and formed as (log Lambda - log 2 pi) / 2 it kept log's absolute error instead -- 1e-15 of the
    -0.0026 at Lambda = 6.25 on the host, 1.4e-14 on the device, where tests/test_domain_paths_gpu.py found it (an
    uncertainty of 0.4 mJy).  Against mpmath at 40 digits."""
    import mpmath
    with mpmath.workdps(40):
        for lam in (6.25, 6.0, 6.28, 6.2831853, 6.283185307179586, 6.3, 7.0, 1.0 / 0.41 ** 2, 3.2, 12.5):
            want = mpmath.log(mpmath.mpf(lam) / (2 * mpmath.pi)) / 2
            got = H.lib.ps_host_ll(0.0, lam)
            assert abs(mpmath.mpf(got) - want) <= 2 * EPS * abs(want), (lam, got, float(want))


# ---------------------------------------------------------------- 3. the reference on a toy of known answer
def test_reference_on_a_linear_gaussian_toy():
    """y = a theta + e, e ~ N(0, C) with three correlated bands, a Gaussian prior on theta (so that no single band carries
    the posterior and k-hat stays below 0.7): the posterior is Gaussian and
    the exact leave-one-band-out predictive density p(y_b | y_-b) is Gaussian in closed form.  The reference's
    elpd_loo from 20 000 exact posterior draws is within its own Monte Carlo error of it, band by band."""
    rng = np.random.RandomState(17)
    a = np.array([1.0, 0.7, 1.6])
    sd = np.array([0.5, 0.8, 0.4])
    R = np.array([[1.0, 0.5, 0.2], [0.5, 1.0, 0.3], [0.2, 0.3, 1.0]])
    Cov = R * sd[:, None] * sd[None, :]
    Lam = np.linalg.inv(Cov)
    y = a * 2.0 + np.linalg.cholesky(Cov) @ rng.standard_normal(3)
    m0, p0 = 2.0, 1.0 / 0.1 ** 2                               # the prior's mean and precision
    prec = a @ Lam @ a + p0
    mean = (a @ Lam @ y + m0 * p0) / prec
    theta = mean + rng.standard_normal(20000) / np.sqrt(prec)
    model = theta[:, None] * a[None, :]
    ll, g, d = LR.ll_rows(y, model, invcov=Lam)
    # ll is ln p(y_b | y_-b, theta): against the conditional Gaussian formed from C directly
    for b in range(3):
        o = [i for i in range(3) if i != b]
        w = Cov[b, o] @ np.linalg.inv(Cov[np.ix_(o, o)])
        cm = model[:, b] + (y[o] - model[:, o]) @ w
        cv = Cov[b, b] - w @ Cov[o, b]
        want = -0.5 * np.log(2 * np.pi * cv) - 0.5 * (y[b] - cm) ** 2 / cv
        assert np.allclose(ll[:, b].astype(np.float64), want, rtol=0, atol=1e-10)
    z = (g / np.sqrt(d)[None, :]).astype(np.float64)
    for b in range(3):
        o = [i for i in range(3) if i != b]
        # the posterior of theta without band b, then the predictive density of y_b given y_-b
        Lo = np.linalg.inv(Cov[np.ix_(o, o)])
        po = a[o] @ Lo @ a[o] + p0
        mo = (a[o] @ Lo @ y[o] + m0 * p0) / po
        w = Cov[b, o] @ Lo
        slope = a[b] - w @ a[o]                                 # E[y_b | y_-b, theta] = w y_-b + slope theta
        cv = Cov[b, b] - w @ Cov[o, b]
        pm, pv = w @ y[o] + slope * mo, cv + slope ** 2 / po
        exact = -0.5 * np.log(2 * np.pi * pv) - 0.5 * (y[b] - pm) ** 2 / pv
        col = LR.column(ll[:, b], z[:, b], dtype=LD, phi=np.zeros(20000, dtype=LD))
        assert col["status"] & ~LR.WAIC_VAR_HIGH == 0 and float(col["khat"]) < 0.7, col["khat"]
        # Monte Carlo error of the self-normalised estimate: the delta method on the ratio of the two weighted means
        lw = LR.psis(ll[:, b], LD)[0]
        wgt = np.exp((lw - LR._lse(lw)).astype(np.float64))
        lik = np.exp((ll[:, b] - col["elpd_loo"]).astype(np.float64))
        se = np.sqrt(np.sum((wgt * (lik - 1.0)) ** 2))
        print("    band %d: elpd_loo %.5f exact %.5f, %.2f of its Monte Carlo error %.2g; k-hat %.2f"
              % (b, float(col["elpd_loo"]), exact, abs(float(col["elpd_loo"]) - exact) / se, se, float(col["khat"])))
        assert abs(float(col["elpd_loo"]) - exact) < 4 * se and se < 0.02
        assert abs(float(col["elpd_waic"]) - exact) < 0.05


def test_reference_precisions_agree():
    """The float64 and the longdouble restatement on synthetic columns with repeats, S from 21 to 62 500."""
    rng = np.random.RandomState(23)
    worst = 0.0
    for S in (21, 64, 455, 456, 3000, 7283, 62500):
        ll = -0.5 * rng.chisquare(3, S) * rng.choice([0.3, 1.0, 3.0])
        rep = rng.uniform(size=S) < 0.3
        ll[1:][rep[1:]] = ll[:-1][rep[1:]]
        phi = rng.uniform(size=S).astype(LD)
        a = LR.column(ll, None, dtype=np.float64, phi=phi.astype(np.float64))
        b = LR.column(ll, None, dtype=LD, phi=phi)
        assert a["status"] == b["status"] and a["tail_len"] == b["tail_len"] and np.array_equal(a["tail"], b["tail"])
        worst = max(worst, LR.distance(a, b))
    print("    float64 vs longdouble: %.3g" % worst)
    assert worst < 1e-10


# ---------------------------------------------------------------- 4. ChainLoo on hand-made tables
class _Like(object):
    data_read = True

    def __init__(self, nsources=1, ndata=4):
        self.nsources = nsources
        self._ndata = ndata
        self._flux = np.arange(1.0, ndata + 1)
        self.data_flux_unc = 0.1 * self._flux
        self._flux_multi = np.tile(self._flux, (nsources, 1))
        self._ivar_multi = np.tile(1.0 / self.data_flux_unc ** 2, (nsources, 1))


@pytest.fixture
def no_device(monkeypatch):
    from mbb_emcee_amd import _native

    def touched(like):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "analysis_context", touched)


def _made(nsrc=2, ndata=4, multi=True, shift=0.0, like=None):
    from mbb_emcee_amd import loo
    req = loo._Request(like or _Like(nsrc if multi else 1, ndata))
    raw = loo._Raw(nsrc, ndata)
    base = np.arange(nsrc * ndata, dtype=np.float64).reshape(nsrc, ndata)
    raw.elpd_loo[:] = -1.0 - 0.5 * base + shift * (1 + base % 3)
    raw.elpd_waic[:] = raw.elpd_loo + 0.01
    raw.lppd[:] = raw.elpd_loo + 0.3
    raw.p_loo[:] = 0.3
    raw.p_waic[:] = 0.29
    raw.khat[:] = 0.1 * base
    raw.loo_pit[:] = np.linspace(0.001, 0.999, nsrc * ndata).reshape(nsrc, ndata)
    raw.n_used[:] = 100
    raw.tail_len[:] = 20
    return loo.ChainLoo(req, raw, multi, 10, 10)


def test_chainloo_sums_se_compare_outliers():
    from mbb_emcee_amd import loo
    r = _made()
    t = r._raw.elpd_loo
    assert np.array_equal(r.elpd_loo, t.sum(axis=1)) and r.elpd_loo.shape == (2,)
    assert np.allclose(r.se_elpd_loo, np.sqrt(4 * t.var(axis=1, ddof=1)), rtol=1e-15)
    assert np.array_equal(r.p_loo, np.full(2, 0.3 * 4)) and np.allclose(r.se_p_loo, 0.0)
    assert np.array_equal(r.p_waic, r._raw.p_waic.sum(axis=1)) and np.array_equal(r.elpd_waic, r._raw.elpd_waic.sum(axis=1))
    assert np.array_equal(r.khat_max, r._raw.khat.max(axis=1)) and r.elpd_loo_band.shape == (2, 4)
    out = r.outliers(0.01)
    assert out.shape == (2, 4) and out[0, 0] and out[1, 3] and out.sum() == 2
    assert r.outliers(0.5).sum() == 4
    r._raw.loo_pit[0, 1] = np.nan
    assert not r.outliers(0.5)[0, 1]
    with pytest.raises(ValueError, match="alpha"):
        r.outliers(0.0)
    one = _made(nsrc=1, ndata=1, multi=False)
    assert np.isnan(one.se_elpd_loo) and one.elpd_loo.shape == () and one.khat.shape == (1,)
    other = _made(shift=0.25)
    diff, se = other.compare(r)
    d = other._raw.elpd_loo - r._raw.elpd_loo
    assert np.array_equal(diff, d.sum(axis=1)) and np.allclose(se, np.sqrt(4 * d.var(axis=1, ddof=1)), rtol=1e-15)
    assert np.all(diff > 0) and np.array_equal(r.compare(other)[0], -diff)
    lk = _Like(2, 4)
    lk._flux_multi = lk._flux_multi * 1.01
    with pytest.raises(ValueError, match="same bands, fluxes and uncertainties"):
        r.compare(_made(like=lk))
    with pytest.raises(ValueError, match="same bands"):
        r.compare(_made(ndata=3))
    with pytest.raises(TypeError):
        r.compare(None)
    arrs = r.arrays()
    assert {"loo_elpd_loo", "loo_elpd_loo_band", "loo_khat", "loo_loo_pit", "loo_p_waic_band", "loo_se_elpd_loo", "loo_status",
            "loo_tail_len", "loo_n_used", "loo_khat_max", "loo_ndata"} <= set(arrs)
    assert set(_made().arrays(prefix="x_")) == {"x_" + k[4:] for k in arrs}
    text = str(r)
    assert "Source 0 of 2" in text and "elpd_loo" in text and "Pareto k-hat per band" in text and "Outlying bands" in text
    assert (loo.ChainLoo.K_HIGH, loo.ChainLoo.TAIL_SHORT, loo.ChainLoo.TAIL_FLAT, loo.ChainLoo.WAIC_VAR_HIGH) == (16, 32, 64, 128)


def test_refusals_before_the_device(no_device):
    from mbb_emcee_amd import chain_loo, loo_rows, _native
    like, chain = _Like(), np.zeros((4, 8, 5))
    for kw, msg in ((dict(burn=8), "burn leaves no step"), (dict(burn=-1), "burn must be"), (dict(thin=0), "burn must be")):
        with pytest.raises(ValueError, match=msg):
            chain_loo(like, chain, **kw)
    with pytest.raises(ValueError, match="2 sources, the likelihood 3"):
        chain_loo(_Like(3), np.zeros((2, 4, 8, 5)))
    with pytest.raises(ValueError, match="empty"):
        chain_loo(like, np.zeros((0, 8, 5)))
    nodata = _Like()
    nodata.data_read = False
    with pytest.raises(Exception, match="Data not read"):
        chain_loo(nodata, chain)
    with pytest.raises(Exception, match="Data not read"):
        loo_rows(nodata, np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r"pars must be \[n, 5\]"):
        loo_rows(like, np.zeros((2, 4)))
    wide = _Like(ndata=257)
    with pytest.raises(ValueError, match="at most 256 bands"):
        chain_loo(wide, chain)
    with pytest.raises(ValueError, match="longer tail"):
        chain_loo(like, np.zeros((2, (_native.PW_MAX_WINDOW + 2) // 2, 5)))
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_loo(like, chain, burn=7, thin=2)
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_loo(_Like(1), np.zeros((6, 4, 8, 5)))
    with pytest.raises(AssertionError, match="the device was touched"):
        loo_rows(like, np.zeros((2, 5)))


# ---------------------------------------------------------------- 5. the sampler's and the fitter's keyword
def _bare_sampler():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary = 10, 5, _Like(), None, None

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_loo_keyword_rules():
    s = _bare_sampler()
    p0 = np.zeros((10, 5))
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(p0, 16, storechain=False, loo=True)
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(p0, 16, loo=dict(burn=16))
    with pytest.raises(ValueError, match="burn leaves no step"):          # burn taken from the summary's keywords
        s.run_mcmc(p0, 16, summary=dict(burn=16), loo=True)
    with pytest.raises(TypeError, match="unexpected keyword"):
        s.run_mcmc(p0, 16, loo=dict(percentile=68.3))
    with pytest.raises(ValueError, match="longer tail"):
        s.run_mcmc(p0, 200000, loo=True)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, storechain=False, summary=dict(burn=15), loo=True)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, loo=False)
    assert s.loo_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.loo()
    s._resident = 16
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.loo(burn=16)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.loo(burn=15)


def test_loo_attribute_is_reset():
    s = _bare_sampler()
    s._open = None
    s.loo_ = object()
    s.reset()
    assert s.loo_ is None
    s.loo_ = object()
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(np.zeros((10, 5)), 4)
    assert s.loo_ is None


def test_sharded_run_is_not_cross_validated():
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k = 10
    s.lnprobfn = _Like()
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded"):
        s.run_mcmc(np.zeros((10, 5)), 4, loo=True)


def test_fitter_cli_and_bindings_know_loo():
    import re
    import mbb_emcee_amd
    from mbb_emcee_amd import mbb_fitter, run_mbb_emcee, _native
    assert mbb_emcee_amd.chain_loo is mbb_emcee_amd.loo.chain_loo
    assert {"ChainLoo", "chain_loo", "loo_rows"} <= set(mbb_emcee_amd.__all__)
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="loo= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), loo=True)
    assert fit.loo is None
    assert run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz"]).loo is False
    assert run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz", "--loo"]).loo is True
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_pointwise", "mbb_sampler_pointwise", "mbb_pointwise_rows"):
        assert name in hdr and name in _native.SIGNATURES
    assert C.sizeof(_native.PointwiseSpec) == 8 and C.sizeof(_native.PointwiseOut) == 10 * 8
    for struct, cls in (("mbb_pointwise_spec", _native.PointwiseSpec), ("mbb_pointwise_out", _native.PointwiseOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip(" *") for decl in body.split(";") if decl.strip()
                 for n in decl.strip().split(None, 1)[1].replace("*", " ").split(",")]
        assert [n for n in names if n] == [f[0] for f in cls._fields_], (struct, names)
    for bit in ("K_HIGH = 16", "TAIL_SHORT = 32", "TAIL_FLAT = 64", "WAIC_VAR_HIGH = 128"):
        assert "MBB_PW_" + bit in hdr
    build = open(os.path.join(ROOT, "mbb_emcee_amd", "build.py")).read()
    assert "mbb_pointwise.hip.h" in build and "mbb_psis.hip.h" in build
    flow = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_flow.hip")).read()
    assert "mbb_pointwise" not in flow and "mbb_psis" not in flow
    lib = os.path.join(ROOT, "mbb_emcee_amd", "libmbb_hip.so")
    if os.path.exists(lib) and shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE).stdout.decode()
        for name in ("mbb_chain_pointwise", "mbb_sampler_pointwise", "mbb_pointwise_rows"):
            assert re.search(r" T %s$" % name, syms, flags=re.M), name
