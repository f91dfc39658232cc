"""CPU side of the evidence tests: the step logic of csrc/mbb_bridge.hip.h in its HOST build (tests/_evidence_host.cpp)
against mpmath, scipy and a longdouble restatement (tests/_evidence_ref.py); the method itself on targets of known
integral, with the reference alone; ``ln_prior_norm`` against quadrature; the interface rules on a faked device.

Bounds.  br_ppnd: AS 241 states 1e-16 relative for PPND16 in exact arithmetic.  On top come the roundings of its
evaluation: two Horner chains of 7 fma (4 eps each allowed, eps = 2^-53), a product and a quotient (1 eps each) -- and in
the tails the argument r = sqrt(-m_log(t)): m_log is held to 2 ulp = 4 eps (tests/test_device_math_cpu.py), the root
halves that and adds its own eps, and z depends on r with a condition number below 1.5 (z ~ sqrt(2) r), so 1.5 x 3 eps.
Together 1e-16 + 14.5 eps = 1.71e-15 relative.  The measured maximum is recorded (``PPND_MEASURED``) and is what the
GPU test of the proposal rows multiplies by sum_j |L_ij|."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import _evidence_ref as ER

EPS = 2.0 ** -53
PPND_BOUND = 1e-16 + 14.5 * EPS
LD = np.longdouble


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    try:
        return ER.HostBridge(tmp_path_factory.mktemp("evidence_host"))
    except RuntimeError as e:
        pytest.skip(str(e))


@pytest.fixture(scope="module")
def g_ev():
    return np.load(os.path.join(GOLDEN, "evidence.npz"))


# ---------------------------------------------------------------- 1. the inverse normal CDF
def ppnd_points():
    """k of u = (k + 1/2) 2^-53: 10^4 spread over the whole range (uniform in u and log-uniform in both tails), the two
    ends, 1/2, and both sides of the seams |u - 1/2| = 0.425 and r = 5 (tail area e^-25)."""
    rng = np.random.RandomState(241)
    top = 2 ** 53
    ks = [int(x) for x in rng.randint(0, 2 ** 31, size=4000).astype(object) * (2 ** 22) + rng.randint(0, 2 ** 22, size=4000)]
    tails = [int(2.0 ** e) for e in rng.uniform(0.0, 52.0, size=3000)]
    ks += tails + [top - 1 - t for t in rng.permutation(tails)]
    ks += [0, 1, top - 1, top - 2, top // 2 - 1, top // 2, top // 2 + 1]
    for frac in (0.5 - 0.425, 0.5 + 0.425, float(np.exp(-25.0)), 1.0 - float(np.exp(-25.0))):
        c = int(frac * top)
        ks += [c - 2, c - 1, c, c + 1, c + 2]
    return ks


def test_ppnd_against_mpmath(H):
    import mpmath as mp
    ks = ppnd_points()
    got = H.ppnd_k(ks)
    assert np.all(np.isfinite(got))
    rel, absmid, absall = 0.0, 0.0, 0.0
    for k, z in zip(ks, got):
        ref = ER.ppf_mp(k)
        err = abs((mp.mpf(float(z)) - ref) / ref)
        rel = max(rel, float(err))
        absall = max(absall, float(abs(mp.mpf(float(z)) - ref)))
        if abs(k - 2 ** 52) < 2 ** 40:
            absmid = max(absmid, float(abs(mp.mpf(float(z)) - ref)))
    print("br_ppnd host build: %d points, max relative error %.3e (bound %.3e), max absolute error %.3e, near 1/2 %.3e"
          % (len(ks), rel, PPND_BOUND, absall, absmid))
    assert rel <= PPND_BOUND
    # what the GPU test of the proposal rows uses is what is measured here
    assert rel <= ER.PPND_MEASURED_REL and absall <= ER.PPND_MEASURED_ABS
    # the ends are finite and symmetric bit for bit; u = 1/2 itself is not a point (k + 1/2 is never 2^52)
    assert got[ks.index(0)] == -got[ks.index(2 ** 53 - 1)] and 8.0 < got[ks.index(2 ** 53 - 1)] < 8.3
    assert H.lib.br_host_centered(2 ** 52) == 2.0 ** -54 and H.lib.br_host_centered(0) == -0.5 + 2.0 ** -54
    assert H.lib.br_host_bits53(0xffffffff, 0xffffffff) == 2 ** 53 - 1 and H.lib.br_host_bits53(1 << 5, 1 << 6) == (1 << 26) + 1


# ---------------------------------------------------------------- 2. Cholesky and lnq
def _cov(d, rho, rng):
    sd = 10.0 ** rng.uniform(-2, 2, size=d)
    c = np.full((d, d), rho) + (1 - rho) * np.eye(d)
    return c * np.outer(sd, sd)


def test_chol_and_lnq_against_scipy(H):
    from itertools import combinations
    from scipy.stats import multivariate_normal
    rng = np.random.RandomState(7)
    worst = 0.0
    for d in range(1, 6):
        for free in combinations(range(5), d):
            free = list(free)
            mask = sum(1 << i for i in free)
            for rho in (0.0, 0.999):
                cov5 = np.full((5, 5), np.nan)                      # held rows and columns are never read
                cov5[np.ix_(free, free)] = _cov(d, rho, rng)
                mu = rng.normal(size=5) * 10
                ok, L, sl = H.chol(cov5, mask)
                assert ok == 1
                Lr = ER.chol(cov5, free)
                assert np.allclose(L[np.ix_(free, free)], Lr.astype(float), rtol=1e-10)
                held = [i for i in range(5) if i not in free]
                assert np.all(L[held, held] == 1.0) and np.all(L[np.triu_indices(5, 1)] == 0.0)
                for _ in range(4):
                    th = mu + rng.normal(size=5) * np.sqrt(np.abs(np.nan_to_num(np.diag(cov5), nan=1.0)))
                    got = H.lnq(th, mu, L, mask, sl)
                    ref = float(ER.lnq(th, mu, Lr, free))
                    # the longdouble restatement against scipy (float64: looser where the matrix is nearly singular)
                    # (on standardised variables: scipy calls a matrix of very unequal variances singular)
                    sd = np.sqrt(np.diag(cov5)[free])
                    sp = multivariate_normal.logpdf((th[free] - mu[free]) / sd, np.zeros(d),
                                                    cov5[np.ix_(free, free)] / np.outer(sd, sd)) - np.log(sd).sum()
                    assert abs(ref - sp) <= (1e-6 if rho else 1e-11) * max(1.0, abs(ref))
                    # condition number of the 0.999 matrix is 1e3 d: the quadratic form carries that times eps
                    tol = (4e3 * d if rho else 8) * 16 * EPS * max(1.0, abs(ref))
                    worst = max(worst, abs(got - ref) / max(1.0, abs(ref)))
                    assert abs(got - ref) <= tol, (free, rho, got, ref)
    print("br_lnq host build against longdouble: max %.2e of max(1, |lnq|)" % worst)
    # a singular matrix, two identical columns, a NaN, a negative variance: reported, L zero, the sum NaN
    x = rng.normal(size=(50, 5)); x[:, 3] = x[:, 1]
    for bad in (np.cov(x.T), np.diag([1.0, 1.0, -1.0, 1.0, 1.0]), np.full((5, 5), np.nan), np.zeros((5, 5))):
        ok, L, sl = H.chol(bad, 31)
        assert ok == 0 and np.all(L == 0.0) and np.isnan(sl)
    ok, L, sl = H.chol(np.full((5, 5), np.nan), 0)                  # nothing free: nothing to factor
    assert ok == 1 and np.array_equal(L, np.eye(5)) and sl == 0.0
    # the free set: the caller's, the model's, the chain's
    assert H.free_mask([0, 0, 0, 0, 0], 0, 0) == 31 and H.free_mask([0, 1, 0, 0, 0], 1, 1) == 0b10001
    assert H.free_mask([0, 0, 0, 0, 0], 1, 0, held=1) == 0b11010 and H.free_mask([1] * 5, 0, 0) == 0
    # a draw: held parameters bit for bit, free ones mu + L z
    cov5 = _cov(5, 0.5, rng)
    ok, L, sl = H.chol(cov5, 0b10011)
    z, mu, held = rng.normal(size=5), rng.normal(size=5), np.array([0.1, 0.2, 0.3, np.pi, 0.5])
    th = H.draw(mu, L, z, 0b10011, held)
    assert th[2] == held[2] and th[3] == held[3]
    Lf = L[np.ix_([0, 1, 4], [0, 1, 4])]
    assert np.allclose(th[[0, 1, 4]], mu[[0, 1, 4]] + Lf @ z[[0, 1, 4]], rtol=1e-14)


# ---------------------------------------------------------------- 3. the bridge terms
def test_bridge_terms_at_the_extremes(H):
    import mpmath as mp
    mp.mp.dps = 50
    s1, s2 = 0.3, 0.7
    for rho in (1e-30, 1.0, 1e30):
        for x in (-800.0, -30.0, -1e-3, 0.0, 1e-3, 30.0, 800.0):
            num, den = H.lib.br_host_term_num(x, rho, s1, s2), H.lib.br_host_term_den(x, rho, s1, s2)
            assert np.isfinite(num) and np.isfinite(den) and num >= 0 and den >= 0
            e = mp.exp(mp.mpf(x))
            rnum = e / (mp.mpf(s1) * e + mp.mpf(s2) * mp.mpf(rho))
            rden = 1 / (mp.mpf(s1) * e + mp.mpf(s2) * mp.mpf(rho))
            for got, ref in ((num, rnum), (den, rden)):
                if ref < mp.mpf(2) ** -1022:
                    assert got <= 2.0 ** -1021                      # (below the normal range: 0 or a subnormal)
                else:
                    assert abs(mp.mpf(got) - ref) / ref <= 16 * EPS, (x, rho, got, ref)
        assert H.lib.br_host_term_num(-np.inf, rho, s1, s2) == 0.0
        assert H.lib.br_host_term_num(np.nan, rho, s1, s2) == 0.0
    assert H.lib.br_host_converged(1.0 + 1e-11, 1.0, 1e-10) == 1 and H.lib.br_host_converged(1.0 + 1e-9, 1.0, 1e-10) == 0
    assert H.lib.br_host_converged(np.nan, 1.0, 1e-10) == 0 and H.lib.br_host_converged(1.0, 1.0, 0.0) == 1
    assert H.lib.br_host_relerr2(2.0, 8.0, 100.0, 4.0, 32.0, 50.0) == 8.0 / (100 * 4.0) + 32.0 / (50 * 16.0)
    assert (H.tol_default, H.maxiter_default) == (1e-10, 1000)


# ---------------------------------------------------------------- 4. a known Z, independent samples
def _truncated_case(seed, n=4000):
    """p~ = c N(0, I2) on x0 >= -1: Z = c Phi(1).  n iid draws; half fit the proposal, half are bridged to."""
    from math import erf, log, sqrt
    rng = np.random.RandomState(seed)
    lnc = 3.7
    x = rng.normal(size=(3 * n, 2))
    x = x[x[:, 0] >= -1.0][:n]
    lnp = lambda y: np.where(y[:, 0] >= -1.0, lnc - 0.5 * np.sum(y * y, axis=1) - np.log(2 * np.pi), -np.inf)   # noqa: E731
    fit, post = x[:n // 2], x[n // 2:]
    mu, cov = fit.mean(axis=0), np.cov(fit.T)
    L = np.linalg.cholesky(cov)
    prop = mu + rng.normal(size=(n // 2, 2)) @ L.T

    def lq(y):
        r = np.linalg.solve(L, (y - mu).T).T
        return -np.log(2 * np.pi) - np.log(np.diag(L)).sum() - 0.5 * np.sum(r * r, axis=1)
    with np.errstate(divide="ignore"):
        return lnp(post) - lq(post), lnp(prop) - lq(prop), lnc + log(0.5 * (1 + erf(1 / sqrt(2))))


def test_known_z_iid(H):
    worst = 0.0
    for seed in range(5):
        l1, l2, truth = _truncated_case(seed)
        ref = ER.ref_bridge(l1, l2)
        host = ER.host_drive(H, l1, l2)
        for r in (ref, host):
            assert r["converged"] and r["niter"] <= 30
            assert abs(r["lnz"] - truth) <= 5 * r["err"] and r["err"] < 0.05, (seed, r["lnz"], truth, r["err"])
            worst = max(worst, abs(r["lnz"] - truth) / r["err"])
        assert abs(host["lnz"] - ref["lnz"]) <= 1e-10 / (1 - ref["contraction"]) + 1e-12
        assert abs(host["err"] - ref["err"]) <= 1e-9 * ref["err"]
        # the shift is a convenience: another one gives the same answer to rounding
        for shift in (-50.0, 50.0):
            sh = ER.host_drive(H, l1, l2, lstar=np.mean(l1) + shift)
            assert abs(sh["lnz"] - host["lnz"]) <= 1e-10 / (1 - ref["contraction"]) + 1e-12
            assert abs(sh["err"] - host["err"]) <= 1e-9 * host["err"]
            assert abs(ER.ref_bridge(l1, l2, lstar=np.mean(l1) + shift)["lnz"] - ref["lnz"]) <= 1e-13
    print("known Z, iid: worst deviation %.2f reported errors" % worst)
    # fewer effective samples: the same fixed point family, a larger error
    l1, l2, truth = _truncated_case(0)
    e_half = ER.ref_bridge(l1, l2, neff=len(l1) / 10)
    assert e_half["err"] > ER.ref_bridge(l1, l2)["err"] and abs(e_half["lnz"] - truth) <= 5 * e_half["err"]


# ---------------------------------------------------------------- 5. the method on a correlated chain
_CHAIN = {}


def stretch_chain(oracle, g_ev, case="b", nw=32, nsteps=600, seed=3):
    """The numpy stretch move on the oracle's lnP of a fixture case: chain [nw, nsteps, 5], lnprob [nw, nsteps]"""
    key = (case, nw, nsteps, seed)
    if key not in _CHAIN:
        from _stretch_ref import stretch_move
        lnp = ER.oracle_lnp(oracle, g_ev, case)
        free = ER.FREE[case]
        rng = np.random.RandomState(seed)
        p = (g_ev["b/mean"] + 0.5 * g_ev["b/sigma"] * np.abs(rng.normal(size=(nw, 2))))[None]
        l = lnp(p)
        chain = np.empty((nw, nsteps, 5)); chain[:] = ER.THETA0
        lp = np.empty((nw, nsteps))
        for t in range(nsteps):
            stretch_move(lnp, p, l, 1, rng, zpow=len(free) - 1.0)
            chain[:, t, free] = p[0]
            lp[:, t] = l[0]
        _CHAIN[key] = (chain, lp)
    return _CHAIN[key]


def reference_evidence(oracle, g_ev, case, chain, lp, burn, n2=None, seed=11, neff="diag"):
    """The reference's whole path on a chain: proposal from the fit half, numpy draws, the oracle's lnP, the bridge."""
    import _diag_ref as DR
    free = ER.FREE[case]
    fit, post = ER.window(chain.shape[1], burn)
    mu, cov = ER.moments(chain, burn)
    L = ER.chol(cov, free)
    xp = chain[:, post].reshape(-1, 5)
    n2 = len(xp) if n2 is None else n2
    rng = np.random.RandomState(seed)
    prop = np.broadcast_to(ER.THETA0, (n2, 5)).copy()
    prop[:, free] = mu[free].astype(float) + rng.normal(size=(n2, len(free))) @ L.astype(float).T
    lnp = ER.oracle_lnp(oracle, g_ev, case)
    l1 = lp[:, post].reshape(-1) - ER.lnq(xp, mu, L, free)
    l2 = lnp(prop[:, free]) - ER.lnq(prop, mu, L, free)
    if neff == "diag":
        d = DR.diagnostics_ref(chain[:, post], 0)
        neff = np.nanmin(d["ess"][free])
    return ER.ref_bridge(l1, l2, neff=neff), neff


@pytest.mark.parametrize("case", ["b", "c"])
def test_method_on_a_correlated_chain(oracle, g_ev, case):
    chain, lp = stretch_chain(oracle, g_ev, case)
    r, neff = reference_evidence(oracle, g_ev, case, chain, lp, 200)
    truth = float(g_ev[case + "/lnz"])
    print("case (%s): lnz %.4f +- %.4f, truth %.4f (%.2f errors), neff %.0f of %d, %d iterations"
          % (case, r["lnz"], r["err"], truth, abs(r["lnz"] - truth) / r["err"], neff, r["n1"], r["niter"]))
    assert r["converged"] and abs(r["lnz"] - truth) <= 5 * r["err"] and r["err"] <= 0.1


def test_exact_gaussian_case_stays_under_its_cap(g_ev):
    """Case (a) as the GPU test runs it -- [1, 8, 64] Gaussian draws of fnorm, N2 = 256 -- with the reference alone, over
    40 seeds: the error stays under the GPU test's cap of 0.05 and the estimate within 5 of it."""
    m, s, truth = float(g_ev["a/mean"]), float(g_ev["a/sigma"]), float(g_ev["a/lnz"])
    peak = truth - 0.5 * np.log(2 * np.pi * s * s)                 # lnP at the mean
    worst_err, worst_dev = 0.0, 0.0
    for seed in range(40):
        rng = np.random.RandomState(seed)
        x = m + s * rng.normal(size=(8, 64))
        lp = peak - 0.5 * ((x - m) / s) ** 2
        mu, sd = x[:, :32].mean(), x[:, :32].std(ddof=1)
        lq = lambda y: -0.5 * np.log(2 * np.pi) - np.log(sd) - 0.5 * ((y - mu) / sd) ** 2    # noqa: E731
        prop = mu + sd * rng.normal(size=256)
        r = ER.ref_bridge((lp - lq(x))[:, 32:].ravel(), peak - 0.5 * ((prop - m) / s) ** 2 - lq(prop))
        worst_err, worst_dev = max(worst_err, r["err"]), max(worst_dev, abs(r["lnz"] - truth) / r["err"])
    print("case (a), reference: largest error %.4f, worst deviation %.2f errors" % (worst_err, worst_dev))
    assert worst_err <= 0.05 and worst_dev <= 5.0


def test_fixture_is_what_the_generator_makes(oracle, g_ev):
    """(a) again from the fixture's data: the closed form; the quadrature's own error estimate is far below the tests'
    bounds."""
    import _map_ref as MR
    like = MR.oracle_like(oracle, None, ER.case_settings(), g_ev["flux"], g_ev["unc"])
    p1 = ER.THETA0.copy(); p1[4] = 1.0
    sb = like(p1, return_flux=True)[1][0].astype(LD)
    f, iv = g_ev["flux"].astype(LD), 1 / g_ev["unc"].astype(LD) ** 2
    A, B = np.sum(sb * sb * iv), np.sum(sb * f * iv)
    assert abs(float(-(np.sum(f * f * iv) - B * B / A) / 2 + np.log(2 * LD(np.pi) / A) / 2) - float(g_ev["a/lnz"])) < 1e-13
    assert g_ev["b/quad_relerr"] < 1e-9 and g_ev["c/quad_relerr"] < 1e-9
    assert abs(float(g_ev["c/lowlim_T"]) - (g_ev["b/mean"][0] - g_ev["b/sigma"][0])) < 1e-12


# ---------------------------------------------------------------- 6. ln_prior_norm
class _Like(object):
    """Stands where a likelihood would: it has data, limits and priors, and touching the device is an error."""
    data_read = True
    nsources = 1
    opthin = noalpha = False
    wavenorm = 500.0

    def __init__(self, nsources=1, opthin=False, noalpha=False):
        self.nsources, self._ndata, self.opthin, self.noalpha = nsources, 3, opthin, noalpha
        self._lowlim = np.array([1, 0.1, 1, 0.1, 1e-3])
        self._has_uplim = [False, True, False, True, False, False]
        self._uplim = np.array([np.inf, 20.0, np.inf, 20.0, np.inf, np.inf])
        self._has_gprior = [False] * 6
        self._gprior_mean, self._gprior_sigma = np.zeros(6), np.ones(6)

    def _sync_device(self):
        raise AssertionError("the device was touched")

    context = property(_sync_device)


def test_ln_prior_norm_against_quadrature():
    from scipy import integrate
    from mbb_emcee_amd.evidence import ln_prior_norm
    like = _Like(opthin=True)
    like._has_uplim[0], like._uplim[0] = True, 60.0                                   # T: wall only
    like._has_gprior[4], like._gprior_mean[4], like._gprior_sigma[4] = True, 40.0, 5.0   # fnorm: prior only
    like._has_gprior[1], like._gprior_mean[1], like._gprior_sigma[1] = True, 1.8, 0.3    # beta: wall and prior
    like._has_gprior[3], like._gprior_mean[3], like._gprior_sigma[3] = True, -1.0, 0.5   # alpha: a prior centred below the limit

    def factor(i):
        lo = like._lowlim[i]

        def w(x):
            v = 1.0
            if like._has_uplim[i] and x > like._uplim[i]:
                v *= np.exp(-0.5 * ((x - like._uplim[i]) / (0.02 * (like._uplim[i] - lo))) ** 2)
            if like._has_gprior[i]:
                v *= np.exp(-0.5 * ((x - like._gprior_mean[i]) / like._gprior_sigma[i]) ** 2)
            return v
        pts = [p for p in (like._uplim[i] if like._has_uplim[i] else None,
                           like._gprior_mean[i] if like._has_gprior[i] else None) if p is not None and p > lo]
        hi = max(pts + [lo]) + 12 * max(like._gprior_sigma[i] if like._has_gprior[i] else 0.0,
                                        0.02 * (like._uplim[i] - lo) if like._has_uplim[i] else 0.0)
        return integrate.quad(w, lo, hi, points=pts or None, epsabs=0, epsrel=1e-12, limit=400)[0]
    for fixed, free in (([0, 1, 0, 1, 1], [0]), ([1, 1, 0, 1, 0], [4]), ([1, 0, 0, 1, 1], [1]), ([1, 1, 0, 0, 1], [3]),
                        ([0, 0, 0, 0, 0], [0, 1, 3, 4])):
        ln, improper, peak = ln_prior_norm(like, fixed)
        ref = sum(np.log(factor(i)) for i in free)
        assert abs(ln - ref) <= 1e-10 * max(1.0, abs(ref)), (free, ln, ref)
        assert not improper.any() and peak is False
    # lambda0 of a thick model with neither a limit nor a prior; a peak-wavelength term
    thick = _Like()
    ln, improper, peak = ln_prior_norm(thick)
    assert list(improper) == [True, False, True, False, True] and peak is False
    assert abs(ln - 2 * np.log(19.9 + 0.02 * 19.9 * np.sqrt(np.pi / 2))) < 1e-13
    thick._has_uplim[5] = True
    assert ln_prior_norm(thick)[2] is True
    assert list(ln_prior_norm(thick, [1, 0, 1, 0, 1])[1]) == [False] * 5
    with pytest.raises(ValueError, match="five entries"):
        ln_prior_norm(thick, [1, 0])


# ---------------------------------------------------------------- 7. the interface rules
def _made(like=None, nsrc=1, multi=False, fixed=None, lnz=(-3.0,), err=(0.03,), held_bits=0):
    from mbb_emcee_amd import evidence, _native
    req = evidence._Request(like or _Like(opthin=True, noalpha=True), 100, fixed, burn=2, thin=3)
    raw = evidence._Raw(nsrc, 40, 100, False)
    raw.lnz[:], raw.lnz_err[:] = lnz, err
    raw.niter[:], raw.n1[:], raw.n_inside[:] = 7, 40, 90
    raw.status[:] = _native.EV_CONVERGED | held_bits
    return evidence.ChainEvidence(req, raw, multi, 10, 8), raw


def test_chain_evidence_properties():
    from mbb_emcee_amd import _native
    like = _Like(opthin=True, noalpha=True)
    like._has_uplim[0], like._uplim[0] = True, 60.0
    like._has_gprior[4], like._gprior_mean[4], like._gprior_sigma[4] = True, 40.0, 5.0
    bits = (1 << (8 + 2)) | (1 << (8 + 3))
    e, raw = _made(like, held_bits=bits)
    norm = e.ln_prior_norm
    assert e.lnz == -3.0 and e.lnz_err == 0.03 and e.niter == 7 and e.n1 == 40 and e.n2 == 100 and e.n_inside == 90
    assert e.ln_evidence == -3.0 - norm and bool(e.converged) and e.neff == 40.0
    assert list(e.held) == [False, False, True, True, False] and e.burn == 2 and e.thin == 3 and e.nsteps_used == 8
    assert e.proposal is None and e.posterior_lnq is None
    arr = e.arrays()
    assert {"evidence_lnz", "evidence_lnz_err", "evidence_ln_evidence", "evidence_status", "evidence_n1", "evidence_n2",
            "evidence_n_inside", "evidence_neff", "evidence_proposal_mean", "evidence_proposal_cov"} <= set(arr)
    assert all(k.startswith("evidence_") for k in arr) and set(e.arrays("e_")) == {"e_" + k[9:] for k in arr}
    assert "ln Z: -3.0000 +- 0.0300 (7 iterations; CONVERGED HELD_lambda0 HELD_alpha)" in str(e)
    assert "ln evidence under normalised priors: %.4f" % (-3.0 - norm) in str(e)
    # beta is free with its default wall, T has neither limit nor prior: improper, no ln_evidence
    plain = _Like(opthin=True, noalpha=True)
    e2, _ = _made(plain, held_bits=bits)
    assert np.isnan(e2.ln_evidence) and list(e2.improper) == [True, False, False, False, True]
    assert "undefined (T, fnorm has neither" in str(e2)
    # ... unless the chain held it
    e3, _ = _made(plain, held_bits=bits | (1 << 8) | (1 << 12))
    assert np.isfinite(e3.ln_evidence)
    # a source axis
    em, _ = _made(_Like(3, True, True), 3, True, lnz=(-1.0, -2.0, -3.0), err=(0.1, 0.2, 0.3), held_bits=bits)
    assert em.lnz.shape == (3,) and em.held.shape == (3, 5) and "Source 0 of 3" in str(em)
    em._raw.status[1] |= _native.EV_COV_SINGULAR
    assert em.status_names(1)[:2] == ["CONVERGED", "COV_SINGULAR"]


def test_bayes_factor_and_its_refusals():
    like = _Like(opthin=True, noalpha=True)
    like._has_uplim[0], like._uplim[0] = True, 60.0
    like._has_gprior[4], like._gprior_mean[4], like._gprior_sigma[4] = True, 40.0, 5.0
    bits = (1 << 10) | (1 << 11)
    a, _ = _made(like, held_bits=bits, lnz=(-3.0,), err=(0.03,))
    b, _ = _made(like, held_bits=bits | (1 << 9), fixed=[0, 1, 0, 0, 0], lnz=(-5.0,), err=(0.04,))
    d, e = a.bayes_factor(b)
    assert d == (-3.0 - a.ln_prior_norm) - (-5.0 - b.ln_prior_norm) and e == pytest.approx(0.05)
    assert a.ln_prior_norm != b.ln_prior_norm                      # (beta's wall is normalised in one and absent in the other)
    # improper in both, free in both: the unknown factor cancels
    plain = _Like(opthin=True, noalpha=True)
    p, _ = _made(plain, held_bits=bits)
    q, _ = _made(plain, held_bits=bits, lnz=(-4.0,))
    assert q.bayes_factor(p)[0] == -1.0
    # improper in one, held in the other
    r, _ = _made(plain, held_bits=bits | (1 << 8), fixed=[1, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="T is free without an upper limit or a prior in one fit"):
        p.bayes_factor(r)
    with pytest.raises(TypeError):
        p.bayes_factor(-3.0)
    m, _ = _made(_Like(2, True, True), 2, True, lnz=(-1.0, -2.0), err=(0.1, 0.1), held_bits=bits)
    with pytest.raises(ValueError, match="different numbers of sources"):
        m.bayes_factor(p)


def test_request_refusals():
    from mbb_emcee_amd import chain_evidence
    like = _Like()
    chain, lp = np.zeros((4, 8, 5)), np.zeros((4, 8))
    for kw, msg in ((dict(burn=-1), "burn must be"), (dict(thin=0), "burn must be"), (dict(burn=8), "burn leaves no step"),
                    (dict(burn=7), "two kept steps"), (dict(thin=8), "two kept steps"), (dict(n2=-1), "n2 must be"),
                    (dict(n2=(1 << 22) + 1), "n2 must be"), (dict(tol=-1e-3), "tol must be"), (dict(tol=np.nan), "tol must be"),
                    (dict(tol=np.inf), "tol must be"), (dict(maxiter=0), "maxiter must be"),
                    (dict(maxiter=100001), "maxiter must be"), (dict(neff=0.0), "neff must be"),
                    (dict(neff=np.nan), "neff must be"),
                    (dict(neff=-5.0), "neff must be"), (dict(neff="ess"), "neff must be"), (dict(fixed=[1, 0]), "five entries"),
                    (dict(first_source=-1), "first_source")):
        with pytest.raises(ValueError, match=msg):
            chain_evidence(like, chain, lp, **kw)
    with pytest.raises(ValueError, match="chain must be"):
        chain_evidence(like, np.zeros((4, 8, 4)), lp)
    with pytest.raises(ValueError, match="needs the chain's lnprob"):
        chain_evidence(like, chain, None)
    with pytest.raises(ValueError, match="lnprob must have"):
        chain_evidence(like, chain, np.zeros((4, 7)))
    with pytest.raises(ValueError, match="lnprob must have"):
        chain_evidence(_Like(3), np.zeros((3, 4, 8, 5)), lp)
    with pytest.raises(ValueError, match="2 sources, the likelihood 3"):
        chain_evidence(_Like(3), np.zeros((2, 4, 8, 5)), np.zeros((2, 4, 8)))
    nodata = _Like()
    nodata.data_read = False
    with pytest.raises(Exception, match="Data not read"):
        chain_evidence(nodata, chain, lp)
    # everything in order: the next thing is the device
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_evidence(like, chain, lp, neff=None, burn=6)
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_evidence(like, chain, lp)                             # (neff="auto": the diagnostics come first)


def _bare_sampler():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary, s.seed = 10, 5, _Like(), None, None, 5

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_evidence_keyword_rules():
    s = _bare_sampler()
    p0 = np.zeros((10, 5))
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(p0, 16, storechain=False, evidence=True)
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(p0, 16, evidence=dict(burn=16))
    with pytest.raises(ValueError, match="two kept steps"):                 # burn taken from the summary's keywords
        s.run_mcmc(p0, 16, summary=dict(burn=15), evidence=True)
    with pytest.raises(TypeError, match="unexpected keyword"):
        s.run_mcmc(p0, 16, evidence=dict(percentile=68.3))
    with pytest.raises(ValueError, match="n2 must be"):
        s.run_mcmc(p0, 16, evidence=dict(n2=-4))
    with pytest.raises(ValueError, match="neff must be"):
        s.run_mcmc(p0, 16, evidence=dict(neff=-1.0))
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, storechain=False, summary=dict(burn=4), evidence=True)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, evidence=False)                                  # (False is no request: the run itself is next)
    assert s.evidence_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.evidence()
    s._resident = 16
    with pytest.raises(ValueError, match="two kept steps"):
        s.evidence(burn=15)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.evidence(burn=4, neff=None)
    # reset() and the start of a run clear the attribute
    s._open = None
    s.evidence_ = object()
    s.reset()
    assert s.evidence_ is None
    s.evidence_ = object()
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 4)
    assert s.evidence_ is None


def test_sharded_run_has_no_evidence():
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.lnprobfn, s.seed, s.k = _Like(), 1, 10
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded"):
        s.run_mcmc(np.zeros((10, 5)), 4, evidence=True)


def test_fitter_and_cli_know_evidence():
    import mbb_emcee_amd
    from mbb_emcee_amd import mbb_fitter, run_mbb_emcee
    assert mbb_emcee_amd.chain_evidence is mbb_emcee_amd.evidence.chain_evidence
    assert "ChainEvidence" in mbb_emcee_amd.__all__ and "chain_evidence" in mbb_emcee_amd.__all__
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="evidence= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), evidence=True)
    assert fit.evidence is None
    p = run_mbb_emcee.build_parser()
    assert p.parse_args(["phot.txt", "out.npz"]).evidence is None
    assert p.parse_args(["phot.txt", "out.npz", "--evidence"]).evidence == -1
    assert p.parse_args(["phot.txt", "out.npz", "--evidence", "5000"]).evidence == 5000


def test_evidence_entries_are_declared_and_bound(tmp_path):
    from mbb_emcee_amd import _native
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_evidence", "mbb_sampler_evidence"):
        assert name in hdr and name in _native.SIGNATURES
    for name, val in (("CONVERGED", 1), ("MAXITER", 2), ("COV_SINGULAR", 4), ("POST_LEFT_OUT", 8), ("NO_OVERLAP", 16),
                      ("ALL_HELD", 32), ("HELD_SHIFT", 8)):
        assert re.search(r"MBB_EV_%s = %d\b" % (name, val), hdr) and getattr(_native, "EV_" + name) == val
        assert getattr(ER, name) == val
    src = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_evidence.hip.h")).read()
    assert "0x%08xu" % ER.STREAM in src and "kMaxN2 = 1 << 22" in src and _native.EV_MAX_N2 == 1 << 22
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if cc:
        c = tmp_path / "sizes.c"
        c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbb_hip.h"\nint main(void) {\n'
                     'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mbb_evidence_spec), offsetof(mbb_evidence_spec, tol), '
                     'offsetof(mbb_evidence_spec, seed), offsetof(mbb_evidence_spec, neff), sizeof(mbb_evidence_out), '
                     'offsetof(mbb_evidence_out, post_lnq));\nreturn 0; }\n')
        exe = str(tmp_path / "sizes")
        subprocess.check_call([cc, "-I" + os.path.join(ROOT, "include"), str(c), "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
        assert got == [C.sizeof(_native.EvidenceSpec), _native.EvidenceSpec.tol.offset, _native.EvidenceSpec.seed.offset,
                       _native.EvidenceSpec.neff.offset, C.sizeof(_native.EvidenceOut), _native.EvidenceOut.post_lnq.offset]
    build = open(os.path.join(ROOT, "mbb_emcee_amd", "build.py")).read()
    assert "mbb_bridge.hip.h" in build and "mbb_evidence.hip.h" in build
    flow = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_flow.hip")).read()
    assert "mbb_evidence" not in flow and "mbb_bridge" not in flow
    lib = os.path.join(ROOT, "mbb_emcee_amd", "libmbb_hip.so")
    if os.path.exists(lib) and shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE).stdout.decode()
        assert [ln.split()[-1] for ln in syms.splitlines() if "evidence" in ln.split()[-1] and " T " in ln] == \
            ["mbb_chain_evidence", "mbb_sampler_evidence"]
