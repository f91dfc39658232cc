"""CPU side of the MAP-fit tests (tests/test_map_gpu.py is the GPU side): the sum-of-squares restatement of -2 ln P
against the oracle, the fixture against a fresh scipy search, the HOST build of csrc/mbb_lm.hip.h function by function
and driven to the fixture's optima (the algorithm without a device), ``MapFit``'s derived quantities on hand-made raw
results, ``map_initial_values``, the argument rules of ``find_map`` and ``--map-init`` on a faked device, the request's
refusals and the declarations of the new entry point.

Gap criterion: lnP_oracle(theta_ref) - lnP_oracle(theta) <= 1e-10 max(1, |lnP|) -- SURVEY.md 8c's tolerance between the
device's likelihood and the oracle's; an optimiser working on a likelihood allowed to differ by that much cannot be asked
for more."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import _map_ref as MR


@pytest.fixture(scope="module")
def g_map():
    return np.load(os.path.join(GOLDEN, "map.npz"))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    try:
        return MR.HostLM(tmp_path_factory.mktemp("map_host"))
    except RuntimeError as e:
        pytest.skip(str(e))


def _case(oracle, g_pb, g_map, name):
    s, nstart = MR.case_specs()[name]
    like = MR.oracle_like(oracle, g_pb, s, g_map[name + "/flux"], g_map[name + "/unc"])
    return s, like


NAMES = sorted(MR.case_specs())


# ---------------------------------------------------------------- the restatement and the fixture
def test_fixture_holds_its_cases(g_map):
    assert sorted(str(n) for n in g_map["names"]) == NAMES and list(g_map["bands"]) == MR.BANDS
    for name, (s, nstart) in MR.case_specs().items():
        assert g_map[name + "/starts"].shape == (nstart, 5)
        for key in ("lowlim", "has_uplim", "uplim", "has_gprior", "gmean", "gsigma"):
            assert np.array_equal(g_map[name + "/" + key], s[key]), (name, key)
        assert np.all(g_map[name + "/starts"] >= s["lowlim"])
    # the figures the cases were specified with
    for name, lnp in (("beta_lowlim", -0.89583138797), ("T_wall", -1.32462867801), ("peak_prior", -0.11454974677),
                      ("peak_wall", -31.5668408237)):
        assert abs(float(g_map[name + "/lnp_ref"]) - lnp) <= 1e-10 * max(1, abs(lnp)), name
    assert g_map["beta_lowlim/theta_ref"][1] == 2.0 and abs(g_map["beta_lowlim/theta_ref"][0] - 11.2394178) < 1e-6
    assert g_map["T_wall/theta_ref"][0] > 11.0 and abs(g_map["T_wall/theta_ref"][0] - 11.1177) < 1e-4


@pytest.mark.parametrize("name", NAMES)
def test_residual_form_is_the_oracles_lnp(oracle, g_pb, g_map, name):
    s, like = _case(oracle, g_pb, g_map, name)
    rng = np.random.default_rng(11)
    rows = [g_map[name + "/theta_ref"]] + list(g_map[name + "/starts"])
    # random rows, some beyond every wall the case has (beta and alpha 20, lambda0 2550, T 11, the peak's)
    for k in range(24):
        p = MR.TRUTH * (1.0 + 0.4 * rng.uniform(-1, 1, 5))
        if k % 4 == 1:
            p[1] = 20.0 + rng.uniform(0, 2)
        if k % 4 == 2:
            p[2] = 2550.0 + rng.uniform(0, 300)
        if k % 4 == 3:
            p[0], p[3] = rng.uniform(8, 11), 20.0 + rng.uniform(0, 1)
        rows.append(np.maximum(p, s["lowlim"]))
    worst = 0.0
    for p in rows:
        lnp = like(p)[0]
        r = MR.residuals(oracle, like, s, p)
        worst = max(worst, abs(-0.5 * (r @ r) - lnp) / max(1.0, abs(lnp)))
    assert worst <= 1e-12, worst


def test_fixture_regenerates(oracle, g_pb, g_map):
    pytest.importorskip("scipy.optimize", reason="the reference search needs scipy")
    for name in NAMES:                              # every case, from its first two starts
        s, like = _case(oracle, g_pb, g_map, name)
        flux, unc = MR.make_data(oracle, g_pb, s)
        assert np.array_equal(flux, g_map[name + "/flux"]) and np.array_equal(unc, g_map[name + "/unc"])
        assert np.array_equal(MR.make_starts(s, g_map[name + "/starts"].shape[0]), g_map[name + "/starts"])
        lnp_ref = float(g_map[name + "/lnp_ref"])
        best = max(MR.ref_search(oracle, like, s, x0)[1] for x0 in g_map[name + "/starts"][:2])
        assert best >= lnp_ref - 1e-10 * max(1.0, abs(lnp_ref)), (name, best, lnp_ref)
        assert like(g_map[name + "/theta_ref"])[0] == lnp_ref
        cov, dis = MR.ref_cov(oracle, like, s, g_map[name + "/theta_ref"])
        assert np.allclose(cov, g_map[name + "/cov_ref"], rtol=1e-9, equal_nan=True) and dis < 1e-7


# ---------------------------------------------------------------- the host build of the step functions
def _spd(rng, scale):
    M = rng.normal(size=(9, 5)) * scale
    return M.T @ M


def test_damped_solve_against_numpy(H):
    rng = np.random.default_rng(3)
    for k in range(40):
        scale = 10.0 ** rng.uniform(-3, 3, 5)
        A, g = _spd(rng, scale), rng.normal(size=5) * scale
        lam = 10.0 ** rng.uniform(-6, 2)
        active = int(rng.integers(1, 32))
        idx = [i for i in range(5) if (active >> i) & 1]
        ok, d = H.solve(A, g, lam, active)
        assert ok == 1
        sub = A[np.ix_(idx, idx)]
        ref = np.linalg.solve(sub + lam * np.diag(np.diag(sub)), g[idx])
        assert np.allclose(d[idx], ref, rtol=1e-9, atol=0), (k, d[idx], ref)
        assert all(d[i] == 0.0 for i in range(5) if i not in idx)


def test_damped_solve_zero_column_and_bad_pivot(H):
    A = np.diag([4.0, 1.0, 0.0, 9.0, 1.0])
    g = np.array([4.0, 1.0, 0.0, 9.0, 1.0])
    ok, d = H.solve(A, g, 1.0, 31)          # a zero column: its diagonal is floored, the system stays regular
    assert ok == 1 and np.all(np.isfinite(d)) and np.allclose(d[[0, 1, 3, 4]], 0.5) and d[2] == 0.0
    ok, d = H.solve(A, g + np.array([0, 0, 1.0, 0, 0]), 1.0, 31)
    assert ok == 1 and np.all(np.isfinite(d))
    # not positive definite: reported, not divided by
    B = np.array([[1.0, 2.0], [2.0, 1.0]])
    A2 = np.eye(5); A2[:2, :2] = B
    ok, d = H.solve(A2, np.ones(5), 1e-9, 31)
    assert ok == 0 and np.array_equal(d, np.zeros(5))
    A3 = np.eye(5); A3[1, 1] = -1.0
    assert H.solve(A3, np.ones(5), 1e-3, 31)[0] == 0
    A4 = np.eye(5); A4[0, 0] = np.nan
    assert H.solve(A4, np.ones(5), 1e-3, 31)[0] == 0
    assert H.solve(A3, np.ones(5), 1e-3, 31 & ~2)[0] == 1       # the bad pivot's parameter outside the active set


def test_projection_and_active_set(H):
    low = np.array([1.0, 2.0, 1.0, 0.1, 1e-3])
    p = np.array([5.0, 2.0, 1.0, 3.0, 1e-3])
    # beta on its limit with g pointing outward: held; lambda0 on its limit with g pointing inward: active; fnorm on
    # its limit with g zero: active
    g = np.array([1.0, -1.0, 2.0, -3.0, 0.0])
    assert H.active(p, low, g, 0) == 0b11101
    assert H.active(p, low, g, 0b00001) == 0b11100                 # a fixed parameter is never active
    assert H.fixed_mask([0, 1, 0, 0, 0], 1, 0) == 0b00110 and H.fixed_mask([0, 0, 0, 0, 0], 0, 1) == 0b01000
    assert H.fixed_mask([1, 0, 0, 0, 1], 1, 1) == 0b11101
    t = H.project(p, np.array([-10.0, -1.0, -5.0, 1.0, 0.5]), low, 0b11101)
    assert np.array_equal(t, [1.0, 2.0, 1.0, 4.0, 1e-3 + 0.5])     # (beta outside the set: its value bit for bit)
    t = H.project(p, np.array([0.25, 9.0, 0.0, -2.875, 0.0]), low, 0b01001)
    assert np.array_equal(t, [5.25, 2.0, 1.0, 0.125, 1e-3])


def test_accept_gain_and_damping(H):
    nan, inf = float("nan"), float("inf")
    assert H.accept(2.0, 1.0) and not H.accept(2.0, 2.0) and not H.accept(2.0, 3.0)
    assert not H.accept(2.0, nan) and not H.accept(2.0, inf) and not H.accept(inf, inf) and H.accept(2.0, -inf) is False
    assert H.pick(2.0, [nan, 1.5, inf, 1.0]) == 3 and H.pick(2.0, [1.0, 1.0, nan, 3.0]) == 0
    assert H.pick(2.0, [nan, inf, 2.0, 5.0]) == -1
    assert H.gain(2.0, 1.0, 2.0) == 0.5 and H.gain(2.0, 1.0, 0.0) == 0.0
    c = H.candidates(1e-3, 2.0)
    assert np.allclose(c, [1e-3 / 3, 1e-3, 2e-3, 8e-3], rtol=1e-15)
    # Nielsen: gain 1 -> a third; gain 1/2 -> unchanged; gain 0 -> doubled; nu back to 2
    for rho, f in ((1.0, 1.0 / 3.0), (0.5, 1.0), (0.0, 2.0), (5.0, 1.0 / 3.0)):
        lam, nu = H.lambda_accept(0.01, rho)
        assert abs(lam - 0.01 * f) <= 1e-17 and nu == 2.0
    lam, nu = H.lambda_reject(1e-3, 2.0)             # after lam, 2 lam, 8 lam were rejected: 64 lam, nu 16
    assert abs(lam - 64e-3) < 1e-17 and nu == 16.0
    assert H.lambda_reject(1e14, 1e6)[0] == H.lam_max and H.lambda_accept(1e-15, 1.0)[0] == H.lam_min
    # the quadratic model: F(p + s) = F - 2 g.s + s.A.s
    rng = np.random.default_rng(5)
    A, g, p = _spd(rng, np.ones(5)), rng.normal(size=5), rng.normal(size=5)
    s = rng.normal(size=5) * 0.1
    assert abs(H.predicted(A, g, p, p + s) - (2 * g @ s - s @ A @ s)) < 1e-12
    assert H.converged_f(1e-14, 0.5, 1e-13) and not H.converged_f(1e-12, 0.5, 1e-13) and H.converged_f(1e-11, 200.0, 1e-13)
    assert H.scaled_step([10.0, 1.0, 0.0, 2.0, 4.0], [10.1, 1.0, 0.0, 2.0, 4.0]) == pytest.approx(0.01)
    assert H.scaled_step(np.zeros(5), np.full(5, 1e-9)) == pytest.approx(1e-9 / H.xfloor)
    assert H.converged_x(1e-10, 1e-9) and not H.converged_x(1e-8, 1e-9)


def test_laplace_inverse(H):
    rng = np.random.default_rng(7)
    A = _spd(rng, 10.0 ** rng.uniform(-2, 2, 5))
    ok, cov = H.laplace(A, 31)
    assert ok == 1 and np.allclose(cov, np.linalg.inv(A), rtol=1e-8)
    ok, cov = H.laplace(A, 0b10011)          # beta's neighbours held: NaN in their rows and columns
    idx = [0, 1, 4]
    assert ok == 1 and np.allclose(cov[np.ix_(idx, idx)], np.linalg.inv(A[np.ix_(idx, idx)]), rtol=1e-8)
    assert np.all(np.isnan(cov[[2, 3], :])) and np.all(np.isnan(cov[:, [2, 3]]))
    v = rng.normal(size=5)
    ok, cov = H.laplace(np.outer(v, v), 0b00111)      # rank one over three parameters
    assert ok == 0 and np.all(np.isnan(cov))
    assert H.laplace(-np.eye(5), 31)[0] == 0 and H.laplace(A, 0)[0] == 0
    assert H.laplace(np.outer(v, v), 0b00100)[0] == 1


@pytest.mark.parametrize("name", NAMES)
def test_host_steps_reach_the_fixture_optimum(oracle, g_pb, g_map, H, name):
    """The algorithm without a device: the host build's step functions around the oracle's residuals."""
    s, like = _case(oracle, g_pb, g_map, name)
    mask = H.fixed_mask([0] * 5, s["opthin"], s["noalpha"])
    lnp_ref = float(g_map[name + "/lnp_ref"])
    for x0 in g_map[name + "/starts"][:2]:
        p, f, niter, nfev, why = MR.lm_drive(H, lambda q: MR.residuals(oracle, like, s, q), x0, s["lowlim"], mask)
        gap = lnp_ref - like(p)[0]
        print("%s: gap %.2e after %d iterations, %d evaluations, stopped by %s" % (name, gap, niter, nfev, why))
        assert gap <= MR.gap_bound(lnp_ref), (name, gap)
        assert why in ("f", "x") and niter < 60


def _valley(corr=0.99, pstar=(0.2, 3.8)):
    """A linear problem r = L (p - p*) in parameters 0 and 1, correlated by `corr`, whose free optimum p* lies below
    parameter 0's lower limit of 1: the constrained optimum is on the limit, p_1 = p*_1 - (A_01 / A_11)(1 - p*_0), and
    the way to it runs along the valley."""
    A2 = np.array([[1.0, corr], [corr, 1.0]]) * 25.0
    L = np.zeros((5, 5))
    L[:2, :2] = np.linalg.cholesky(A2).T
    ps = np.array([pstar[0], pstar[1], 0.0, 0.0, 0.0])
    low = np.array([1.0, 0.1, -1.0, -1.0, -1.0])
    opt = np.array([1.0, pstar[1] - corr * (1.0 - pstar[0]), 0.0, 0.0, 0.0])
    rfun = lambda q: L @ (np.asarray(q) - ps)            # noqa: E731
    return rfun, (lambda q: L), low, opt


def test_convergence_is_not_declared_from_clipped_steps(H):
    """Planted A and g: every candidate of the first damping values is clipped onto the limit with a negative predicted
    reduction.  That is a rejection -- lam rises -- never CONVERGED_F."""
    rfun, jac, low, opt = _valley()
    fopt = float(rfun(opt) @ rfun(opt))
    J = jac(None)
    A = J.T @ J
    mask = 0b11100
    for start in ([1.1397, 2.8603, 0, 0, 0], [1.5, 2.5, 0, 0, 0], [3.0, 1.0, 0, 0, 0], [1.0, 3.5, 0, 0, 0], [1.001, 2.0, 0, 0, 0]):
        p0 = np.array(start, dtype=np.float64)
        p, f, niter, nfev, why = MR.lm_drive(H, rfun, p0, low, mask, jac=jac)
        print("valley from %s: stopped by %s after %d iterations at %s, F - F_opt %.2e" % (start, why, niter, p[:2], f - fopt))
        assert why in ("f", "x") and f - fopt <= 1e-12 * max(1.0, fopt), (start, p, f, fopt)
        assert p[0] == 1.0 and abs(p[1] - opt[1]) <= 1e-6
    # the situation itself, on the step functions: at the reviewer's stop point all four first candidates are clipped
    # and predict an increase
    p = np.array([1.1397, 2.8603, 0.0, 0.0, 0.0])
    g = -J.T @ rfun(p)
    act = H.active(p, low, g, mask)
    assert act == 0b00011
    for lam in H.candidates(H.lam_start, 2.0):
        ok, d = H.solve(A, g, lam, act)
        t = H.project(p, d, low, act)
        assert ok and H.clipped(p, d, low, act) and t[0] == 1.0 and H.predicted(A, g, p, t) < 0
    ok, d = H.solve(A, g, 1e4, act)                       # a short step is left alone
    assert ok and not H.clipped(p, d, low, act) and H.predicted(A, g, p, H.project(p, d, low, act)) > 0
    assert not H.clipped(p, np.array([-10.0, 0, 0, 0, 0]), low, 0b00010)       # outside the active set: never clipped
    assert H.clipped(p, np.array([0.0, -2.8, 0, 0, 0]), low, 0b00010)
    # no candidate solves (A not positive definite at any of the damping values): no convergence either, lam rises
    bad = lambda q: np.zeros((5, 5))                      # noqa: E731 -- J = 0: A = 0, diag floored, d = 0
    p, f, niter, nfev, why = MR.lm_drive(H, rfun, np.array([2.0, 2.0, 0, 0, 0]), low, mask, jac=bad, maxiter=5)
    assert np.array_equal(p, [2.0, 2.0, 0, 0, 0])


def test_host_steps_stop_by_each_rule(oracle, g_pb, g_map, H):
    s, like = _case(oracle, g_pb, g_map, "thin_noalpha_s5")
    mask = H.fixed_mask([0] * 5, True, True)
    rf = lambda q: MR.residuals(oracle, like, s, q)       # noqa: E731
    x0 = g_map["thin_noalpha_s5/starts"][0]
    assert MR.lm_drive(H, rf, x0, s["lowlim"], mask, maxiter=1)[4] == "maxiter"
    assert MR.lm_drive(H, rf, x0, s["lowlim"], mask, ftol=0.0, xtol=1e-3)[4] == "x"
    assert MR.lm_drive(H, rf, x0, s["lowlim"], mask, ftol=1e-3, xtol=0.0)[4] == "f"


# ---------------------------------------------------------------- MapFit on hand-made results
def _handmade(nsrc=2, nstart=3, ndata=4, multi=True):
    from mbb_emcee_amd import optimize, _native

    class Req(object):
        pass
    req = Req()
    req.ndata, req.fixed = ndata, np.array([0, 0, 1, 0, 0])
    req.flux = np.arange(1.0, 1.0 + nsrc * ndata).reshape(nsrc, ndata)
    req.sigma = np.full((nsrc, ndata), 0.5)
    raw = optimize._Raw(nsrc, nstart, ndata)
    raw.params[:] = np.array([12.0, 1.8, 150.0, 3.0, 40.0]) + np.arange(nsrc)[:, None]
    raw.model_flux[:] = req.flux - 1.0
    raw.cov[:] = np.nan
    raw.cov[0][np.ix_([0, 1, 4], [0, 1, 4])] = np.diag([4.0, 0.25, 9.0])
    raw.status[0] = _native.MAP_CONVERGED_F | (1 << (_native.MAP_AT_LOWLIM_SHIFT + 3))
    if nsrc > 1:
        raw.status[1] = _native.MAP_START_INVALID
    raw.lnprob[:], raw.chisq[:], raw.q[:] = -1.5, 3.0, 0.2
    return optimize.MapFit(req, raw, multi), raw


def test_mapfit_derived_quantities():
    from mbb_emcee_amd import MapFit
    mf, raw = _handmade()
    assert mf.params.shape == (2, 5) and mf.covariance.shape == (2, 5, 5) and mf.nsources == 2 and mf.nstart == 3
    sg = mf.sigma
    assert np.array_equal(sg[0][[0, 1, 4]], [2.0, 0.5, 3.0]) and np.all(np.isnan(sg[0][[2, 3]])) and np.all(np.isnan(sg[1]))
    assert np.array_equal(mf.pulls, np.full((2, 4), 2.0))
    assert mf.status_names() == [["CONVERGED_F", "AT_LOWLIM(alpha)"], ["START_INVALID"]]
    assert list(mf.failed) == [False, True]
    assert MapFit.names_of(2 | 4 | 16 | 32 | (1 << 8) | (1 << 12)) == ["CONVERGED_X", "MAXITER", "COV_SINGULAR", "ALL_FIXED",
                                                                       "AT_LOWLIM(T)", "AT_LOWLIM(fnorm)"]
    one, _ = _handmade(nsrc=1, multi=False)
    assert one.params.shape == (5,) and one.sigma.shape == (5,) and one.pulls.shape == (4,) and one.lnprob.shape == ()
    text = str(one)
    assert "T/(1+z): 12.00 +-2.00 [K]" in text and "lambda0 (1+z): 150.00 (fixed)" in text and "alpha: 3.00" in text
    assert "ChiSquare of best fit point: 3.00" in text and "AT_LOWLIM(alpha)" in text
    assert set(one.arrays()) >= {"map_params", "map_sigma", "map_pulls", "map_status"}


# ---------------------------------------------------------------- map_initial_values
def _fitter(nwalkers=400, seed=2):
    from mbb_emcee_amd import mbb_fitter
    fit = mbb_fitter(nwalkers=nwalkers, sampler="native", seed=seed)
    fit.set_data([100.0, 250.0, 350.0, 500.0], [10.0, 30.0, 25.0, 12.0], [1.0, 2.0, 2.0, 1.5])
    return fit


@pytest.mark.filterwarnings("ignore:the MAP fit of source")
def test_map_initial_values():
    fit = _fitter()
    mf, raw = _handmade()
    raw.params[0] = [12.0, 1.8, 150.0, 3.0, 40.0]
    raw.params[1] = [30.0, 1.2, 300.0, 2.0, 4000.0]
    initsigma = np.array([3.0, 0.1, 20.0, 0.5, 5.0])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        p0 = fit.map_initial_values(mf, initsigma, scale=1.0)
    assert p0.shape == (2, 400, 5)
    assert len(w) == 1 and "source 1" in str(w[0].message) and "START_INVALID" in str(w[0].message)
    # centres per source
    for s in range(2):
        assert np.all(np.abs(p0[s].mean(axis=0) - raw.params[s]) < 5 * np.maximum(p0[s].std(axis=0), 1e-12) / 20 + 1e-12)
    sd0, sd1 = p0[0].std(axis=0), p0[1].std(axis=0)
    # source 0: Laplace sigma (2, 0.5, NaN, NaN, 3) capped by initsigma -> (2, 0.1, 20, 0.5, 3)
    assert np.all(np.abs(sd0 / np.array([2.0, 0.1, 20.0, 0.5, 3.0]) - 1) < 0.15), sd0
    # source 1 failed: the plain ball
    assert np.all(np.abs(sd1 / initsigma - 1) < 0.15), sd1
    half = fit.map_initial_values(mf, initsigma, scale=0.5)
    assert abs(half[0][:, 0].std() - 1.0) < 0.15 and abs(half[0][:, 4].std() - 1.5) < 0.25
    # limits respected: an optimum on beta's lower limit, a wide ball
    fit.like.set_lowlim("beta", 1.8)
    p1 = fit.map_initial_values(mf, np.array([3.0, 1.0, 20.0, 0.5, 5.0]))
    assert np.all(p1[..., 1] >= 1.8) and np.all(p1[..., 1] <= 20.0) and np.all(p1[..., 0] >= 1.0)
    # fixed parameters get no scatter
    fit.fix_param("T")
    p2 = fit.map_initial_values(mf, initsigma)
    assert np.all(p2[0][:, 0] == 12.0) and np.all(p2[1][:, 0] == 30.0) and p2[0][:, 1].std() > 0
    one, _ = _handmade(nsrc=1, multi=False)
    assert fit.map_initial_values(one, initsigma).shape == (400, 5)
    with pytest.raises(ValueError, match="expected length"):
        fit.map_initial_values(one, [1.0, 2.0])


def test_default_ball_and_generator_are_untouched():
    """generate_initial_values consumes the same generator in the same order as before: two fitters with one seed, one
    of which made MAP balls in between from another generator's numbers, agree."""
    a, b = _fitter(50, seed=9), _fitter(50, seed=9)
    iv, sg = [12.0, 1.8, 150.0, 3.0, 40.0], [3.0, 0.1, 20.0, 0.5, 5.0]
    first = a.generate_initial_values(iv, sg)
    assert np.array_equal(first, b.generate_initial_values(iv, sg))
    ref = np.random.RandomState(9)
    assert np.array_equal(first, np.array(iv) + np.array(sg) * ref.randn(50, 5))


# ---------------------------------------------------------------- argument rules on a faked device
def test_find_map_argument_rules(monkeypatch):
    from mbb_emcee_amd import optimize
    calls = []

    def fake(like, start, nstart=None, fixed=None, **kw):
        calls.append((np.array(start), nstart, list(fixed), kw))
        return "mapfit"
    monkeypatch.setattr(optimize, "map_fit", fake)
    fit = _fitter(20, seed=4)
    fit.fix_param("alpha")
    iv, sg = [12.0, 1.8, 150.0, 3.0, 40.0], [3.0, 0.1, 20.0, 0.5, 5.0]
    assert fit.find_map(iv, sg, nstart=6, maxiter=50) == "mapfit"
    start, nstart, fixed, kw = calls[-1]
    ball = _fitter(20, seed=4)
    ball.fix_param("alpha")
    assert start.shape == (1, 6, 5) and np.array_equal(start[0], ball.generate_initial_values(iv, sg)[:6])
    assert nstart == 6 and fixed == [False, False, False, True, False] and kw == {"maxiter": 50, "squeeze": True}
    assert np.all(start[0][:, 3] == 3.0)
    for bad in (0, 65, 21):
        with pytest.raises(ValueError):
            fit.find_map(iv, sg, nstart=bad)
    with pytest.raises(ValueError, match="initvals and initsigma"):
        fit.find_map()
    with pytest.raises(ValueError, match="best_fit"):
        fit.find_map(start="somewhere")
    with pytest.raises(ValueError, match="summary="):
        fit.find_map(start="best_fit")
    fit.find_map(start=np.ones((1, 2, 5)), xtol=1e-6)
    assert calls[-1][0].shape == (1, 2, 5) and calls[-1][3] == {"xtol": 1e-6}
    # a catalogue: the same ball for every source
    fit.like.set_phot_multi([100.0, 250.0, 350.0, 500.0], np.ones((3, 4)), np.ones((3, 4)))
    fit.find_map(iv, sg, nstart=4)
    assert calls[-1][0].shape == (3, 4, 5) and np.array_equal(calls[-1][0][0], calls[-1][0][2])
    assert calls[-1][3] == {"squeeze": False}


def test_request_refusals():
    from mbb_emcee_amd import likelihood, optimize
    like = likelihood()
    with pytest.raises(Exception, match="Data not read"):
        optimize._Request(like, np.ones(5))
    like.set_phot([100.0, 250.0, 500.0], [1.0, 2.0, 1.0], [0.1, 0.2, 0.1])
    ok = np.array([12.0, 1.8, 150.0, 3.0, 40.0])
    for bad in (np.ones(4), np.ones((2, 3, 4, 5)), np.ones((2, 6))):
        with pytest.raises(ValueError, match="start must be"):
            optimize._Request(like, bad)
    for bad in (np.array([12.0, np.nan, 150.0, 3.0, 40.0]), np.array([np.inf, 1.8, 150.0, 3.0, 40.0])):
        with pytest.raises(ValueError, match="finite"):
            optimize._Request(like, bad)
    for kw in ({"nstart": 0}, {"nstart": 65}, {"maxiter": 0}, {"maxiter": 1001}, {"ftol": -1.0}, {"xtol": np.nan},
               {"ftol": np.inf}, {"fixed": [0, 1]}):
        with pytest.raises(ValueError):
            optimize._Request(like, ok, **kw)
    with pytest.raises(ValueError, match="starts given"):
        optimize._Request(like, np.tile(ok, (1, 3, 1)), nstart=2)
    # shapes: one start for all, per source, several per source; missing starts are drawn inside the limits by the
    # caller's generator, the fixed ones and those the model does not use left alone
    r = optimize._Request(like, ok)
    assert r.start.shape == (1, 1, 5) and not r.multi
    r = optimize._Request(like, np.tile(ok, (4, 1)))
    assert r.start.shape == (4, 1, 5) and r.multi and r.nsrc == 4
    like2 = likelihood(opthin=True)
    like2.set_phot([100.0, 250.0, 500.0], [1.0, 2.0, 1.0], [0.1, 0.2, 0.1])
    like2.set_lowlim("beta", 1.7)
    r1 = optimize._Request(like2, ok, nstart=64, fixed=[0, 0, 0, 0, 1], rng=np.random.default_rng(3))
    r2 = optimize._Request(like2, ok, nstart=64, fixed=[0, 0, 0, 0, 1], rng=np.random.default_rng(3))
    assert r1.start.shape == (1, 64, 5) and np.array_equal(r1.start, r2.start) and np.array_equal(r1.start[0, 0], ok)
    assert np.all(r1.start[..., 1] >= 1.7) and np.all(r1.start[..., 2] == 150.0) and np.all(r1.start[..., 4] == 40.0)
    assert r1.start[0, 1:, 0].std() > 0.5 and np.all(np.abs(r1.start[..., 0] / 12.0 - 1) <= 0.25)
    like.set_phot_multi([100.0, 250.0, 500.0], np.ones((3, 3)), np.ones((3, 3)))
    with pytest.raises(ValueError, match="sources"):
        optimize._Request(like, np.tile(ok, (2, 1)))
    sp = optimize._Request(like, ok, nstart=2, fixed=[1, 0, 0, 0, 0], maxiter=7, ftol=1e-5, xtol=1e-4).spec()
    assert (sp.nsrc, sp.nstart, sp.maxiter, list(sp.fixed), sp.ftol, sp.xtol) == (3, 2, 7, [1, 0, 0, 0, 0], 1e-5, 1e-4)


# ---------------------------------------------------------------- declarations
def test_defaults_agree_with_the_header(H):
    from mbb_emcee_amd import optimize
    assert (optimize.MAXITER, optimize.FTOL, optimize.XTOL) == (H.maxiter, H.ftol, H.xtol)
    assert H.ncand == 4 and 4 <= 256 // 64 <= 11


def test_declarations(tmp_path):
    from mbb_emcee_amd import _native, build
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    assert "int mbb_map_fit(mbb_ctx *ctx, const mbb_map_spec *spec, const mbb_map_out *out);" in hdr
    assert "mbb_map_fit" in _native.SIGNATURES
    for dep in ("mbb_lm.hip.h", "mbb_map.hip.h"):
        assert any(d.endswith(dep) for d in build.DEPS), dep
    for name, val in (("MBB_MAP_MAX_STARTS", _native.MAP_MAX_STARTS), ("MBB_MAP_MAX_ITER", _native.MAP_MAX_ITER)):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == val
    for name, val in (("CONVERGED_F", 1), ("CONVERGED_X", 2), ("MAXITER", 4), ("START_INVALID", 8), ("COV_SINGULAR", 16),
                      ("ALL_FIXED", 32), ("STENCIL_FAILED", 64), ("AT_LOWLIM_SHIFT", 8)):
        assert int(re.search(r"MBB_MAP_%s = (\d+)" % name, hdr).group(1)) == val == getattr(_native, "MAP_" + name)
    # the struct sizes and the offsets of their last members, as the host compiler lays the header's out
    cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no host C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mbb_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu\\n", sizeof(mbb_map_spec), offsetof(mbb_map_spec, start), sizeof(mbb_map_out), '
                   'offsetof(mbb_map_out, status_all));\nreturn 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call([cc, "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(_native.MapSpec), _native.MapSpec.start.offset, C.sizeof(_native.MapOut),
                   _native.MapOut.status_all.offset]
    # only the one new symbol is exported
    if os.path.exists(_native.LIB_PATH) and shutil.which("nm"):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH]).decode()
        assert [ln.split()[-1] for ln in syms.splitlines() if "map" in ln.split()[-1].lower() and " T " in ln] == ["mbb_map_fit"]


def test_cli_switch_is_parsed():
    from mbb_emcee_amd import run_mbb_emcee
    p = run_mbb_emcee.build_parser()
    assert p.parse_args(["phot", "out"]).map_init == 0
    assert p.parse_args(["phot", "out", "--map-init"]).map_init == 8
    assert p.parse_args(["phot", "out", "--map-init", "12"]).map_init == 12


def test_cli_map_init_on_a_faked_device(tmp_path, monkeypatch, capsys):
    """main() with --map-init: find_map is called with the initial values, the ball's widths and nstart; its result goes
    to map_initial_values, whose walkers are the run's; the map_* arrays are written.  Without the switch neither is
    called and the walkers are generate_initial_values'."""
    from mbb_emcee_amd import run_mbb_emcee
    log = []

    class FakeMap(object):
        def __str__(self):
            return "FAKE MAP RESULT"

        def arrays(self, prefix="map_"):
            return {prefix + "params": np.arange(5.0), prefix + "sigma": np.ones(5)}

    class FakeSampler(object):
        chain, lnprobability, acceptance_fraction = np.zeros((6, 3, 5)), np.zeros((6, 3)), np.full(6, 0.5)

    class FakeLike(object):
        data_wave = data_flux = data_flux_unc = np.ones(3)

    class FakeFit(object):
        def __init__(self, **kw):
            self.sampler, self.like = FakeSampler(), FakeLike()

        def fix_param(self, name):
            log.append(("fix", name))

        def generate_initial_values(self, iv, sg):
            log.append(("ball", np.array(iv), np.array(sg)))
            return "BALL"

        def find_map(self, iv, sg, nstart=None):
            log.append(("find_map", np.array(iv), np.array(sg), nstart))
            return FakeMap()

        def map_initial_values(self, mf, sg):
            log.append(("map_initial_values", mf, np.array(sg)))
            return "MAP BALL"

        def run(self, nburn, nsteps, p0, **kw):
            log.append(("run", nburn, nsteps, p0))
    monkeypatch.setattr(run_mbb_emcee, "mbb_fitter", FakeFit)
    out = str(tmp_path / "o.npz")
    run_mbb_emcee.main(["phot.txt", out, "-n", "6", "-b", "2", "-N", "3", "--initT", "14", "--map-init", "5"])
    calls = [c[0] for c in log]
    assert calls == ["find_map", "map_initial_values", "run"]
    assert log[0][1][0] == 14.0 and np.array_equal(log[0][2], [2, 0.2, 100, 0.3, 5.0]) and log[0][3] == 5
    assert isinstance(log[1][1], FakeMap) and np.array_equal(log[1][2], log[0][2])
    assert log[2][1:] == (2, 3, "MAP BALL")
    assert "FAKE MAP RESULT" in capsys.readouterr().out
    res = np.load(out)
    assert np.array_equal(res["map_params"], np.arange(5.0)) and np.array_equal(res["map_sigma"], np.ones(5))
    del log[:]
    run_mbb_emcee.main(["phot.txt", out, "-n", "6", "-b", "2", "-N", "3", "--map-init"])
    assert log[0][0] == "find_map" and log[0][3] == 8
    del log[:]
    run_mbb_emcee.main(["phot.txt", out, "-n", "6", "-b", "2", "-N", "3"])
    assert [c[0] for c in log] == ["ball", "run"] and log[1][3] == "BALL" and "map_params" not in np.load(out)
