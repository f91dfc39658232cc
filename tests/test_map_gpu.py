"""GPU side of the MAP-fit tests: k_map_lm (csrc/mbb_map.hip.h) through ``optimize.map_fit`` and the fitter, against the
fixture tests/golden/map.npz (made by tests/make_golden_map.py with scipy; not needed here) and the oracle.

Gap criterion, the core: gap = lnP_oracle(theta_ref) - lnP_oracle(theta_device) <= 1e-10 max(1, |lnP|) -- SURVEY.md 8c's
tolerance between the device's likelihood and the oracle's; an optimiser working on a likelihood that is allowed to differ
by that much cannot be asked for more.  A negative gap passes.  Laplace covariance: |cov_dev - cov_ref|_ij /
sqrt(cov_ii cov_jj) <= 100 x the reference's own disagreement between its two difference steps (the fixture's cov_dis);
the factor covers the device's differencing on top of the reference's.  Shapes are the smallest at which the kernel can
still go wrong: six bands whose sample counts are no multiples of 64, four or eight starts, one to three sources."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, parity_record, rec_allclose
import _map_ref as MR

pytestmark = pytest.mark.gpu

NAMES = sorted(MR.case_specs())


@pytest.fixture(scope="module")
def g_map():
    return np.load(os.path.join(GOLDEN, "map.npz"))


def make_like(s, flux, unc):
    import mbb_emcee_amd as mbb
    plain = s["waves"] is not None
    like = mbb.likelihood(response=not plain, opthin=s["opthin"], noalpha=s["noalpha"], device=0)
    like.set_phot(s["waves"] if plain else s["bands"], flux, unc)
    cov = MR.covariance(s, np.asarray(unc, dtype=np.float64))
    if cov is not None:
        like.set_cov(cov)
    for i in range(5):
        like.set_lowlim(i, s["lowlim"][i])
    for i in range(6):
        if s["has_uplim"][i]:
            like.set_uplim(i, s["uplim"][i])
        if s["has_gprior"][i]:
            like.set_gaussian_prior(i, s["gmean"][i], s["gsigma"][i])
    return like


_CACHE = {}


def case(oracle, g_pb, g_map, name):
    """(settings, device likelihood, oracle likelihood, MapFit from the fixture's starts), made once per case"""
    if name not in _CACHE:
        from mbb_emcee_amd import optimize
        s, nstart = MR.case_specs()[name]
        flux, unc = g_map[name + "/flux"], g_map[name + "/unc"]
        like = make_like(s, flux, unc)
        orc = MR.oracle_like(oracle, g_pb, s, flux, unc)
        _CACHE[name] = (s, like, orc, optimize.map_fit(like, g_map[name + "/starts"][None], squeeze=True))
    return _CACHE[name]


def check_gap(orc, theta, lnp_ref, kind="MAP gap"):
    lnp = orc(theta)[0]
    gap = float(lnp_ref) - lnp
    bound = MR.gap_bound(lnp_ref)
    print("%s: gap %.3e, bound %.3e" % (kind, gap, bound))
    parity_record(kind + " / max(1,|lnP|)", max(gap, 0.0) / max(1.0, abs(float(lnp_ref))), 1e-10)
    assert np.isfinite(lnp) and gap <= bound, (gap, bound)
    return gap


# ---------------------------------------------------------------- the gap criterion on every fixture case
@pytest.mark.parametrize("name", NAMES)
def test_gap_criterion(oracle, g_pb, g_map, name):
    from mbb_emcee_amd import MapFit
    s, like, orc, mf = case(oracle, g_pb, g_map, name)
    check_gap(orc, mf.params, g_map[name + "/lnp_ref"])
    # every start reaches it (each case has one optimum), converged, well under maxiter
    for j in range(mf.nstart):
        check_gap(orc, mf.params_all[j], g_map[name + "/lnp_ref"], kind="MAP gap (every start)")
        assert mf.status_all[j] & (MapFit.CONVERGED_F | MapFit.CONVERGED_X) and not mf.status_all[j] & MapFit.MAXITER
    assert 0 < mf.niter < 60 and mf.nfev > mf.niter and 0 <= mf.start_index < mf.nstart
    # bits: lnprob is like(params); chisq, q and the band fluxes are mbb_goodness_rows'
    from mbb_emcee_amd import goodness
    assert np.array_equal(np.atleast_1d(mf.lnprob), like(mf.params[None]))
    assert np.array_equal(mf.lnprob_all, like(mf.params_all))
    chisq, q, st, fl = goodness.goodness_rows(like, mf.params[None], want_flux=True)
    assert np.array_equal(chisq[0], mf.chisq) and np.array_equal(q[0], mf.q) and np.array_equal(fl[0], mf.model_flux)
    assert mf.lnprob == mf.lnprob_all.max() and mf.start_index == int(np.argmax(mf.lnprob_all))


@pytest.mark.parametrize("name", NAMES)
def test_laplace_covariance(oracle, g_pb, g_map, name):
    s, like, orc, mf = case(oracle, g_pb, g_map, name)
    ref, dis = g_map[name + "/cov_ref"], float(g_map[name + "/cov_dis"])
    cov = mf.covariance
    assert np.array_equal(np.isnan(cov), np.isnan(ref))
    err = np.nanmax(MR.cov_error(cov, ref))
    print("%s: covariance error %.3e, bound %.3e (100 x the reference's %.3e)" % (name, err, 100 * dis, dis))
    parity_record("Laplace covariance / sqrt(cov_ii cov_jj)", err, 100 * dis)
    assert err <= 100 * dis
    assert np.array_equal(cov, cov.T, equal_nan=True)
    assert np.array_equal(mf.sigma, np.sqrt(np.diag(cov)), equal_nan=True)


def test_limit_wall_and_prior_cases(oracle, g_pb, g_map):
    from mbb_emcee_amd import MapFit
    s, like, orc, mf = case(oracle, g_pb, g_map, "beta_lowlim")
    assert mf.params[1] == 2.0 and "AT_LOWLIM(beta)" in mf.status_names()
    assert set(mf.status_names()) <= {"CONVERGED_F", "CONVERGED_X", "AT_LOWLIM(beta)"}
    assert mf.status >> MapFit.AT_LOWLIM_SHIFT == 0b00010
    cov = mf.covariance
    assert np.all(np.isnan(cov[1])) and np.all(np.isnan(cov[:, 1])) and np.all(np.isfinite(cov[np.ix_([0, 4], [0, 4])]))
    rec_allclose(mf.params[[0, 4]], [11.2394178, 41.2377778], rtol=1e-8, kind="MAP parameters on the beta limit")
    s, like, orc, mf = case(oracle, g_pb, g_map, "T_wall")
    assert mf.params[0] > 11.0 and abs(mf.params[0] - 11.1177) < 1e-4        # beyond the soft wall
    for name in ("peak_prior", "peak_wall"):
        s, like, orc, mf = case(oracle, g_pb, g_map, name)
        check_gap(orc, mf.params, g_map[name + "/lnp_ref"], kind="MAP gap (peak wavelength)")


def test_optimum_on_a_limit_along_the_correlated_valley(oracle, g_pb, g_map):
    """The T-beta degeneracy with beta's lower limit: starts up the valley (cold and steep) from which the full step
    overshoots the limit, is clipped onto it and predicts no gain.  The search must go on to the constrained optimum,
    not stop there."""
    from mbb_emcee_amd import optimize, MapFit
    s, like, orc, mf0 = case(oracle, g_pb, g_map, "beta_lowlim")
    opt = g_map["beta_lowlim/theta_ref"]
    starts = np.array([[9.0, 3.2, opt[2], opt[3], 45.0], [10.0, 2.6, opt[2], opt[3], 43.0], [10.8, 2.2, opt[2], opt[3], 42.0],
                       [11.0, 2.05, opt[2], opt[3], 41.0], [8.0, 4.0, opt[2], opt[3], 50.0], [11.2, 2.001, opt[2], opt[3], 41.2]])
    mf = optimize.map_fit(like, starts[None], squeeze=True)
    for j in range(len(starts)):
        check_gap(orc, mf.params_all[j], g_map["beta_lowlim/lnp_ref"], kind="MAP gap (valley onto a limit)")
        assert mf.params_all[j, 1] == 2.0 and mf.status_all[j] >> MapFit.AT_LOWLIM_SHIFT == 0b00010
        assert mf.status_all[j] & (MapFit.CONVERGED_F | MapFit.CONVERGED_X)


def test_sharded_context_is_refused():
    """Two ranks as processes on this GPU with a communicator over tests/rccl_standin/: mbb_map_fit answers
    MBB_ERR_STATE with its message, writes nothing, and fits again once the communicator is gone
    (tests/_map_rank_worker.py)."""
    import subprocess
    from _filecomm import launch
    d = os.path.join(ROOT, "tests", "rccl_standin")
    so, src = os.path.join(d, "librccl_standin.so"), os.path.join(d, "rccl_standin.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-shared", "-fPIC", "-o", so, src, "-lrt"])
    ok, text = launch(os.path.join(ROOT, "tests", "_map_rank_worker.py"), 2, extra_env={"MBB_RCCL_LIB": so}, timeout=300.0)
    assert ok and "MAP_RANKS_OK 0" in text and "MAP_RANKS_OK 1" in text, text[-6000:]


def test_sample_and_covariance_paths(oracle, g_pb, g_map):
    """Many-sample and one-sample bands whose counts are no multiples of 64 (staged); more than 2560 samples (read from
    global memory); a 12-band covariance in LDS; a 70-band covariance read from global memory (the context accepts
    one).  Each held to the gap criterion."""
    for name, nsamp, nb in (("path_mix", 1690, 8), ("path_big", 2796, 7), ("path_cov12", 2373, 12), ("path_cov70", 70, 70)):
        s, like, orc, mf = case(oracle, g_pb, g_map, name)
        freq, wt, offs = like.band_tables()
        assert freq.size == nsamp and offs.size == nb + 1 and (nb == 70 or np.any(np.diff(offs) % 64 != 0))
        check_gap(orc, mf.params, g_map[name + "/lnp_ref"], kind="MAP gap (%s)" % name)
    assert case(oracle, g_pb, g_map, "path_cov12")[1]._has_covmatrix and case(oracle, g_pb, g_map, "path_cov70")[1]._has_covmatrix


# ---------------------------------------------------------------- planted optima and the smallest cases
@pytest.mark.parametrize("variant", sorted(MR.VARIANTS))
def test_planted_optimum(oracle, g_pb, variant):
    from mbb_emcee_amd import optimize
    s = MR.settings(variant, 5)
    plain = MR.oracle_like(oracle, g_pb, s, np.ones(6), np.ones(6))
    m = plain(MR.TRUTH, return_flux=True)[1][0]
    unc = 0.05 * m + 0.5
    like, orc = make_like(s, m, unc), MR.oracle_like(oracle, g_pb, s, m, unc)
    mf = optimize.map_fit(like, MR.make_starts(s, 4)[None], squeeze=True)
    m2lnp = -2.0 * orc(mf.params)[0]
    print("%s: -2 lnP at the device's optimum %.3e" % (variant, m2lnp))
    parity_record("planted optimum -2 lnP", m2lnp, 1e-10)
    assert m2lnp <= 1e-10
    if s["opthin"]:
        idx = MR.free_index(s)
        cov, dis = MR.ref_cov(oracle, orc, s, MR.TRUTH)
        assert np.all(np.sqrt(np.diag(cov)[idx]) / MR.TRUTH[idx] <= 1.0)         # what the parameter bound follows from
        rec_allclose(mf.params[idx], MR.TRUTH[idx], rtol=1e-5, kind="planted optimum parameters")


def _delta_like(waves, flux, unc, opthin=True, noalpha=True):
    import mbb_emcee_amd as mbb
    like = mbb.likelihood(opthin=opthin, noalpha=noalpha, device=0)
    like.set_phot(waves, flux, unc)
    return like


def test_two_delta_bands_are_exactly_determined(oracle):
    from mbb_emcee_amd import optimize, MapFit
    waves, truth = np.array([250.0, 500.0]), np.array([14.0, 1.5, 150.0, 3.0, 25.0])
    orc0 = oracle.OracleLikelihood(np.ones(2), np.ones(2), wave=waves, opthin=True, noalpha=True)
    m = orc0(truth, return_flux=True)[1][0]
    like = _delta_like(waves, m, 0.1 * m)
    mf = optimize.map_fit(like, truth * np.array([1.2, 1.0, 1.0, 1.0, 0.8]), fixed=[0, 1, 0, 0, 0])
    print("two delta bands: chisq %.3e after %d iterations, T %.12g fnorm %.12g" % (mf.chisq, mf.niter, mf.params[0], mf.params[4]))
    assert mf.chisq <= 1e-18 and mf.niter <= 20 and mf.status & (MapFit.CONVERGED_F | MapFit.CONVERGED_X)
    rec_allclose(mf.params, truth, rtol=1e-9, kind="two delta bands")
    assert mf.params[1] == 1.5 and mf.params[2] == 150.0 and mf.params[3] == 3.0
    assert np.all(np.isfinite(mf.covariance[np.ix_([0, 4], [0, 4])])) and np.all(np.isnan(mf.covariance[1]))


def test_one_delta_band_three_free_parameters(oracle):
    from mbb_emcee_amd import optimize, MapFit
    like = _delta_like([350.0], [30.0], [2.0])
    mf = optimize.map_fit(like, [12.0, 1.8, 150.0, 3.0, 20.0])
    assert mf.status & MapFit.COV_SINGULAR and np.all(np.isnan(mf.covariance))
    assert mf.status & (MapFit.CONVERGED_F | MapFit.CONVERGED_X | MapFit.MAXITER) and np.isfinite(mf.lnprob)
    assert mf.chisq <= 1e-12 and mf.niter < 100


@pytest.mark.parametrize("nfree", [0, 1, 2, 3, 4, 5])
def test_free_parameter_counts(oracle, g_pb, g_map, nfree):
    from mbb_emcee_amd import optimize, MapFit
    name = "thick_walpha_s5"
    s, like, orc, full = case(oracle, g_pb, g_map, name)
    order = [4, 0, 1, 3, 2]                                     # fnorm, T, beta, alpha, lambda0 become free in turn
    fixed = [1] * 5
    for i in order[:nfree]:
        fixed[i] = 0
    start = g_map[name + "/starts"][0]
    mf = optimize.map_fit(like, start, fixed=fixed)
    held = [i for i in range(5) if fixed[i]]
    assert np.array_equal(mf.params[held], start[held])
    assert np.all(np.isnan(mf.covariance[held])) if held else True
    if nfree == 0:
        assert mf.status == MapFit.ALL_FIXED and mf.niter == 0 and np.array_equal(mf.params, start)
        assert np.array_equal(np.atleast_1d(mf.lnprob), like(start[None]))
        return
    assert mf.status & (MapFit.CONVERGED_F | MapFit.CONVERGED_X) and not mf.status & MapFit.ALL_FIXED
    assert mf.lnprob >= like(start[None])[0]
    # the optimum over the free ones: no better point on a small cross around it, by the oracle
    free = [i for i in range(5) if not fixed[i]]
    best = orc(mf.params)[0]
    for i in free:
        for sign in (-1.0, 1.0):
            p = mf.params.copy()
            p[i] *= 1.0 + sign * 1e-4
            assert orc(p)[0] <= best + MR.gap_bound(best)
    if nfree == 5:
        check_gap(orc, mf.params, g_map[name + "/lnp_ref"], kind="MAP gap (five free)")


# ---------------------------------------------------------------- bad inputs and stopping
def test_bad_starts_and_stopping(oracle, g_pb, g_map):
    from mbb_emcee_amd import optimize, MapFit
    name = "thin_walpha_s5"
    s, like, orc, good = case(oracle, g_pb, g_map, name)
    starts = g_map[name + "/starts"][:4].copy()
    starts[1, 0] = 0.5                                           # below T's lower limit
    starts[2, 3] = -1.0                                          # the constructor fails: alpha <= 0 (below its limit too)
    mf = optimize.map_fit(like, starts[None], squeeze=True)
    for j in (1, 2):
        assert mf.status_all[j] == MapFit.START_INVALID and np.array_equal(mf.params_all[j], starts[j])
        assert np.isneginf(mf.lnprob_all[j]) or np.isnan(mf.lnprob_all[j])
    for j in (0, 3):                                             # the other starts of that source are unaffected: bit for bit
        assert np.array_equal(mf.params_all[j], good.params_all[j]) and mf.lnprob_all[j] == good.lnprob_all[j]
        assert mf.status_all[j] == good.status_all[j]
    assert mf.start_index in (0, 3) and not mf.failed
    bad = optimize.map_fit(like, starts[1])
    assert bad.failed and bad.status == MapFit.START_INVALID and bad.niter == 0 and np.array_equal(bad.params, starts[1])
    assert np.all(np.isnan(bad.covariance))
    # a constructor failure that is inside the limits: alpha's lower limit moved below zero
    like2 = make_like(s, g_map[name + "/flux"], g_map[name + "/unc"])
    like2.set_lowlim("alpha", -5.0)
    st2 = starts[0].copy()
    st2[3] = -1.0
    assert optimize.map_fit(like2, st2).status == MapFit.START_INVALID
    one = optimize.map_fit(like, starts[0], maxiter=1)
    assert one.status & MapFit.MAXITER and one.niter == 1 and one.lnprob >= like(starts[0][None])[0]
    # wild starts drive trial steps into failing rows: the search ends, with a finite lnprob no worse than the start's
    wild = np.array([[80.0, 0.11, 150.0, 19.0, 1e-2], [1.01, 19.0, 150.0, 0.11, 5000.0], [300.0, 5.0, 150.0, 0.2, 1e4],
                     [2.0, 0.1, 150.0, 15.0, 1e-3]])
    w = optimize.map_fit(like, wild[None], squeeze=True)
    lp0 = like(wild)
    assert np.all(np.isfinite(w.lnprob_all)) and np.all(w.lnprob_all >= lp0) and np.all(w.niter <= 200)
    assert np.all(w.status_all & (MapFit.CONVERGED_F | MapFit.CONVERGED_X | MapFit.MAXITER | MapFit.STENCIL_FAILED))


# ---------------------------------------------------------------- bits
def test_sources_and_starts_do_not_see_each_other(oracle, g_pb, g_map):
    import mbb_emcee_amd as mbb
    from mbb_emcee_amd import optimize
    name = "thin_walpha_s5"
    s, like1, orc, _ = case(oracle, g_pb, g_map, name)
    flux, unc = g_map[name + "/flux"], g_map[name + "/unc"]
    scales = np.array([1.0, 30.0, 1000.0])
    multi = make_like(s, flux, unc)
    multi.set_phot_multi(MR.BANDS, flux[None] * scales[:, None], unc[None] * scales[:, None])
    for nstart in (1, 5):
        starts = np.repeat(g_map[name + "/starts"][None, :nstart], 3, axis=0).copy()
        starts[..., 4] *= scales[:, None]
        all3 = optimize.map_fit(multi, starts)
        again = optimize.map_fit(multi, starts)
        for key in ("params", "lnprob", "chisq", "q", "model_flux", "covariance", "niter", "nfev", "start_index", "status",
                    "params_all", "lnprob_all", "status_all"):
            assert np.array_equal(getattr(all3, key), getattr(again, key), equal_nan=True), key       # two runs: the same bits
        for k in range(3):
            single = make_like(s, flux * scales[k], unc * scales[k])
            own = optimize.map_fit(single, starts[k][None], squeeze=True)
            for key in ("params", "lnprob", "chisq", "q", "model_flux", "covariance", "niter", "nfev", "start_index", "status",
                        "params_all", "lnprob_all", "status_all"):
                assert np.array_equal(getattr(all3, key)[k], getattr(own, key), equal_nan=True), (nstart, k, key)
        rec_allclose(all3.params[:, 4] / scales, np.full(3, all3.params[0, 4]), rtol=1e-8, kind="MAP fnorm across flux scales")
    # a smaller call after a larger one, and a larger after a smaller (the context's buffers)
    small = optimize.map_fit(multi, starts[:, :2])
    assert np.array_equal(small.params_all, all3.params_all[:, :2])
    big = optimize.map_fit(multi, np.tile(starts, (1, 4, 1)))
    assert big.nstart == 20 and np.array_equal(big.params_all[:, :5], all3.params_all)


def test_ties_and_planted_best_start(oracle, g_pb, g_map):
    from mbb_emcee_amd import optimize, MapFit
    name = "thin_walpha_s5"
    s, like, orc, good = case(oracle, g_pb, g_map, name)
    st = g_map[name + "/starts"]
    tie = optimize.map_fit(like, np.array([st[2], st[2], st[2]])[None], squeeze=True)
    assert tie.start_index == 0 and tie.lnprob_all[0] == tie.lnprob_all[1] == tie.lnprob_all[2]
    # every parameter fixed: each start's result is the start, and the one planted at the optimum is picked
    planted = np.array([st[0], st[1], good.params, st[3]])
    mf = optimize.map_fit(like, planted[None], fixed=[1] * 5, squeeze=True)
    assert mf.start_index == 2 and np.array_equal(mf.params, good.params) and mf.status == MapFit.ALL_FIXED
    assert np.array_equal(mf.lnprob_all, like(planted))
    # a NaN never wins: an invalid start first
    inv = planted.copy()
    inv[0, 0] = 0.5
    mf = optimize.map_fit(like, inv[None], fixed=[1] * 5, squeeze=True)
    assert mf.start_index == 2 and mf.status_all[0] == MapFit.START_INVALID


# ---------------------------------------------------------------- through the public ways
def test_find_map_initial_values_and_run():
    import mbb_emcee_amd as mbb
    rng = np.random.default_rng(4)
    bands = ["PACS_100um", "PACS_160um", "SPIRE_250um", "SPIRE_350um", "SPIRE_500um", "SCUBA2_850um"]
    fit = mbb.mbb_fitter(nwalkers=40, response=True, opthin=True, noalpha=False, seed=3)
    fit.like.set_phot(bands, np.ones(6), np.ones(6))
    truth = np.array([[12.0, 1.8, 150.0, 3.0, 40.0], [18.0, 1.4, 150.0, 2.5, 900.0], [9.0, 2.1, 150.0, 3.5, 7.0]])
    m = fit.like.model_flux(truth)
    unc = 0.05 * m + 0.5 * m.max(axis=1, keepdims=True) / 100.0
    fit.like.set_phot_multi(bands, m + unc * rng.standard_normal(m.shape), unc)
    fit.fix_param("lambda0")
    initsigma = np.array([2.0, 0.2, 0.0, 0.3, 5.0])
    mf = fit.find_map(start=truth[:, None, :] * (1.0 + 0.1 * rng.uniform(-1, 1, (3, 4, 5))))
    assert mf.params.shape == (3, 5) and not np.any(mf.failed)
    assert np.all(mf.params[:, 2] == mf.params_all[np.arange(3), mf.start_index, 2])        # lambda0 is held: each start's own
    assert np.all(np.abs(mf.params[:, [0, 1, 4]] / truth[:, [0, 1, 4]] - 1) < 0.5)
    p0 = fit.map_initial_values(mf, initsigma, scale=1.0)
    assert p0.shape == (3, 40, 5)
    lo = np.array([fit.lowlim(i) for i in range(5)])
    hi = np.array([fit.uplim(i) if fit.has_uplim(i) else np.inf for i in range(5)])
    assert np.all(p0 >= lo) and np.all(p0 <= hi) and np.all(np.isfinite(fit.like(p0)))
    assert np.all(p0[:, :, 2] == mf.params[:, None, 2])
    # no wider than the Laplace sigma, and initsigma where there is none (a source whose data do not constrain alpha has
    # a singular curvature: COV_SINGULAR, every sigma NaN)
    width = np.where(np.isfinite(mf.sigma[:, 4]), np.minimum(mf.sigma[:, 4], initsigma[4]), initsigma[4])
    assert np.all(p0[..., 4].std(axis=1) <= 1.5 * width)
    assert np.array_equal(np.isnan(mf.sigma[:, 4]), (mf.status & mf.COV_SINGULAR) != 0)
    fit.run(10, 30, p0, summary=True, convergence=True, goodness=True)
    assert type(fit.summary).__name__ == "ChainSummary" and type(fit.convergence).__name__ == "ChainDiagnostics"
    assert type(fit.goodness).__name__ == "ChainGoodness" and fit.summary.best_fit[0].shape == (3, 5)
    # polishing the chain's best entry never loses
    pol = fit.find_map(start="best_fit")
    assert pol.params.shape == (3, 5) and np.all(pol.lnprob >= fit.summary.best_fit[1])
    assert np.all(pol.lnprob <= mf.lnprob + 1e-9 * np.maximum(1.0, np.abs(mf.lnprob)))


def test_c_abi_refusals(oracle, g_pb, g_map):
    import ctypes as C
    from mbb_emcee_amd import _native, optimize, likelihood
    s, like, orc, _ = case(oracle, g_pb, g_map, "thin_walpha_s5")
    ctx = _native.analysis_context(like)
    st = g_map["thin_walpha_s5/starts"]

    def call(edit=None, null=None, nsrc=1, nstart=2, ctx=ctx):
        req = optimize._Request(like, st[:nstart][None])
        raw = optimize._Raw(nsrc, nstart, 6)
        sp, out = req.spec(), raw.out()
        sp.nsrc = nsrc
        if edit:
            edit(sp, req)
        if null:
            setattr(out if hasattr(out, null) else sp, null, None)
        rc = ctx.lib.mbb_map_fit(ctx.h, C.byref(sp), C.byref(out))
        return rc, ctx.lib.mbb_last_error().decode()
    assert call()[0] == 0
    assert ctx.lib.mbb_map_fit(ctx.h, None, None) == -2
    for null in ("params", "lnprob", "chisq", "q", "cov", "niter", "nfev", "start_index", "status", "start"):
        rc, msg = call(null=null)
        assert rc == -2 and "null map argument" in msg, null
    for null in ("model_flux", "lnprob_all", "params_all", "status_all"):            # optional
        assert call(null=null)[0] == 0, null
    for edit, text in ((lambda sp, r: setattr(sp, "nstart", 0), "starts per source"),
                       (lambda sp, r: setattr(sp, "nstart", 65), "starts per source"),
                       (lambda sp, r: setattr(sp, "maxiter", 0), "iterations"),
                       (lambda sp, r: setattr(sp, "maxiter", 1001), "iterations"),
                       (lambda sp, r: setattr(sp, "nsrc", 0), "a source at least"),
                       (lambda sp, r: setattr(sp, "ftol", float("nan")), "ftol and xtol"),
                       (lambda sp, r: setattr(sp, "xtol", float("inf")), "ftol and xtol"),
                       (lambda sp, r: setattr(sp, "xtol", -1.0), "ftol and xtol"),
                       (lambda sp, r: r.start.__setitem__((0, 1, 3), np.nan), "start of source 0, start 1 is not finite")):
        rc, msg = call(edit=edit)
        assert rc == -2 and text in msg, (text, msg)
    # the sources: a one-source context serves any number, a context of three refuses two
    assert call(nsrc=1)[0] == 0
    multi = make_like(s, g_map["thin_walpha_s5/flux"], g_map["thin_walpha_s5/unc"])
    multi.set_phot_multi(MR.BANDS, np.tile(g_map["thin_walpha_s5/flux"], (3, 1)), np.tile(g_map["thin_walpha_s5/unc"], (3, 1)))
    mctx = _native.analysis_context(multi)
    req = optimize._Request(like, st[:2][None])
    raw = optimize._Raw(2, 2, 6)
    sp, out = req.spec(), raw.out()
    sp.nsrc = 2
    sp.start = _native._d(np.ascontiguousarray(np.tile(st[:2], (2, 1, 1))))
    assert mctx.lib.mbb_map_fit(mctx.h, C.byref(sp), C.byref(out)) == -2 and "sources" in mctx.lib.mbb_last_error().decode()
    # bands or data not set: MBB_ERR_STATE
    empty = _native.Context(0)
    sp.nsrc = 1
    assert empty.lib.mbb_map_fit(empty.h, C.byref(sp), C.byref(out)) == -3 and "bands not set" in empty.lib.mbb_last_error().decode()
    nodata = likelihood(opthin=True, device=0)
    with pytest.raises(Exception, match="Data not read"):
        optimize.map_fit(nodata, st[0])


def test_cli_map_init(tmp_path, capsys):
    from mbb_emcee_amd import run_mbb_emcee, likelihood
    waves = np.array([100.0, 160.0, 250.0, 350.0, 500.0, 850.0])
    like = likelihood(opthin=True, noalpha=True, device=0)
    like.set_phot(waves, np.ones(6), np.ones(6))
    m = like.model_flux(np.array([[12.0, 1.8, 150.0, 3.0, 40.0]]))[0]
    phot = tmp_path / "phot.txt"
    phot.write_text("".join("%g %.8g %.8g\n" % (w, f, 0.05 * f + 0.5) for w, f in zip(waves, m)))
    out = str(tmp_path / "fit.npz")
    run_mbb_emcee.main([str(phot), out, "-n", "20", "-b", "5", "-N", "10", "--opthin", "--noalpha", "--seed", "3",
                        "--initT", "14", "--initBeta", "1.5", "--initFnorm", "35", "--map-init", "4"])
    text = capsys.readouterr().out
    assert "T/(1+z): 12.00 +-" in text and "Optically thin case assumed" in text and "start" in text and "CONVERGED" in text
    res = np.load(out)
    rec_allclose(res["map_params"][[0, 1, 4]], [12.0, 1.8, 40.0], rtol=1e-5, kind="CLI planted optimum")
    assert res["chain"].shape == (20, 10, 5) and np.all(np.isfinite(res["lnprobability"]))
    # the walkers started around the optimum, no wider than the Laplace errors
    assert np.all(np.abs(res["chain"][:, 0, 0] - 12.0) < 8 * res["map_sigma"][0] + 1e-9)
