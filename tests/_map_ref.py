"""Reference of the MAP fit (csrc/mbb_lm.hip.h, csrc/mbb_map.hip.h) for its tests.

-2 ln P of this library is a sum of squares: ``residuals`` restates it as a vector r with r^T r = -2 ln P -- the data
residuals from the oracle's band fluxes, one residual d / lw per soft wall that is exceeded, one per Gaussian prior, the
peak wavelength's through ``OracleSED.max_wave`` -- and tests/test_map_cpu.py holds r^T r to the oracle's own lnP.
``ref_search`` minimises it with scipy.optimize.least_squares (all tolerances 1e-15, x_scale = |x0|), ``ref_cov`` is
(J^T J)^-1 from a central-difference Jacobian.  ``lm_drive`` is the kernel's loop in Python around the HOST build of the
step functions (tests/_map_host.cpp): the algorithm without a device.  The cases of tests/golden/map.npz are made here
(``cases``) and written by tests/make_golden_map.py; the GPU tests read that file and the oracle, never scipy."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT, golden_bands

BANDS = ["PACS_100um", "PACS_160um", "SPIRE_250um", "SPIRE_350um", "SPIRE_500um", "SCUBA2_850um"]
TRUTH = np.array([12.0, 1.8, 150.0, 3.0, 40.0])
VARIANTS = {"thin_noalpha": (True, True), "thin_walpha": (True, False),
            "thick_noalpha": (False, True), "thick_walpha": (False, False)}
LOWLIM = np.array([1, 0.1, 1, 0.1, 1e-3])
H1, H2 = 2.0 ** -17, 2.0 ** -16        # the reference Jacobian's two relative steps: about eps^(1/3), and twice that


# the further cases of the kernel's two sample paths and two covariance paths (thin with alpha, seed 5, four starts)
MIX_BANDS = BANDS + ["D_delta_70um", "E_delta_1100um"]                  # many-sample and one-sample bands
BIG_BANDS = BANDS + ["SCUBA2_450um"]                                    # 2796 samples: beyond what is staged in LDS
COV12_BANDS = BANDS[:5] + ["SCUBA_850um", "PACS_70um", "MIPS_160um", "SABOCA_350um", "LABOCA_870um", "Bolocam_1.1mm",
                           "MAMBO2_1.2mm"]
COV70_WAVES = np.geomspace(60.0, 1500.0, 70)                            # plain wavelengths: more bands than C^-1 has LDS for


def settings(variant, seed, lowlim=None, uplim=None, gprior=None, bands=None, waves=None, rho=None):
    """One case's settings: default limits plus an upper limit of 2550 on lambda0; the thick variants with a prior
    lambda0 ~ N(150, 40).  uplim / gprior: {index: value} / {index: (mean, sigma)} on top, index 5 the peak wavelength."""
    opthin, noalpha = VARIANTS[variant]
    s = {"variant": variant, "opthin": opthin, "noalpha": noalpha, "seed": int(seed),
         "lowlim": LOWLIM.copy(), "has_uplim": np.array([0, 1, 1, 1, 0, 0]),
         "uplim": np.array([np.inf, 20.0, 2550.0, 20.0, np.inf, np.inf]),
         "has_gprior": np.zeros(6, dtype=int), "gmean": np.zeros(6), "gsigma": np.ones(6),
         "bands": list(BANDS) if bands is None and waves is None else bands, "waves": waves, "rho": rho}
    if not opthin:
        s["has_gprior"][2], s["gmean"][2], s["gsigma"][2] = 1, 150.0, 40.0
    for i, v in (lowlim or {}).items():
        s["lowlim"][i] = v
    for i, v in (uplim or {}).items():
        s["has_uplim"][i], s["uplim"][i] = 1, v
    for i, (m, sg) in (gprior or {}).items():
        s["has_gprior"][i], s["gmean"][i], s["gsigma"][i] = 1, m, sg
    return s


def case_specs():
    """name -> (settings, number of starts): the four variants at noise seeds 5, 6, 7 with eight starts, and four extra
    cases on seed 5 with four."""
    out = {}
    for v in VARIANTS:
        for seed in (5, 6, 7):
            out["%s_s%d" % (v, seed)] = (settings(v, seed), 8)
    out["beta_lowlim"] = (settings("thin_noalpha", 5, lowlim={1: 2.0}), 4)
    out["T_wall"] = (settings("thin_noalpha", 5, uplim={0: 11.0}), 4)
    out["peak_prior"] = (settings("thin_walpha", 5, gprior={5: (260.0, 5.0)}), 4)
    out["peak_wall"] = (settings("thick_noalpha", 5, uplim={5: 230.0}), 4)
    out["path_mix"] = (settings("thin_walpha", 5, bands=MIX_BANDS), 4)
    out["path_big"] = (settings("thin_walpha", 5, bands=BIG_BANDS), 4)
    out["path_cov12"] = (settings("thin_walpha", 5, bands=COV12_BANDS, rho=0.3), 4)
    out["path_cov70"] = (settings("thin_walpha", 5, waves=COV70_WAVES, rho=0.2), 4)
    return out


def band_tables(g_pb, names):
    """golden_bands, and a name of the form X_delta_<wave>um as the one sample of weight 1 it is"""
    out = []
    for n in names:
        parts = n.split("_")
        if len(parts) == 3 and parts[1] == "delta" and parts[2].endswith("um"):
            out.append((np.array([float(parts[2][:-2])]), np.array([1.0]), 1.0))
        else:
            out.extend(golden_bands(g_pb, [n]))
    return out


def ndata(s):
    return len(s["bands"]) if s["waves"] is None else len(s["waves"])


def covariance(s, unc):
    """The data's covariance of a case with one: unc_i unc_j (delta_ij + rho (1 - delta_ij)); else None"""
    if s["rho"] is None:
        return None
    n = len(unc)
    return np.outer(unc, unc) * (np.eye(n) + s["rho"] * (1.0 - np.eye(n)))


def oracle_like(O, g_pb, s, flux, unc):
    cov = covariance(s, np.asarray(unc, dtype=np.float64))
    return O.OracleLikelihood(flux, unc, bands=None if s["waves"] is not None else band_tables(g_pb, s["bands"]),
                              wave=s["waves"], cov=cov,
                              opthin=s["opthin"], noalpha=s["noalpha"], lowlim=s["lowlim"], has_uplim=s["has_uplim"],
                              uplim=s["uplim"], has_gprior=s["has_gprior"], gprior_mean=s["gmean"],
                              gprior_sigma=s["gsigma"])


def make_data(O, g_pb, s):
    """(flux, unc) of a case: the oracle's model fluxes m at the truth, sigma = 0.05 m + 0.5 mJy, noise
    default_rng(seed).standard_normal."""
    # (the model at the truth whatever the case's limits are: the truth's beta is below the limit of the beta >= 2 case)
    plain = settings(s["variant"], s["seed"], bands=s["bands"], waves=s["waves"])
    like = oracle_like(O, g_pb, plain, np.ones(ndata(s)), np.ones(ndata(s)))
    m = like(TRUTH, return_flux=True)[1][0]
    unc = 0.05 * m + 0.5
    return m + unc * np.random.default_rng(s["seed"]).standard_normal(ndata(s)), unc


def make_starts(s, n):
    """truth (1 + 0.25 U(-1, 1)), put onto the lower limits where a draw falls below one (the beta >= 2 case: the
    truth's beta is 1.8, and a start below a limit is no start)."""
    rng = np.random.default_rng(1000 + s["seed"])
    st = TRUTH * (1.0 + 0.25 * rng.uniform(-1.0, 1.0, size=(n, 5)))
    return np.maximum(st, s["lowlim"])


def free_index(s, fixed=(0, 0, 0, 0, 0)):
    return [i for i in range(5) if not fixed[i] and not (i == 2 and s["opthin"]) and not (i == 3 and s["noalpha"])]


def residuals(O, like, s, p):
    """r with r^T r = -2 ln P(p) for a row inside the lower limits (likelihood.py:672-752, :790-834)."""
    p = np.asarray(p, dtype=np.float64)
    fl = like(p, return_flux=True)[1][0]
    d = like.flux - fl
    if hasattr(like, "invcov"):
        # d^T C^-1 d = |L^T d|^2 with C^-1 = L L^T
        r = list(np.linalg.cholesky(like.invcov).T @ d)
    else:
        r = list(d * np.sqrt(like.ivar))
    peak = None
    if s["has_uplim"][5] or s["has_gprior"][5]:
        peak = O.OracleSED(p[0], p[1], p[2], p[3], p[4], noalpha=s["noalpha"], opthin=s["opthin"]).max_wave()
    for i in range(6):
        v = peak if i == 5 else p[i]
        if s["has_uplim"][i]:
            lw = 0.02 * (s["uplim"][i] - (0.0 if i == 5 else s["lowlim"][i]))
            r.append((v - s["uplim"][i]) / lw if v > s["uplim"][i] else 0.0)
        if s["has_gprior"][i]:
            r.append((v - s["gmean"][i]) / s["gsigma"][i])
    return np.array(r)


def ref_search(O, like, s, x0, fixed=(0, 0, 0, 0, 0)):
    """(theta, lnP by the oracle) from x0 by scipy.optimize.least_squares over the free parameters: method "lm", or
    "trf" with bounds when the unbounded search ends below a lower limit."""
    from scipy.optimize import least_squares
    idx = free_index(s, fixed)
    x0 = np.asarray(x0, dtype=np.float64)

    def fun(x):
        p = x0.copy()
        p[idx] = x
        if np.any(p < s["lowlim"]):
            # (method "lm" has no bounds: a large finite residual sends it back; "trf" never comes here)
            return np.full(nres, 1e8)
        return residuals(O, like, s, p)
    nres = residuals(O, like, s, x0).size
    kw = dict(ftol=1e-15, xtol=1e-15, gtol=1e-15, x_scale=np.abs(x0[idx]))
    sol = least_squares(fun, x0[idx], method="lm", **kw)
    p = x0.copy()
    p[idx] = sol.x
    on_bound = False
    if np.any(p[idx] <= s["lowlim"][idx] * (1 + 1e-6)) or not np.isfinite(like(p)[0]):
        on_bound = True
    # the bounded search too wherever a limit could matter, and the better of the two
    sol2 = least_squares(fun, x0[idx], method="trf", bounds=(s["lowlim"][idx], np.inf), **kw)
    p2 = x0.copy()
    p2[idx] = sol2.x
    l1, l2 = like(p)[0], like(p2)[0]
    if on_bound or (np.isfinite(l2) and l2 > l1):
        p, l1 = p2, l2
    # "trf" keeps its iterates strictly inside: a parameter that ended within 1e-9 of its limit is put onto it
    snap = np.array(p)
    for i in idx:
        if snap[i] - s["lowlim"][i] <= 1e-9 * max(1.0, abs(s["lowlim"][i])):
            snap[i] = s["lowlim"][i]
    if like(snap)[0] >= l1 - 1e-13 * max(1.0, abs(l1)):
        p, l1 = snap, like(snap)[0]
    return p, float(l1)


def ref_jacobian(O, like, s, p, idx, h):
    cols = []
    for i in idx:
        hi = h * abs(p[i])
        a, b = np.array(p, dtype=np.float64), np.array(p, dtype=np.float64)
        a[i] -= hi; b[i] += hi
        cols.append((residuals(O, like, s, b) - residuals(O, like, s, a)) / (b[i] - a[i]))
    return np.array(cols).T


def ref_cov(O, like, s, p, fixed=(0, 0, 0, 0, 0)):
    """(cov [5, 5] = (J^T J)^-1 over the parameters that are free and off their lower limit, NaN elsewhere; the largest
    |cov(H1) - cov(H2)|_ij / sqrt(cov_ii cov_jj): the reference's own disagreement between its two step sizes)"""
    idx = [i for i in free_index(s, fixed) if p[i] > s["lowlim"][i]]
    covs = []
    for h in (H1, H2):
        J = ref_jacobian(O, like, s, p, idx, h)
        c = np.full((5, 5), np.nan)
        c[np.ix_(idx, idx)] = np.linalg.inv(J.T @ J)
        covs.append(c)
    return covs[0], float(np.nanmax(cov_error(covs[1], covs[0])))


def cov_error(cov, ref):
    """|cov - ref|_ij / sqrt(ref_ii ref_jj), NaN where the reference has none"""
    sd = np.sqrt(np.diagonal(ref, axis1=-2, axis2=-1))
    return np.abs(cov - ref) / (sd[..., :, None] * sd[..., None, :])


def gap_bound(lnp):
    """SURVEY.md 8c's tolerance between the device's likelihood and the oracle's: the most an optimum may lose"""
    return 1e-10 * max(1.0, abs(float(lnp)))


# ---------------------------------------------------------------- the host build of the step functions
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)


def _d(a):
    return a.ctypes.data_as(_dp)


class HostLM(object):
    """tests/_map_host.cpp compiled with the host compiler (as tests/_goodness_host.cpp is), numpy in and out."""

    def __init__(self, tmpdir):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        if not cxx:
            raise RuntimeError("no host C++ compiler")
        so = os.path.join(str(tmpdir), "libmap_host.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               os.path.join(ROOT, "tests", "_map_host.cpp"), "-o", so])
        L = self.lib = C.CDLL(so)
        L.lm_constants.argtypes = [_dp]
        L.lm_host_fixed_mask.argtypes = [_ip, C.c_int, C.c_int]; L.lm_host_fixed_mask.restype = C.c_uint
        L.lm_host_active.argtypes = [_dp, _dp, _dp, C.c_uint]; L.lm_host_active.restype = C.c_uint
        L.lm_host_solve.argtypes = [_dp, _dp, C.c_double, C.c_uint, _dp]
        L.lm_host_project.argtypes = [_dp, _dp, _dp, C.c_uint, _dp]
        L.lm_host_predicted.argtypes = [_dp, _dp, _dp, _dp]; L.lm_host_predicted.restype = C.c_double
        L.lm_host_clipped.argtypes = [_dp, _dp, _dp, C.c_uint]
        L.lm_host_accept.argtypes = [C.c_double, C.c_double]
        L.lm_host_gain.argtypes = [C.c_double] * 3; L.lm_host_gain.restype = C.c_double
        L.lm_host_candidates.argtypes = [C.c_double, C.c_double, _dp]
        L.lm_host_lambda_accept.argtypes = [C.c_double, C.c_double, _dp, _dp]
        L.lm_host_lambda_reject.argtypes = [_dp, _dp]
        L.lm_host_pick.argtypes = [C.c_double, _dp, C.c_int]
        L.lm_host_converged_f.argtypes = [C.c_double] * 3
        L.lm_host_scaled_step.argtypes = [_dp, _dp]; L.lm_host_scaled_step.restype = C.c_double
        L.lm_host_converged_x.argtypes = [C.c_double, C.c_double]
        L.lm_host_laplace.argtypes = [_dp, C.c_uint, _dp]
        k = np.zeros(9)
        L.lm_constants(_d(k))
        self.ncand, self.ntries, self.lam_start = int(k[0]), int(k[1]), k[2]
        self.ftol, self.xtol, self.maxiter, self.xfloor, self.lam_min, self.lam_max = k[3], k[4], int(k[5]), k[6], k[7], k[8]

    @staticmethod
    def _v(a):
        return np.ascontiguousarray(a, dtype=np.float64)

    def fixed_mask(self, fixed, opthin, noalpha):
        f = np.ascontiguousarray(fixed, dtype=np.int32)
        return int(self.lib.lm_host_fixed_mask(f.ctypes.data_as(_ip), int(opthin), int(noalpha)))

    def active(self, p, lowlim, g, fixed):
        return int(self.lib.lm_host_active(_d(self._v(p)), _d(self._v(lowlim)), _d(self._v(g)), fixed))

    def solve(self, A, g, lam, active):
        d = np.full(5, np.nan)
        ok = self.lib.lm_host_solve(_d(self._v(A)), _d(self._v(g)), lam, active, _d(d))
        return int(ok), d

    def project(self, p, d, lowlim, active):
        t = np.empty(5)
        self.lib.lm_host_project(_d(self._v(p)), _d(self._v(d)), _d(self._v(lowlim)), active, _d(t))
        return t

    def clipped(self, p, d, lowlim, active):
        return bool(self.lib.lm_host_clipped(_d(self._v(p)), _d(self._v(d)), _d(self._v(lowlim)), active))

    def predicted(self, A, g, p, trial):
        return float(self.lib.lm_host_predicted(_d(self._v(A)), _d(self._v(g)), _d(self._v(p)), _d(self._v(trial))))

    def accept(self, f, ft):
        return bool(self.lib.lm_host_accept(f, ft))

    def gain(self, f, ft, pred):
        return float(self.lib.lm_host_gain(f, ft, pred))

    def candidates(self, lam, nu):
        c = np.empty(self.ncand)
        self.lib.lm_host_candidates(lam, nu, _d(c))
        return c

    def lambda_accept(self, lam_taken, rho):
        lam, nu = C.c_double(), C.c_double()
        self.lib.lm_host_lambda_accept(lam_taken, rho, C.byref(lam), C.byref(nu))
        return lam.value, nu.value

    def lambda_reject(self, lam, nu):
        lam, nu = C.c_double(lam), C.c_double(nu)
        self.lib.lm_host_lambda_reject(C.byref(lam), C.byref(nu))
        return lam.value, nu.value

    def pick(self, f, ft):
        ft = self._v(ft)
        return int(self.lib.lm_host_pick(f, _d(ft), ft.size))

    def converged_f(self, pred, f, ftol):
        return bool(self.lib.lm_host_converged_f(pred, f, ftol))

    def scaled_step(self, p, trial):
        return float(self.lib.lm_host_scaled_step(_d(self._v(p)), _d(self._v(trial))))

    def converged_x(self, step, xtol):
        return bool(self.lib.lm_host_converged_x(step, xtol))

    def laplace(self, A, free):
        cov = np.empty((5, 5))
        ok = self.lib.lm_host_laplace(_d(self._v(A)), free, _d(cov))
        return int(ok), cov


def lm_drive(H, rfun, p0, lowlim, fixed_mask, maxiter=None, ftol=None, xtol=None, jac=None):
    """The kernel's loop around the host step functions: rfun(p) -> the residual vector, or None for a failing row.
    Returns (p, F, niter, nfev, why) with why one of "f", "x", "maxiter"."""
    maxiter = H.maxiter if maxiter is None else maxiter
    ftol = H.ftol if ftol is None else ftol
    xtol = H.xtol if xtol is None else xtol
    lowlim = np.asarray(lowlim, dtype=np.float64)
    nfev = [0]

    def F(p):
        nfev[0] += 1
        if np.any(p < lowlim):
            return np.inf
        r = rfun(p)
        return np.inf if r is None else float(r @ r)

    def normal(p):
        r0 = rfun(p)
        if jac is not None:                  # (a planted problem brings its own Jacobian)
            J = jac(p)
            return J.T @ J, -J.T @ r0
        J = np.zeros((r0.size, 5))
        for i in range(5):
            if (fixed_mask >> i) & 1:
                continue
            h = 2.0 ** -17 * max(abs(p[i]), H.xfloor)
            a, b = p.copy(), p.copy()
            nfev[0] += 2
            if p[i] - h < lowlim[i]:         # the second-order one-sided difference, as the kernel takes it there
                a[i] += h; b[i] += 2.0 * h
                J[:, i] = (4.0 * rfun(a) - 3.0 * r0 - rfun(b)) / (b[i] - p[i])
            else:
                a[i] -= h; b[i] += h
                J[:, i] = (rfun(b) - rfun(a)) / (b[i] - a[i])
        return J.T @ J, -J.T @ r0

    p = np.array(p0, dtype=np.float64)
    f = F(p)
    lam, nu, moved, why, niter = H.lam_start, 2.0, True, "maxiter", 0
    for it in range(maxiter):
        if moved:
            A, g = normal(p)
        niter += 1
        moved = False
        act = H.active(p, lowlim, g, fixed_mask)
        if not act:
            return p, f, niter, nfev[0], "f"
        stop = False
        for tr in range(H.ntries):
            cand = H.candidates(lam, nu)
            trials, preds, fts, steps, judged = [], [], [], [], []
            for c in cand:
                ok, d = H.solve(A, g, c, act)
                t = H.project(p, d, lowlim, act)
                pr = H.predicted(A, g, p, t)
                trials.append(t); preds.append(pr)
                if ok:
                    steps.append(H.scaled_step(p, t))
                    if not H.clipped(p, d, lowlim, act):
                        judged.append(pr)
                fts.append(F(t) if ok and pr > 0 else np.inf)
            best = H.pick(f, fts)
            pmax, smin = max([0.0] + judged), min(steps + [np.inf])
            if best >= 0:
                rho = H.gain(f, fts[best], preds[best])
                lam, nu = H.lambda_accept(cand[best], rho)
                if H.converged_x(steps[best], xtol):
                    why, stop = "x", True
                p, f, moved = trials[best], fts[best], True
            else:
                lam, nu = H.lambda_reject(lam, nu)
                if H.converged_x(smin, xtol):
                    why, stop = "x", True
            if judged and H.converged_f(pmax, f, ftol):      # (only a step the projection left alone says so)
                why, stop = "f", True
            if stop or moved:
                break
        if stop:
            break
    return p, f, niter, nfev[0], why
