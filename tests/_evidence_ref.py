"""Reference of the evidence (csrc/mbb_bridge.hip.h, csrc/mbb_evidence.hip.h) for its tests.

``ref_bridge`` is the bridge-sampling fixed point and its error in numpy longdouble, from ln l1 and ln l2 alone;
``window``, ``moments``, ``chol``, ``lnq`` restate the window split, the proposal fit and the Gaussian's log density in
longdouble; ``draws`` makes the proposal rows from a Python-integer Philox (tests/_draws_ref.py's) and mpmath's inverse
normal CDF.  ``HostBridge`` is the HOST build of the step functions (tests/_evidence_host.cpp) and ``host_drive`` the
kernel's loop in Python around it: the algorithm without a device.  The cases of tests/golden/evidence.npz are made here
(``case_settings``, ``make_cases``) and written by tests/make_golden_evidence.py; the tests read that file and the
oracle, never scipy's integrators."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from conftest import ROOT
import _map_ref as MR
from _draws_ref import philox4x32

LD = np.longdouble
STREAM = 0x42524447                     # "BRDG"
WAVES = np.array([100.0, 250.0, 350.0, 500.0])          # four delta bands
THETA0 = np.array([12.0, 1.8, 150.0, 3.0, 40.0])        # the data's truth; the held parameters stay here
# br_ppnd's host build against mpmath on the 10^4 points of tests/test_evidence_cpu.py (which holds it to these): the
# largest relative error 6.283e-16, the largest absolute error 4.127e-15 (in the far tails, |z| ~ 8)
PPND_MEASURED_REL, PPND_MEASURED_ABS = 6.3e-16, 4.2e-15
CONVERGED, MAXITER, COV_SINGULAR, POST_LEFT_OUT, NO_OVERLAP, ALL_HELD, HELD_SHIFT = 1, 2, 4, 8, 16, 32, 8


# ---- the window, the proposal ------------------------------------------------------------------------------------
def window(nsteps, burn=0, thin=1):
    """(steps of the fit half, steps of the posterior half): of the kept steps the first nkept // 2, and the rest"""
    kept = np.arange(int(burn), int(nsteps), int(thin))
    nfit = len(kept) // 2
    return kept[:nfit], kept[nfit:]


def moments(chain, burn=0, thin=1):
    """mean [5] and covariance [5, 5] (ddof = 1) over the fit half of chain [nw, nsteps, 5], in longdouble"""
    fit, _ = window(chain.shape[1], burn, thin)
    x = chain[:, fit].reshape(-1, 5).astype(LD)
    mu = x.sum(axis=0) / LD(x.shape[0])
    d = x - mu
    return mu, (d.T @ d) / LD(x.shape[0] - 1)


def chol(cov, free, dt=LD):
    """L [d, d] (longdouble, or dt) of cov over the free indices, or None when a pivot is not positive"""
    a = np.asarray(cov, dtype=dt)[np.ix_(free, free)]
    d = len(free)
    L = np.zeros((d, d), dtype=dt)
    for j in range(d):
        s = a[j, j] - np.dot(L[j, :j], L[j, :j])
        if not s > 0:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, d):
            L[i, j] = (a[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def lnq(theta, mu, L, free, dt=LD):
    """ln N(theta; mu, L L^T) over the free indices, longdouble (or dt); theta [..., 5]"""
    d = len(free)
    r = (np.asarray(theta, dtype=dt)[..., free] - np.asarray(mu, dtype=dt)[free])
    y = np.zeros(r.shape, dtype=dt)
    for i in range(d):
        y[..., i] = (r[..., i] - np.sum(L[i, :i] * y[..., :i], axis=-1)) / L[i, i]
    return -dt(d) / 2 * np.log(2 * dt(np.pi)) - np.sum(np.log(np.diag(L))) - np.sum(y * y, axis=-1) / 2


def moments64(chain, burn=0, thin=1):
    """``moments`` in float64: what plain numpy makes of the same inputs"""
    fit, _ = window(chain.shape[1], burn, thin)
    x = chain[:, fit].reshape(-1, 5)
    mu = x.sum(axis=0) / x.shape[0]
    d = x - mu
    return mu, (d.T @ d) / (x.shape[0] - 1)


def uniforms_k(seed, src, n):
    """k [n, 5] (Python integers of 53 bits) of draws 0 .. n - 1 of source number src: word pairs (0,1) .. (8,9) of the
    three Philox blocks at counter (i, src, STREAM, 0..2)"""
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    out = []
    for i in range(n):
        w = []
        for b in range(3):
            w.extend(philox4x32((i, src, STREAM, b), key))
        out.append([((w[2 * k] >> 5) << 26) | (w[2 * k + 1] >> 6) for k in range(5)])
    return out


def ppf_mp(k):
    """the normal deviate of u = (k + 1/2) 2^-53 by mpmath at 50 digits, as an mpf"""
    import mpmath as mp
    mp.mp.dps = 50
    u = (mp.mpf(int(k)) + mp.mpf(1) / 2) / mp.mpf(2) ** 53
    return mp.sqrt(2) * mp.erfinv(2 * u - 1) if abs(2 * u - 1) < mp.mpf("0.9") else _ppf_tail(u)


def _ppf_tail(u):
    import mpmath as mp
    # erfinv loses digits next to +-1: solve the complementary function for the tail area instead
    t = u if u < mp.mpf(1) / 2 else 1 - u
    z = mp.findroot(lambda x: mp.erfc(x / mp.sqrt(2)) / 2 - t, mp.sqrt(-2 * mp.log(t)) - mp.mpf("0.3"))
    return -z if u < mp.mpf(1) / 2 else z


def draws(seed, src, n, mu, L5, free, held):
    """Proposal rows [n, 5] in longdouble: theta = mu + L z over the free set, held values elsewhere; L5 is the 5 x 5
    factor as reported (float64 values), z by mpmath"""
    ks = uniforms_k(seed, src, n)
    out = np.empty((n, 5), dtype=LD)
    zs = np.empty((n, 5), dtype=LD)
    for i in range(n):
        for k in range(5):
            zs[i, k] = LD(str(ppf_mp(ks[i][k])))
    L5 = np.asarray(L5, dtype=LD)
    for k in range(5):
        if k in free:
            out[:, k] = LD(mu[k]) + sum(L5[k, j] * zs[:, j] for j in free if j <= k)
        else:
            out[:, k] = held[k]
    return out, zs


# ---- the bridge ------------------------------------------------------------------------------------------------------
def _num(b, rho, s1, s2):
    b = np.asarray(b, dtype=LD)
    out = np.zeros(b.shape, dtype=LD)
    ok = np.isfinite(b)
    pos = ok & (b > 0)
    neg = ok & ~pos
    out[pos] = 1 / (s1 + s2 * rho * np.exp(-b[pos]))
    e = np.exp(b[neg])
    out[neg] = e / (s1 * e + s2 * rho)
    return out


def _den(a, rho, s1, s2):
    a = np.asarray(a, dtype=LD)
    out = np.empty(a.shape, dtype=LD)
    pos = a > 0
    e = np.exp(-a[pos])
    out[pos] = e / (s1 + s2 * rho * e)
    out[~pos] = 1 / (s1 * np.exp(a[~pos]) + s2 * rho)
    return out


def ref_bridge(lnl1, lnl2, neff=None, tol=1e-15, maxiter=10000, lstar=None):
    """The fixed point in longdouble.  lnl1: ln l1 at the posterior samples (the non-finite ones are left out);
    lnl2: ln l2 at the proposal draws (-inf and NaN contribute nothing).  Returns a dict: lnz, err, niter, converged,
    rhos (every iterate), contraction (the largest ratio of successive changes seen over the last iterations)."""
    a = np.asarray(lnl1, dtype=LD)
    a = a[np.isfinite(a)]
    b = np.asarray(lnl2, dtype=LD)
    n1, n2 = LD(a.size), LD(b.size)
    n1e = n1 if neff is None else LD(min(max(float(neff), 1.0), float(n1)))
    s1, s2 = n1e / (n1e + n2), n2 / (n1e + n2)
    ls = a.sum() / n1 if lstar is None else LD(lstar)
    a, b = a - ls, b - ls
    rho, rhos, conv = LD(1), [LD(1)], False
    for it in range(1, maxiter + 1):
        new = (_num(b, rho, s1, s2).sum() / n2) / (_den(a, rho, s1, s2).sum() / n1)
        conv = abs(new - rho) <= LD(tol) * new
        rho = new
        rhos.append(rho)
        if conv:
            break
    f1, f2 = _num(b, rho, s1, s2), _den(a, rho, s1, s2)
    m1, m2 = f1.sum() / n2, f2.sum() / n1
    v1, v2 = ((f1 - m1) ** 2).sum() / (n2 - 1), ((f2 - m2) ** 2).sum() / (n1 - 1)
    re2 = v1 / (n2 * m1 * m1) + v2 / (n1e * m2 * m2)
    d = np.abs(np.diff(np.array(rhos, dtype=LD)))
    ratios = [float(d[i + 1] / d[i]) for i in range(len(d) - 1) if d[i] > 0 and d[i + 1] > 1e-17 * rho]
    return dict(lnz=float(np.log(rho) + ls), err=float(np.sqrt(re2)), niter=it, converged=bool(conv),
                rhos=rhos, contraction=max(ratios) if ratios else 0.0, n1=int(n1), lstar=float(ls))


# ---- the host build --------------------------------------------------------------------------------------------------
_dp, _ip, _up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)


def _d(a):
    return a.ctypes.data_as(_dp)


class HostBridge(object):
    """tests/_evidence_host.cpp compiled with the host compiler (as tests/_map_host.cpp is), numpy in and out."""

    def __init__(self, tmpdir):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        if not cxx:
            raise RuntimeError("no host C++ compiler")
        so = os.path.join(str(tmpdir), "libevidence_host.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               os.path.join(ROOT, "tests", "_evidence_host.cpp"), "-o", so])
        L = self.lib = C.CDLL(so)
        dbl, uint = C.c_double, C.c_uint
        L.br_constants.argtypes = [_dp]
        L.br_host_centered.argtypes = [C.c_ulonglong]; L.br_host_centered.restype = dbl
        L.br_host_bits53.argtypes = [uint, uint]; L.br_host_bits53.restype = C.c_ulonglong
        L.br_host_ppnd.argtypes = [dbl]; L.br_host_ppnd.restype = dbl
        L.br_host_ppnd_k.argtypes = [_up, C.c_int, _dp]
        L.br_host_log.argtypes = [dbl]; L.br_host_log.restype = dbl
        L.br_host_free_mask.argtypes = [_ip, C.c_int, C.c_int, uint]; L.br_host_free_mask.restype = uint
        L.br_host_chol.argtypes = [_dp, uint, _dp, _dp]
        L.br_host_lnq.argtypes = [_dp, _dp, _dp, uint, dbl]; L.br_host_lnq.restype = dbl
        L.br_host_draw.argtypes = [_dp, _dp, _dp, uint, _dp, _dp]
        L.br_host_term_num.argtypes = [dbl] * 4; L.br_host_term_num.restype = dbl
        L.br_host_term_den.argtypes = [dbl] * 4; L.br_host_term_den.restype = dbl
        L.br_host_converged.argtypes = [dbl] * 3
        L.br_host_relerr2.argtypes = [dbl] * 6; L.br_host_relerr2.restype = dbl
        L.br_host_sums.argtypes = [_dp, C.c_int, _dp, C.c_int, dbl, dbl, dbl, _dp]
        L.br_host_moments.argtypes = [_dp, C.c_int, _dp, C.c_int, dbl, dbl, dbl, _dp]
        c = np.empty(4)
        L.br_constants(_d(c))
        self.tol_default, self.maxiter_default, self.pivot_rel, self.ln2pi = c[0], int(c[1]), c[2], c[3]

    def ppnd_k(self, k):
        k = np.ascontiguousarray(k, dtype=np.uint64)
        z = np.empty(k.size)
        self.lib.br_host_ppnd_k(k.ctypes.data_as(_up), k.size, _d(z))
        return z

    def free_mask(self, fixed, opthin, noalpha, held=0):
        f = np.ascontiguousarray(fixed, dtype=np.int32)
        return int(self.lib.br_host_free_mask(f.ctypes.data_as(_ip), int(opthin), int(noalpha), int(held)))

    def chol(self, cov, free_mask):
        cov = np.ascontiguousarray(cov, dtype=np.float64)
        L, sl = np.empty((5, 5)), np.empty(1)
        ok = self.lib.br_host_chol(_d(cov), int(free_mask), _d(L), _d(sl))
        return int(ok), L, float(sl[0])

    def lnq(self, theta, mu, L, free_mask, sumlog):
        t, m, LL = (np.ascontiguousarray(x, dtype=np.float64) for x in (theta, mu, L))
        return float(self.lib.br_host_lnq(_d(t), _d(m), _d(LL), int(free_mask), float(sumlog)))

    def draw(self, mu, L, z, free_mask, held):
        m, LL, zz, h = (np.ascontiguousarray(x, dtype=np.float64) for x in (mu, L, z, held))
        out = np.empty(5)
        self.lib.br_host_draw(_d(m), _d(LL), _d(zz), int(free_mask), _d(h), _d(out))
        return out


def host_drive(H, lnl1, lnl2, neff=None, tol=None, maxiter=None, lstar=None):
    """k_ev_bridge's loop around the host build of the step functions (sums in plain order)."""
    a = np.ascontiguousarray(np.asarray(lnl1, dtype=np.float64)[np.isfinite(lnl1)])
    b = np.ascontiguousarray(lnl2, dtype=np.float64)
    tol = H.tol_default if tol is None else tol
    maxiter = H.maxiter_default if maxiter is None else maxiter
    n1, n2 = float(a.size), float(b.size)
    n1e = n1 if neff is None else min(max(float(neff), 1.0), n1)
    s1, s2 = n1e / (n1e + n2), n2 / (n1e + n2)
    ls = a.sum() / n1 if lstar is None else float(lstar)
    a, b = np.ascontiguousarray(a - ls), np.ascontiguousarray(b - ls)
    rho, conv, it, out = 1.0, False, 0, np.empty(4)
    while it < maxiter and not conv:
        H.lib.br_host_sums(_d(a), a.size, _d(b), b.size, rho, s1, s2, _d(out))
        new = (out[0] / n2) / (out[1] / n1)
        it += 1
        conv = bool(H.lib.br_host_converged(new, rho, tol))
        rho = new
    H.lib.br_host_moments(_d(a), a.size, _d(b), b.size, rho, s1, s2, _d(out))
    re2 = H.lib.br_host_relerr2(out[0], out[1], n2, out[2], out[3], n1e)
    return dict(lnz=H.lib.br_host_log(rho) + ls, err=float(np.sqrt(re2)), niter=it, converged=conv)


# ---- the fixture's cases ---------------------------------------------------------------------------------------------
FIXED = {"a": (1, 1, 0, 0, 0), "b": (0, 1, 0, 0, 0), "c": (0, 1, 0, 0, 0)}       # thin, no alpha: lambda0 and alpha held
FREE = {"a": [4], "b": [0, 4], "c": [0, 4]}


def case_settings(lowlim_T=None):
    """Thin model without alpha at four plain wavelengths, default limits; no upper limit or prior touches a free
    parameter; (c) adds a lower limit on T."""
    return MR.settings("thin_noalpha", 11, waves=WAVES, lowlim=None if lowlim_T is None else {0: float(lowlim_T)})


def oracle_lnp(O, g, case):
    """lnP(free parameters [..., d]) of a fixture case by the oracle, the held parameters at THETA0"""
    s = case_settings(float(g["c/lowlim_T"]) if case == "c" else None)
    like = MR.oracle_like(O, None, s, g["flux"], g["unc"])
    free = FREE[case]

    def lnp(x):
        x = np.asarray(x, dtype=np.float64)
        p = np.broadcast_to(THETA0, x.shape[:-1] + (5,)).copy()
        p[..., free] = x
        return like(p.reshape(-1, 5)).reshape(x.shape[:-1])
    return lnp


def device_like(g, case, scale=1.0, lowlim_T=None):
    """The package's likelihood of a fixture case (scale: the data times that)"""
    import mbb_emcee_amd as mbb
    s = case_settings(float(g["c/lowlim_T"]) if case == "c" else lowlim_T)
    like = mbb.likelihood(response=False, opthin=True, noalpha=True, device=0)
    like.set_phot(WAVES, scale * g["flux"], scale * g["unc"])
    for i in range(5):
        like.set_lowlim(i, s["lowlim"][i])
    for i in range(6):
        if s["has_uplim"][i]:
            like.set_uplim(i, s["uplim"][i])
    return like


def make_cases(O):
    """The fixture: data, and the exact ln Z of the three cases (scipy's integrators; the tests do not need them)."""
    from scipy import integrate
    s = case_settings()
    flux, unc = MR.make_data(O, None, s)
    g = {"flux": flux, "unc": unc, "waves": WAVES, "theta0": THETA0}
    like = MR.oracle_like(O, None, s, flux, unc)
    # (a) fnorm alone: the model is fnorm times the fluxes at fnorm = 1
    p1 = THETA0.copy(); p1[4] = 1.0
    sb = like(p1, return_flux=True)[1][0].astype(LD)
    f, iv = flux.astype(LD), (1 / unc.astype(LD) ** 2)
    A, B = np.sum(sb * sb * iv), np.sum(sb * f * iv)
    chi_min = np.sum(f * f * iv) - B * B / A
    g["a/lnz"] = np.array(float(-chi_min / 2 + np.log(2 * LD(np.pi) / A) / 2))
    g["a/mean"], g["a/sigma"] = np.array(float(B / A)), np.array(float(1 / np.sqrt(A)))
    # (b) T and fnorm: the posterior's mean and width from a grid, then dblquad over +-12 sigma
    lnp = oracle_lnp(O, dict(g, **{"c/lowlim_T": np.array(1.0)}), "b")
    T = np.linspace(6.0, 25.0, 1521); F = np.linspace(float(B / A) * 0.4, float(B / A) * 2.0, 801)
    grid = lnp(np.stack(np.meshgrid(T, F, indexing="ij"), axis=-1))
    w = np.exp(grid - grid.max()); w /= w.sum()
    mT, mF = (w.sum(axis=1) * T).sum(), (w.sum(axis=0) * F).sum()
    sT, sF = np.sqrt((w.sum(axis=1) * (T - mT) ** 2).sum()), np.sqrt((w.sum(axis=0) * (F - mF) ** 2).sum())
    peak = grid.max()

    def integrand(fn, t):
        return np.exp(lnp(np.array([t, fn])) - peak)

    def total(t_lo):
        v, e = integrate.dblquad(integrand, t_lo, mT + 12 * sT, mF - 12 * sF, mF + 12 * sF, epsabs=0, epsrel=1e-10)
        return np.log(v) + peak, e / v
    g["b/lnz"], g["b/quad_relerr"] = (np.array(x) for x in total(max(mT - 12 * sT, 1.0)))
    g["b/mean"], g["b/sigma"] = np.array([mT, mF]), np.array([sT, sF])
    # (c) a lower limit on T one posterior sigma below the mean
    g["c/lowlim_T"] = np.array(mT - sT)
    g["c/lnz"], g["c/quad_relerr"] = (np.array(x) for x in total(float(mT - sT)))
    return g
