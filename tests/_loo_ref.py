"""The definitions of include/mbb_hip.h's out-of-sample fit restated in numpy, in a dtype of the caller's choice
(float64 or longdouble), with mpmath for Phi.  Nothing here knows the device code: it is what the device code is held to.

    ll_rows(flux, model, ivar= | invcov=)    the pointwise term [n, nb] from band fluxes
    tail_len(S)                              M = ceil(min(0.2 S, 3 sqrt S)), as `loo` forms it
    gpd_fit(x)                               Zhang & Stephens' (k, sigma), the prior's k-hat and the fallback decision
    psis(ll)                                 the smoothed log weights of one column, k-hat, M, the fallback, tail indices
    column(ll, z)                            every per-band statistic of one column, as a dict
    STATUS bits
"""
import numpy as np

LD = np.longdouble
K_HIGH, TAIL_SHORT, TAIL_FLAT, WAIC_VAR_HIGH = 16, 32, 64, 128
EMPTY, HAS_NAN = 1, 2
FIT_OK, FIT_SHORT, FIT_FLAT = 0, 1, 2


def _ln2pi(dtype):
    return np.log(2 * np.arccos(dtype(-1)))


def ll_rows(flux, model, ivar=None, invcov=None, dtype=LD):
    """ll [n, nb], g [n, nb] and Lambda_bb [nb] from the data [nb] and band fluxes [n, nb]."""
    f, m = np.asarray(flux, dtype=dtype), np.asarray(model, dtype=dtype)
    r = f[None, :] - m
    if invcov is not None:
        lam = np.asarray(invcov, dtype=dtype)
        g = r @ lam.T
        d = np.diag(lam).copy()
    else:
        d = np.asarray(ivar, dtype=dtype)
        g = r * d[None, :]
    ll = (np.log(d) - _ln2pi(dtype))[None, :] / 2 - g * g / d[None, :] / 2
    return ll, g, d


def ll_bound(flux, model, ivar=None, invcov=None):
    """The rounding bound of ll computed in float64 from the same band fluxes: gamma_(nb+4) (sum_j |L_bj| |r_j|)^2 / L_bb
    plus 2 eps of the constant (eps = 2^-52; gamma_k = k u / (1 - k u) with u = eps / 2)."""
    eps = np.finfo(np.float64).eps / 2
    f, m = np.asarray(flux, dtype=LD), np.asarray(model, dtype=LD)
    r = np.abs(f[None, :] - m)
    if invcov is not None:
        lam = np.abs(np.asarray(invcov, dtype=LD))
        a = r @ lam.T
        d = np.diag(lam)
    else:
        d = np.asarray(ivar, dtype=LD)
        a = r * d[None, :]
    nb = f.size
    gam = (nb + 4) * eps / (1 - (nb + 4) * eps)
    const = np.abs(np.log(d) - _ln2pi(LD)) / 2
    return (gam * a * a / d[None, :] + 2 * np.finfo(np.float64).eps * const[None, :]).astype(np.float64)


def tail_len(S):
    return int(np.ceil(min(0.2 * S, 3 * np.sqrt(S)))) if S > 0 else 0


def gpd_fit(x, dtype=LD):
    """(why, k, sigma, khat) of an ascending tail x >= 0"""
    x = np.asarray(x, dtype=dtype)
    M = x.size
    inf, nan = dtype(np.inf), dtype(np.nan)
    if M < 5:
        return FIT_SHORT, nan, nan, inf
    xstar = x[int(np.floor(M / 4 + 0.5)) - 1]
    if not x[-1] > x[0] or not xstar > 0:
        return FIT_FLAT, nan, nan, inf
    m = 30 + int(np.floor(np.sqrt(M)))
    j = np.arange(1, m + 1).astype(dtype)
    with np.errstate(all="ignore"):
        theta = 1 / x[-1] + (1 - np.sqrt(m / (j - dtype(0.5)))) / (3 * xstar)
        kj = np.array([np.sum(np.log1p(-t * x)) / M for t in theta], dtype=dtype)
        l = M * (np.log(-theta / kj) - kj - 1)
        w = np.exp(l - np.max(l))
        w = w / np.sum(w)
        th = np.sum(theta * w)
        k = np.sum(np.log1p(-th * x)) / M
        sigma = -k / th
        khat = (k * M + 5) / (dtype(M) + 10)
    if not (np.isfinite(k) and np.isfinite(sigma) and np.isfinite(khat)):
        return FIT_FLAT, nan, nan, inf
    return FIT_OK, k, sigma, khat


def gpd_quantile(p, khat, sigma):
    return sigma * np.expm1(-khat * np.log1p(-p)) / khat


def _lse(v):
    mx = np.max(v)
    return mx + np.log(np.sum(np.exp(v - mx)))


def psis(ll, dtype=LD):
    """The log weights of the finite entries of one column, in window order: (lw, khat, M, why, tail) with tail the
    positions (among the finite entries) of the M tail entries in ascending (lw, index) order."""
    ll = np.asarray(ll, dtype=dtype)
    S = ll.size
    neg = -ll
    lw = neg - np.max(neg)
    M = tail_len(S)
    order = np.argsort(lw, kind="stable")          # ascending (lw, index)
    tail = order[S - M:]
    if M < 5:
        return lw, dtype(np.inf), M, FIT_SHORT, tail
    c = lw[order[S - M - 1]]
    x = np.exp(lw[tail]) - np.exp(c)
    why, k, sigma, khat = gpd_fit(x, dtype)
    if why != FIT_OK:
        return lw, khat, M, why, tail
    p = (np.arange(1, M + 1).astype(dtype) - dtype(0.5)) / M
    lw = lw.copy()
    lw[tail] = np.log(gpd_quantile(p, khat, sigma) + np.exp(c))
    lw = np.minimum(lw, 0)
    return lw, khat, M, why, tail


def norm_cdf_mp(z):
    """Phi(z) by mpmath at 30 digits, as longdouble"""
    import mpmath
    mpmath.mp.dps = 30
    tiny = mpmath.mpf(10) ** -4900              # (below it a longdouble is 0 anyway)
    return np.array([(LD(mpmath.nstr(p, 25)) if p > tiny else LD(0)) if np.isfinite(v) else LD(np.nan)
                     for v, p in ((v, mpmath.ncdf(mpmath.mpf(float(v))) if np.isfinite(v) else None)
                                  for v in np.atleast_1d(z))], dtype=LD)


def norm_cdf(z, dtype=LD):
    """Phi through mpmath (the values are exact to the dtype for float64 arguments)"""
    return norm_cdf_mp(np.asarray(z, dtype=np.float64)).astype(dtype)


def column(ll, z, dtype=LD, phi=None):
    """Every per-band statistic of one window column: ll [n] (non-finite entries are left out), z = g / sqrt(Lambda_bb)
    [n].  phi: Phi(z) of the finite entries when the caller has it already."""
    ll = np.asarray(ll, dtype=dtype)
    ok = np.isfinite(ll)
    n, S = ll.size, int(ok.sum())
    nan = dtype(np.nan)
    out = dict(n_used=S, tail_len=tail_len(S), lppd=nan, p_waic=nan, elpd_waic=nan, elpd_loo=nan, p_loo=nan,
               khat=dtype(np.inf), loo_pit=nan, status=(EMPTY if S == 0 else 0) | (HAS_NAN if S < n else 0))
    if S == 0:
        out["status"] |= TAIL_SHORT | K_HIGH
        return out
    v = ll[ok]
    out["lppd"] = _lse(v) - np.log(dtype(S))
    if S >= 2:
        mean = np.sum(v) / S
        out["p_waic"] = np.sum((v - mean) ** 2) / (S - 1)
    out["elpd_waic"] = out["lppd"] - out["p_waic"]
    lw, khat, M, why, tail = psis(v, dtype)
    out["khat"] = khat
    out["elpd_loo"] = _lse(v + lw) - _lse(lw)
    out["p_loo"] = out["lppd"] - out["elpd_loo"]
    if phi is None:
        phi = norm_cdf(np.asarray(z)[ok], dtype)
    out["loo_pit"] = np.sum(np.exp(lw - _lse(lw)) * phi)
    out["tail"] = np.nonzero(ok)[0][tail]
    out["status"] |= ((K_HIGH if khat > 0.7 else 0) | (TAIL_SHORT if why == FIT_SHORT else 0) |
                      (TAIL_FLAT if why == FIT_FLAT else 0) | (WAIC_VAR_HIGH if out["p_waic"] > 0.4 else 0))
    return out


FLOATS = ("lppd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "khat", "loo_pit")


def distance(a, b):
    """The largest |a - b| / max(1, |b|) over the floating-point outputs of two column() results (both infinite or both
    NaN: 0)."""
    worst = 0.0
    for k in FLOATS:
        x, y = LD(a[k]), LD(b[k])
        if (np.isnan(x) and np.isnan(y)) or x == y:
            continue
        if not (np.isfinite(x) and np.isfinite(y)):
            return np.inf
        worst = max(worst, float(abs(x - y) / max(LD(1), abs(y))))
    return worst
