"""The definitions of include/mbb_hip.h's reweighting restated in numpy, in a dtype of the caller's choice (float64 or
longdouble) for the floating-point part and in integers for the weights.  Nothing here knows the device code: it is what
the device code is held to.  PSIS itself is tests/_loo_ref.py's, imported: lw = psis(-r).

    classes(lp, lq)            (used, zero, left out) masks of a window's entries
    scalars(r_used, nzero)     lw of the used entries, k-hat, M, the fallback, ess and lnz_ratio, as a dict
    quantise(lw)               u = floor(e^lw 2^32 + 1/2) as int64, from longdouble
    target(p, U)               t = ceil((p / 100.0) * float(U)) clamped to [1, U], in float64 as the definition says
    wquantile(x, u, p)         the smallest x with sum_{x_j <= x} u_j >= t: integers throughout
    wmean(x, u), wcov(X, u)    sum u x / U and sum u d d^T / U in a dtype
    STATUS bits
"""
import numpy as np

import _loo_ref as LR

LD = LR.LD
EMPTY, HAS_NAN = 1, 2
K_HIGH, TAIL_SHORT, TAIL_FLAT, HAS_ZERO, ALL_ZERO = 16, 32, 64, 128, 65536
ONE = 1 << 32


def classes(lp, lq):
    lp, lq = np.asarray(lp, dtype=np.float64), np.asarray(lq, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        r = lq - lp
    used = np.isfinite(r)
    zero = ~used & np.isfinite(lp) & np.isneginf(lq)
    return used, zero, ~used & ~zero


def scalars(r_used, nzero=0, dtype=LD, smooth=True):
    """Of the used entries' r [S] in window order: dict(lw [S], khat, M, why, ess, lnz_ratio, status bits of the fit)."""
    r = np.asarray(r_used, dtype=dtype)
    S = r.size
    nan = dtype(np.nan)
    if S == 0:
        return dict(lw=r, khat=dtype(np.inf), M=0, why=LR.FIT_SHORT, ess=nan,
                    lnz_ratio=dtype(-np.inf) if nzero else nan,
                    status=EMPTY | K_HIGH | TAIL_SHORT | (HAS_ZERO | ALL_ZERO if nzero else 0))
    lw, khat, M, why, tail = LR.psis(-r, dtype)
    if not smooth:
        lw = r - np.max(r)
    e = np.exp(lw)
    s1, s2 = np.sum(e), np.sum(e * e)
    return dict(lw=lw, khat=khat, M=M, why=why, ess=s1 * s1 / s2, tail=tail,
                lnz_ratio=np.max(r) + np.log(s1) - np.log(dtype(S + nzero)),
                status=(K_HIGH if khat > 0.7 else 0) | (TAIL_SHORT if why == LR.FIT_SHORT else 0) |
                       (TAIL_FLAT if why == LR.FIT_FLAT else 0) | (HAS_ZERO if nzero else 0))


def distance(a, b):
    """The largest |a - b| / max(1, |b|) over lw, khat, ess / S and lnz_ratio of two scalars() results (both infinite or
    both NaN: 0).  (ess is compared per entry: it is a count.)"""
    S = max(1, np.asarray(b["lw"]).size)
    worst = 0.0
    pairs = [(a["khat"], b["khat"]), (LD(a["ess"]) / S, LD(b["ess"]) / S), (a["lnz_ratio"], b["lnz_ratio"])]
    pairs += list(zip(np.asarray(a["lw"]), np.asarray(b["lw"])))
    xs = np.array([p[0] for p in pairs], dtype=LD)
    ys = np.array([p[1] for p in pairs], dtype=LD)
    same = (np.isnan(xs) & np.isnan(ys)) | (xs == ys)
    if not np.all(np.isfinite(xs[~same]) & np.isfinite(ys[~same])):
        return np.inf
    if np.any(~same):
        worst = float(np.max(np.abs(xs[~same] - ys[~same]) / np.maximum(LD(1), np.abs(ys[~same]))))
    return worst


def quantise(lw):
    """u of log weights (float64, -inf allowed) as int64, formed in longdouble"""
    lw = np.asarray(lw, dtype=np.float64)
    with np.errstate(under="ignore"):
        v = np.floor(np.exp(lw.astype(LD)) * LD(ONE) + LD(0.5))
    return np.minimum(v, LD(ONE)).astype(np.int64)


def target(p, U):
    U = int(U)
    if U == 0:
        return 0
    t = int(np.ceil((float(p) / 100.0) * float(U)))
    return min(max(t, 1), U)


def wquantile(x, u, p):
    """The weighted inverted-CDF quantile at percent p of values x with integer weights u (entries of weight 0 take no
    part); NaN with no weight."""
    x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.int64)
    keep = u > 0
    x, u = x[keep], u[keep]
    U = int(u.sum())
    if U == 0:
        return np.nan
    order = np.argsort(x, kind="stable")
    cum = np.cumsum(u[order])                       # (int64: U < 2^53)
    return x[order][int(np.searchsorted(cum, target(p, U), side="left"))]


def wmean(x, u, dtype=LD):
    u = np.asarray(u, dtype=np.int64)
    return np.sum(u.astype(dtype) * np.asarray(x, dtype=dtype)) / dtype(int(u.sum()))


def wcov(X, u, dtype=LD):
    """sum u d d^T / U of the columns of X [n, 5] about their weighted means (no ddof correction)"""
    u = np.asarray(u, dtype=np.int64)
    X = np.asarray(X, dtype=dtype)
    w = u.astype(dtype)
    U = dtype(int(u.sum()))
    d = X - (w[:, None] * X).sum(axis=0) / U
    return (w[:, None, None] * d[:, :, None] * d[:, None, :]).sum(axis=0) / U
