"""The population hyper-likelihood's definitions (include/mbb_hip.h: "the population of a catalogue") restated in numpy,
with the dtype as an argument: float64, and longdouble as the reference the device and the float64 form are held to."""
import numpy as np

LD = np.longdouble
IDENTITY, LOG10 = 0, 1
WALL_REL_WIDTH = 0.02
UNDERFLOW = -745.0
FLOATS = ("lnl_src", "ess", "mean", "cov")


def pi_of(dt):
    return dt(4) * np.arctan(dt(1))


def flat_prior():
    """The spec of a likelihood without upper limits and Gaussian priors."""
    return dict(has_uplim=[0] * 5, has_gprior=[0] * 5, lowlim=[0.0] * 5, uplim=[np.inf] * 5, gmean=[0.0] * 5, givar=[1.0] * 5)


def like_prior(like):
    """... of a ``likelihood``: what population._Request takes from it."""
    hu = [int(bool(b)) for b in like._has_uplim[:5]]
    return dict(has_uplim=hu, has_gprior=[int(bool(b)) for b in like._has_gprior[:5]],
                lowlim=[float(v) for v in like._lowlim[:5]],
                uplim=[float(v) if h else np.inf for v, h in zip(like._uplim[:5], hu)],
                gmean=[float(v) for v in like._gprior_mean[:5]], givar=[float(v) for v in like._gprior_ivar[:5]])


def prior_factor(theta, k, prior, dt):
    """ln of the separable prior factor of parameter k at theta (an array), unnormalised."""
    th = np.asarray(theta, dtype=dt)
    lp = np.zeros(th.shape, dtype=dt)
    if prior["has_uplim"][k]:
        up, low = dt(prior["uplim"][k]), dt(prior["lowlim"][k])
        lw = dt(WALL_REL_WIDTH) * (up - low)
        d = th - up
        with np.errstate(invalid="ignore", over="ignore"):
            lp = np.where(th > up, lp - dt(0.5) * d * d / (lw * lw), lp)
    if prior["has_gprior"][k]:
        d = th - dt(prior["gmean"][k])
        with np.errstate(invalid="ignore", over="ignore"):
            lp = lp + dt(-0.5) * dt(prior["givar"][k]) * d * d
    return lp


def window(chain, burn=0, thin=1):
    """[nw, nsteps, 5] -> the window's entries [n, 5] in [walker][step] order."""
    c = np.asarray(chain)[:, burn::thin]
    return c.reshape(-1, 5)


def entries(rows, cols, transforms, prior, dt):
    """(x [n, d], b [n]) of chain rows [n, 5]; b = -inf marks an entry that is left out (its x is 0)."""
    rows = np.asarray(rows, dtype=np.float64)
    n, d = rows.shape[0], len(cols)
    x = np.zeros((n, d), dtype=dt)
    lnpi = np.zeros(n, dtype=dt)
    ok = np.ones(n, dtype=bool)
    for i, (k, t) in enumerate(zip(cols, transforms)):
        th = rows[:, k].astype(dt)
        good = np.isfinite(rows[:, k]) & ((rows[:, k] > 0) if t == LOG10 else True)
        ok &= good
        ths = np.where(good, th, dt(1))
        if t == LOG10:
            x[:, i] = np.log(ths) / np.log(dt(10))
            lnpi = lnpi + np.log(ths * np.log(dt(10)))
        else:
            x[:, i] = ths
        lnpi = lnpi + prior_factor(ths, k, prior, dt)
    ok &= np.isfinite(lnpi)
    x[~ok] = 0
    b = np.where(ok, -lnpi, dt(-np.inf))
    return x, b


def chol_rows(mu, L):
    """A candidate as the library takes it: (mu, L row by row)."""
    L = np.asarray(L, dtype=np.float64)
    return np.concatenate([np.asarray(mu, dtype=np.float64), L[np.tril_indices(L.shape[0])]])


def bad_candidate(mu, L):
    L = np.asarray(L, dtype=np.float64)
    il = np.tril_indices(L.shape[0])
    return not (np.all(np.isfinite(mu)) and np.all(np.isfinite(L[il])) and np.all(np.diag(L) > 0))


def logdens(x, b, mu, L, dt):
    """a_j = -1/2 |L^-1 (x_j - mu)|^2 - sum ln L_ii - (d / 2) ln 2 pi + b_j by forward substitution."""
    d = x.shape[1]
    mu, L = np.asarray(mu, dtype=dt), np.asarray(L, dtype=dt)
    z = np.zeros(x.shape, dtype=dt)
    q = np.zeros(x.shape[0], dtype=dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(d):
            y = x[:, i] - mu[i]
            for k in range(i):
                y = y - L[i, k] * z[:, k]
            z[:, i] = y / L[i, i]
            q = q + z[:, i] * z[:, i]
        return dt(-0.5) * q - np.sum(np.log(np.diag(L))) - dt(d) / dt(2) * np.log(dt(2) * pi_of(dt)) + b


def source(x, b, mu, L, dt, moments=True):
    """One (candidate, source): dict of lnl_src, ess, mean [d], cov [d, d], n_used, underflow."""
    d = x.shape[1]
    used = b > -np.inf
    n_used = int(used.sum())
    nan = dt(np.nan)
    out = dict(lnl_src=nan, ess=nan, mean=np.full(d, nan), cov=np.full((d, d), nan), n_used=n_used, underflow=False)
    if n_used == 0 or bad_candidate(mu, L):
        return out
    a = logdens(x[used], b[used], mu, L, dt)
    adds = a > -np.inf                               # (NaN and -inf add nothing)
    a, xs = a[adds], x[used][adds]
    if a.size == 0 or a.max() < UNDERFLOW:
        out.update(lnl_src=dt(-np.inf), underflow=True)
        return out
    m = a.max()
    w = np.exp(a - m)
    s = w.sum()
    out["lnl_src"] = m + np.log(s) - np.log(dt(n_used))
    out["ess"] = s * s / (w * w).sum()
    if moments:
        mean = (w[:, None] * xs).sum(axis=0) / s
        dx = xs - mean
        out["mean"] = mean
        out["cov"] = np.einsum("j,ji,jk->ik", w, dx, dx) / s
    return out


def evaluate(xb, cands, dt, moments=True):
    """xb: [(x, b)] per source; cands: [(mu, L)].  Returns dict of lnl [H], n_src_used [H], underflow [H], bad [H] and
    lnl_src, ess [H, nsrc], mean [H, nsrc, d], cov [H, nsrc, d, d]."""
    H, ns, d = len(cands), len(xb), xb[0][0].shape[1]
    out = dict(lnl=np.full(H, np.nan, dtype=dt), n_src_used=np.zeros(H, dtype=np.int32),
               underflow=np.zeros(H, dtype=bool), bad=np.zeros(H, dtype=bool),
               lnl_src=np.full((H, ns), np.nan, dtype=dt), ess=np.full((H, ns), np.nan, dtype=dt),
               mean=np.full((H, ns, d), np.nan, dtype=dt), cov=np.full((H, ns, d, d), np.nan, dtype=dt))
    for h, (mu, L) in enumerate(cands):
        if bad_candidate(mu, L):
            out["bad"][h] = True
            continue
        total, used = dt(0), 0
        for n, (x, b) in enumerate(xb):
            r = source(x, b, mu, L, dt, moments)
            for k in FLOATS:
                out[k][h, n] = r[k]
            if r["n_used"] == 0:
                continue
            out["underflow"][h] |= r["underflow"]
            total = total + r["lnl_src"]
            used += 1
        out["n_src_used"][h] = used
        out["lnl"][h] = total if used else np.nan
    return out


def distance(a, b, keys=FLOATS):
    """The largest |a - b| / max(1, |b|) over the floating-point tables of two evaluate() results (both NaN or equal,
    infinities included: 0; otherwise a value that is not finite on one side: inf)."""
    worst = 0.0
    for k in keys:
        x, y = np.asarray(a[k], dtype=LD), np.asarray(b[k], dtype=LD)
        same = (np.isnan(x) & np.isnan(y)) | (x == y)
        if np.any(~same & ~(np.isfinite(x) & np.isfinite(y))):
            return np.inf
        if np.any(~same):
            worst = max(worst, float(np.max(np.abs(x - y)[~same] / np.maximum(LD(1), np.abs(y[~same])))))
    return worst
