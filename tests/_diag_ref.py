"""References of the chain diagnostics (mbb_diag.hip.h): direct sums in numpy.longdouble of exactly the definitions in
include/mbb_hip.h -- no FFT, so their own rounding is negligible beside the bounds -- and the synthetic chains the CPU
and GPU tests share.

    rho_k = c_k / c_0,  c_k = sum_{i < n - k} y_i y_{i+k},  y the series minus its mean
    tau(m) = 2 sum_{k <= m} rho_k - 1;  M the first m with m >= c tau(m), else n - 1;  tau = tau(M)
"""
import functools

import numpy as np

LD = np.longdouble
SHORT, CONSTANT, HAS_NAN, UNRELIABLE = 1, 2, 4, 8
EPS = float(np.finfo(np.float64).eps)


def _rho_block(y, c0, k0, k1):
    n = y.size
    return np.array([np.sum(y[:n - k] * y[k:]) / c0 if k < n else LD(0) for k in range(k0, k1)], dtype=LD)


def _series_state(x):
    """(flag, y, c0) of one series: flag HAS_NAN / CONSTANT / 0."""
    if not np.all(np.isfinite(x)):
        return HAS_NAN, None, None
    y = x - np.sum(x) / LD(x.size)
    c0 = np.sum(y * y)
    if np.all(x == x[0]) or not c0 > 0:
        return CONSTANT, None, None
    return 0, y, c0


def tau_ref(series, c=5.0, nacf=0):
    """series [nser, n] (longdouble): the rho_k of every series averaged, windowed once.
    -> dict(tau, window, status, rho (the lags computed: at least 0 .. max(M, nacf - 1)), taus)"""
    series = np.asarray(series, dtype=LD)
    nser, n = series.shape
    if n < 8:
        return dict(tau=np.nan, window=-1, status=SHORT, rho=np.full(nacf, np.nan), taus=np.zeros(0))
    states = [_series_state(s) for s in series]
    status = 0
    for f, _, _ in states:
        status |= f
    if status:
        return dict(tau=np.nan, window=-1, status=status, rho=np.full(nacf, np.nan), taus=np.zeros(0))
    rho = np.zeros(0, dtype=LD)
    M, csum, taus = -1, LD(0), []
    k0 = 0
    while k0 < n and (M < 0 or k0 < nacf):
        k1 = min(n, k0 + 64)
        blk = sum(_rho_block(y, c0, k0, k1) for _, y, c0 in states) / LD(nser)
        rho = np.concatenate((rho, blk))
        if M < 0:
            for k in range(k0, k1):
                csum += rho[k]
                t = 2 * csum - 1
                taus.append(t)
                if k >= LD(c) * t:
                    M = k
                    break
        k0 = k1
    if M < 0:
        M = n - 1
    taus = np.array(taus[:M + 1], dtype=LD)
    return dict(tau=taus[M], window=M, status=0, rho=rho, taus=taus)


def rhat_ref(x):
    """Split R-hat of x [nw, n] (longdouble)."""
    x = np.asarray(x, dtype=LD)
    nw, n = x.shape
    h = n // 2
    if h < 2:
        return np.nan, np.nan
    seqs = np.concatenate((x[:, :h], x[:, n - h:]), axis=0)
    means = np.sum(seqs, axis=1) / LD(h)
    var = np.sum((seqs - means[:, None]) ** 2, axis=1) / LD(h - 1)
    W = np.sum(var) / LD(2 * nw)
    mm = np.sum(means) / LD(2 * nw)
    B = LD(h) * np.sum((means - mm) ** 2) / LD(2 * nw - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt((LD(h - 1) / LD(h) * W + B / LD(h)) / W), W


def _xfac(x):
    """1 + mean|x| / sigma of a series"""
    x = np.asarray(x, dtype=np.float64)
    s = x.std()
    return 1.0 + (np.abs(x).mean() / s if s > 0 else 0.0)


def diagnostics_ref(chain, burn=0, c=5.0, tol=50.0, method="mean", nacf=0):
    """Everything mbb_chain_diagnostics returns for one source's chain [nw, nsteps, 5], with the derived bounds of
    the issue beside it: rho_bound = 16 (log2(n nw) + 2) eps (1 + mean|x| / sigma), tau_bound = 2 (M + 1) rho_bound,
    rhat_rbound = the rho bound with sigma = sqrt(W)."""
    chain = np.asarray(chain, dtype=np.float64)
    nw, nsteps, _ = chain.shape
    n = nsteps - burn
    out = dict(tau=np.empty(5), window=np.empty(5, dtype=np.int32), ess=np.empty(5), rhat=np.empty(5),
               status=np.empty(5, dtype=np.int32), acf=np.full((5, nacf), np.nan), margin=np.full(5, np.inf),
               rho_bound=np.zeros(5), tau_bound=np.zeros(5), rhat_rbound=np.zeros(5), rho=[None] * 5)
    for p in range(5):
        x = chain[:, burn:, p].astype(LD)
        with np.errstate(invalid="ignore"):
            series = (np.sum(x, axis=0) / LD(nw))[None] if method == "mean" else x
            r = tau_ref(series, c, nacf)
        st = r["status"]
        tau = r["tau"]
        if st == 0 and n < tol * tau:
            st |= UNRELIABLE
        out["tau"][p], out["window"][p], out["status"][p] = tau, r["window"], st
        out["ess"][p] = nw * n / tau if r["status"] == 0 else np.nan
        out["acf"][p] = np.asarray(r["rho"][:nacf], dtype=np.float64) if nacf else out["acf"][p]
        out["rho"][p] = r["rho"]
        with np.errstate(invalid="ignore"):
            rh, W = rhat_ref(x)
        out["rhat"][p] = rh
        lg = 16.0 * (np.log2(n * nw) + 2.0) * EPS
        if r["status"] == 0:
            out["margin"][p] = float(np.min(np.abs(np.arange(r["window"] + 1) - LD(c) * r["taus"])))
            out["rho_bound"][p] = lg * max(_xfac(s) for s in np.asarray(series, dtype=np.float64))
            out["tau_bound"][p] = 2.0 * (r["window"] + 1) * out["rho_bound"][p]
        if np.isfinite(rh) and W > 0:
            xs = chain[:, burn:, p]
            out["rhat_rbound"][p] = lg * (1.0 + np.abs(xs).mean() / float(np.sqrt(W)))
    return out


# ---- the synthetic chains --------------------------------------------------------------------------------------
def ar1(rng, nw, n, phi):
    """Stationary AR(1) series of unit variance, one per walker: [nw, n]"""
    e = rng.standard_normal((nw, n))
    x = np.empty((nw, n))
    x[:, 0] = e[:, 0]
    s = np.sqrt(1.0 - phi * phi)
    for t in range(1, n):
        x[:, t] = phi * x[:, t - 1] + s * e[:, t]
    return x


PHIS = (0.5, 0.8, 0.3, 0.9, 0.65)
MUS = (30.0, 1.8, 2500.0, 4.0, -40.0)
SIGMAS = (2.0, 0.2, 100.0, 0.3, 5.0)


def ar1_chain(seed, nw, nsteps, phis=PHIS, mus=MUS, sigmas=SIGMAS):
    """[nw, nsteps, 5]: per-walker AR(1) series mu + sigma x with another phi, mu and sigma per parameter."""
    rng = np.random.default_rng(seed)
    ch = np.empty((nw, nsteps, 5))
    for p in range(5):
        ch[:, :, p] = mus[p] + sigmas[p] * ar1(rng, nw, nsteps, phis[p])
    return ch


def ramp_chain(seed, nw=10, nsteps=100):
    """A ramp plus small noise: the chain has not forgotten where it started (M ~ 73 of 100 steps)."""
    rng = np.random.default_rng(seed)
    t = np.arange(nsteps, dtype=np.float64)
    ch = np.empty((nw, nsteps, 5))
    for p in range(5):
        ch[:, :, p] = MUS[p] + SIGMAS[p] * (0.05 * (p + 1) * t[None, :] + 0.1 * rng.standard_normal((nw, nsteps)))
    return ch


# The lag block of k_diag_acf is 256: chains whose window (parameter 0, method "mean") is the last lag of the first
# block and the first lag of the second.  phi and seeds found on the CPU (tests/test_diagnostics_cpu.py checks them).
SEAM_PHI = 0.962
SEAM_NSTEPS = 1500
SEAM_SEEDS = {255: 1011, 256: 1167}


def seam_chain(M):
    return ar1_chain(SEAM_SEEDS[M], 1, SEAM_NSTEPS, phis=(SEAM_PHI, 0.5, 0.8, 0.3, 0.9))


def _src3():
    return np.stack([ar1_chain(300 + s, 10, 300, phis=tuple(np.roll((0.2, 0.5, 0.7, 0.85, 0.93), s)),
                               mus=tuple(m * (1 + s) for m in MUS)) for s in range(3)])


def _const_column():
    ch = ar1_chain(12, 7, 257)
    ch[:, :, 3] = 4.0
    return ch


def _const_walker():
    ch = ar1_chain(13, 7, 257)
    ch[4, :, 2] = 2500.0
    return ch


def _nan(step):
    ch = ar1_chain(14, 10, 120)
    ch[3, step, 1] = np.nan
    return ch


# name -> (builder of the chain [nw, nsteps, 5] or [nsrc, nw, nsteps, 5], keywords of the call)
CASES = {
    "n7": (lambda: ar1_chain(1, 10, 7), {}),
    "n8": (lambda: ar1_chain(2, 10, 8), {}),
    "n257": (lambda: ar1_chain(3, 7, 257), {}),
    "n257_walkers": (lambda: ar1_chain(3, 7, 257), dict(method="walkers")),
    "n1000": (lambda: ar1_chain(4, 34, 1000), {}),
    "n1000_walkers_nacf_beyond_M": (lambda: ar1_chain(4, 34, 1000), dict(method="walkers", nacf=300)),
    "n1000_nacf_beyond_M": (lambda: ar1_chain(4, 34, 1000), dict(nacf=300)),
    "seam_255": (lambda: seam_chain(255), dict(nacf=8)),
    "seam_256": (lambda: seam_chain(256), dict(nacf=8)),
    "ramp": (lambda: ramp_chain(5), dict(nacf=100)),
    "ramp_walkers": (lambda: ramp_chain(5), dict(method="walkers")),
    "nw250": (lambda: ar1_chain(6, 250, 64), dict(nacf=4)),
    "nw250_walkers": (lambda: ar1_chain(6, 250, 64), dict(method="walkers")),
    "nw1_walkers": (lambda: ar1_chain(7, 1, 257), dict(method="walkers", nacf=16)),
    "nsrc3": (_src3, dict(nacf=32)),
    "nsrc3_walkers": (_src3, dict(method="walkers")),
    "burn_n_odd": (lambda: ar1_chain(8, 10, 120), dict(burn=19, nacf=5)),
    "burn_n_odd_walkers": (lambda: ar1_chain(8, 10, 120), dict(burn=19, method="walkers")),
    "constant_column": (_const_column, dict(nacf=3)),
    "constant_column_walkers": (_const_column, dict(method="walkers")),
    "one_constant_walker": (_const_walker, dict(method="walkers", nacf=3)),
    "one_constant_walker_mean": (_const_walker, {}),
    "NaN_inside_the_window": (lambda: _nan(40), dict(burn=19, nacf=2)),
    "NaN_inside_the_window_walkers": (lambda: _nan(40), dict(burn=19, method="walkers")),
    "NaN_outside_the_window": (lambda: _nan(7), dict(burn=19)),
    "c_3_tol_10": (lambda: ar1_chain(9, 10, 300), dict(c=3.0, tol=10.0)),
    "longest": (lambda: ar1_chain(10, 2, 16384, phis=(0.9, 0.5, 0.8, 0.3, 0.65)), dict(nacf=260)),
    "longest_walkers": (lambda: ar1_chain(10, 2, 16384, phis=(0.9, 0.5, 0.8, 0.3, 0.65)), dict(method="walkers")),
}


@functools.lru_cache(maxsize=None)
def case_chain(name):
    ch = CASES[name][0]()
    ch.setflags(write=False)
    return ch


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """The reference of a case, one dict per source (computed once, shared)."""
    ch, kw = case_chain(name), CASES[name][1]
    c4 = ch if ch.ndim == 4 else ch[None]
    return tuple(diagnostics_ref(c, **kw) for c in c4)
