"""The rows that span the prior volume, and the reference of the frequency integral over it.  numpy (and scipy inside
lir_reference) only: nothing here touches the device.

    wide_rows()     the 600 rows of tests/test_gpu_parity.py::test_wide_parameter_ranges_vs_oracle (the same recipe and
                    seed): T 3-200 K, beta 0-4.5 (exactly 0 in the first 8 rows), lambda0 5-3000 um, alpha 0.1-10,
                    fnorm 0.01-1000 mJy
    grid_rows()     the 225 rows of test_table_ends_and_first_rows_vs_oracle: T 1-5000 K x lambda0 1-4500 um x beta
    bad_rows()      six rows no SED can be built from (or, for a model that does not read the column, good rows)
    lir_reference   the integral of f_nu over a wavelength range by scipy's adaptive quad in t = log nu, split at the
                    SED's two kinks, with its own error estimate
    RANGES          the three integration ranges [um]: rest-frame L_IR, the same seen at z = 2.3, and a narrow one
    device_rule     the device's fixed rule (csrc/mbb_kernels.hip.h, sed_integrate_row) restated in numpy
    make_like, make_oracle   the likelihood of either set (built without a device) and the oracle's of what it holds
    huge_rows()     beta, alpha or both at 1e79 to 1e300 in three good rows
    ensemble(name)  the frozen starting ensembles of the sampler tests: wide250, wide576, grid224
    stretch_draws, proposals, accept_margin, emulate   the device sampler's draws, proposal and accept rule in numpy
tests/test_domain_paths_cpu.py asserts what the GPU tests of tests/test_domain_paths_gpu.py rely on,
tests/test_domain_sampler_cpu.py what tests/test_domain_sampler_gpu.py and tests/test_domain_boundary_gpu.py do.
"""
import numpy as np

UM_TO_GHZ = 299792458e-3
WIDE_BANDS = ["PACS_100um", "SPIRE_250um", "SPIRE_500um", "SCUBA2_850um", "GISMO_2mm"]
WIDE_FLUX = np.array([30.0, 60.0, 25.0, 6.0, 0.5])
GRID_BANDS = ["PACS_70um", "PACS_160um", "SPIRE_250um", "SPIRE_500um", "SCUBA2_850um", "Bolocam_1.1mm"]
GRID_FLUX = np.array([20.0, 60.0, 50.0, 25.0, 6.0, 2.0])
Z = 2.3
OPZ = 1.0 + Z
RANGES = [(8.0, 1000.0), (8.0 * OPZ, 1000.0 * OPZ), (42.5, 122.5)]
FLUX_FLOOR = 1e-280                      # below it the oracle's flux is 0 or next to it: no relative error is asked


def unc_of(flux):
    return 0.1 * flux + 0.2


def wide_rows():
    rng = np.random.RandomState(4242)
    n = 600
    pars = np.column_stack([np.exp(rng.uniform(np.log(3), np.log(200), n)), rng.uniform(0.0, 4.5, n),
                            np.exp(rng.uniform(np.log(5), np.log(3000), n)),
                            np.exp(rng.uniform(np.log(0.1), np.log(10), n)),
                            np.exp(rng.uniform(np.log(0.01), np.log(1000), n))])
    pars[:8, 1] = 0.0                                        # beta = 0 exactly
    return np.ascontiguousarray(pars)


def grid_rows():
    Ts = np.array([1.0, 1.2, 1.5, 2.0, 2.5, 3.0, 3.2, 3.6, 4.0, 5.0, 8.0, 150.0, 300.0, 1000.0, 5000.0])
    l0s = np.array([1.0, 30.0, 600.0, 3000.0, 4500.0])
    betas = np.array([0.5, 1.8, 3.5])
    T, L0, B = (x.ravel() for x in np.meshgrid(Ts, l0s, betas, indexing="ij"))
    n = T.size
    return np.ascontiguousarray(np.column_stack([T, B, L0, np.full(n, 2.5), np.full(n, 40.0)]))


# (what is wrong, the column it is wrong in): a model that does not read the column takes the row as a good one
BAD = [("NaN T", 0), ("infinite fnorm", 4), ("alpha = -1", 3), ("alpha = 0", 3), ("T = 0", 0), ("NaN beta", 1)]
BAD_AT = (0, 63, 64, 255, 256, 605)     # where they stand among the 606 rows of with_bad_rows()


def bad_rows():
    good = np.array([25.0, 1.7, 180.0, 2.2, 35.0])
    rows = np.tile(good, (6, 1))
    rows[0, 0] = np.nan
    rows[1, 4] = np.inf
    rows[2, 3] = -1.0
    rows[3, 3] = 0.0
    rows[4, 0] = 0.0
    rows[5, 1] = np.nan
    return rows


def with_bad_rows():
    """(the 606 rows: the wide rows with the six bad ones at BAD_AT; the positions of the wide rows among them)"""
    wide, bad = wide_rows(), bad_rows()
    n = wide.shape[0] + bad.shape[0]
    assert BAD_AT[-1] == n - 1
    is_bad = np.zeros(n, dtype=bool)
    is_bad[list(BAD_AT)] = True
    rows = np.empty((n, 5))
    rows[is_bad] = bad
    rows[~is_bad] = wide
    return rows, np.flatnonzero(~is_bad)


# ---------------------------------------------------------------- the boundary call and the sampler forms
LOWLIM = np.array([1.0, 0.1, 1.0, 0.1, 1e-3])     # the likelihood's default lower limits: a row below one has lnprob -inf
PEAK_PRIOR = (120.0, 40.0)                         # the lambda_peak Gaussian prior of the wide test: (mean, sigma)
GRID_LAMBDA0_UPLIM = 5000.0
HUGE = (1e79, 1e80, 1e81, 1e100, 1e300)
SOURCE_SCALES = (1.0, 0.3, 4.0)                    # the multi-source call's three sources: WIDE_FLUX (GRID_FLUX) times these
SEED = 77
STEPS = (8, 3, 2)                                  # stored, then unstored, then stored again
GOLDEN_GAMMA = 0x9E3779B97F4A7C15                  # the step's number times this is added to the seed: the step's key


def make_like(mbb, which, opthin, noalpha, cov=None, prior=None, scale=1.0):
    """The likelihood of the wide test's five bands or of the grid test's six (`which` wide or grid), response=True,
    the data of those tests: the grid with lambda0's upper limit at 5000 um, the wide set with the lambda_peak prior
    unless `prior` says otherwise; `cov` a full covariance or None; `scale` times the fluxes (and unc_of those).  No device
    is touched until it is evaluated."""
    names, flux = (GRID_BANDS, GRID_FLUX * scale) if which == "grid" else (WIDE_BANDS, WIDE_FLUX * scale)
    like = mbb.likelihood(opthin=opthin, noalpha=noalpha, response=True)
    like.set_phot(names, flux, unc_of(flux))
    if which == "grid":
        like.set_uplim("lambda0", GRID_LAMBDA0_UPLIM)                  # (3 x max wavelength would cut the grid short)
    if which != "grid" if prior is None else prior:
        like.set_gaussian_prior("lambda_peak", *PEAK_PRIOR)
    if cov is not None:
        like.set_cov(cov)
    return like


def make_oracle(oracle, like, flux=None):
    """The oracle's likelihood of what `like` holds: its passband tables, limits, priors and covariance; `flux` another
    source's data through the same bands (with unc_of its uncertainties; diagonal only)."""
    bands = [(r.wavelength, r._sedmult, r._normfac) for r in like._responses]
    has_g = [int(b) for b in like._has_gprior]
    kw = dict(bands=bands, opthin=like.opthin, noalpha=like.noalpha, wavenorm=like.wavenorm, lowlim=like.lowlims,
              has_uplim=[int(b) for b in like.has_uplims], uplim=like.uplims, has_gprior=has_g,
              gprior_mean=list(like._gprior_mean), gprior_sigma=[s if h else 1.0 for s, h in zip(like._gprior_sigma, has_g)])
    if flux is not None:
        return oracle.OracleLikelihood(flux, unc_of(flux), **kw)
    cov = like._covmatrix if like._has_covmatrix else None
    return oracle.OracleLikelihood(like._flux, like._flux_unc, cov=cov, **kw)


# Good rows to put the huge exponents into.  What (x_norm / x0)^beta = (lambda0 / wavenorm)^beta does at the normalisation
# decides whether an optically thick SED with such a beta can be built at all: 0 below the normalisation wavelength of
# 500 um (no SED: the normalisation divides by it), infinite above it (a SED: 1 - e^-y is 1 there, and the optical-depth
# factor a step at lambda0).  The optically thin normalisation has x_norm^-(3 + beta), x_norm = 28.78 K / T: both sides
# of T = 28.78 K.  So: lambda0 on both sides of 500 um, T on both sides of 28.78 K.
HUGE_BASE = np.array([[25.0, 1.7, 180.0, 2.2, 35.0], [25.0, 1.7, 600.0, 2.2, 35.0], [40.0, 1.7, 600.0, 2.2, 35.0]])


def huge_rows():
    """Each row of HUGE_BASE with beta, alpha, or both at each of HUGE: 45 rows, and what was set in each."""
    rows, what = [], []
    for good in HUGE_BASE:
        for v in HUGE:
            for name, cols in (("beta", [1]), ("alpha", [3]), ("beta and alpha", [1, 3])):
                r = good.copy()
                r[cols] = v
                rows.append(r)
                what.append("T %g, lambda0 %g: %s = %g" % (good[0], good[2], name, v))
    return np.ascontiguousarray(rows), what


def wide_finite(n):
    """The first n wide rows at or above every lower limit: the rows whose lnprob is finite, whatever the model (the
    gate reads all five columns; tests/test_domain_sampler_cpu.py asserts that the oracle agrees, model by model)."""
    rows = wide_rows()
    keep = np.flatnonzero(~(rows < LOWLIM).any(axis=1))
    assert keep.size >= n, (keep.size, n)
    return np.ascontiguousarray(rows[keep[:n]])


def ensemble(name):
    """The frozen starting ensembles of the sampler tests: `wide250`, `wide576`, `grid224`."""
    if name.startswith("wide"):
        return wide_finite(int(name[4:]))
    assert name == "grid224"
    return np.ascontiguousarray(grid_rows()[:224])


def zpow_of(p0):
    """The exponent of z in the accept test: the columns the ensemble spans, less one (a column that is constant over
    the ensemble stays so exactly under the stretch move and does not count: mbb_sampler_set_state).  4 for the wide
    ensembles, 2 for the grid's, whose alpha and fnorm are one value each."""
    return float(max(int(np.count_nonzero(np.ptp(p0, axis=0) != 0.0)) - 1, 0))


_DRAWS = {}


def stretch_draws(seed, step_no, nw, a=2.0):
    """What the device draws for step number `step_no` of the sampler's life (1 for the first step) -- csrc/mbb_stretch.hip.h
    restated with the arithmetic of tests/test_gpu_parity.py::_host_stretch_step --: for each half (0: the first half moves)
    z [half], the partner's index in the other half [half], ln u [half].  The draws do not depend on the model: made once."""
    key = (int(seed), int(step_no), int(nw), float(a))
    if key not in _DRAWS:
        from test_gpu_parity import _philox4x32
        half = nw // 2
        k = (seed + GOLDEN_GAMMA * step_no) & 0xFFFFFFFFFFFFFFFF
        out = []
        for h in range(2):
            s_begin = half if h else 0
            zz, pj, lu = np.empty(half), np.empty(half, dtype=np.int64), np.empty(half)
            for w in range(half):
                r = _philox4x32([s_begin + w, h, 0, 0], k & 0xFFFFFFFF, k >> 32)
                u1 = ((r[0] >> 5) * 67108864.0 + (r[1] >> 6)) / 9007199254740992.0
                u2 = r[2] / 4294967296.0
                u3 = (r[3] + 0.5) / 4294967296.0
                zz[w] = ((a - 1.0) * u1 + 1.0) ** 2 / a
                pj[w] = min(int(u2 * half), half - 1)
                lu[w] = np.log(u3)
            for x in (zz, pj, lu):
                x.setflags(write=False)
            out.append((zz, pj, lu))
        _DRAWS[key] = out
    return _DRAWS[key]


def proposals(prev, now_first, seed, step_no):
    """The stretch move's proposals of one step from positions that are given, not emulated: `prev` [nw, 5] the ensemble
    before the step, `now_first` [nw / 2, 5] its first half after the step's first half-step (the second half draws its
    partners there).  With the device's one rounding: it forms fma(-z, c - s, c), so c - s is rounded to double and the
    product and the sum are carried in long double (two roundings in double are 1.7e-13 off where c and z (c - s) nearly
    cancel).  Returns (q [nw, 5], z [nw], ln u [nw])."""
    nw = prev.shape[0]
    half = nw // 2
    LD = np.longdouble
    (z0, j0, u0), (z1, j1, u1) = stretch_draws(seed, step_no, nw)
    q = np.empty((nw, 5))
    for mine, c, z in ((slice(0, half), prev[half + j0], z0), (slice(half, nw), now_first[j1], z1)):
        d = c - prev[mine]
        q[mine] = (c.astype(LD) - z[:, None].astype(LD) * d.astype(LD)).astype(np.float64)
    return q, np.concatenate([z0, z1]), np.concatenate([u0, u1])


def accept_margin(zpow, z, lnu, new, old):
    """(m, decidable): m = zpow ln z + new - old - ln u, the move is made iff m > 0; decidable where |m| exceeds
    2e-10 (max(1, |new|) + max(1, |old|)), twice the bound lnprob is held to on each side.  A proposal at -inf is
    decidable: it is rejected."""
    with np.errstate(invalid="ignore"):
        m = zpow * np.log(z) + new - old - lnu
        tol = 2e-10 * (np.maximum(1.0, np.abs(new)) + np.maximum(1.0, np.abs(old)))
        decidable = np.isneginf(new) | (np.abs(m) > tol)
    return m, decidable


def emulate(lnprob, p0, seed, nsteps, steps_done=0):
    """The stretch-move sampler on the host with the device's draws and `lnprob` (rows -> values) as the likelihood.
    Returns the chain [nw, nsteps, 5], its lnprob [nw, nsteps], which moves were made [nw, nsteps] and which of them
    were decidable [nw, nsteps]."""
    nw = p0.shape[0]
    half = nw // 2
    zpow = zpow_of(p0)
    pos, lnp = p0.copy(), lnprob(p0)
    assert np.all(np.isfinite(lnp))
    chain, lnps = np.empty((nw, nsteps, 5)), np.empty((nw, nsteps))
    moved, decid = np.zeros((nw, nsteps), dtype=bool), np.zeros((nw, nsteps), dtype=bool)
    for t in range(nsteps):
        draws = stretch_draws(seed, steps_done + t + 1, nw)
        for h, (zz, pj, lu) in enumerate(draws):
            mine = slice(half, nw) if h else slice(0, half)
            c = pos[(0 if h else half) + pj]
            q = c - zz[:, None] * (c - pos[mine])
            new = lnprob(q)
            assert not np.isnan(new).any(), q[np.isnan(new)]
            m, d = accept_margin(zpow, zz, lu, new, lnp[mine])
            acc = m > 0
            pos[mine] = np.where(acc[:, None], q, pos[mine])
            lnp[mine] = np.where(acc, new, lnp[mine])
            moved[mine, t], decid[mine, t] = acc, d
        chain[:, t], lnps[:, t] = pos, lnp
    return chain, lnps, moved, decid


def lir_rows():
    """Every fifth wide row and every grid row: the rows the frequency integral is checked on."""
    return wide_rows()[::5], grid_rows()


def breaks_um(sed, opthin, noalpha, lambda0):
    """(merge wavelength or None, lambda0 or None): where f_nu has its kinks."""
    return (None if noalpha else sed.wavemerge), (None if opthin else float(lambda0))


def _pieces(sed, lo_um, hi_um, opthin, noalpha, lambda0):
    """The range in t = log nu [GHz], cut at the kinks that lie strictly inside it."""
    lo_um, hi_um = min(lo_um, hi_um), max(lo_um, hi_um)
    t0, t1 = np.log(UM_TO_GHZ / hi_um), np.log(UM_TO_GHZ / lo_um)
    cuts = [np.log(UM_TO_GHZ / w) for w in breaks_um(sed, opthin, noalpha, lambda0) if w is not None]
    return [t0] + sorted(t for t in cuts if t0 < t < t1) + [t1]


def lir_reference(sed, lo_um, hi_um, opthin, noalpha, lambda0):
    """(value, error estimate) of the integral of f_nu d nu over [lo_um, hi_um] in mJy GHz: scipy's quad of
    f_nu(e^t) e^t in t = log nu, piece by piece between the merge frequency (f_nu is only C1 there) and c / lambda0
    (for large beta the optical-depth factor is nearly a step there)."""
    import ctypes as C
    from scipy.integrate import quad
    from oracle import oracle as O
    fn, s = O.lib().mbbo_fnu, C.byref(sed.s)
    x, y = np.empty(1), np.empty(1)
    px, py = O._d(x), O._d(y)

    def g(t):
        nu = np.exp(t)
        x[0] = nu
        fn(s, px, 1, py)
        return y[0] * nu

    edge = _pieces(sed, lo_um, hi_um, opthin, noalpha, lambda0)
    val = err = 0.0
    for a, b in zip(edge[:-1], edge[1:]):
        v, e = quad(g, a, b, epsrel=1e-13, epsabs=0, limit=500)
        val += v
        err += e
    return val, err


_TABLES = {}


def lir_table(oracle, opthin, noalpha):
    """lir_reference of lir_rows() (wide first, then grid) over RANGES for one model: (values, error estimates), each
    [rows, 3]; made once per session and shared read-only.  An integration warning is an error."""
    import warnings
    key = (bool(opthin), bool(noalpha))
    if key not in _TABLES:
        rows = np.concatenate(lir_rows())
        val, err = np.empty((rows.shape[0], len(RANGES))), np.empty((rows.shape[0], len(RANGES)))
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            for i, p in enumerate(rows):
                sed = oracle.OracleSED(*p, opthin=opthin, noalpha=noalpha)
                for j, (lo, hi) in enumerate(RANGES):
                    val[i, j], err[i, j] = lir_reference(sed, lo, hi, opthin, noalpha, p[2])
        val.setflags(write=False)
        err.setflags(write=False)
        _TABLES[key] = (val, err)
    return _TABLES[key]


_GL = {}


def device_rule(sed, lo_um, hi_um, opthin, noalpha, lambda0, npanel=8, ngl=64):
    """sed_integrate_row restated: t0, t1 = log of the bounds; tm = the merge point clamped into [t0, t1] (t1 without
    alpha), tz = log nu0 clamped into [t0, tm] (t0 for the optically thin model); the pieces [t0, tz], [tz, tm],
    [tm, t1] that are not empty, each in npanel panels of an ngl-point Gauss-Legendre rule; fed the oracle's f_nu."""
    if ngl not in _GL:
        _GL[ngl] = np.polynomial.legendre.leggauss(ngl)
    gx, gw = _GL[ngl]
    lo_um, hi_um = min(lo_um, hi_um), max(lo_um, hi_um)
    t0, t1 = np.log(UM_TO_GHZ / hi_um), np.log(UM_TO_GHZ / lo_um)
    wm, w0 = breaks_um(sed, opthin, noalpha, lambda0)
    tm = t1 if wm is None else min(max(np.log(UM_TO_GHZ / wm), t0), t1)
    tz = t0 if w0 is None else min(max(np.log(UM_TO_GHZ / w0), t0), tm)
    edge = [t0, tz, tm, t1]
    ts, ws = [], []
    for a, b in zip(edge[:-1], edge[1:]):
        if not b > a:
            continue
        pw = (b - a) / npanel
        mid = a + (np.arange(npanel) + 0.5) * pw
        ts.append((mid[:, None] + 0.5 * pw * gx[None, :]).ravel())
        ws.append(np.tile(0.5 * pw * gw, npanel))
    t, w = np.concatenate(ts), np.concatenate(ws)
    nu = np.exp(t)
    return float(np.sum(sed.f_nu(nu) * nu * w))
