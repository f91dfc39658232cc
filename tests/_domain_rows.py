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
tests/test_domain_paths_cpu.py asserts what the GPU tests of tests/test_domain_paths_gpu.py rely on.
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
