"""What the out-of-sample-fit GPU tests share (tests/test_loo_gpu.py, tests/test_loo_seams_gpu.py): the likelihood of a
band case, chains made of the fixture chains' rows, the longdouble reference of a chain's tables fed the device's own
ll, and the comparisons of a device result with it or with another device result."""
import numpy as np

from conftest import golden_bands
import _loo_ref as LR

LD = LR.LD
VARIANTS = [("thin_walpha", True, False), ("thick_walpha", False, False),
            ("thick_noalpha", False, True), ("thin_noalpha", True, True)]
BANDS4 = ["PACS_160um", "SPIRE_250um", "SPIRE_500um", "SCUBA2_850um"]
DELTA = [250.0, 500.0, 850.0]
TABLES = ("n_used", "tail_len", "status") + LR.FLOATS
_CACHE = {}


def _same_bits(a, b):
    return all(np.array_equal(getattr(a._raw, f), getattr(b._raw, f), equal_nan=True) for f in TABLES)


def _data(oracle, g_lnl, g_pb, chain, opthin, noalpha, case, scale=1.0):
    """The data of a band case, without a device: the oracle's model at the chain's middle row, pushed 5% up and down
    band by band, with uncertainties scale (0.1 flux + 1); cov12 gives them cfg4's correlations, cov65 is 65 delta
    bands with correlation 0.3^|i-j|.  Returns (the oracle's band keywords, what set_phot takes first, flux, unc,
    cov or None)."""
    if case.startswith("delta") or case == "cov65":
        first = DELTA[:int(case[5:])] if case.startswith("delta") else list(np.linspace(100.0, 900.0, 65))
        okw = dict(wave=first)
    else:
        first = BANDS4 if case == "bands4" else [str(b) for b in g_lnl["cfg4/bands"]]
        okw = dict(bands=golden_bands(g_pb, first))
    nb = len(first)
    free = dict(opthin=opthin, noalpha=noalpha, lowlim=np.full(5, -np.inf), has_uplim=[0] * 6)
    rows = np.asarray(chain).reshape(-1, 5)
    truth = rows[rows.shape[0] // 2]
    model = oracle.OracleLikelihood(np.ones(nb), np.ones(nb), **okw, **free)(truth, return_flux=True)[1][0]
    flux = model * (1.0 + 0.05 * (-1.0) ** np.arange(nb))
    unc = scale * (0.1 * flux + 1.0)
    cov = None
    if case == "cov12":
        c4 = g_lnl["cfg4/thick_walpha/cov"]
        d = np.sqrt(np.diag(c4))
        cov = (c4 / d[:, None] / d[None, :]) * unc[:, None] * unc[None, :]
    if case == "cov65":
        idx = np.arange(nb)
        cov = 0.3 ** np.abs(idx[:, None] - idx[None, :]) * unc[:, None] * unc[None, :]
    return okw, first, flux, unc, cov


def _setup(mbb, oracle, g_lnl, g_pb, chain, opthin, noalpha, case, scale=1.0):
    """A likelihood of a band case on the device, holding _data's photometry."""
    key = ("setup", opthin, noalpha, case, scale)
    if key in _CACHE:
        return _CACHE[key]
    okw, first, flux, unc, cov = _data(oracle, g_lnl, g_pb, chain, opthin, noalpha, case, scale)
    like = mbb.likelihood(response="bands" in okw, opthin=opthin, noalpha=noalpha)
    like.set_phot(first, flux, unc)
    if cov is not None:
        like.set_cov(cov)
    _CACHE[key] = like
    return like


def _weights(like):
    return dict(invcov=like._invcovmatrix) if like._has_covmatrix else dict(ivar=like._ivar)


def _chain(g_res, name, shape, seed=1):
    """A chain of the given [nsrc, nw, nsteps] whose rows are the fixture chain's, a third of them repeats of the row
    before, as rejected stretch moves leave them."""
    rows = g_res[name + "/chain"].reshape(-1, 5)
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    pick = rng.randint(0, rows.shape[0], n)
    out = rows[pick] * (1.0 + 1e-3 * rng.standard_normal((n, 5)))
    out = out.reshape(shape[0] * shape[1], shape[2], 5)
    rep = rng.uniform(size=out.shape[:2]) < 1.0 / 3.0
    for t in range(1, shape[2]):
        out[rep[:, t], t] = out[rep[:, t], t - 1]
    return np.ascontiguousarray(out.reshape(tuple(shape) + (5,)))


# The one-band (delta1, thick_walpha, scale 1) windows of tests/test_loo_seams_gpu.py, which tests/test_loo_seams_cpu.py
# checks beforehand without a device: label -> ([1, nw, nsteps], _chain's seed, NaN rows planted, S, M, splits, P).
# 16 385 = 113 x 145, 116 508 = 228 x 511, 116 509 = 263 x 443 and 1 864 135 = 455 x 4097 factor as they are, so only the
# last case plants NaN rows.
SEAM_DELTA1 = {
    "S 16384": ((1, 128, 128), 101, 0, 16384, 384, 1, 512),
    "S 16385": ((1, 113, 145), 102, 0, 16385, 385, 2, 512),
    "S 116508": ((1, 228, 511), 103, 0, 116508, 1024, 8, 1024),
    "S 116509": ((1, 263, 443), 104, 0, 116509, 1025, 8, 2048),
    "S max": ((1, 455, 4097), 105, 0, 1864135, 4096, 64, 4096),
    "S max, 1000 NaN": ((1, 455, 4097), 105, 1000, 1863135, 4095, 64, 4096),
}
NDTR_ABOVE = 20000        # windows longer than this take Phi from scipy.special.ndtr in float64 instead of mpmath


def _seam_nan_rows(shape, nan):
    """Where the NaN rows of a SEAM_DELTA1 case stand among the nw * nsteps rows of its source: evenly, both ends."""
    return np.linspace(0, shape[1] * shape[2] - 1, nan).astype(np.int64)


def _ndtr_error(z):
    """The largest absolute error of scipy.special.ndtr in float64 against mpmath on 2000 of the finite z, taken evenly
    through the sorted values, both ends included."""
    from scipy.special import ndtr
    zs = np.sort(z[np.isfinite(z)])
    pick = zs[np.unique(np.round(np.linspace(0, zs.size - 1, 2000)).astype(np.int64))]
    return float(np.max(np.abs(ndtr(pick).astype(LD) - LR.norm_cdf_mp(pick))))


def _columns(ll, z, ndtr=None):
    """_loo_ref.column of every band of one source's window in longdouble and in float64 on the same ll [n, nb] and
    z [n, nb]: (longdouble results, float64 results).  Phi is mpmath's up to NDTR_ABOVE entries; above it (or where
    the caller says so) scipy's ndtr in float64 for both, whose error the caller measures with _ndtr_error and adds to
    loo_pit's bound."""
    if ndtr is None:
        ndtr = ll.shape[0] > NDTR_ABOVE
    ref, f64 = [], []
    for b in range(ll.shape[1]):
        ok = np.isfinite(ll[:, b])
        if ndtr:
            from scipy.special import ndtr as scipy_ndtr
            phi = scipy_ndtr(z[ok, b])
        else:
            phi = LR.norm_cdf_mp(z[ok, b])
        ref.append(LR.column(ll[:, b], z[:, b], dtype=LD, phi=phi.astype(LD)))
        f64.append(LR.column(ll[:, b], z[:, b], dtype=np.float64, phi=phi.astype(np.float64)))
    return ref, f64


def _distances(got, r):
    """(_loo_ref.distance over the tables but loo_pit, loo_pit's own) of two column() results"""
    rest = dict(got)
    rest["loo_pit"] = r["loo_pit"]
    only = dict(r)
    only["loo_pit"] = got["loo_pit"]
    return LR.distance(rest, r), LR.distance(only, r)


def _groups(nb, cells, mb):
    """pw_run's band groups, restated: group = max(1, min(nb, budget / (16 cells))) bands, two float64 columns each"""
    group = max(1, min(nb, (mb << 20) // (16 * cells)))
    return [min(group, nb - b0) for b0 in range(0, nb, group)]


def _selects(ng):
    """... and the select launches of a group of ng bands, kSelCols = 3 at a time: the nbat of sel_of()"""
    return [min(3, ng - 3 * q) for q in range((ng + 2) // 3)]


def _oracle_ll_and_z(oracle, data, rows, opthin, noalpha):
    """_ll_and_z without a device: ll and z in longdouble from the oracle's band fluxes of the rows, rounded to float64
    (data: what _data returned)."""
    okw, first, flux, unc, cov = data
    free = dict(opthin=opthin, noalpha=noalpha, lowlim=np.full(5, -np.inf), has_uplim=[0] * 6)
    model = oracle.OracleLikelihood(flux, unc, **okw, **free)(rows, return_flux=True)[1]
    w = dict(invcov=np.linalg.inv(cov)) if cov is not None else dict(ivar=1.0 / unc ** 2)
    ll, g, d = LR.ll_rows(flux, model, **w)
    return ll.astype(np.float64), (g / np.sqrt(d)[None, :]).astype(np.float64)


def _ll_and_z(like, rows):
    """The device's own ll [n, nb] of parameter rows through a one-source likelihood (mbb_pointwise_rows), and
    z = g / sqrt(Lambda_bb) [n, nb] from the device's band fluxes in longdouble, rounded to float64."""
    from mbb_emcee_amd import goodness, loo
    ll, st = loo.loo_rows(like, rows)
    model = goodness.goodness_rows(like, rows, want_flux=True)[3]
    _, g, d = LR.ll_rows(like._flux, model, **_weights(like))
    return ll, (g / np.sqrt(d)[None, :]).astype(np.float64)


def _reference(mbb, like, chain4, burn=0, thin=1, dtype=LD, keep=None):
    """_loo_ref.column of every (source, band) of a window of a chain through a one-source likelihood, fed the device's
    own ll; z from the device's band fluxes in longdouble."""
    out = []
    for src in range(chain4.shape[0]):
        rows = np.ascontiguousarray(chain4[src][:, burn::thin].reshape(-1, 5))
        ll, z = _ll_and_z(like, rows)
        cols = []
        for b in range(ll.shape[1]):
            ok = np.isfinite(ll[:, b])
            phi = keep.get((src, b)) if keep is not None else None
            if phi is None:
                phi = LR.norm_cdf_mp(z[ok, b])
                if keep is not None:
                    keep[(src, b)] = phi
            cols.append(LR.column(ll[:, b], z[:, b], dtype=dtype, phi=phi.astype(dtype)))
        out.append(cols)
    return out


def _check_tables(dev, ref, label, row_bits=0, split_pit=False):
    """Counts, tail lengths and status of a device result against the reference's, exactly (row_bits: the row-status
    bits of failing rows inside the window, which the reference does not form); returns the largest _loo_ref.distance
    of the floating-point tables, or with split_pit the pair (of the tables but loo_pit, of loo_pit)."""
    raw = dev._raw
    worst, worst_pit = 0.0, 0.0
    for src, cols in enumerate(ref):
        for b, r in enumerate(cols):
            where = "%s source %d band %d" % (label, src, b)
            assert raw.n_used[src, b] == r["n_used"], where
            assert raw.tail_len[src, b] == r["tail_len"], where
            assert raw.status[src, b] == r["status"] | row_bits, (where, raw.status[src, b], r["status"], row_bits)
            got = {k: getattr(raw, k)[src, b] for k in LR.FLOATS}
            if split_pit:
                d, p = _distances(got, r)
                worst, worst_pit = max(worst, d), max(worst_pit, p)
            else:
                worst = max(worst, LR.distance(got, r))
    return (worst, worst_pit) if split_pit else worst


def _with_budget(mbb, like, mb, chain, **kw):
    from mbb_emcee_amd import _native
    ctx = _native.analysis_context(like)
    ctx.set_option("pointwise_budget_mb", mb)
    try:
        return mbb.chain_loo(like, chain, **kw)
    finally:
        ctx.set_option("pointwise_budget_mb", 16384)
