"""The analysis kernels' SED evaluation -- fnu_sample<..., TAB = false>: polynomial exp / expm1 and a true division, with
its own band sums -- held to the oracle over the whole prior volume, as tests/test_gpu_parity.py holds the tabulated
sample of the likelihood kernels: the 600 wide rows (T 3-200 K, beta 0-4.5, lambda0 5-3000 um, alpha 0.1-10, fnorm
0.01-1000 mJy) and the 225-row grid of table ends (T 1-5000 K, lambda0 1-4500 um) of tests/_domain_rows.py, and six
rows no SED can be built from, through

  a. k_good_flux / k_good_chi     goodness.goodness_rows: band fluxes, chisq, q
  b. k_pw_g                       loo.loo_rows and chain_loo on one-cell windows
  c. k_pred_fill, k_sed_eval      chain_predictions on one-cell windows, postprocess.predict_flux
  d. k_sed_integrate(_src)        postprocess.freq_integral and the summary's derived L_IR with a redshift per source
  e. the prologue's peak          postprocess.peak_wavelength and the summary's derived peaklambda
  f. k_sum_dustmass               the summary's derived dust mass
  g. the six failing rows among the wide ones, through all of the above.

Bounds, and where they come from:
  * f_nu and band fluxes: relative 1e-12 where the oracle's value exceeds 1e-280; elsewhere the device's
    value is finite, >= 0 and < 1e-270 (beyond x = 709.78 m_div divides by 8e307, not by infinity);
  * chisq: -2 lnL of the oracle (no priors here) at 1e-10 max(1, |lnL|);
  * q: tests/test_goodness_gpu.py's -- against mpmath at the device's own chisq, relative 4 x scipy's largest error on
    the same points where the true q >= 1e-290, in [0, 1e-289] below; the grid's six bands leave only a dozen such
    points, too few for scipy's error on them to mean much, and six is an even order: the derived bound of that file's
    section 11 for even orders, (9 + 1.5 ceil(nb/2)) eps -- the tighter of the two wherever both were measured -- is
    what the grid is held to.  A chisq beyond 3000 is not taken to mpmath: Q(3, 1500) < 1e-640;
  * ll: tests/test_loo_gpu.py::test_per_row_ll's -- longdouble on the device's own fluxes within _loo_ref.ll_bound;
  * the frequency integral: relative 1e-12 plus the reference's own error estimate for that row and range (the
    integrand is positive and held to 1e-12; the fixed rule's truncation is below 1e-13 everywhere,
    tests/test_domain_paths_cpu.py);
  * peak wavelength: relative 1e-10 (it is xmerge's kind of root);
  * dust mass: relative 1e-13 of oracle.post_dustmass; a row beyond it is decided by 50 digits
    (_summary_ref.dustmass_mp), as tests/test_summary_derived_gpu.py::_check_dust_entries does;
  * status words, NaN places and everything said to be "the same bits": exact.
No sampler, no served call and no resident kernel is used here: the boundary call's three ways and the multi-source call
over the same rows are tests/test_domain_boundary_gpu.py's, the device sampler's forms tests/test_domain_sampler_gpu.py's."""
import numpy as np
import pytest

from conftest import VARIANTS, lnl_close, parity_record, rec_allclose
import _domain_rows as D
import _goodness_ref as GR
import _loo_ref as LR
import _summary_ref as SR

pytestmark = pytest.mark.gpu

FLUX_RTOL = 1e-12
SMALL = 1e-270
WAVES = [8.0, 24.0, 70.0, 250.0, 1100.0, 3000.0]
PBANDS = ["PACS_70um", "SPIRE_500um", "SCUBA2_450um"]            # (SCUBA2_450um is in no fit)
SPECS = WAVES + PBANDS
DL = 18700.0                                                    # Mpc, with z = 2.3
DL0 = 100.0                                                     # Mpc, with z = 0
KAPPAS = [(2.64, 125.0), (1.5, 250.0)]
PEAK, LIR, DUST = 5, 6, 7                                       # the summary's derived columns
_CACHE = {}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


# ---------------------------------------------------------------- set-up
def _rows(which):
    if which not in _CACHE:
        r = {"wide": D.wide_rows, "grid": D.grid_rows, "bad": lambda: D.with_bad_rows()[0]}[which]()
        r.setflags(write=False)
        _CACHE[which] = r
    return _CACHE[which]


def _cov(unc):
    """A full covariance as tests/test_gpu_parity.py::test_random_configurations_vs_oracle builds one, seed 1000."""
    rng = np.random.RandomState(1000)
    nb = unc.size
    A = rng.normal(0, 1, (nb, nb))
    return np.diag(unc ** 2) + 0.02 * np.median(unc) ** 2 * A.dot(A.T)


def _setup(mbb, oracle, which, opthin, noalpha, cov=False):
    """(likelihood, the oracle's likelihood with its limits, the oracle's without any limit) of the wide test's five
    bands (`wide`, `bad`) or the grid test's six (`grid`), response=True, the data of those tests, no priors."""
    key = ("setup", which == "grid", opthin, noalpha, cov)
    if key not in _CACHE:
        names, flux = (D.GRID_BANDS, D.GRID_FLUX) if which == "grid" else (D.WIDE_BANDS, D.WIDE_FLUX)
        unc = D.unc_of(flux)
        like = mbb.likelihood(opthin=opthin, noalpha=noalpha, response=True)
        like.set_phot(names, flux, unc)
        if which == "grid":
            like.set_uplim("lambda0", 5000.0)                           # (3 x max wavelength would cut the grid short)
        c = _cov(unc) if cov else None
        if cov:
            like.set_cov(c)
        bands = [(r.wavelength, r._sedmult, r._normfac) for r in like._responses]
        kw = dict(bands=bands, cov=c, opthin=opthin, noalpha=noalpha, wavenorm=500.0)
        orc = oracle.OracleLikelihood(flux, unc, lowlim=like.lowlims, has_uplim=[int(b) for b in like.has_uplims],
                                      uplim=like.uplims, **kw)
        free = oracle.OracleLikelihood(flux, unc, lowlim=np.full(5, -np.inf), has_uplim=[0] * 6, **kw)
        _CACHE[key] = (like, orc, free)
    return _CACHE[key]


def _weights(like):
    return dict(invcov=like._invcovmatrix) if like._has_covmatrix else dict(ivar=like._ivar)


def _expected(like, which, want_peak=False):
    """(row status as like.context.sed_prologue reports it, which rows are good ones for this model).  The wide and the
    grid rows are all good and must have status 0; of the six failing rows, one whose bad column the model does not
    read (alpha without alpha) is a good row -- status 0 --, and the others are held to give NaN with whatever status
    the prologue reports for them."""
    rows = _rows(which)
    st = like.context.sed_prologue(rows, like.opthin, like.noalpha, like.wavenorm, want_peak=want_peak)[1]
    good = np.ones(rows.shape[0], dtype=bool)
    if which == "bad":
        for pos, (what, col) in zip(D.BAD_AT, D.BAD):
            good[pos] = (col == 3 and like.noalpha)
    assert np.all(st[good] == 0), (which, np.flatnonzero(good & (st != 0)))
    # a row no SED can be built from is reported.  T = 0 is the regression case: h/kT is infinite, and the optically
    # thin models' normalisation came out as 0 -- band fluxes of 0 and a finite chisq with status 0
    assert np.all(st[~good] != 0), (which, np.flatnonzero(~good & (st == 0)))
    return st, good


def _word(code, value):
    """The status word of a chain analysis' one-cell source: the row's bit from ROW_SHIFT on, HAS_NAN where it gave NaN."""
    from mbb_emcee_amd import _native
    code, value = np.asarray(code), np.asarray(value)
    code = code.reshape(code.shape + (1,) * (value.ndim - code.ndim))
    return np.where(code != 0, 1 << (_native.SUM_ROW_SHIFT + code), 0) | np.where(np.isnan(value), _native.SUM_HAS_NAN, 0)


def _hold_flux(kind, got, ref, good):
    """got [n, ...] against the oracle's ref on the good rows -- relative 1e-12 above 1e-280, next to 0 elsewhere --;
    NaN on the others."""
    assert np.all(np.isnan(got[~good])), kind
    g, r = got[good], ref[good]
    assert not np.isnan(g).any() and not np.isnan(r).any(), kind
    big = r > D.FLUX_FLOOR
    err = np.max(np.abs(g[big] / r[big] - 1.0))
    small = g[~big]
    print("    %s: %d values, worst relative %.3g; %d where the oracle is below %g, the device's largest there %.3g"
          % (kind, big.sum(), err, small.size, D.FLUX_FLOOR, small.max() if small.size else 0.0))
    parity_record(kind + " (rel)", err, FLUX_RTOL)
    assert err < FLUX_RTOL, kind
    assert np.all(np.isfinite(small)) and np.all(small >= 0.0) and np.all(small < SMALL), (kind, small.max())


def _oracle_on(good, n, fn):
    """fn(index) for the good rows, NaN for the others: [n, ...]"""
    out = None
    for i in np.flatnonzero(good):
        v = np.atleast_1d(fn(i))
        if out is None:
            out = np.full((n,) + v.shape, np.nan)
        out[i] = v
    return out


def _hold_q(nb, chisq, q, label):
    from scipy.special import gammaincc
    assert np.all((q >= 0) & (q <= 1)), label
    far = chisq >= 3000.0
    assert np.all(q[far] <= 1e-289), label
    x, qq = chisq[~far], q[~far]
    truth = [GR.q_mp(nb, v) for v in x]
    big = np.array([t >= GR.Q_FLOOR for t in truth], dtype=bool)
    print("    %s: %d rows with chisq < 3000, %d of them with q >= %g" % (label, x.size, big.sum(), GR.Q_FLOOR))
    low = qq[~big]
    assert np.all(low >= 0.0) and np.all(low <= 1e-289), label
    if not big.any():
        return
    dev = GR.rel_errors(truth, big, qq)
    scipy_err = GR.rel_errors(truth, big, gammaincc(0.5 * nb, 0.5 * x)).max()
    print("    %s: q worst relative %.3g; scipy's on the same points %.3g" % (label, dev.max(), scipy_err))
    if nb % 2:
        rec_allclose(scipy_err, 0.0, rtol=0, atol=1e-12, kind="scipy gammaincc vs mpmath on the test's points")
        rec_allclose(dev / (4.0 * scipy_err), 0.0, rtol=0, atol=1, kind="q over the prior volume [4 x scipy's error]")
    else:
        rec_allclose(dev / (GR.horner_bound_eps(nb) * GR.EPS), 0.0, rtol=0, atol=1,
                     kind="q over the prior volume, even order [(9 + 1.5 ceil(nb/2)) eps]")


# ---------------------------------------------------------------- a. k_good_flux, k_good_chi
def _once(fn):
    """The result of a check of (set, model[, covariance]) made once and shared read-only: the failing-rows test compares
    with what the tests before it saw."""
    def cached(mbb, oracle, *key):
        k = (fn.__name__,) + key
        if k not in _CACHE:
            val = fn(mbb, oracle, *key)
            for a in val:
                a.setflags(write=False)
            _CACHE[k] = val
        return _CACHE[k]
    return cached


@_once
def _goodness(mbb, oracle, which, opthin, noalpha, cov):
    from mbb_emcee_amd import goodness
    like, orc, free = _setup(mbb, oracle, which, opthin, noalpha, cov)
    rows = _rows(which)
    st, good = _expected(like, which)
    chisq, q, gst, fl = goodness.goodness_rows(like, rows, want_flux=True)
    label = "%s%s" % (which, " cov" if cov else "")
    assert np.array_equal(gst, st), label
    ref_lnl, ref_fl = np.full(rows.shape[0], np.nan), np.full(fl.shape, np.nan)
    ref_lnl[good], ref_fl[good] = free(rows[good], nthreads=4, return_flux=True)
    assert np.all(free.status == 0)
    _hold_flux("band flux of k_good_flux, %s" % label, fl, ref_fl, good)
    assert np.all(np.isnan(chisq[~good])) and np.all(np.isnan(q[~good])), label
    # wherever the likelihood's own oracle -- lower limits and all -- has a finite lnL the status is 0 and it is the same
    # number; goodness of fit knows no limits: the oracle without them is the reference on every good row
    gated = orc(rows[good], nthreads=4)
    fin = np.isfinite(gated)
    assert fin.sum() > 0.9 * fin.size and np.array_equal(gated[fin], ref_lnl[good][fin]), label
    assert np.all(gst[good][fin] == 0)
    lnl_close(-0.5 * chisq[good], ref_lnl[good], kind="chisq / 2 of k_good_chi%s" % (" (covariance)" if cov else ""))
    _hold_q(fl.shape[1], chisq[good], q[good], label)
    return chisq, q, gst, fl


@pytest.mark.parametrize("which,cov", [("wide", False), ("grid", False), ("wide", True)])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_band_fluxes_chisq_and_q(mbb, oracle, name, opthin, noalpha, which, cov):
    """a. goodness_rows over the volume: band fluxes, chisq and q, diagonal and with a full covariance."""
    _goodness(mbb, oracle, which, opthin, noalpha, cov)


# ---------------------------------------------------------------- b. k_pw_g
@_once
def _loo(mbb, oracle, which, opthin, noalpha, cov):
    from mbb_emcee_amd import goodness, loo
    like = _setup(mbb, oracle, which, opthin, noalpha, cov)[0]
    rows = _rows(which)
    st, good = _expected(like, which)
    ll, lst = loo.loo_rows(like, rows)
    assert np.array_equal(lst, st) and ll.shape == (rows.shape[0], int(like._ndata))
    assert np.all(np.isnan(ll[~good]))
    model = goodness.goodness_rows(like, rows[good], want_flux=True)[3]
    ref = LR.ll_rows(like._flux, model, **_weights(like))[0]
    bound = LR.ll_bound(like._flux, model, **_weights(like))
    err = np.abs((ll[good].astype(LR.LD) - ref).astype(np.float64)) / bound
    print("    %s%s: ll %.4g .. %.4g, worst %.3g of its bound" % (which, " cov" if cov else "", ll[good].min(), ll[good].max(),
                                                                 err.max()))
    parity_record("ll per row over the prior volume [its bound]", err.max(), 1.0)
    assert err.max() <= 1.0
    return ll, lst


@pytest.mark.parametrize("which,cov", [("wide", False), ("grid", False), ("wide", True)])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_pointwise_ll(mbb, oracle, name, opthin, noalpha, which, cov):
    """b. loo_rows over the volume; the first 48 wide rows as one-cell windows of chain_loo are the same bits.  The grid
    is the regression case of ps_ll's constant: its sixth band has an uncertainty of 0.4, Lambda_bb = 6.25 next to 2 pi,
    where (log Lambda - log 2 pi) / 2 = -0.0027 formed as a difference kept log's absolute error and was 31 x outside
    the bound; as log(Lambda / 2 pi) / 2 with the quotient carried to twice the working precision it is at 0.22 of it."""
    ll, _ = _loo(mbb, oracle, which, opthin, noalpha, cov)
    if which == "wide":
        like = _setup(mbb, oracle, which, opthin, noalpha, cov)[0]
        one = mbb.chain_loo(like, np.ascontiguousarray(_rows(which)[:48]).reshape(-1, 1, 1, 5))
        assert np.array_equal(one._raw.lppd, ll[:48]) and np.all(one._raw.n_used == 1)
        assert np.all(one._raw.status == (LR.TAIL_SHORT | LR.K_HIGH))


# ---------------------------------------------------------------- c. k_pred_fill, k_sed_eval
def _predict_reference(mbb, oracle, which, opthin, noalpha, good):
    key = ("predref", which, opthin, noalpha)
    if key not in _CACHE:
        like = _setup(mbb, oracle, which, opthin, noalpha)[0]
        rows = _rows(which)
        freq = D.UM_TO_GHZ / np.array(WAVES)
        ref = np.full((rows.shape[0], len(SPECS)), np.nan)
        ref[:, :len(WAVES)] = _oracle_on(good, rows.shape[0],
                                         lambda i: oracle.OracleSED(*rows[i], opthin=opthin, noalpha=noalpha).f_nu(freq))
        tables = [(r.wavelength, r._sedmult, r._normfac) for r in (like._responsewheel[b] for b in PBANDS)]
        orc = oracle.OracleLikelihood(np.ones(3), np.ones(3), bands=tables, opthin=opthin, noalpha=noalpha,
                                      lowlim=np.full(5, -np.inf))
        ref[good, len(WAVES):] = orc(rows[good], nthreads=4, return_flux=True)[1]
        assert np.all(orc.status == 0)
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


@_once
def _predict(mbb, oracle, which, opthin, noalpha):
    like = _setup(mbb, oracle, which, opthin, noalpha)[0]
    rows = _rows(which)
    st, good = _expected(like, which)
    ref = _predict_reference(mbb, oracle, which, opthin, noalpha, good)
    p = mbb.chain_predictions(like, np.ascontiguousarray(rows).reshape(-1, 1, 1, 5), SPECS, keep=False)
    got = p.mean
    assert got.shape == ref.shape and np.all(p.n_used == 1)
    assert np.array_equal(p.status, _word(st, got)), which
    assert np.array_equal(p.min, got, equal_nan=True) and np.array_equal(p.max, got, equal_nan=True)
    nw = len(WAVES)
    _hold_flux("f_nu of k_pred_fill, %s" % which, got[:, :nw], ref[:, :nw], good)
    _hold_flux("band flux of k_pred_fill, %s" % which, got[:, nw:], ref[:, nw:], good)
    # k_sed_eval on the same rows and wavelengths: the same bits; the bands of predict_flux go through the likelihood kernel
    sed, est = like.context.sed_eval(rows, like.opthin, like.noalpha, like.wavenorm, D.UM_TO_GHZ / np.array(WAVES))
    assert np.array_equal(est, st) and np.array_equal(sed, got[:, :nw], equal_nan=True), which
    return got, p.status.astype(np.int64)


@pytest.mark.parametrize("which", ["wide", "grid"])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_predicted_fluxes(mbb, oracle, name, opthin, noalpha, which):
    """c. chain_predictions on one-cell windows: six wavelengths from 8 to 3000 um and three passbands, one of them in
    no fit; postprocess.predict_flux's wavelengths are the same bits, its bands within 1e-12 of the oracle."""
    from mbb_emcee_amd import postprocess as pp
    got, _ = _predict(mbb, oracle, which, opthin, noalpha)
    like = _setup(mbb, oracle, which, opthin, noalpha)[0]
    rows = _rows(which)
    good = np.ones(rows.shape[0], dtype=bool)
    ref = _predict_reference(mbb, oracle, which, opthin, noalpha, good)
    host = pp.predict_flux(like, rows, SPECS)
    nw = len(WAVES)
    assert np.array_equal(host[:, :nw], got[:, :nw]), which
    _hold_flux("band flux of predict_flux, %s" % which, host[:, nw:], ref[:, nw:], good)


# ---------------------------------------------------------------- d. the frequency integral
def _lir_summaries(mbb, like, rows):
    """The derived L_IR of rows as one-cell sources with a redshift per source, divided back by the prefactor, for the
    three ranges [n, 3] -- two calls over rest-frame 8-1000 um with z = 0 and z = 2.3 in turn (each source takes each
    once), one over 42.5-122.5 um at z = 0 with two distances in turn --, the values as they came [n, 3], the prefactors
    [n, 3] and the status words [n, 3]."""
    n = rows.shape[0]
    chain = np.ascontiguousarray(rows).reshape(-1, 1, 1, 5)
    lnp = np.zeros((n, 1, 1))
    even = (np.arange(n) % 2 == 0)
    val, pre, st = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 3), dtype=np.int64)
    for first in (True, False):
        at_rest = even == first
        z = np.where(at_rest, 0.0, D.Z)
        dl = np.where(at_rest, DL0, DL)
        s = mbb.chain_summary(like, chain, lnp, derived=("lir",), redshift=z, lumdist_mpc=dl, keep=False)
        assert np.all(s._raw.n_used[:, LIR] == 1)
        for j, sel in ((0, at_rest), (1, ~at_rest)):
            val[sel, j], st[sel, j] = s._raw.mean[sel, LIR], s._raw.status[sel, LIR]
            pre[sel, j] = 3.11749657e4 * (dl[sel] * dl[sel])
    dl = np.where(even, DL0, DL)
    s = mbb.chain_summary(like, chain, lnp, derived=("lir",), redshift=np.zeros(n), lumdist_mpc=dl,
                          lir_range=D.RANGES[2], keep=False)
    val[:, 2], st[:, 2], pre[:, 2] = s._raw.mean[:, LIR], s._raw.status[:, LIR], 3.11749657e4 * (dl * dl)
    return val / pre, val, pre, st


def _integrals(mbb, like, rows):
    """like.context.sed_integrate (what postprocess.freq_integral calls) over the three ranges: (1e-17 x values [n, 3],
    row status [n, 3])."""
    out, st = np.empty((rows.shape[0], 3)), np.empty((rows.shape[0], 3), dtype=np.int64)
    for j, (lo, hi) in enumerate(D.RANGES):
        v, s = like.context.sed_integrate(rows, like.opthin, like.noalpha, like.wavenorm, D.UM_TO_GHZ / hi, D.UM_TO_GHZ / lo)
        out[:, j], st[:, j] = 1e-17 * v, s
    return out, st


def _hold_integral(kind, got, ref, err):
    """got [n, 3] in erg/s/cm^2 against lir_reference's values [n, 3] in mJy GHz and their error estimates"""
    rel = np.abs(got / (1e-17 * ref) - 1.0)
    bound = 1e-12 + err / ref
    i, j = np.unravel_index(np.argmax(rel / bound), rel.shape)
    print("    %s: worst relative %.3g (row %d, range %d, its bound %.3g); largest relative error anywhere %.3g"
          % (kind, rel[i, j], i, j, bound[i, j], rel.max()))
    parity_record(kind + " (rel)", rel.max(), bound.max())
    rec_allclose(rel / bound, 0.0, rtol=0, atol=1, kind=kind + " [1e-12 + the reference's error estimate]")


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_frequency_integral(mbb, oracle, name, opthin, noalpha):
    """d. Every fifth wide row and every grid row over 8-1000 um, the same at z = 2.3 and 42.5-122.5 um, by
    postprocess.freq_integral (k_sed_integrate) and by the summary's L_IR with a redshift per source
    (k_sed_integrate_src, k_sum_lir_src), against quad split at the kinks -- never the reference's own unsplit quad,
    which is off by up to 3.9e-7 at the merge point.  Both routes integrate the same bounds: the same bits."""
    from mbb_emcee_amd import postprocess as pp
    like = _setup(mbb, oracle, "grid", opthin, noalpha)[0]            # (the band set does not matter here)
    rows = np.concatenate(D.lir_rows())
    ref, err = D.lir_table(oracle, opthin, noalpha)
    host = np.stack([pp.freq_integral(like, rows, lo, hi) for lo, hi in D.RANGES], axis=-1)
    _hold_integral("frequency integral of k_sed_integrate vs split quad", host, ref, err)
    back, val, pre, st = _lir_summaries(mbb, like, rows)
    assert np.all(st == 0)
    _hold_integral("L_IR of k_sed_integrate_src / its prefactor vs split quad", back, ref, err)
    assert np.array_equal(val, pre * host), np.argwhere(val != pre * host)[:5]
    # (and postprocess.lir is that product)
    assert np.array_equal(pp.lir(like, rows[::2], 0.0, DL0), val[::2, 0])


# ---------------------------------------------------------------- e. peak wavelength
def _peaks(mbb, like, rows):
    """(the summary's derived peak wavelength of rows as one-cell sources, its status words)"""
    s = mbb.chain_summary(like, np.ascontiguousarray(rows).reshape(-1, 1, 1, 5), np.zeros((rows.shape[0], 1, 1)),
                          derived=("peaklambda",), keep=False)
    assert np.all(s._raw.n_used[:, PEAK] == 1)
    return s._raw.mean[:, PEAK].copy(), s._raw.status[:, PEAK].copy()


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_peak_wavelength(mbb, oracle, name, opthin, noalpha):
    """e. The fit's own model's peak of every wide row against the oracle's max_wave."""
    from mbb_emcee_amd import postprocess as pp
    like = _setup(mbb, oracle, "wide", opthin, noalpha)[0]
    rows = _rows("wide")
    ref = np.array([oracle.OracleSED(*p, opthin=opthin, noalpha=noalpha).max_wave() for p in rows])
    host = pp.peak_wavelength(like, rows)
    rec_allclose(host, ref, rtol=1e-10, kind="peak wavelength over the prior volume vs oracle")
    got, st = _peaks(mbb, like, rows)
    assert np.all(st == 0) and np.array_equal(got, host)


# ---------------------------------------------------------------- f. dust mass
def _dust(mbb, like, rows, kappa, kappa_wave):
    s = mbb.chain_summary(like, np.ascontiguousarray(rows).reshape(-1, 1, 1, 5), np.zeros((rows.shape[0], 1, 1)),
                          derived=("dustmass",), redshift=D.Z, lumdist_mpc=DL, kappa=kappa, kappa_wave=kappa_wave, keep=False)
    assert np.all(s._raw.n_used[:, DUST] == 1)
    return s._raw.mean[:, DUST].copy(), s._raw.status[:, DUST].copy()


def _hold_dust(oracle, opthin, rows, got, kappa, kappa_wave, what):
    """1e-13 of the oracle's closed form; where a row exceeds that, 50 digits decide (test_summary_derived_gpu.py's
    _check_dust_entries, for any model and kappa)."""
    host = oracle.post_dustmass(rows, D.Z, DL, wavenorm=500.0, opthin=opthin, kappa=kappa, kappa_wave=kappa_wave)
    rel = np.abs(got - host) / np.abs(host)
    print("    %s dustmass: max rel %.3g over %d rows" % (what, rel.max(), got.size))
    parity_record("dust mass over the prior volume vs oracle (rel)", rel.max(), 1e-13)
    for i in np.flatnonzero(~(rel <= 1e-13)):
        truth = SR.dustmass_mp(rows[i], opthin, 500.0, D.Z, DL, kappa, kappa_wave)
        dev, hst = abs(got[i] - truth) / abs(truth), abs(host[i] - truth) / abs(truth)
        print("    row %s: device %.3g, host %.3g of the 50-digit value" % (rows[i], dev, hst))
        parity_record("dust mass over the prior volume vs 50 digits (rel)", dev, 1e-13)
        assert dev <= 1e-13, (what, rows[i], got[i], host[i], truth)


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_dust_mass(mbb, oracle, name, opthin, noalpha):
    """f. The summary's derived dust mass of every wide row at z = 2.3, default and another (kappa, kappa_wave)."""
    like = _setup(mbb, oracle, "wide", opthin, noalpha)[0]
    rows = _rows("wide")
    for kappa, kappa_wave in KAPPAS:
        got, st = _dust(mbb, like, rows, kappa, kappa_wave)
        assert np.all(st == 0) and np.all(np.isfinite(got)) and np.all(got > 0)
        _hold_dust(oracle, opthin, rows, got, kappa, kappa_wave, "%s kappa %g at %g um" % (name, kappa, kappa_wave))


# ---------------------------------------------------------------- g. failing rows
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_failing_rows(mbb, oracle, name, opthin, noalpha):
    """g. A NaN T, an infinite fnorm, alpha = -1, alpha = 0, T = 0 and a NaN beta at rows 0, 63, 64, 255, 256 and 605 of
    606 -- first and last row, either side of the wave and of the 256-thread workgroup -- through (a) to (f): NaN and
    the prologue's status there (its bit in the one-cell source's word for the chain analyses), each value held as in
    (a) to (f) where the model does not read the bad column, and every other row bit for bit what it is without them."""
    from mbb_emcee_amd import _native
    rows, keep = D.with_bad_rows()
    wide = _rows("wide")
    assert np.array_equal(rows[keep], wide)
    like = _setup(mbb, oracle, "bad", opthin, noalpha)[0]
    st, good = _expected(like, "bad")
    assert (~good).sum() == (4 if noalpha else 6)
    print("    %s: the prologue's status of the six rows %s" % (name, st[list(D.BAD_AT)]))
    for cov in (False, True):
        a, b = _goodness(mbb, oracle, "bad", opthin, noalpha, cov), _goodness(mbb, oracle, "wide", opthin, noalpha, cov)
        for x, y in zip(a, b):
            assert np.array_equal(x[keep], y, equal_nan=True)
        a, b = _loo(mbb, oracle, "bad", opthin, noalpha, cov), _loo(mbb, oracle, "wide", opthin, noalpha, cov)
        for x, y in zip(a, b):
            assert np.array_equal(x[keep], y, equal_nan=True)
    # chain_loo: the first 66 rows hold three of the six
    ll = _loo(mbb, oracle, "bad", opthin, noalpha, False)[0]
    one = mbb.chain_loo(like, np.ascontiguousarray(rows[:66]).reshape(-1, 1, 1, 5))
    assert np.array_equal(one._raw.lppd, ll[:66], equal_nan=True)
    code = st[:66, None]
    assert np.array_equal(one._raw.status >> _native.SUM_ROW_SHIFT, np.where(code != 0, 1 << code, 0) + 0 * one._raw.status)
    assert np.array_equal(one._raw.n_used, np.where(np.isnan(ll[:66]), 0, 1))
    ok = good[:66]
    assert np.all(one._raw.status[ok] == (LR.TAIL_SHORT | LR.K_HIGH))
    # c
    a, b = _predict(mbb, oracle, "bad", opthin, noalpha), _predict(mbb, oracle, "wide", opthin, noalpha)
    for x, y in zip(a, b):
        assert np.array_equal(x[keep], y, equal_nan=True)
    # d: every fifth of the 606 rows does not meet all six, so all of them; the good ones among the six against quad
    like0 = _setup(mbb, oracle, "bad", opthin, noalpha)[0]
    host, hst = _integrals(mbb, like0, rows)
    assert np.array_equal(hst, np.repeat(st[:, None], 3, axis=1)) and np.array_equal(np.isnan(host), np.repeat(~good[:, None], 3, axis=1))
    back, val, pre, sst = _lir_summaries(mbb, like0, rows)
    assert np.array_equal(val, pre * host, equal_nan=True)
    assert np.array_equal(sst, _word(st, val))
    host_w, _ = _integrals(mbb, like0, wide)
    assert np.array_equal(host[keep], host_w)
    extra = [p for p in D.BAD_AT if good[p]]
    for p in extra:
        sed = oracle.OracleSED(*rows[p], opthin=opthin, noalpha=noalpha)
        ref = np.array([D.lir_reference(sed, lo, hi, opthin, noalpha, rows[p, 2]) for lo, hi in D.RANGES])
        _hold_integral("frequency integral of k_sed_integrate vs split quad", host[p:p + 1], ref[None, :, 0], ref[None, :, 1])
    # e
    pst = _expected(like, "bad", want_peak=True)[0]
    out = like.context.sed_prologue(rows, opthin, noalpha, like.wavenorm, want_peak=True)[0][:, 5]
    got, sst = _peaks(mbb, like, rows)
    assert np.array_equal(got, out, equal_nan=True) and np.array_equal(np.isnan(got), ~good)
    assert np.array_equal(sst, _word(pst, got))
    assert np.array_equal(got[keep], _peaks(mbb, like, wide)[0])
    for p in extra:
        rec_allclose(got[p], oracle.OracleSED(*rows[p], opthin=opthin, noalpha=noalpha).max_wave(), rtol=1e-10,
                     kind="peak wavelength over the prior volume vs oracle")
    # f: the closed form reads T, beta, fnorm (and lambda0 when optically thick), never alpha: the two alpha rows are
    # good rows for it in every model; a NaN in is a NaN out with HAS_NAN and no row bit (no SED is built), T = 0 and
    # an infinite fnorm give an infinite mass
    for kappa, kappa_wave in KAPPAS:
        got, sst = _dust(mbb, like, rows, kappa, kappa_wave)
        assert np.array_equal(got[keep], _dust(mbb, like, wide, kappa, kappa_wave)[0])
        fin = np.isfinite(got)
        assert np.all(sst[fin] == 0) and np.all(sst[np.isnan(got)] == _native.SUM_HAS_NAN) and np.all(sst >> _native.SUM_ROW_SHIFT == 0)
        for pos, (what, col) in zip(D.BAD_AT, D.BAD):
            if col == 3:
                _hold_dust(oracle, opthin, rows[pos:pos + 1], got[pos:pos + 1], kappa, kappa_wave, what)
            elif what.startswith("NaN"):
                assert np.isnan(got[pos]), what
            else:
                assert not np.isfinite(got[pos]), (what, got[pos])
