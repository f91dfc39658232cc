"""Goodness of fit on the GPU (csrc/mbb_goodness.hip.h through mbb_chain_goodness / mbb_sampler_goodness /
mbb_goodness_rows and mbb_emcee_amd/goodness.py) against the CPU oracle's band fluxes, longdouble and mpmath
(tests/_goodness_ref.py) and numpy.

Tolerances, and where they come from:
  * chisq per entry: with A = diag(ivar) or |C^-1| elementwise, r = f - m and m the oracle's band fluxes,
    |d chisq| <= 2e-12 |r|^T A |m| + 1e-24 |m|^T A |m| + (2 nb + 4) eps |r|^T A |r|: SURVEY 8c's 1e-12 per band flux
    propagated, then the rounding of the subtraction, the products and an nb-term sum (_goodness_ref.chisq_bound);
  * q per entry: against mpmath at the device's own chisq, the very double read back, so that only the function is
    judged: relative, where the true q >= 1e-290, 4 x the largest relative error scipy.special.gammaincc shows against
    mpmath on the same (nb, chisq) points of the case (the device's exp has its own argument reduction, and x up to 700
    amplifies an ulp of it); below 1e-290, 0 <= q <= 1e-289;
  * statistics of a column whose entries are known bit for bit (the device's own per-entry column, read back through
    a 1 x 1 window per entry): tests/test_predict_gpu.py's bounds -- the mean within 64 eps mean|x| of numpy's,
    percentiles within 4 ulp of numpy's inside the bracket of their two order statistics, min, max and n_used exact;
  * the band fluxes of the maximum-likelihood entry: relative 1e-12 from the oracle's;
  * counts, indices, status bits and everything said to be "the same bits": exact.
The entries are every row of the fixture chains tests/test_predict_gpu.py uses (tests/golden/results.npz: 32 x 16 per
model variant)."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_bands, rec_allclose
import _goodness_ref as GR
import _summary_ref as SR

pytestmark = pytest.mark.gpu

EPS = SR.EPS
VARIANTS = [("thin_walpha", True, False), ("thick_walpha", False, False),
            ("thick_noalpha", False, True), ("thin_noalpha", True, True)]
BANDS4 = ["PACS_160um", "SPIRE_250um", "SPIRE_500um", "SCUBA2_850um"]
DELTA = [250.0, 500.0, 850.0]
BAND_CASES = ["bands4", "delta1", "delta2", "delta3", "cov12"]
SCALES = (100.0, 1.0, 0.01)
RAW_FIELDS = ("n_used", "mean", "min", "max", "status", "pct", "at_mean", "ml", "ml_index", "ml_model", "best", "best_index")
NW, NSTEPS = 34, 64
_CACHE = {}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _same_bits(a, b, fields=RAW_FIELDS):
    return all(np.array_equal(getattr(a._raw, f), getattr(b._raw, f), equal_nan=True) for f in fields)


def _setup(mbb, oracle, g_lnl, g_pb, chain, opthin, noalpha, case, scale=1.0):
    """(likelihood, oracle likelihood) of a band case: the data is the oracle's model at the chain's middle row, pushed
    5% up and down band by band, with uncertainties scale (0.1 flux + 1); cov12 gives them cfg4's correlations."""
    key = ("setup", opthin, noalpha, case, scale)
    if key in _CACHE:
        return _CACHE[key]
    if case.startswith("delta"):
        wave = DELTA[:int(case[5:])]
        okw = dict(wave=wave)
        like = mbb.likelihood(opthin=opthin, noalpha=noalpha)
        first = wave
    else:
        names = BANDS4 if case == "bands4" else [str(b) for b in g_lnl["cfg4/bands"]]
        okw = dict(bands=golden_bands(g_pb, names))
        like = mbb.likelihood(response=True, opthin=opthin, noalpha=noalpha)
        first = names
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
    like.set_phot(first, flux, unc)
    if cov is not None:
        like.set_cov(cov)
    orc = oracle.OracleLikelihood(flux, unc, cov=cov, **okw, **free)
    _CACHE[key] = (like, orc)
    return _CACHE[key]


def _entries(mbb, like, chain, **kw):
    """The device's own per-entry (chisq, q) [rows] each: every chain row as a source of one walker and one step
    through the one-source likelihood; mean, min, max and every percentile are then the cell."""
    rows = np.ascontiguousarray(chain).reshape(-1, 1, 1, 5)
    g = mbb.chain_goodness(like, rows, **kw)
    raw = g._raw
    assert g.chisq_mean.shape == (rows.shape[0],)                       # (the leading axis stays: the chain has sources)
    assert np.all(raw.n_used == 1) and np.all(raw.status == 0)
    for k in range(raw.pct.shape[-1]):
        assert np.array_equal(raw.pct[..., k], raw.mean)
    assert np.array_equal(raw.min, raw.mean) and np.array_equal(raw.max, raw.mean)
    # one entry: theta-bar is the entry, the ML entry too
    assert np.array_equal(raw.at_mean[:, :5], rows[:, 0, 0]) and np.array_equal(raw.ml[:, :5], rows[:, 0, 0])
    assert np.array_equal(raw.at_mean[:, 5:], raw.mean) and np.array_equal(raw.ml[:, 5:], raw.mean)
    assert np.all(raw.ml_index == 0) and np.all(raw.best_index == -1) and np.all(np.isnan(raw.best))
    return raw.mean[:, 0].copy(), raw.mean[:, 1].copy(), g


def _weights(like):
    return dict(invcov=like._invcovmatrix) if like._has_covmatrix else dict(ivar=like._ivar)


# ---------------------------------------------------------------- 1. per entry
@pytest.mark.parametrize("case", BAND_CASES)
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_per_entry_chisq_and_q(mbb, oracle, g_lnl, g_pb, g_res, name, opthin, noalpha, case):
    """1. Every row of the fixture chain as a one-cell source, at the uncertainties scaled by 100, 1 and 0.01: chisq
    against longdouble on the oracle's band fluxes, q against mpmath at the device's own chisq."""
    mpmath = pytest.importorskip("mpmath")
    from scipy.special import gammaincc
    chain = g_res[name + "/chain"]
    rows = chain.reshape(-1, 5)
    pts_x, pts_q = [], []
    nb = None
    for scale in SCALES:
        like, orc = _setup(mbb, oracle, g_lnl, g_pb, chain, opthin, noalpha, case, scale)
        nb = orc.nb
        chi, q, g = _entries(mbb, like, chain)
        model = orc(rows, return_flux=True)[1]
        assert np.all(orc.status == 0) and np.all(np.isfinite(model))
        ref = GR.chisq(like._flux, model, **_weights(like))
        bound = GR.chisq_bound(like._flux, model, **_weights(like))
        err = np.abs((chi.astype(GR.LD) - ref).astype(np.float64)) / bound
        print("    %s %s scale %g: chisq %.3g .. %.3g, worst %.3g of its bound" % (name, case, scale, chi.min(), chi.max(), err.max()))
        rec_allclose(err, 0.0, rtol=0, atol=1, kind="chisq per entry [its bound]")
        # the ML entry's band fluxes are the oracle's, its pulls follow
        rec_allclose(g._raw.ml_model, model, rtol=1e-12, kind="band flux of the ML entry vs oracle")
        assert g.ndata == nb and g.pulls.shape == (rows.shape[0], nb)
        pts_x.append(chi); pts_q.append(q)
    x, q = np.concatenate(pts_x), np.concatenate(pts_q)
    assert x.min() < 0.05 and x.max() > 1490.0, (x.min(), x.max())
    truth = [GR.q_mp(nb, v) for v in x]
    big = np.array([t >= GR.Q_FLOOR for t in truth])
    assert big.sum() >= x.size // 3 and (~big).sum() >= 1
    rel = lambda got: np.array([float(abs(mpmath.mpf(float(g_)) - t) / t) for g_, t, b in zip(got, truth, big) if b])   # noqa: E731
    scipy_err = rel(gammaincc(0.5 * nb, 0.5 * x)).max()
    rec_allclose(scipy_err, 0.0, rtol=0, atol=1e-12, kind="scipy gammaincc vs mpmath on the test's points")
    dev = rel(q)
    print("    %s %s: q worst relative %.3g; scipy's on the same points %.3g" % (name, case, dev.max(), scipy_err))
    rec_allclose(dev / (4.0 * scipy_err), 0.0, rtol=0, atol=1, kind="q per entry [4 x scipy's error]")
    low = q[~big]
    assert np.all(low >= 0.0) and np.all(low <= 1e-289)
    assert np.all((q >= 0) & (q <= 1))


# ---------------------------------------------------------------- 2. statistics, theta-bar, ML, best
def _check_column(raw, s, c, col, qs, label):
    ref = SR.column_reference(col, qs)
    assert raw.n_used[s, c] == ref["n"], label
    if ref["scale"] == 0.0:                                             # (a column of zeros: q of a hopeless fit)
        assert raw.mean[s, c] == 0.0, label
    else:
        err = abs(raw.mean[s, c] - ref["mean"]) / (EPS * ref["scale"])
        rec_allclose(err, 0.0, rtol=0, atol=64, kind="goodness mean [eps mean|x|]")
    for k, q in enumerate(qs):
        a, b = SR.bracket(ref["sorted"], q)
        rec_allclose(SR.ulps_off(raw.pct[s, c, k], ref["pct"][k], a, b), 0.0, rtol=0, atol=4, kind="goodness percentile [ulp]")
    assert raw.min[s, c] == ref["min"] and raw.max[s, c] == ref["max"], label


def _check_source(mbb, like, g, s, chain_s, lnprob_s, chi_s, q_s, burn, thin, label, model_of=None):
    """Source s of a result against numpy on its exact per-entry columns chi_s, q_s [nw, nsteps]."""
    from mbb_emcee_amd import goodness
    raw = g._raw
    qs = g.percentiles[0]
    wc, wq = chi_s[:, burn::thin], q_s[:, burn::thin]
    _check_column(raw, s, 0, np.ascontiguousarray(wc).reshape(-1), qs, label + " chisq")
    _check_column(raw, s, 1, np.ascontiguousarray(wq).reshape(-1), qs, label + " q")
    assert raw.status[s, 0] == 0 and raw.status[s, 1] == 0
    # theta-bar: the summary's bits, and its chisq and q the rows' function of it
    lp = lnprob_s if lnprob_s is not None else np.zeros(chain_s.shape[:2])
    summ = mbb.chain_summary(like, chain_s, lp, burn=burn, thin=thin, keep=False)
    assert np.array_equal(raw.at_mean[s, :5], summ._raw.mean[0, :5]), label
    c1, q1, st1 = goodness.goodness_rows(like, raw.at_mean[s:s + 1, :5])
    assert st1[0] == 0 and raw.at_mean[s, 5] == c1[0] and raw.at_mean[s, 6] == q1[0], label
    # the ML entry: numpy's first argmin over the window in [walker][step] order
    w, k = np.unravel_index(np.argmin(wc), wc.shape)
    step = burn + k * thin
    assert tuple(raw.ml_index[s]) == (w, step), (label, raw.ml_index[s], (w, step))
    assert np.array_equal(raw.ml[s, :5], chain_s[w, step]) and raw.ml[s, 5] == chi_s[w, step] and raw.ml[s, 6] == q_s[w, step]
    if model_of is not None:
        rec_allclose(raw.ml_model[s], model_of(chain_s[w, step]), rtol=1e-12, kind="band flux of the ML entry vs oracle")
    if lnprob_s is None:
        assert np.all(raw.best_index[s] == -1) and np.all(np.isnan(raw.best[s]))
    else:
        assert np.array_equal(raw.best_index[s], summ._raw.best_index[0]), label
        bw, bs = raw.best_index[s]
        assert raw.best[s, 0] == chi_s[bw, bs] and raw.best[s, 1] == q_s[bw, bs]


@pytest.mark.parametrize("name,opthin,noalpha,case", [VARIANTS[0] + ("cov12",), VARIANTS[1] + ("bands4",),
                                                      VARIANTS[2] + ("delta3",), VARIANTS[3] + ("delta1",)])
def test_statistics_theta_bar_and_ml(mbb, oracle, g_lnl, g_pb, g_res, name, opthin, noalpha, case):
    """2. The fixture chain as one source of 32 x 16, with rows duplicated so that the minimum chisq is tied: whole,
    burned, thinned and one-kept-step windows, with and without lnprob."""
    chain = g_res[name + "/chain"].copy()
    lnprob = g_res[name + "/lnprobability"].copy()
    like, orc = _setup(mbb, oracle, g_lnl, g_pb, chain, opthin, noalpha, case)
    chi0, _, _ = _entries(mbb, like, chain)
    w0, s0 = np.unravel_index(np.argmin(chi0.reshape(32, 16)), (32, 16))
    for w, s in ((3, 15), (20, 6), (31, 0), (20, 15)):                 # the minimum, planted in four more cells
        chain[w, s] = chain[w0, s0]
    lnprob[5, 7] = lnprob[9, 2] = lnprob.max() + 1.0                    # ... and a tied maximum of lnprob
    chi, q, _ = _entries(mbb, like, chain)
    chi, q = chi.reshape(32, 16), q.reshape(32, 16)
    assert (chi == chi.min()).sum() >= 5
    model_of = lambda p: orc(p, return_flux=True)[1][0]                 # noqa: E731
    for burn, thin, lp in ((0, 1, lnprob), (5, 1, lnprob), (1, 3, None), (0, 7, lnprob), (15, 1, lnprob), (4, 12, None)):
        g = mbb.chain_goodness(like, chain, lnprob=lp, percentile=(68.3, 95.4), percentiles=(50.0, 0.0, 100.0),
                               burn=burn, thin=thin)
        assert g.chisq_mean.shape == () and g.nwalkers == 32 and g.nsteps_used == len(range(burn, 16, thin))
        _check_source(mbb, like, g, 0, chain, lp, chi, q, burn, thin, "%s %s burn %d thin %d" % (name, case, burn, thin), model_of)
        assert g.p_d == g.chisq_mean - g.chisq_at_mean and g.dic == g.chisq_mean + g.p_d
        assert g.ppp == g._raw.mean[0, 1] and g.chisq_min == g.max_likelihood[1]
        cen = g.chisq_cen()
        assert cen.shape == (3,) and cen[0] == g.chisq_mean and np.all(cen[1:] >= 0)
        if lp is not None:
            assert g.best_fit_chisq == g._raw.best[0, 0]
        assert "ChiSquare over the chain" in str(g)
        assert _same_bits(g, mbb.chain_goodness(like, chain, lnprob=lp, percentile=(68.3, 95.4), percentiles=(50.0, 0.0, 100.0),
                                                burn=burn, thin=thin))


# ---------------------------------------------------------------- 3. limits and priors
def test_limits_and_priors_change_nothing(mbb, oracle, g_lnl, g_pb, g_res):
    """3. A lower limit above part of the chain, an upper wall and a Gaussian prior: the same bits as without; the
    likelihood itself does see them."""
    from mbb_emcee_amd import goodness
    chain = g_res["thick_walpha/chain"]
    rows = chain.reshape(-1, 5)
    for case in ("bands4", "cov12"):
        plain, _ = _setup(mbb, oracle, g_lnl, g_pb, chain, False, False, case)
        ref = mbb.chain_goodness(plain, chain, lnprob=g_res["thick_walpha/lnprobability"], burn=2)
        cr, qr, sr, fr = goodness.goodness_rows(plain, rows, want_flux=True)
        lim = mbb.likelihood(response=True)
        lim.set_phot(plain._response_names, plain._flux, plain._flux_unc)
        if case == "cov12":
            lim.set_cov(plain._covmatrix)
        tmid = float(np.median(rows[:, 0]))
        lim.set_lowlim("T", tmid)
        lim.set_uplim("beta", float(np.median(rows[:, 1])))
        lim.set_gaussian_prior("alpha", 2.0, 0.1)
        assert np.isneginf(lim(rows)).sum() >= 100 and not np.array_equal(lim(rows), plain(rows))
        got = mbb.chain_goodness(lim, chain, lnprob=g_res["thick_walpha/lnprobability"], burn=2)
        assert _same_bits(got, ref), case
        cl, ql, sl, fl = goodness.goodness_rows(lim, rows, want_flux=True)
        assert np.array_equal(cl, cr) and np.array_equal(ql, qr) and np.array_equal(fl, fr) and np.all(sl == 0)
        assert np.all(np.isfinite(cl[rows[:, 0] < tmid]))               # a row below the lower limit has a chisq


# ---------------------------------------------------------------- 4. sources
def test_multi_source(mbb, oracle, g_lnl, g_pb, g_res):
    """4. Three sources with data of different scales: each is bit for bit the one-source likelihood with its data
    alone, and against numpy on its own per-entry column; then one shared one-source context for a three-source chain."""
    chain = np.ascontiguousarray(g_res["thick_walpha/chain"][:30].reshape(3, 10, 16, 5))
    lnprob = np.ascontiguousarray(g_res["thick_walpha/lnprobability"][:30].reshape(3, 10, 16))
    base, _ = _setup(mbb, oracle, g_lnl, g_pb, g_res["thick_walpha/chain"], False, False, "bands4")
    flux = base._flux[None, :] * np.array([1.0, 37.0, 0.004])[:, None]
    unc = 0.1 * flux + np.array([1.0, 5.0, 0.01])[:, None]
    multi = mbb.likelihood(response=True)
    multi.set_phot_multi(BANDS4, flux, unc)
    kw = dict(percentile=(68.3, 95.4), burn=3, thin=2)
    g = mbb.chain_goodness(multi, chain, lnprob=lnprob, **kw)
    assert g.chisq_cen().shape == (3, 3) and g.pulls.shape == (3, 4) and g.max_likelihood[0].shape == (3, 5)
    assert len(set(g.chisq_mean)) == 3
    for s in range(3):
        one = mbb.likelihood(response=True)
        one.set_phot(BANDS4, flux[s], unc[s])
        alone = mbb.chain_goodness(one, chain[s], lnprob=lnprob[s], **kw)
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(g._raw, f)[s], getattr(alone._raw, f)[0], equal_nan=True), (s, f)
        chi, q, _ = _entries(mbb, one, chain[s])
        _check_source(mbb, one, g, s, chain[s], lnprob[s], chi.reshape(10, 16), q.reshape(10, 16), 3, 2, "source %d" % s)
        # (a multi-source likelihood keeps 1 / unc^2: the pulls' sigma is that, back through a square root)
        np.testing.assert_allclose(g.pulls[s], (flux[s] - g._raw.ml_model[s]) / unc[s], rtol=8 * EPS)
        assert np.array_equal(alone.pulls, (flux[s] - g._raw.ml_model[s]) / unc[s])
    # rows grouped by source, as the likelihood's own batches
    from mbb_emcee_amd import goodness
    c3, q3, s3 = goodness.goodness_rows(multi, chain.reshape(-1, 5))
    for s in range(3):
        chi, q, _ = _entries(mbb, _one(mbb, flux[s], unc[s]), chain[s])
        assert np.array_equal(c3.reshape(3, -1)[s], chi) and np.array_equal(q3.reshape(3, -1)[s], q)
    with pytest.raises(ValueError, match="equal blocks"):
        goodness.goodness_rows(multi, chain.reshape(-1, 5)[:-1])
    # one shared one-source context serves a three-source chain; the result keeps its leading axis
    shared = mbb.chain_goodness(base, chain, lnprob=lnprob, **kw)
    assert shared.chisq_mean.shape == (3,) and shared.pulls.shape == (3, 4)
    for s in range(3):
        alone = mbb.chain_goodness(base, chain[s], lnprob=lnprob[s], **kw)
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(shared._raw, f)[s], getattr(alone._raw, f)[0], equal_nan=True), (s, f)
    with pytest.raises(ValueError, match="2 sources, the likelihood 3"):
        mbb.chain_goodness(multi, chain[:2])


def _one(mbb, flux, unc):
    one = mbb.likelihood(response=True)
    one.set_phot(BANDS4, flux, unc)
    return one


# ---------------------------------------------------------------- 5. chunk seam
def test_chunk_seam(mbb, oracle, g_lnl, g_pb, g_res):
    """5. A compact [3, 300, 300] chain, 270 000 rows: the second fill chunk (2^18 rows) begins inside the last source.
    It is tiled from 64 distinct rows whose cell values come from one 64-source call, so every source's statistics are
    numpy's on the gathered column, exactly."""
    from conftest import ROOT
    assert SR.chunk_rows(ROOT) == 1 << 18
    like, _ = _setup(mbb, oracle, g_lnl, g_pb, g_res["thick_walpha/chain"], False, False, "bands4")
    rows = g_res["thick_walpha/chain"].reshape(-1, 5)[::8][:64]
    chi, q, _ = _entries(mbb, like, rows)
    assert len(set(chi)) == 64
    rng = np.random.RandomState(21)
    idx = rng.randint(0, 64, size=(3, 300, 300))
    chain = np.ascontiguousarray(rows[idx])
    assert 2 * 300 * 300 < (1 << 18) < 3 * 300 * 300
    for burn, thin in ((0, 1), (7, 3)):
        g = mbb.chain_goodness(like, chain, percentile=(68.3, 95.4), percentiles=(0.0, 100.0), burn=burn, thin=thin)
        qs = g.percentiles[0]
        for s in range(3):
            wi = idx[s][:, burn::thin]
            _check_column(g._raw, s, 0, chi[wi].reshape(-1), qs, "seam source %d chisq" % s)
            _check_column(g._raw, s, 1, q[wi].reshape(-1), qs, "seam source %d q" % s)
            w, k = np.unravel_index(np.argmin(chi[wi]), wi.shape)
            assert tuple(g._raw.ml_index[s]) == (w, burn + k * thin) and g._raw.ml[s, 5] == chi.min()
            assert np.array_equal(g._raw.ml[s, :5], rows[np.argmin(chi)])
        assert np.all(g._raw.status == 0)


# ---------------------------------------------------------------- 6. bad rows
def test_bad_rows(mbb, oracle, g_lnl, g_pb, g_res):
    """6. SED-failing and NaN rows outside the window change nothing; inside it they set the row-status bit and HAS_NAN
    and make the mean NaN, as a summary's derived column reports them; the ML entry skips them; a source of NaN rows
    has NaN everywhere and index -1."""
    from mbb_emcee_amd import _native
    base = np.ascontiguousarray(g_res["thick_walpha/chain"][:30].reshape(3, 10, 16, 5))
    like, _ = _setup(mbb, oracle, g_lnl, g_pb, g_res["thick_walpha/chain"], False, False, "bands4")
    kw = dict(burn=4, thin=3)                                           # kept steps 4, 7, 10, 13
    good = mbb.chain_goodness(like, base, **kw)
    assert np.all(good.status == 0) and np.all(good.n_used == 40)
    out = base.copy()
    out[1, 2, 5, 3] = -1.0                                              # alpha <= 0 at a step that is not kept
    out[2, 0, 8, 0] = np.nan
    assert _same_bits(mbb.chain_goodness(like, out, **kw), good)
    ins = base.copy()
    ins[1, 2, 7, 3] = -1.0
    ml1 = tuple(good._raw.ml_index[1])
    ins[1, ml1[0], ml1[1], 1] = -0.5                                    # beta < 0 at the ML entry itself
    g = mbb.chain_goodness(like, ins, **kw)
    bits = (1 << (_native.SUM_ROW_SHIFT + _native.ROW_BAD_ALPHA)) | (1 << (_native.SUM_ROW_SHIFT + _native.ROW_BAD_BETA))
    assert np.all(g.status[1] == (bits | _native.SUM_HAS_NAN)) and np.all(g.status[[0, 2]] == 0)
    assert np.all(np.isnan(g._raw.mean[1])) and np.all(np.isnan(g._raw.pct[1])) and np.all(g._raw.n_used[1] == 40)
    for f in RAW_FIELDS:
        assert np.array_equal(getattr(g._raw, f)[[0, 2]], getattr(good._raw, f)[[0, 2]], equal_nan=True), f
    with pytest.raises(ValueError, match="alpha must be positive|beta must be non-negative"):
        g.chisq_cen()
    # the ML entry of source 1 is the best of the rows that are left
    chi = _entries(mbb, like, base[1])[0].reshape(10, 16)
    chi[2, 7] = chi[ml1] = np.nan
    wc = chi[:, 4::3]
    w, k = np.unravel_index(np.nanargmin(wc), wc.shape)
    assert tuple(g._raw.ml_index[1]) == (w, 4 + 3 * k) and g._raw.ml[1, 5] == wc[w, k] and np.all(np.isfinite(g._raw.ml_model[1]))
    # a NaN parameter: HAS_NAN and the NONFINITE row bit, no raise
    nn = base.copy()
    nn[0, 3, 10, 0] = np.nan
    g = mbb.chain_goodness(like, nn, **kw)
    assert g.status[0, 0] == ((1 << (_native.SUM_ROW_SHIFT + _native.ROW_NONFINITE)) | _native.SUM_HAS_NAN)
    assert np.isnan(g.chisq_cen()[0, 0]) and np.isfinite(g._raw.ml[0, 5]) and np.isnan(g._raw.at_mean[0, 0])
    # a whole source of NaN rows
    allnan = base.copy()
    allnan[2] = np.nan
    g = mbb.chain_goodness(like, allnan, lnprob=np.zeros((3, 10, 16)), **kw)
    assert np.all(np.isnan(g._raw.ml[2])) and np.all(g._raw.ml_index[2] == -1) and np.all(np.isnan(g._raw.ml_model[2]))
    assert np.all(np.isnan(g._raw.at_mean[2])) and np.all(np.isnan(g._raw.mean[2])) and np.all(np.isnan(g._raw.best[2]))
    assert np.array_equal(g._raw.ml[:2], good._raw.ml[:2]) and np.array_equal(g._raw.mean[:2], good._raw.mean[:2])


# ---------------------------------------------------------------- 7. stale state
def test_smaller_call_after_a_larger_one(mbb, oracle, g_lnl, g_pb, g_res):
    """7. A small call gives the same bits before and after a larger one with other data, other bands and failing rows
    has used the same work buffers."""
    chain = g_res["thick_walpha/chain"]
    small_like, _ = _setup(mbb, oracle, g_lnl, g_pb, chain, False, False, "delta2")
    small = np.ascontiguousarray(chain[:3, :5])
    lp = np.ascontiguousarray(g_res["thick_walpha/lnprobability"][:3, :5])
    before = mbb.chain_goodness(small_like, small, lnprob=lp, burn=1)
    big = np.ascontiguousarray(np.tile(chain, (4, 1, 1)).reshape(4, 32, 16, 5))
    big[1, :, 3, 3] = -1.0
    for case in ("cov12", "delta2", "bands4"):
        like, _ = _setup(mbb, oracle, g_lnl, g_pb, chain, False, False, case)
        g = mbb.chain_goodness(like, big, lnprob=np.zeros((4, 32, 16)), percentile=(68.3, 95.4, 99.7))
        assert g.status[1, 0] != 0 and np.all(g.status[[0, 2, 3]] == 0)
        assert _same_bits(mbb.chain_goodness(small_like, small, lnprob=lp, burn=1), before), case
    assert _same_bits(mbb.chain_goodness(small_like, small, burn=1), before, RAW_FIELDS[:10])
    assert np.all(mbb.chain_goodness(small_like, small, burn=1)._raw.best_index == -1)


# ---------------------------------------------------------------- 8. resident chain
def _sampler_case(mbb, g_lnl, multi):
    """The golden 8-band photometry, one source or three (tests/test_predict_gpu.py's)."""
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rng = np.random.RandomState(11)
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    if multi:
        ns = 3
        truths = np.column_stack([rng.uniform(8, 20, ns), rng.uniform(1.2, 2.4, ns), rng.uniform(300, 900, ns),
                                  rng.uniform(2, 4.5, ns), rng.uniform(10, 80, ns)])
        flux = one.model_flux(truths)
        lk = mbb.likelihood(response=True)
        lk.set_phot_multi(bands, flux, 0.1 * flux + 1.0)
        p0 = truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, NW, 5)))
    else:
        truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
        flux = one.model_flux(truth)[0]
        lk = mbb.likelihood(response=True)
        lk.set_phot(bands, flux, 0.1 * flux + 1.0)
        p0 = truth * (1.0 + 0.02 * rng.normal(size=(NW, 5)))
    return lk, p0, bands


@pytest.mark.parametrize("multi", [False, True])
def test_resident_chain(mbb, g_lnl, multi):
    """8. sampler.goodness() and run_mcmc(storechain=False, summary=, goodness=) equal chain_goodness on the chain a
    storechain=True run of the same seed brings back, bit for bit; the summary, diagnostics, marginals, predictions and
    draws of that run are what they are without goodness= -- also when asked again after it has used the shared
    derived-column block."""
    lk, p0, bands = _sampler_case(mbb, g_lnl, multi)
    a = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.goodness_ is None
    gkw = dict(percentile=(68.3, 95.4), burn=5, thin=2)
    host = mbb.chain_goodness(lk, a.chain, lnprob=a.lnprobability, **gkw)
    res = a.goodness(**gkw)
    assert _same_bits(res, host) and res.nsteps_used == 30 and res.nwalkers == NW
    assert res.chisq_mean.shape == ((3,) if multi else ()) and np.all(res.status == 0) and np.all(res.n_used == NW * 30)
    assert np.all(res.best_index >= 0) and np.all(res.chisq_min <= res.best_fit_chisq)
    skw = dict(burn=5, thin=2, derived=("peaklambda",), percentile=(68.3, 95.4))
    mkw = dict(bins=24, bins2d=6)
    specs = [bands[3], 70.0]
    b = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b.run_mcmc(p0, NSTEPS, storechain=False, summary=dict(skw), convergence=True, marginals=dict(mkw), predict=specs, draws=9,
               goodness=dict(percentile=(68.3, 95.4)))
    assert b.chain.shape[-2] == 0 and b.goodness_.burn == 5 and b.goodness_.thin == 2             # the summary's window
    assert _same_bits(b.goodness_, host) and _same_bits(b.goodness(**gkw), host)
    c = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    c.run_mcmc(p0, NSTEPS, storechain=False, summary=dict(skw), convergence=True, marginals=dict(mkw), predict=specs, draws=9)
    assert c.goodness_ is None
    assert SR.raw_equal(b.summary, c.summary)
    for f in ("tau", "ess", "rhat", "window", "status"):
        assert np.array_equal(getattr(b.convergence_, f), getattr(c.convergence_, f), equal_nan=True), f
    for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below", "n_above", "n_nonfinite", "status"):
        assert np.array_equal(getattr(b.marginals_._raw, f), getattr(c.marginals_._raw, f), equal_nan=True), f
    for f in ("n_used", "mean", "min", "max", "pct", "status"):
        assert np.array_equal(getattr(b.predictions_._raw, f), getattr(c.predictions_._raw, f), equal_nan=True), f
    for k, v in c.draws_.arrays().items():
        assert np.array_equal(b.draws_.arrays()[k], v, equal_nan=True), k
    # after goodness() has used the derived-column block again: the other analyses from the resident chain
    b.goodness(**gkw)
    assert np.array_equal(b.summary.peaklambda_cen(90.0), c.summary.peaklambda_cen(90.0))
    assert np.array_equal(b.convergence(burn=5).tau, c.convergence(burn=5).tau)
    assert np.array_equal(b.predictions(specs, burn=5).mean, c.predictions(specs, burn=5).mean)
    mb, mc = b.marginals(derived=("peaklambda",), **mkw), c.marginals(derived=("peaklambda",), **mkw)
    for f in ("counts1", "edges1", "counts2", "status"):
        assert np.array_equal(getattr(mb._raw, f), getattr(mc._raw, f), equal_nan=True), f
    b.run_mcmc(None, 3, storechain=False)                   # the next run: nothing of it is resident
    assert b.goodness_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.goodness()
    b.run_mcmc(None, 9, goodness=True)
    last = mbb.chain_goodness(lk, b.chain[..., -9:, :], lnprob=b.lnprobability[..., -9:])
    assert b.goodness_.nsteps_used == 9 and _same_bits(b.goodness_, last)
    b.reset()
    assert b.goodness_ is None


def test_fitter_and_cli_goodness(mbb, g_lnl, tmp_path, capsys):
    """mbb_fitter.run(..., goodness=...) and the CLI's --goodness end to end: the numbers are those of the chain the
    fit returns; without the flag nothing new is printed or written."""
    from mbb_emcee_amd import run_mbb_emcee
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    flux = one.model_flux(truth)[0]
    fit = mbb.mbb_fitter(nwalkers=NW, response=True, seed=3)
    fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    fit.run(20, NSTEPS, p0, goodness=True)
    assert fit.goodness is not None and fit.summary is None
    assert _same_bits(fit.goodness, mbb.chain_goodness(fit.like, fit.sampler.chain, lnprob=fit.sampler.lnprobability))
    fit.run(20, 16, p0, goodness=dict(burn=2), summary=True)
    assert _same_bits(fit.goodness, mbb.chain_goodness(fit.like, fit.sampler.chain, lnprob=fit.sampler.lnprobability, burn=2))
    fit.run(20, 16, p0)
    assert fit.goodness is None                                          # the default leaves none
    capsys.readouterr()
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", str(NW), "-b", "20", "-N", str(NSTEPS), "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--goodness"]) == 0
    text = capsys.readouterr().out
    assert "ChiSquare over the chain" in text and "Posterior predictive p-value" in text and "DIC" in text
    got = np.load(out)
    new = {k for k in got.files if k.startswith("goodness_")}
    assert {"goodness_dic", "goodness_pulls", "goodness_ml_params", "goodness_mean", "goodness_best_fit_chisq"} <= new
    like = mbb.likelihood(str(pf), response=True)
    want = mbb.chain_goodness(like, got["chain"], lnprob=got["lnprobability"])
    for k, v in want.arrays().items():
        assert np.array_equal(got[k], v, equal_nan=True), k
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == "" and not any(k.startswith("goodness_") for k in np.load(out).files)


# ---------------------------------------------------------------- 9. refusals of the C-ABI
def _native_call(like, chain, lnprob=None, qs=(16.0, 84.0), burn=0, thin=1, nsrc=None, nw=None, nsteps=None, edit=None):
    from mbb_emcee_amd import _native, goodness
    ctx = _native.analysis_context(like)
    s = _native.GoodnessSpec()
    s.npct, s.burn, s.thin = len(qs), burn, thin
    for i, q in enumerate(qs[:_native.SUMMARY_MAX_PCT]):
        s.pct[i] = q
    raw = goodness._Raw(chain.shape[0], int(like._ndata), max(1, min(len(qs), _native.SUMMARY_MAX_PCT)))
    out = raw.out()
    if edit:
        edit(s, out)
    rc = ctx.lib.mbb_chain_goodness(ctx.h, _native._d(chain), None if lnprob is None else _native._d(lnprob),
                                    chain.shape[0] if nsrc is None else nsrc, chain.shape[1] if nw is None else nw,
                                    chain.shape[2] if nsteps is None else nsteps, C.byref(s), C.byref(out))
    return rc, raw, ctx


def test_native_refusals_leave_the_context_usable(mbb, oracle, g_lnl, g_pb, g_res):
    """9. The C-ABI's refusals, each before anything is allocated or uploaded and each followed by a good call that
    gives the right answer: MBB_ERR_ARG for arguments and sources, MBB_ERR_STATE without bands or data, and
    mbb_sampler_goodness's MBB_ERR_STATE without a resident chain."""
    from mbb_emcee_amd import _native, goodness
    like, _ = _setup(mbb, oracle, g_lnl, g_pb, g_res["thick_walpha/chain"], False, False, "bands4")
    chain = np.ascontiguousarray(g_res["thick_walpha/chain"][None, :7, :])          # 1 x 7 x 16
    rc, ref, ctx = _native_call(like, chain, burn=2)
    assert rc == 0 and np.all(ref.n_used == 7 * 14)

    def good():
        rc, raw, _ = _native_call(like, chain, burn=2)
        assert rc == 0
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(raw, f), getattr(ref, f), equal_nan=True), f

    nan = float("nan")
    bad = [(dict(qs=()), "percentiles per"), (dict(qs=tuple(range(9))), "percentiles per"),
           (dict(qs=(50.0, 100.5)), "[0, 100]"), (dict(qs=(-1.0,)), "[0, 100]"), (dict(qs=(nan,)), "[0, 100]"),
           (dict(burn=16), "burn"), (dict(burn=-1), "burn"), (dict(thin=0), "burn"),
           (dict(nsteps=0), "empty chain"), (dict(nw=0), "empty chain"), (dict(nsrc=0), "empty chain")]
    for kw, msg in bad:
        kw = dict(kw)
        kw.setdefault("burn", 2)
        rc, _, _ = _native_call(like, chain, **kw)
        assert rc == -2 and msg in ctx.lib.mbb_last_error().decode(), (msg, rc, ctx.lib.mbb_last_error())
        good()
    # more than 2^32 - 1 samples per column: refused from the shape alone, before the (far too short) chain is read
    rc, _, _ = _native_call(like, chain, nw=1 << 16, nsteps=1 << 16)
    assert rc == -2 and "2^32 - 1 samples per column" in ctx.lib.mbb_last_error().decode()
    good()
    # the chain's sources: the context's, or the context holds one
    three = np.ascontiguousarray(np.tile(chain, (3, 1, 1, 1)))
    assert _native_call(like, three)[0] == 0
    multi = mbb.likelihood(response=True)
    multi.set_phot_multi(BANDS4, np.tile(like._flux, (3, 1)), np.tile(like._flux_unc, (3, 1)))
    assert _native_call(multi, three)[0] == 0
    rc, _, mctx = _native_call(multi, np.ascontiguousarray(three[:2]))
    assert rc == -2 and "sources" in mctx.lib.mbb_last_error().decode()
    assert _native_call(multi, three)[0] == 0

    def drop(field, of_spec=False):
        def edit(spec, out):
            setattr(out, field, None)
        return edit
    for field in [f[0] for f in _native.GoodnessOut._fields_]:
        assert _native_call(like, chain, edit=drop(field))[0] == -2, field
    s, out = _native.GoodnessSpec(), goodness._Raw(1, 4, 1).out()
    s.npct, s.burn, s.thin = 1, 0, 1
    s.pct[0] = 50.0
    assert ctx.lib.mbb_chain_goodness(ctx.h, None, None, 1, 7, 16, C.byref(s), C.byref(out)) == -2
    assert ctx.lib.mbb_chain_goodness(ctx.h, _native._d(chain), None, 1, 7, 16, None, C.byref(out)) == -2
    assert ctx.lib.mbb_chain_goodness(ctx.h, _native._d(chain), None, 1, 7, 16, C.byref(s), None) == -2
    good()
    # the rows call
    p = np.ascontiguousarray(chain.reshape(-1, 5))
    n = p.shape[0]
    c, q, st = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
    rows = lambda pp, nn, cc, qq, ss: ctx.lib.mbb_goodness_rows(ctx.h, pp, nn, cc, qq, ss, None)   # noqa: E731
    assert rows(_native._d(p), n, _native._d(c), _native._d(q), _native._i(st)) == 0
    assert rows(None, n, _native._d(c), _native._d(q), _native._i(st)) == -2
    assert rows(_native._d(p), 0, _native._d(c), _native._d(q), _native._i(st)) == -2
    assert rows(_native._d(p), n, None, _native._d(q), _native._i(st)) == -2
    assert rows(_native._d(p), n, _native._d(c), None, _native._i(st)) == -2
    assert rows(_native._d(p), n, _native._d(c), _native._d(q), None) == -2
    good()
    # no bands or data: MBB_ERR_STATE
    bare = _native.Context(None)
    bare.set_model(False, False, 500.0)
    assert bare.lib.mbb_chain_goodness(bare.h, _native._d(chain), None, 1, 7, 16, C.byref(s), C.byref(out)) == -3
    assert "bands not set" in bare.lib.mbb_last_error().decode()
    assert bare.lib.mbb_goodness_rows(bare.h, _native._d(p), n, _native._d(c), _native._d(q), _native._i(st), None) == -3
    bare.set_bands(*like.band_tables())
    assert bare.lib.mbb_chain_goodness(bare.h, _native._d(chain), None, 1, 7, 16, C.byref(s), C.byref(out)) == -3
    assert "data not set" in bare.lib.mbb_last_error().decode()
    # the sampler call
    lk, p0, _ = _sampler_case(mbb, g_lnl, False)
    sm = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=5)
    sctx, h = sm._handle()
    raw8 = goodness._Raw(1, 8, 1)
    out8 = raw8.out()
    assert sctx.lib.mbb_sampler_goodness(sctx.h, h, C.byref(s), C.byref(out8)) == -3
    assert "resident" in sctx.lib.mbb_last_error().decode()
    sm.run_mcmc(p0, 8, storechain=False)
    assert sctx.lib.mbb_sampler_goodness(sctx.h, h, C.byref(s), C.byref(out8)) == -3
    sm.run_mcmc(None, 8)
    assert sctx.lib.mbb_sampler_goodness(sctx.h, h, C.byref(s), C.byref(out8)) == 0 and raw8.n_used[0, 0] == NW * 8
    assert sctx.lib.mbb_sampler_goodness(sctx.h, h, None, C.byref(out8)) == -2
    assert sctx.lib.mbb_sampler_goodness(sctx.h, h, C.byref(s), None) == -2
    assert sctx.lib.mbb_sampler_goodness(sctx.h, None, C.byref(s), C.byref(out8)) == -2
    s.npct = 0
    assert sctx.lib.mbb_sampler_goodness(sctx.h, h, C.byref(s), C.byref(out8)) == -2
    s.npct = 1
    assert sctx.lib.mbb_sampler_goodness(sctx.h, h, C.byref(s), C.byref(out8)) == 0
    assert _same_bits(sm.goodness(), mbb.chain_goodness(lk, sm.chain, lnprob=sm.lnprobability))
