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
  * every row's band fluxes (goodness_rows(want_flux=True)) in the band layouts of section 10: relative 1e-12 from the
    oracle's;
  * q at every order 1 .. 256 through the test-only probe (section 11): on the order's 70 points
    (_goodness_ref.order_grid; asserted: at least 60 with a true q >= 1e-290, at least one below), relative 4 x the
    largest error scipy.special.gammaincc shows on those points; the even orders also (9 + 1.5 ceil(nb/2)) eps -- no
    library function enters them: m_exp twice at 2 ulp each, ceil(nb/2) Horner steps of one IEEE division and one fma
    at 1.5 ulp a step, three products (tests/test_goodness_cpu.py's derivation with the step count left free) --; the
    odd orders have the device library's erfc, the one term whose error this project does not own, and keep the outer
    bound only, their observed maximum recorded;
  * the kernel's q against the probe's m_gammq_half at the kernel's own chisq: bit for bit (one header, one set of
    device flags, no contraction: -ffp-contract=off);
  * counts, indices, status bits and everything said to be "the same bits": exact.
The entries are every row of the fixture chains tests/test_predict_gpu.py uses (tests/golden/results.npz: 32 x 16 per
model variant).

Section 10 runs what k_good_flux, k_good_chi and their host driver branch on (LAYOUTS): one-sample and many-sample
bands in one launch, many-sample bands shorter than a wave, samples read from global memory (STAGE = false) and the
2560 / 2561 seam of that decision, C^-1 in LDS and in global memory at 64 / 65 bands, kMaxBands = 256 bands with and
without a covariance, row counts off the wave and the workgroup, failing rows at their ends, several sources beyond the
seams, the row-chunk loop of mbb_goodness_rows, and the refusal at 257 bands.  The uncertainty scales of each case were
chosen on the CPU with the oracle alone (LAYOUT_SCALES); what they have to achieve is asserted.

The MAP fit reports these functions' values: tests/test_map_gpu.py asserts MapFit.chisq, q and model_flux bit for bit
equal to mbb_goodness_rows', so what they are worth rests on the tests here."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, golden_bands, parity_record, rec_allclose
import _goodness_ref as GR
import _hp_common as hp
import _map_ref as MR
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


# ---------------------------------------------------------------- 10. the band layouts the kernels branch on
MIX_ORDER = ["PACS_100um", "D_delta_70um", "PACS_160um", "E_delta_1100um", "SPIRE_250um", "SPIRE_350um", "SPIRE_500um",
             "SCUBA2_850um"]                                          # MIX_BANDS, one-sample and many-sample bands in turn
SHORT_BANDS = ["ALMA_box_145_7.5", "ALMA_alma_343", "SMA_gauss_345_8", "GISMO_2mm", "LABOCA_870um"]    # 11, 29, 43, 53, 94
LDS_SAMPLES, LDS_COV, MAX_BANDS = 2560, 64, 256                      # kLdsSamples, kLdsCov, kMaxBands (held to the source below)
# case -> (passbands, number of plain wavelengths, rho of the covariance, samples all bands have together, what is run)
LAYOUTS = {
    "mix": (MIX_ORDER, None, None, 1690, "both halves of k_good_flux in one launch, band order"),
    "short": (SHORT_BANDS, None, None, 230, "many-sample bands shorter than a wave"),
    "big": (MR.BIG_BANDS, None, None, 2796, "STAGE = false"),
    "seam2560": (MR.BIG_BANDS[:-1] + ["FILL"], None, None, LDS_SAMPLES, "the last staged count"),
    "seam2561": (MR.BIG_BANDS[:-1] + ["FILL"], None, None, LDS_SAMPLES + 1, "the first unstaged count"),
    "cov64": (None, LDS_COV, 0.2, LDS_COV, "the largest C^-1 in LDS"),
    "cov65": (None, LDS_COV + 1, 0.2, LDS_COV + 1, "the smallest C^-1 in global memory"),
    "cov256": (None, MAX_BANDS, 0.2, MAX_BANDS, "kMaxBands, nb^2 = 65 536 terms per row"),
    "delta256": (None, MAX_BANDS, None, MAX_BANDS, "kMaxBands, diagonal"),
    "bigcov": (MR.BIG_BANDS, None, 0.3, 2796, "unstaged samples and a covariance together"),
}
V = {v[0]: v for v in VARIANTS}
ONE_THIN_ONE_THICK = {"short": ("thin_walpha", "thick_noalpha"), "seam2560": ("thin_noalpha", "thick_walpha"),
                      "seam2561": ("thin_noalpha", "thick_walpha"), "cov64": ("thin_walpha", "thick_walpha"),
                      "cov65": ("thin_walpha", "thick_walpha"), "cov256": ("thin_noalpha", "thick_noalpha"),
                      "delta256": ("thin_walpha", "thick_noalpha"), "bigcov": ("thin_noalpha", "thick_walpha")}
LAYOUT_RUNS = [(c, v) for c in LAYOUTS for v in ([x[0] for x in VARIANTS] if c in ("mix", "big") else ONE_THIN_ONE_THICK[c])]


def _filler(tmp, n):
    """A passband of exactly n samples, from a file (tests/test_gpu_parity.py's way)."""
    from mbb_emcee_amd import response
    x = np.linspace(380.0, 520.0, n)
    t = np.exp(-0.5 * ((x - 450.0) / 40.0) ** 2)
    fn = os.path.join(str(tmp), "fill%d.txt" % n)
    np.savetxt(fn, np.column_stack([x, t]))
    r = response("FILL%d" % n)
    r.setup(fn, xtype="wave", xunits="microns", senstype="energy", normtype="power", xnorm=450.0, normparam=-1.0)
    return r


class _Layout(object):
    """A band case on both sides: the device likelihood, the oracle's band fluxes of the chain's rows (they do not depend
    on the data), and the data of _setup's recipe -- the oracle's model at the chain's middle row pushed 5% up and down
    band by band -- whose uncertainties scale (0.1 flux + 1), correlated with rho where the case has one, set() puts in
    place."""

    def __init__(self, mbb, oracle, g_pb, chain, opthin, noalpha, case, tmp):
        names, nwave, self.rho, self.nsamples, _ = LAYOUTS[case]
        self.case, self.rows = case, np.ascontiguousarray(np.asarray(chain).reshape(-1, 5))
        free = dict(opthin=opthin, noalpha=noalpha, lowlim=np.full(5, -np.inf), has_uplim=[0] * 6)
        if names is None:
            self.first = np.geomspace(60.0, 1500.0, nwave)
            self.like = mbb.likelihood(opthin=opthin, noalpha=noalpha)
            okw = dict(wave=self.first)
        else:
            self.like = mbb.likelihood(response=True, opthin=opthin, noalpha=noalpha)
            self.first, tables = [], []
            for n in names:
                if n == "FILL":
                    r = _filler(tmp, self.nsamples - (2796 - 1108))      # (BIG_BANDS without SCUBA2_450um has 1688 samples)
                    self.like._responsewheel._responses[r.name] = r
                    self.first.append(r.name)
                    tables.append((r.wavelength, r._sedmult, r._normfac))
                else:
                    self.first.append(n)
                    tables.extend(MR.band_tables(g_pb, [n]))
            okw = dict(bands=tables)
        self.nb = len(self.first)
        orc = oracle.OracleLikelihood(np.ones(self.nb), np.ones(self.nb), **okw, **free)
        self.model = orc(self.rows, return_flux=True)[1]
        assert np.all(orc.status == 0) and np.all(np.isfinite(self.model)) and self.model.shape == (self.rows.shape[0], self.nb)
        self.flux = self.model[self.rows.shape[0] // 2] * (1.0 + 0.05 * (-1.0) ** np.arange(self.nb))
        self.set(1.0)

    def set(self, scale):
        unc = scale * (0.1 * self.flux + 1.0)
        self.like.set_phot(self.first, self.flux, unc)
        if self.rho is not None:
            n = self.nb
            self.like.set_cov(np.outer(unc, unc) * (np.eye(n) + self.rho * (1.0 - np.eye(n))))      # (_map_ref.covariance's)
        return self.like

    def reference(self):
        """(chisq in longdouble on the oracle's band fluxes, its bound), for the data set() put in place"""
        w = _weights(self.like)
        return GR.chisq(self.like._flux, self.model, **w), GR.chisq_bound(self.like._flux, self.model, **w)


@pytest.fixture(scope="module")
def layouts(mbb, oracle, g_pb, g_res, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("goodness_fill")

    def get(case, name):
        if ("layout", case, name) not in _CACHE:
            _CACHE[("layout", case, name)] = _Layout(mbb, oracle, g_pb, g_res[name + "/chain"], V[name][1], V[name][2], case, tmp)
        return _CACHE[("layout", case, name)]
    return get


LAYOUT_SCALES = {           # chosen on the CPU with the oracle alone (the conditions on them are asserted in the test)
    ("mix", "thin_walpha"): (1.0, 1.5, 2.0), ("mix", "thick_walpha"): (1.0, 1.5, 2.0),
    ("mix", "thick_noalpha"): (0.5, 0.7, 1.0), ("mix", "thin_noalpha"): (2.0, 3.0, 5.0),
    ("short", "thin_walpha"): (0.3, 0.5, 1.0), ("short", "thick_noalpha"): (0.5, 0.7, 1.0),
    ("big", "thin_walpha"): (1.0, 1.5, 2.0), ("big", "thick_walpha"): (1.0, 1.5, 2.0),
    ("big", "thick_noalpha"): (0.5, 0.7, 1.5), ("big", "thin_noalpha"): (1.5, 2.0, 3.0),
    ("seam2560", "thin_noalpha"): (1.5, 2.0, 3.0), ("seam2560", "thick_walpha"): (1.0, 1.5, 2.0),
    ("seam2561", "thin_noalpha"): (1.5, 2.0, 3.0), ("seam2561", "thick_walpha"): (1.0, 1.5, 2.0),
    ("cov64", "thin_walpha"): (1.0, 1.5, 2.0), ("cov64", "thick_walpha"): (1.0, 1.5, 2.0),
    ("cov65", "thin_walpha"): (1.0, 1.5, 2.0), ("cov65", "thick_walpha"): (1.0, 1.5, 2.0),
    ("cov256", "thin_noalpha"): (1.0, 1.5, 2.0), ("cov256", "thick_noalpha"): (1.5, 2.0, 3.0),
    ("delta256", "thin_walpha"): (2.0, 3.0, 5.0), ("delta256", "thick_noalpha"): (2.0, 3.0, 5.0),
    ("bigcov", "thin_noalpha"): (1.5, 2.0, 3.0), ("bigcov", "thick_walpha"): (1.0, 1.5, 2.0),
}


@pytest.fixture(scope="module")
def probe():
    p = hp.probe_module().load()
    assert not p.is_host
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _ulps_apart(a, b):
    """distance in representable doubles between two arrays of non-negative finite doubles"""
    return np.abs(_bits(a) - _bits(b))


def _same_entry_point(probe, nb, chi, q):
    """The kernel's q is the probe's m_gammq_half at the kernel's own chisq: the function part A judged is the one
    k_good_chi calls.  Both are compiled from csrc/mbb_gammq.hip.h with the same device flags; bit for bit."""
    want = probe.gammq(nb, chi)
    nan = np.isnan(chi)
    assert np.array_equal(np.isnan(q), nan) and np.array_equal(np.isnan(want), nan)
    apart = _ulps_apart(q[~nan], want[~nan])
    parity_record("q of the kernel vs the probe's m_gammq_half [ulp]", apart.max() if apart.size else 0, 0)
    assert np.array_equal(q, want, equal_nan=True), (nb, apart.max(), chi[~nan][apart.argmax()])


def test_layout_constants_are_the_sources():
    src = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_goodness.hip.h")).read()
    assert "constexpr int kLdsSamples = %d;" % LDS_SAMPLES in src and "constexpr int kLdsCov = %d;" % LDS_COV in src
    assert "constexpr int kLdsSamples = 2560;" in src and "constexpr int kLdsCov = 64;" in src
    assert "constexpr int kMaxBands = mbbm::kGammqMaxNb;" in src
    gq = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_gammq.hip.h")).read()
    assert "constexpr int kGammqMaxNb = %d;" % MAX_BANDS in gq and GR.MAX_NB == MAX_BANDS
    assert set(LAYOUT_SCALES) == set(LAYOUT_RUNS)
    for c in LAYOUTS:                                                   # at least one thin and one thick variant of each
        vs = [v for cc, v in LAYOUT_RUNS if cc == c]
        assert any(V[v][1] for v in vs) and any(not V[v][1] for v in vs), c


@pytest.mark.parametrize("case,name", LAYOUT_RUNS)
def test_band_layouts(mbb, oracle, layouts, probe, case, name):
    """10. Every row of the fixture chain at three uncertainty scales, in a band layout the kernels branch on (LAYOUTS):
    every row's band fluxes against the oracle's, chisq within its bound through the chain path and through
    goodness_rows (the same bits), q against mpmath at the device's own chisq and bit for bit the probe's
    m_gammq_half."""
    pytest.importorskip("mpmath")
    from scipy.special import gammaincc
    from mbb_emcee_amd import goodness
    L = layouts(case, name)
    nb, rows = L.nb, L.rows
    pts_x, pts_q = [], []
    for scale in LAYOUT_SCALES[(case, name)]:
        like = L.set(scale)
        freq, wt, offs = like.band_tables()
        assert freq.size == L.nsamples and offs.size == nb + 1, (case, freq.size)
        assert like._has_covmatrix == (L.rho is not None)
        chi, q, st, fl = goodness.goodness_rows(like, rows, want_flux=True)
        assert np.all(st == 0) and fl.shape == (rows.shape[0], nb)
        rec_allclose(fl, L.model, rtol=1e-12, kind="band flux per row vs oracle")
        cc, qc, g = _entries(mbb, like, rows)
        assert np.array_equal(cc, chi) and np.array_equal(qc, q)            # the chain path: the same bits
        ref, bound = L.reference()
        err = np.abs((chi.astype(GR.LD) - ref).astype(np.float64)) / bound
        print("    %s %s scale %g: chisq %.3g .. %.3g, worst %.3g of its bound" % (name, case, scale, chi.min(), chi.max(), err.max()))
        rec_allclose(err, 0.0, rtol=0, atol=1, kind="chisq per entry, band layouts [its bound]")
        assert g.ndata == nb and np.array_equal(g._raw.ml_model, fl)        # (one entry per source: it is the ML entry)
        _same_entry_point(probe, nb, chi, q)
        pts_x.append(chi); pts_q.append(q)
    x, q = np.concatenate(pts_x), np.concatenate(pts_q)
    truth = [GR.q_mp(nb, v) for v in x]
    big = np.array([t >= GR.Q_FLOOR for t in truth])
    informative = np.array([GR.Q_FLOOR <= t <= 0.99 for t in truth])
    print("    %s %s: %d of %d entries with 1e-290 <= true q <= 0.99, %d above, %d below 1e-290"
          % (name, case, informative.sum(), x.size, sum(t > 0.99 for t in truth), (~big).sum()))
    # conditions on the inputs: the scales make the case judge the function
    assert 4 * informative.sum() >= x.size and any(t > 0.99 for t in truth) and (~big).sum() >= 1
    scipy_err = GR.rel_errors(truth, big, gammaincc(0.5 * nb, 0.5 * x)).max()
    rec_allclose(scipy_err, 0.0, rtol=0, atol=1e-12, kind="scipy gammaincc vs mpmath on the test's points")
    dev = GR.rel_errors(truth, big, q)
    print("    %s %s: q worst relative %.3g; scipy's on the same points %.3g" % (name, case, dev.max(), scipy_err))
    rec_allclose(dev / (4.0 * scipy_err), 0.0, rtol=0, atol=1, kind="q per entry, band layouts [4 x scipy's error]")
    assert np.all(q[~big] >= 0.0) and np.all(q[~big] <= 1e-289) and np.all((q >= 0) & (q <= 1))


def test_staging_seam_shares_its_bands_bit_for_bit(layouts):
    """2560 samples are staged in LDS, 2561 are read from global memory: the six bands the two cases share give the same
    bits in both, so moving the seam by one (<= to < in good_eval) changes nothing that is right on both sides."""
    from mbb_emcee_amd import goodness
    for name in ONE_THIN_ONE_THICK["seam2560"]:
        a, b = layouts("seam2560", name), layouts("seam2561", name)
        la, lb = a.set(1.0), b.set(1.0)
        na, nb_ = la.band_tables()[0].size, lb.band_tables()[0].size
        assert (na, nb_) == (LDS_SAMPLES, LDS_SAMPLES + 1) and a.nb == b.nb == 7
        assert np.array_equal(la.band_tables()[2][:7], lb.band_tables()[2][:7])          # the shared bands: the same samples
        _, _, sa, fa = goodness.goodness_rows(la, a.rows, want_flux=True)
        _, _, sb, fb = goodness.goodness_rows(lb, b.rows, want_flux=True)
        assert np.all(sa == 0) and np.all(sb == 0)
        assert np.array_equal(fa[:, :6], fb[:, :6]), name
        assert not np.array_equal(fa[:, 6], fb[:, 6])                                     # (the filler bands do differ)
        # ... and with the filler's datum given no weight, chisq and q too
        for L in (a, b):
            unc = 0.1 * L.flux + 1.0
            unc[6] = np.inf
            L.like.set_phot(L.first, L.flux, unc)
        ca, qa, _ = goodness.goodness_rows(a.like, a.rows)
        cb, qb, _ = goodness.goodness_rows(b.like, b.rows)
        assert np.array_equal(ca, cb) and np.array_equal(qa, qb) and np.all(np.isfinite(ca)) and np.all(ca > 0)
    # the same for C^-1 in LDS and in global memory: 64 wavelengths are the first 64 of no 65-wavelength case (geomspace),
    # so that seam is held by cov64 and cov65 each being right; here only that they are on either side of kLdsCov
    assert LAYOUTS["cov64"][1] == LDS_COV and LAYOUTS["cov65"][1] == LDS_COV + 1


def test_mix_layout_runs_both_halves(layouts):
    """A condition on the input of `mix`: one-sample bands of weight exactly 1 (k_good_flux's lane-per-row half) between
    bands of many samples (its wave-per-row half)."""
    like = layouts("mix", "thin_walpha").set(1.0)
    freq, wt, offs = like.band_tables()
    n = np.diff(offs)
    assert list(n == 1) == [False, True, False, True, False, False, False, False] and np.all(wt[offs[:-1][n == 1]] == 1.0)
    assert freq.size == 1690 and np.all(n[n > 1] % 64 != 0)
    short = layouts("short", "thin_walpha").set(1.0)
    assert list(np.diff(short.band_tables()[2])) == [11, 29, 43, 53, 94]


@pytest.mark.parametrize("name", ["thin_walpha", "thick_noalpha"])
def test_row_counts_off_the_wave_and_the_workgroup(layouts, name):
    """goodness_rows on the first n rows of `mix`, n around the wave (64) and the workgroup (256): chisq, q, status and
    fluxes are those of the same rows inside the 512-row call."""
    from mbb_emcee_amd import goodness
    L = layouts("mix", name)
    like = L.set(LAYOUT_SCALES[("mix", name)][1])
    full = goodness.goodness_rows(like, L.rows, want_flux=True)
    assert np.all(full[2] == 0) and np.all(np.isfinite(full[3]))
    for n in (1, 63, 64, 65, 255, 257):
        part = goodness.goodness_rows(like, L.rows[:n], want_flux=True)
        for got, want in zip(part, full):
            assert got.shape[0] == n and np.array_equal(got, want[:n]), n


@pytest.mark.parametrize("name", ["thin_walpha", "thick_walpha"])
def test_failing_rows_in_a_mixed_layout(layouts, name):
    """Rows the constructor refuses (test_bad_rows': alpha <= 0, beta < 0, a NaN) at the ends of waves and workgroups
    of a 300-row `mix` call: a nonzero status, NaN in every band, one-sample and many-sample alike, NaN chisq and q;
    every other row keeps its bits."""
    from mbb_emcee_amd import goodness
    L = layouts("mix", name)
    like = L.set(LAYOUT_SCALES[("mix", name)][1])
    rows = L.rows[:300].copy()
    clean = goodness.goodness_rows(like, rows, want_flux=True)
    assert np.all(clean[2] == 0)
    where = [0, 63, 64, 255, 256, 299]
    for k, i in enumerate(where):
        if k % 3 == 0:
            rows[i, 3] = -1.0
        elif k % 3 == 1:
            rows[i, 1] = -0.5
        else:
            rows[i, 0] = np.nan
    chi, q, st, fl = goodness.goodness_rows(like, rows, want_flux=True)
    assert np.all(st[where] != 0) and np.all(np.isnan(fl[where])) and np.all(np.isnan(chi[where])) and np.all(np.isnan(q[where]))
    rest = np.setdiff1d(np.arange(300), where)
    for got, want in zip((chi, q, st, fl), clean):
        assert np.array_equal(got[rest], want[rest])


@pytest.mark.parametrize("case", ["cov65", "big"])
def test_multi_source_beyond_the_seams(mbb, layouts, case):
    """Three sources of different scale with diagonal uncertainties, 65 wavelengths (more than C^-1 has LDS for, were
    there one) and `big` (unstaged samples): each source is bit for bit its own one-source call."""
    from mbb_emcee_amd import goodness
    L = layouts(case, "thick_walpha")
    response = not isinstance(L.first, np.ndarray)
    flux = L.flux[None, :] * np.array([1.0, 37.0, 0.004])[:, None]
    unc = 0.1 * flux + np.array([1.0, 5.0, 0.01])[:, None]
    multi = mbb.likelihood(response=response, opthin=False, noalpha=False)
    multi.set_phot_multi(L.first, flux, unc)
    rows = L.rows[:3 * 100]
    c3, q3, s3, f3 = goodness.goodness_rows(multi, rows, want_flux=True)
    chain = np.ascontiguousarray(rows.reshape(3, 10, 10, 5))
    g = mbb.chain_goodness(multi, chain, percentile=(68.3, 95.4), burn=1, thin=2)
    assert np.all(s3 == 0) and len(set(g.chisq_mean)) == 3
    one = mbb.likelihood(response=response, opthin=False, noalpha=False)
    for s in range(3):
        one.set_phot(L.first, flux[s], unc[s])
        c1, q1, s1, f1 = goodness.goodness_rows(one, rows[100 * s:100 * (s + 1)], want_flux=True)
        sl = slice(100 * s, 100 * (s + 1))
        assert np.array_equal(c3[sl], c1) and np.array_equal(q3[sl], q1) and np.array_equal(f3[sl], f1) and np.all(s1 == 0)
        alone = mbb.chain_goodness(one, chain[s], percentile=(68.3, 95.4), burn=1, thin=2)
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(g._raw, f)[s], getattr(alone._raw, f)[0], equal_nan=True), (case, s, f)


def test_row_chunks_of_goodness_rows(mbb, oracle, g_lnl, g_pb, g_res):
    """The row-chunk loop of mbb_goodness_rows (2^18 rows a chunk), two wavelengths, rows tiled from a fixture chain:
    one source and 2^18 + 65 rows -- the rows around the seam and the first 64 are bit for bit a call of those rows
    alone --; three sources of 87 403 rows, the seam inside the last -- each is bit for bit its one-source call."""
    from mbb_emcee_amd import goodness
    seam = SR.chunk_rows(ROOT)
    assert seam == 1 << 18
    like, _ = _setup(mbb, oracle, g_lnl, g_pb, g_res["thick_walpha/chain"], False, False, "delta2")
    base = g_res["thick_walpha/chain"].reshape(-1, 5)
    n = seam + 65
    rows = np.ascontiguousarray(np.tile(base, (n // base.shape[0] + 1, 1))[:n])
    chi, q, st, fl = goodness.goodness_rows(like, rows, want_flux=True)
    # (a chain repeats the rows of rejected moves; enough of the 129 rows around the seam differ for a misplaced one to show)
    assert np.all(st == 0) and np.all(np.isfinite(chi)) and len(set(chi[seam - 64:seam + 65])) > 64
    for sl in (slice(seam - 64, seam + 65), slice(0, 64)):
        part = goodness.goodness_rows(like, rows[sl], want_flux=True)
        for got, want in zip(part, (chi, q, st, fl)):
            assert np.array_equal(got, want[sl]), sl
    # ... and every row is the row of the chain it was tiled from
    c0, q0, _, f0 = goodness.goodness_rows(like, base, want_flux=True)
    idx = np.arange(n) % base.shape[0]
    assert np.array_equal(chi, c0[idx]) and np.array_equal(q, q0[idx]) and np.array_equal(fl, f0[idx])
    per = 87403
    assert 2 * per < seam < 3 * per
    flux = like._flux[None, :] * np.array([1.0, 37.0, 0.004])[:, None]
    unc = 0.1 * flux + np.array([1.0, 5.0, 0.01])[:, None]
    multi = mbb.likelihood()
    multi.set_phot_multi(DELTA[:2], flux, unc)
    rows3 = np.ascontiguousarray(np.tile(base, (3 * per // base.shape[0] + 1, 1))[:3 * per])
    c3, q3, s3 = goodness.goodness_rows(multi, rows3)
    one = mbb.likelihood()
    for s in range(3):
        one.set_phot(DELTA[:2], flux[s], unc[s])
        sl = slice(per * s, per * (s + 1))
        c1, q1, s1 = goodness.goodness_rows(one, rows3[sl])
        assert np.array_equal(c3[sl], c1) and np.array_equal(q3[sl], q1) and np.array_equal(s3[sl], s1) and np.all(s1 == 0), s
    assert len({c3[0], c3[per], c3[2 * per]}) == 3


def test_257_bands_are_refused_through_the_c_abi(layouts):
    """A context with 257 bands: mbb_chain_goodness and mbb_goodness_rows return MBB_ERR_ARG with their message and
    write nothing; the same context then serves a 256-band call correctly."""
    from mbb_emcee_amd import _native, goodness
    from mbb_emcee_amd.modified_blackbody import um_to_GHz
    L = layouts("delta256", "thin_walpha")
    ref = goodness.goodness_rows(L.set(3.0), L.rows[:64], want_flux=True)
    ctx = _native.Context(None)
    ctx.set_model(True, False, 500.0)
    wave = np.geomspace(60.0, 1500.0, 257)
    ctx.set_bands(um_to_GHz / wave, np.ones(257), np.arange(258, dtype=np.int32))
    ctx.set_data(np.ones(257), ivar=np.ones(257))
    p = np.ascontiguousarray(L.rows[:64])
    c, q, fl = np.full(64, 7.0), np.full(64, 7.0), np.full((64, 257), 7.0)
    st = np.full(64, 7, dtype=np.int32)
    rc = ctx.lib.mbb_goodness_rows(ctx.h, _native._d(p), 64, _native._d(c), _native._d(q), _native._i(st), _native._d(fl))
    assert rc == -2 and ctx.lib.mbb_last_error().decode() == "more than 256 bands in a goodness call"
    assert np.all(c == 7.0) and np.all(q == 7.0) and np.all(st == 7) and np.all(fl == 7.0)
    s = _native.GoodnessSpec()
    s.npct, s.burn, s.thin = 1, 0, 1
    s.pct[0] = 50.0
    raw = goodness._Raw(1, 257, 1)
    before = {f: getattr(raw, f).copy() for f in RAW_FIELDS}
    out = raw.out()
    chain = np.ascontiguousarray(p.reshape(1, 4, 16, 5))
    rc = ctx.lib.mbb_chain_goodness(ctx.h, _native._d(chain), None, 1, 4, 16, C.byref(s), C.byref(out))
    assert rc == -2 and ctx.lib.mbb_last_error().decode() == "more than 256 bands in a goodness call"
    for f in RAW_FIELDS:
        assert np.array_equal(getattr(raw, f), before[f], equal_nan=True), f
    # the same context, 256 bands: the likelihood's own answer
    ctx.set_bands(*L.like.band_tables())
    ctx.set_data(L.like._flux, ivar=L.like._ivar)
    fl = np.full((64, 256), 7.0)
    rc = ctx.lib.mbb_goodness_rows(ctx.h, _native._d(p), 64, _native._d(c), _native._d(q), _native._i(st), _native._d(fl))
    assert rc == 0
    for got, want in zip((c, q, st, fl), ref):
        assert np.array_equal(got, want)
    raw = goodness._Raw(1, 256, 1)
    out = raw.out()
    assert ctx.lib.mbb_chain_goodness(ctx.h, _native._d(chain), None, 1, 4, 16, C.byref(s), C.byref(out)) == 0
    rc, own, _ = _native_call(L.like, chain, qs=(50.0,))                    # (the likelihood's own context)
    assert rc == 0 and raw.n_used[0, 0] == 64 and raw.min[0, 0] == ref[0].min() and raw.ml[0, 5] == ref[0].min()
    for f in RAW_FIELDS:
        assert np.array_equal(getattr(raw, f), getattr(own, f), equal_nan=True), f


# ---------------------------------------------------------------- 11. Q(nb/2, chisq/2) at every order, on the device
@pytest.mark.parametrize("parity", [0, 1], ids=["even", "odd"])
def test_q_at_every_order(probe, parity):
    """11. m_gammq_half through the probe at every order of one parity, 2 .. 256 or 1 .. 255, on the order's 70 points
    (_goodness_ref.order_grid) against mpmath.  Outer bound, every order: 4 x the largest relative error
    scipy.special.gammaincc shows on the order's own points.  Even orders also the derived bound (9 + 1.5 ceil(nb/2)) eps
    (_goodness_ref.horner_bound_eps): no library function enters them.  Odd orders have the device library's erfc."""
    pytest.importorskip("mpmath")
    from scipy.special import gammaincc
    orders = [n for n in range(1, GR.MAX_NB + 1) if n % 2 == parity]
    assert len(orders) == 128
    grids = [GR.order_truth(n) for n in orders]
    got = probe.gammq(np.array(orders, dtype=np.float64)[:, None], np.array([g[0] for g in grids]))       # one call
    assert got.shape == (128, 70)
    worst_eps, worst_outer, worst_derived, least_outer = 0.0, 0.0, 0.0, np.inf
    for n, (x, truth, big), q in zip(orders, grids, got):
        # the condition of the grid itself: it judges the function at this order, on both sides of the floor
        assert big.sum() >= 60 and (~big).sum() >= 1, (n, big.sum())
        assert np.all(q[~big] >= 0.0) and np.all(q[~big] <= 1e-289), (n, q[~big])
        rel = GR.rel_errors(truth, big, q)
        outer = 4.0 * GR.rel_errors(truth, big, gammaincc(0.5 * n, 0.5 * x)).max()
        at = x[big][rel.argmax()]
        worst_eps, worst_outer = max(worst_eps, rel.max() / GR.EPS), max(worst_outer, rel.max() / outer)
        least_outer = min(least_outer, outer / GR.EPS)
        assert rel.max() <= outer, (n, rel.max() / GR.EPS, outer / GR.EPS, at)
        if parity == 0:
            worst_derived = max(worst_derived, rel.max() / (GR.horner_bound_eps(n) * GR.EPS))
            assert rel.max() <= GR.horner_bound_eps(n) * GR.EPS, (n, rel.max() / GR.EPS, GR.horner_bound_eps(n), at)
    name = "q per order, %s nb" % ("odd", "even")[parity == 0]
    print("    %s: worst %.1f eps, %.3g of 4 x scipy's error on the order's points%s"
          % (name, worst_eps, worst_outer, ", %.3g of the derived bound" % worst_derived if parity == 0 else ""))
    parity_record(name + " [4 x scipy's error on the order's points]", worst_outer, 1.0)
    # what was seen, in eps; beside it the smallest outer bound any order of this parity had (each order is held to its own)
    parity_record(name + " [eps; beside it the smallest outer bound of any order]", worst_eps, least_outer)
    if parity == 0:
        parity_record(name + " [(9 + 1.5 ceil(nb/2)) eps]", worst_derived, 1.0)


def test_q_edges_on_the_device(probe):
    """tests/test_goodness_cpu.py's test_host_build_edges through the probe's device build."""
    inf, nan = float("inf"), float("nan")
    orders = (1, 2, 3, 8, 63, 64, 255, 256)
    q = probe.gammq(np.array(orders, dtype=np.float64)[:, None], np.array([0.0, -0.0, -5.0, -inf, inf, nan, 1e10, 1e300, 5e-324]))
    for nb, v in zip(orders, q):
        assert np.array_equal(v[:4], np.ones(4)) and v[4] == 0.0 and np.isnan(v[5]), (nb, v)
        assert v[6] == 0.0 and v[7] == 0.0 and v[8] == 1.0, (nb, v)
    x = np.concatenate([np.geomspace(1e-300, 1e12, 2000), np.linspace(1380.0, 3100.0, 500)])
    x.sort()
    for nb, v in zip(orders, probe.gammq(np.array(orders, dtype=np.float64)[:, None], x)):
        assert not np.isnan(v).any() and np.all(v >= 0) and np.all(v <= 1), nb
        big = v > 1e-280
        assert np.all(np.diff(v[big]) <= 4 * GR.EPS * v[big][:-1]), nb
    # what the probe refuses, before any launch
    for bad in (0.0, 257.0, 1.5, nan, -1.0, inf):
        with pytest.raises(RuntimeError, match="domain"):
            probe.gammq(bad, [1.0])
