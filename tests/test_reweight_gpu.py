"""Reweighting on the GPU (csrc/mbb_reweight.hip.h and mbb_rwsteps.hip.h through mbb_chain_reweight /
mbb_sampler_reweight and mbb_emcee_amd/reweight.py) against tests/_reweight_ref.py: PSIS from tests/_loo_ref.py in
longdouble, the weights and the weighted order statistics in integers.

Tolerances, and where they come from:
  * target_lnprob and log_ratio: the target's own ``like(rows)`` and its IEEE difference from the chain's lnprob, exact;
  * log_weight, khat, ess and lnz_ratio: against the longdouble restatement fed the device's own log_ratio, within 64 x the
    largest distance of the float64 restatement from the longdouble one over this file's cases, computed here on the CPU
    from the restatement alone (the loo tests' recipe: the factor covers the device's tree-ordered sums and an exp / log
    within 2 ulp that is not correctly rounded); the bound is asserted < 1e-9;
  * weight: within 1 of floor(e^lw 2^32 + 1/2) formed in longdouble from the device's own log_weight (the device's exp
    is good to an ulp, 2^-21 of a unit at most: only a fraction at 1/2 can flip); weight_sum their integer sum, exact;
  * every weighted quantile: the integer restatement from the device's own weights and the chain's own bits, exact;
  * mean and covariance: against longdouble from the device's weights, under the same 64 x recipe;
  * counts, tail lengths, status, best entries and everything said to be "the same bits": exact.
The chains are tests/_loo_cases._chain's (rows of the fixture chains, a third of them repeats); lnprob of a host chain
is the run's own ``like(rows)``.  The inputs are chosen in tests/_reweight_cases.py and checked without a device in
tests/test_reweight_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import parity_record
import _loo_ref as LR
import _reweight_ref as RR
import _reweight_cases as RC
from _loo_cases import _chain

pytestmark = pytest.mark.gpu

LD = LR.LD
ONE = RR.ONE
QS = dict(percentile=68.3, percentiles=(0.0, 50.0, 100.0))
RAW_FIELDS = ("n_used", "n_zero", "n_left_out", "weight_sum", "khat", "ess", "lnz_ratio", "mean", "pct", "cov", "best",
              "tail_len", "status", "col_status", "best_index")
NW, NSTEPS = 34, 64


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


@pytest.fixture(scope="module")
def world(mbb, oracle, g_lnl, g_pb, g_res):
    """(the data of the run's band case, the run's likelihood)"""
    data = RC.data_of(oracle, g_lnl, g_pb, g_res)
    return data, RC.device_like(mbb, data)


def _lp(like, chain):
    """lnprob of a host chain [nw, nsteps, 5] or [nsrc, nw, nsteps, 5] by like(rows)"""
    c = np.asarray(chain)
    if c.ndim == 3:
        return like(np.ascontiguousarray(c.reshape(-1, 5))).reshape(c.shape[:2])
    if like.nsources > 1:
        return like(np.ascontiguousarray(c.reshape(c.shape[0], -1, 5))).reshape(c.shape[:3])
    return np.stack([_lp(like, c[s]) for s in range(c.shape[0])])


def _same_bits(a, b, fields=RAW_FIELDS, src_a=None, src_b=None):
    for f in fields:
        x, y = getattr(a._raw, f), getattr(b._raw, f)
        x = x if src_a is None else x[src_a]
        y = y if src_b is None else y[src_b]
        if not np.array_equal(x, y, equal_nan=True):
            return f
    return True


def _window(chain3, burn=0, thin=1):
    return np.ascontiguousarray(chain3[:, burn::thin].reshape(-1, 5))


def _columns(rows, extra=None):
    cols = np.full((rows.shape[0], 8), np.nan)
    cols[:, :5] = rows
    for slot, v in (extra or {}).items():
        cols[:, slot] = v
    return cols


# ---------------------------------------------------------------- 1. identity
def test_identity(mbb, world, g_res):
    """1. The run's own likelihood as the target: r is 0 exactly, no tail to fit, every weight 2^32, ess = S,
    lnz_ratio = 0, and the quantiles are numpy's unweighted inverted-CDF ones exactly."""
    data, run = world
    chain = RC.chain_of(g_res, "S 512 identity")[0]
    lp = _lp(run, chain)
    res = mbb.chain_reweight(run, chain, lp, keep=True, **QS)
    assert np.array_equal(res.target_lnprob, lp.ravel()) and np.all(res.log_ratio == 0.0) and np.all(res.log_weight == 0.0)
    assert res.n_used == 512 and res.n_zero == 0 and res.n_left_out == 0 and res.tail_len == 68
    assert res.status == (RR.TAIL_FLAT | RR.K_HIGH) and np.isinf(res.khat)
    assert np.all(res.weight == ONE) and res.weight_sum == 512 * ONE
    assert res.ess == 512.0 and res.lnz_ratio == 0.0
    rows = _window(chain)
    for slot in range(5):
        for k, q in enumerate(res.qs):
            assert res.percentiles[slot, k] == np.quantile(rows[:, slot], q / 100.0, method="inverted_cdf"), (slot, q)
    assert np.all(res.column_status[:5] == 0) and np.all(res.column_status[5:] == res.ABSENT)
    assert np.all(np.isnan(res.mean[5:])) and np.all(np.isnan(res.percentiles[5:]))
    best, lq, (w, s) = res.best_fit
    flat = int(np.argmax(lp.ravel()))
    assert (w, s) == (flat // 64, flat % 64) and lq == lp.ravel()[flat] and np.array_equal(best, chain[w, s])


# ---------------------------------------------------------------- 2. a prior added
@pytest.mark.parametrize("width", ["low", "mid", "high"])
def test_prior_added(mbb, world, g_res, width):
    """2. A Gaussian prior on beta at three widths, one per k-hat class: target_lnprob is the target's own like(rows) bit
    for bit, log_ratio its IEEE difference from the chain's lnprob."""
    data, run = world
    target = RC.device_like(mbb, data, prior=(RC.PRIOR_MEAN, RC.WIDTHS[width]))
    chain = RC.chain_of(g_res, "S 512 " + width)[0]
    lp = _lp(run, chain)
    res = mbb.chain_reweight(target, chain, lp, keep=True)
    lq = target(_window(chain))
    assert np.array_equal(res.target_lnprob, lq)
    assert np.array_equal(res.log_ratio, lq - lp.ravel())
    sc = dict(khat=res.khat, why=LR.FIT_OK)
    print("    width %s: k-hat %.3f ess %.1f lnz_ratio %.3f" % (width, res.khat, res.ess, res.lnz_ratio))
    assert RC.klass(sc) == width and bool(res.status & res.K_HIGH) == (width == "high")
    # the prior alone separates the two densities: r is its log density up to the rounding of lq's sum
    beta = _window(chain)[:, 1]
    assert np.allclose(res.log_ratio, -0.5 * ((beta - RC.PRIOR_MEAN) / RC.WIDTHS[width]) ** 2, rtol=0, atol=1e-9 * np.abs(lq).max())


# ---------------------------------------------------------------- 3. PSIS, weights, quantiles, moments
@pytest.fixture(scope="module")
def psis_cases(mbb, world, g_res):
    """Every PSIS case of tests/_reweight_cases.py: label -> (chain [nw, nsteps, 5], lnprob, the device's kept result, the
    restatement's scalars in longdouble and in float64, the used mask).  The S = 455 case holds alpha constant."""
    data, run = world
    out = {}
    for label, (shape, seed, prior, planned) in RC.PSIS.items():
        chain = RC.chain_of(g_res, label)[0]
        if label == "S 455":
            chain[..., 3] = 4.0
        lp = _lp(run, chain)
        target = run if prior is None else RC.device_like(mbb, data, prior=prior)
        res = mbb.chain_reweight(target, chain, lp, keep=True, **QS)
        ref, used, zero, left = RC.restate(lp, res, 0, LD)
        f64 = RC.restate(lp, res, 0, np.float64)[0]
        out[label] = (chain, lp, res, ref, f64, used)
    return out


def test_psis_against_longdouble(psis_cases):
    """3a. log_weight, khat, ess and lnz_ratio against the longdouble restatement fed the device's own log_ratio; counts,
    tail lengths and status exact; every case in the class tests/test_reweight_cpu.py found with the oracle."""
    spread = max(RR.distance(f64, ref) for _, _, _, ref, f64, _ in psis_cases.values())
    bound = 64.0 * spread
    print("    float64 restatement vs longdouble: %.3g; bound %.3g" % (spread, bound))
    assert 0.0 < bound < 1e-9
    worst = 0.0
    for label, (chain, lp, res, ref, f64, used) in psis_cases.items():
        raw = res._raw
        S = chain.shape[0] * chain.shape[1]
        assert used.all() and raw.n_used[0] == S and raw.n_zero[0] == 0 and raw.n_left_out[0] == 0, label
        assert raw.tail_len[0] == ref["M"] == LR.tail_len(S), label
        assert raw.status[0] == ref["status"], (label, raw.status[0], ref["status"])
        assert RC.klass(ref) == RC.PSIS[label][3], (label, float(ref["khat"]))
        d = RR.distance(RC.device_scalars(res, 0, used), ref)
        print("    %-16s k-hat %7.3f ess %9.2f lnz_ratio %9.4f  worst %.3g" % (label, raw.khat[0], raw.ess[0], raw.lnz_ratio[0], d))
        worst = max(worst, d)
    parity_record("reweight scalars vs longdouble [max(1, |x|)]", worst, bound)
    assert worst <= bound
    seen = {int(r[2]._raw.n_used[0]): int(r[2]._raw.tail_len[0]) for r in psis_cases.values()}
    for s, m in ((20, 4), (21, 5), (35, 7), (455, 64), (456, 65), (512, 68), (7283, 257), (16384, 384), (16385, 385)):
        assert seen.get(s) == m, (s, seen)


def test_raw_weights_keep_the_fit(mbb, world, g_res, psis_cases):
    """smooth=False: the raw log weights r - max r exactly, the same k-hat, and the restatement's ess and lnz_ratio."""
    data, run = world
    chain, lp, res, ref, f64, used = psis_cases["S 512 mid"]
    target = RC.device_like(mbb, data, prior=RC.PSIS["S 512 mid"][2])
    rawres = mbb.chain_reweight(target, chain, lp, keep=True, smooth=False)
    assert np.array_equal(rawres.log_ratio, res.log_ratio) and rawres.khat == res.khat and rawres.status == res.status
    assert np.array_equal(rawres.log_weight, res.log_ratio - res.log_ratio.max())
    want = RC.restate(lp, rawres, 0, LD, smooth=False)[0]
    assert RR.distance(RC.device_scalars(rawres, 0, used), want) < 1e-12
    assert rawres.ess != res.ess


def test_weights(psis_cases):
    """3b. weight within 1 of floor(e^lw 2^32 + 1/2) from the device's own log_weight in longdouble, differing only where
    the fraction is at 1/2; weight_sum exactly their sum."""
    flips = total = 0
    for label, (chain, lp, res, ref, f64, used) in psis_cases.items():
        raw = res._raw
        want = RR.quantise(raw.log_weight[0])
        d = np.abs(raw.weight[0] - want)
        v = np.exp(raw.log_weight[0].astype(LD)) * LD(ONE) + LD(0.5)
        frac = (v - np.floor(v)).astype(np.float64)
        assert d.max() <= 1 and np.all(np.minimum(frac, 1 - frac)[d > 0] < 1e-5), (label, d.max())
        assert raw.weight[0].min() >= 0 and raw.weight[0].max() <= ONE
        assert int(raw.weight_sum[0]) == int(raw.weight[0].sum(dtype=np.int64)), label
        flips += int((d > 0).sum()); total += d.size
    print("    %d of %d weights differ from the longdouble floor by 1" % (flips, total))
    parity_record("reweight integer weight vs longdouble floor (abs)", 1.0 if flips else 0.0, 1.0)


def test_quantiles_are_exact(mbb, world, g_res, psis_cases):
    """3c. Every weighted quantile (15.85, 84.15, 0, 50, 100) of every parameter against the integer restatement from the
    device's own weights: exact.  The chains carry their natural repeated rows (ties); the S = 455 case a constant
    column; a one-kept-step window; a window with burn and thin."""
    for label, (chain, lp, res, ref, f64, used) in psis_cases.items():
        RC.check_quantiles(res, 0, _columns(_window(chain)), range(5), label)
        rows = _window(chain)
        assert np.unique(rows, axis=0).shape[0] < rows.shape[0] or rows.shape[0] < 30, label       # (ties)
    const = psis_cases["S 455"][2]
    assert np.all(const.percentiles[3] == 4.0) and const.mean[3] == 4.0 and const.covariance[3, 3] == 0.0
    data, run = world
    target = RC.device_like(mbb, data, prior=(RC.PRIOR_MEAN, RC.WIDTHS["mid"]))
    chain, lp = psis_cases["S 512 mid"][:2]
    for kw, n in ((dict(burn=63), 8), (dict(burn=5, thin=3), 8 * 20), (dict(thin=64), 8)):
        res = mbb.chain_reweight(target, chain, lp, keep=True, **QS, **kw)
        assert res.n_used == n and res.weight.shape == (n,) and res.nsteps_used == n // 8
        RC.check_quantiles(res, 0, _columns(_window(chain, **kw)), range(5), str(kw))
        assert np.array_equal(res.target_lnprob, target(_window(chain, **kw)))
        if n == 8:
            assert res.status & res.TAIL_SHORT and np.array_equal(res.log_weight, res.log_ratio - res.log_ratio.max())


def test_mean_covariance_best(psis_cases):
    """3d. Mean and covariance against longdouble from the device's own weights, within 64 x the float64 restatement's
    distance from it; best is numpy's first argmax of target_lnprob over the used entries (the chains' repeated rows are
    ties: the first of them wins)."""
    def dist(a, b):
        a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
        return float(np.max(np.abs(a - b) / np.maximum(LD(1), np.abs(b))))
    spread = worst = 0.0
    ties = 0
    for label, (chain, lp, res, ref, f64, used) in psis_cases.items():
        raw = res._raw
        rows, u = _window(chain), raw.weight[0]
        mean, cov = np.array([RR.wmean(rows[:, k], u) for k in range(5)]), RR.wcov(rows, u)
        mean64 = np.array([RR.wmean(rows[:, k], u, np.float64) for k in range(5)])
        spread = max(spread, dist(mean64, mean), dist(RR.wcov(rows, u, np.float64), cov))
        worst = max(worst, dist(raw.mean[0, :5], mean), dist(raw.cov[0], cov))
        assert np.array_equal(raw.cov[0], raw.cov[0].T)
        lq = raw.target_lnprob[0]
        flat = int(np.argmax(lq))
        ties += int((lq == lq[flat]).sum() > 1)
        nsteps = chain.shape[1]
        assert tuple(raw.best_index[0]) == (flat // nsteps, flat % nsteps), label
        assert raw.best[0, 5] == lq[flat] and np.array_equal(raw.best[0, :5], rows[flat])
    bound = 64.0 * spread
    print("    mean and covariance: worst %.3g, float64 restatement %.3g, bound %.3g; %d cases with a tied best" % (worst, spread, bound, ties))
    assert 0.0 < bound < 1e-9 and ties >= 1
    parity_record("reweight mean and covariance vs longdouble [max(1, |x|)]", worst, bound)
    assert worst <= bound


def test_planted_best_ties(mbb, world, g_res):
    """The best entry's row planted again later in its own walker and in an earlier walker: the first in [walker][step]
    order wins."""
    data, run = world
    target = RC.device_like(mbb, data, prior=(RC.PRIOR_MEAN, RC.WIDTHS["low"]))
    chain = RC.chain_of(g_res, "S 512 low")[0].copy()
    lq = target(_window(chain)).reshape(8, 64)
    w, s = np.unravel_index(int(np.argmax(lq)), lq.shape)
    chain[7, 60] = chain[w, s]
    chain[0, 3] = chain[w, s]
    res = mbb.chain_reweight(target, chain, _lp(run, chain))
    lq = target(_window(chain))
    assert res.best_fit[2] == (0, 3) == tuple(int(v) for v in np.unravel_index(int(np.argmax(lq)), (8, 64)))
    assert (lq == lq.max()).sum() >= 3


# ---------------------------------------------------------------- 4. zero weights
def test_zero_weights(mbb, world, g_res):
    """4. The target raises T's lower limit into the chain: n_zero exact, u = 0 there, those entries take no part in the
    PSIS fit (the restatement sees the used entries alone), every quantile of T is at or above the limit; with the limit
    above every entry ALL_ZERO, NaN statistics and lnz_ratio -inf."""
    data, run = world
    chain = RC.chain_of(g_res, "S 512 low")[0]
    lp = _lp(run, chain)
    rows = _window(chain)
    target = RC.device_like(mbb, data, prior=(RC.PRIOR_MEAN, RC.WIDTHS["mid"]), t_limit=RC.T_LIMIT)
    res = mbb.chain_reweight(target, chain, lp, keep=True, **QS)
    below = rows[:, 0] < RC.T_LIMIT
    assert res.n_zero == below.sum() >= 51 and res.n_used == (~below).sum() >= 51 and res.n_left_out == 0
    assert np.all(res.weight[below] == 0) and np.all(np.isneginf(res.log_weight[below])) and np.all(np.isneginf(res.target_lnprob[below]))
    assert res.status & res.HAS_ZERO and not res.status & (res.ALL_ZERO | res.EMPTY | res.HAS_NAN)
    ref, used, zero, left = RC.restate(lp, res, 0, LD)
    assert np.array_equal(zero, below) and res.tail_len == ref["M"] == LR.tail_len(int(used.sum()))
    assert RR.distance(RC.device_scalars(res, 0, used), ref) < 1e-11
    assert (res.status & ~res.HAS_ZERO) == (ref["status"] & ~RR.HAS_ZERO)
    RC.check_quantiles(res, 0, _columns(rows), range(5), "limit")
    assert np.all(res.percentiles[0] >= RC.T_LIMIT)
    assert res.best_fit[0][0] >= RC.T_LIMIT
    none = mbb.chain_reweight(RC.device_like(mbb, data, t_limit=RC.T_LIMIT_ALL), chain, lp, keep=True, **QS)
    assert none.n_zero == 512 and none.n_used == 0 and none.weight_sum == 0 and np.all(none.weight == 0)
    assert none.status == (none.ALL_ZERO | none.HAS_ZERO | none.EMPTY | none.TAIL_SHORT | none.K_HIGH)
    assert np.isneginf(none.lnz_ratio) and np.isnan(none.ess) and np.isinf(none.khat)
    assert np.all(np.isnan(none.mean)) and np.all(np.isnan(none.percentiles)) and np.all(np.isnan(none.covariance))
    assert none.best_fit[2] == (-1, -1) and np.all(np.isnan(none.best_fit[0]))
    assert np.all(none.column_status[:5] == none.EMPTY)


# ---------------------------------------------------------------- 5. entries left out
def test_left_out(mbb, world, g_res):
    """5. NaN rows and failing SED rows, lnprob cells of -inf and NaN: outside the window they change nothing; inside it
    they are left out, counted, flagged, and the other sources keep their bits; a whole source of NaN rows."""
    from mbb_emcee_amd import _native
    data, run = world
    target = RC.device_like(mbb, data, prior=(RC.PRIOR_MEAN, RC.WIDTHS["low"]))
    # (with the default lower limits of 0.1 a negative alpha or beta is below a limit -- an entry of weight zero -- before
    # the SED constructor sees it; this target lets the constructor fail on them)
    target.set_lowlim("alpha", -10.0)
    target.set_lowlim("beta", -10.0)
    base = _chain(g_res, RC.RUN[0], (3, 10, 16), seed=12)
    lp = _lp(run, base)
    kw = dict(burn=4, thin=3, keep=True, **QS)                        # kept steps 4, 7, 10, 13: n = 40
    good = mbb.chain_reweight(target, base, lp, **kw)
    assert np.all(good.n_used == 40) and np.all(good.tail_len == 8) and np.all(good.n_left_out == 0)
    out, lpo = base.copy(), lp.copy()
    out[1, 2, 5, 3] = -1.0
    out[2, 0, 8, 0] = np.nan
    lpo[0, 3, 6] = np.nan
    lpo[1, 3, 9] = -np.inf
    assert _same_bits(mbb.chain_reweight(target, out, lpo, **kw), good) is True
    ins, lpi = base.copy(), lp.copy()
    ins[1, 2, 7, 3] = -1.0                                             # a failing row: alpha
    ins[1, 5, 4, 1] = -0.5                                             # ... beta
    ins[1, 0, 13, 0] = np.nan                                          # ... not finite
    lpi[1, 6, 4] = -np.inf
    lpi[1, 7, 10] = np.nan
    g = mbb.chain_reweight(target, ins, lpi, **kw)
    bits = sum(1 << (_native.SUM_ROW_SHIFT + r) for r in (_native.ROW_BAD_ALPHA, _native.ROW_BAD_BETA, _native.ROW_NONFINITE))
    assert g.n_used[1] == 35 and g.n_left_out[1] == 5 and g.n_zero[1] == 0 and g.tail_len[1] == 7
    assert (g.status[1] & ~(g.K_HIGH | g.TAIL_FLAT)) == (bits | g.HAS_NAN)
    assert _same_bits(g, good, src_a=[0, 2], src_b=[0, 2]) is True
    gone = np.zeros((10, 16), dtype=bool)
    for w, s in ((2, 7), (5, 4), (0, 13), (6, 4), (7, 10)):
        gone[w, s] = True
    gone = gone[:, 4::3].ravel()
    assert np.all(g.weight[1][gone] == 0) and np.all(np.isneginf(g.log_weight[1][gone]))
    ref, used, zero, left = RC.restate(lpi[1][:, 4::3], g, 1, LD)
    assert np.array_equal(left, gone) and RR.distance(RC.device_scalars(g, 1, used), ref) < 1e-11
    # the parameter columns of the rows left out are not looked at: a NaN there poisons nothing
    assert np.all(g.column_status[1, :5] == 0) and np.all(np.isfinite(g.mean[1, :5]))
    RC.check_quantiles(g, 1, _columns(_window(ins[1], 4, 3)), range(5), "left out")
    allnan, lpa = base.copy(), lp.copy()
    allnan[2] = np.nan
    g = mbb.chain_reweight(target, allnan, lpa, **kw)
    assert g.n_used[2] == 0 and g.n_left_out[2] == 40 and g.tail_len[2] == 0 and np.isnan(g.lnz_ratio[2])
    assert g.status[2] & g.EMPTY and g.status[2] & g.HAS_NAN and g.status[2] & g.TAIL_SHORT and not g.status[2] & g.ALL_ZERO
    assert np.all(np.isnan(g.mean[2])) and np.all(np.isnan(g.percentiles[2])) and g.weight_sum[2] == 0
    assert _same_bits(g, good, src_a=[0, 1], src_b=[0, 1]) is True


# ---------------------------------------------------------------- 6. other data, another model
def test_band_dropped(mbb, world, g_res):
    """6a. The target has 3 of the run's 4 bands (diagonal case): r + ll_b of the dropped band stays within
    1e-10 max(1, |lq|, |lp|) of the band's constant, the project's lnL tolerance applied to both terms.  (The constant:
    like() is -chisq / 2 plus limits and priors and carries no normalisation, the pointwise term does,
    ll_b = ln(ivar_b / 2 pi) / 2 - r_b^2 ivar_b / 2: so lq - lp + ll_b = ln(ivar_b / 2 pi) / 2 for every entry, formed here
    in longdouble from the run's own uncertainties.)"""
    from mbb_emcee_amd import loo
    data, run = world
    chain = RC.chain_of(g_res, "S 512 low")[0]
    lp = _lp(run, chain)
    ll = loo.loo_rows(run, _window(chain))[0]
    for b in (0, 3):
        keep = [i for i in range(4) if i != b]
        res = mbb.chain_reweight(RC.device_like(mbb, data, keep=keep), chain, lp, keep=True)
        const = (np.log(LD(run._ivar[b])) - np.log(2 * np.arccos(LD(-1)))) / 2
        err = np.abs(((res.log_ratio.astype(LD) + ll[:, b].astype(LD)) - const).astype(np.float64)) / np.maximum(
            1.0, np.maximum(np.abs(res.target_lnprob), np.abs(lp.ravel())))
        print("    band %d dropped: worst %.3g, k-hat %.3f" % (b, err.max(), res.khat))
        parity_record("reweight r + ll_b, a band dropped / max(1,|lq|,|lp|)", err.max(), 1e-10)
        assert err.max() <= 1e-10 and res.n_used == 512


@pytest.mark.parametrize("what", ["a band added", "thin for thick"])
def test_other_targets(mbb, oracle, g_lnl, g_pb, world, g_res, what):
    """6b. A target with one more band (the 12-band case's first five, diagonal), and an optically thin target for a
    thick run: target_lnprob is the target's own, everything else the restatement's."""
    data, run = world
    chain = RC.chain_of(g_res, "S 456")[0]
    lp = _lp(run, chain)
    if what == "a band added":
        okw, first, flux, unc, cov = RC.data_of(oracle, g_lnl, g_pb, g_res, case="cov12")
        extra = [i for i, nm in enumerate(first) if nm not in data[1]][0]
        wide = (data[0], list(data[1]) + [first[extra]], np.append(data[2], flux[extra]), np.append(data[3], unc[extra]), None)
        target = RC.device_like(mbb, wide)
        assert int(target._ndata) == int(run._ndata) + 1
    else:
        target = RC.device_like(mbb, data, opthin=True)
    res = mbb.chain_reweight(target, chain, lp, keep=True, **QS)
    assert np.array_equal(res.target_lnprob, target(_window(chain)))
    assert np.array_equal(res.log_ratio, res.target_lnprob - lp.ravel())
    ref, used, zero, left = RC.restate(lp, res, 0, LD)
    assert used.all() and res.status == ref["status"] and res.tail_len == ref["M"]
    d = RR.distance(RC.device_scalars(res, 0, used), ref)
    print("    %s: k-hat %.3f ess %.1f lnz_ratio %.3f, worst %.3g" % (what, res.khat, res.ess, res.lnz_ratio, d))
    assert d < 1e-11
    RC.check_quantiles(res, 0, _columns(_window(chain)), range(5), what)


# ---------------------------------------------------------------- 7. sources
def test_sources(mbb, world, g_res):
    """7. Three sources of different scales are each bit for bit their own one-source call; a one-source target serves a
    three-source chain; a [3, 300, 300] chain whose gather slab seam (262144 // 3 entries) falls inside every source
    matches the restatement; a smaller call after a larger one leaves no stale cells."""
    data, run = world
    scales = (0.2, 1.0, 5.0)
    prior = (RC.PRIOR_MEAN, RC.WIDTHS["low"])
    three = _chain(g_res, RC.RUN[0], (3, 8, 40), seed=8)
    three[0, ..., 4] *= 0.2
    three[2, ..., 4] *= 5.0
    runm = RC.device_like(mbb, data, multi=scales)
    lp = _lp(runm, three)
    tm = RC.device_like(mbb, data, multi=scales, prior=prior)
    res = mbb.chain_reweight(tm, three, lp, keep=True, burn=3, **QS)
    assert np.all(res.n_used == 8 * 37)
    for src, s in enumerate(scales):
        one = RC.device_like(mbb, data, multi=None, prior=prior)
        one.set_phot(data[1], data[2] * s, data[3] * s)
        alone = mbb.chain_reweight(one, three[src], lp[src], keep=True, burn=3, **QS)
        assert _same_bits(alone, res, RAW_FIELDS + ("target_lnprob", "log_ratio", "log_weight", "weight"), 0, src) is True, src
    # a one-source target for all three sources
    t1 = RC.device_like(mbb, data, prior=prior)
    same = np.ascontiguousarray(np.stack([three[1]] * 3))
    same[2, :, 20:] = three[1][:, :20]
    lp3 = _lp(run, same)
    r3 = mbb.chain_reweight(t1, same, lp3, keep=True, **QS)
    assert _same_bits(r3, r3, src_a=0, src_b=1) is True
    alone = mbb.chain_reweight(t1, same[2], lp3[2], keep=True, **QS)
    assert _same_bits(alone, r3, RAW_FIELDS + ("target_lnprob", "log_weight", "weight"), 0, 2) is True
    # the slab seam, and stale cells
    small = _chain(g_res, RC.RUN[0], (1, 6, 9), seed=4)
    lps = _lp(run, small)
    before = mbb.chain_reweight(t1, small, lps, keep=True, **QS)
    big = _chain(g_res, RC.RUN[0], (3, 300, 300), seed=6)
    lpb = _lp(run, big)
    bigres = mbb.chain_reweight(t1, big, lpb, keep=True, **QS)
    assert _same_bits(mbb.chain_reweight(t1, small, lps, keep=True, **QS), before,
                      RAW_FIELDS + ("target_lnprob", "log_weight", "weight")) is True
    assert np.all(bigres.n_used == 90000) and np.all(bigres.tail_len == 900)
    for src in range(3):
        rows = _window(big[src])
        assert np.array_equal(bigres.target_lnprob[src], t1(rows)), src
        ref, used, zero, left = RC.restate(lpb[src], bigres, src, LD)
        d = RR.distance(RC.device_scalars(bigres, src, used), ref)
        assert used.all() and d < 1e-10 and bigres.status[src] == ref["status"], (src, d)
        RC.check_quantiles(bigres, src, _columns(rows), range(5), "seam")
        assert int(bigres.weight_sum[src]) == int(bigres.weight[src].sum(dtype=np.int64))
    alone = mbb.chain_reweight(t1, big[1], lpb[1], **QS)
    assert _same_bits(alone, bigres, src_a=0, src_b=1) is True


# ---------------------------------------------------------------- 8. derived columns
def test_derived_columns(mbb, world, g_res):
    """8. Weighted quantiles of peak wavelength, L_IR and dust mass are exact against the integer restatement on the
    values chain_draws(how="even", n = nw nkept) returns, which are the summary's bits; one redshift per source, one
    source's unknown."""
    data, run = world
    target = RC.device_like(mbb, data, prior=(RC.PRIOR_MEAN, RC.WIDTHS["low"]))
    chain = _chain(g_res, RC.RUN[0], (3, 8, 40), seed=21)
    lp = _lp(run, chain)
    z, dl = np.array([1.5, np.nan, 2.5]), np.array([11000.0, np.nan, 20000.0])
    dkw = dict(derived=("peaklambda", "lir", "dustmass"), redshift=z, lumdist_mpc=dl, burn=4, thin=2)
    res = mbb.chain_reweight(target, chain, lp, keep=True, **QS, **dkw)
    dr = mbb.chain_draws(target, chain, n=8 * 18, how="even", **dkw)
    for src in range(3):
        rows = _window(chain[src], 4, 2)
        assert np.array_equal(dr.params[src], rows)
        cols = _columns(rows, {5: dr.peaklambda[src], 6: dr.lir[src], 7: dr.dustmass[src]})
        slots = range(8) if src != 1 else range(6)
        RC.check_quantiles(res, src, cols, slots, "derived")
        u = res.weight[src]
        for slot in slots:
            want = float(RR.wmean(cols[:, slot], u))
            assert abs(res.mean[src, slot] - want) <= 1e-12 * abs(want), (src, slot)
    assert np.all(np.isnan(res.mean[1, 6:])) and np.all(np.isnan(res.percentiles[1, 6:]))
    assert np.all(res.column_status[1, 6:] & res.HAS_NAN) and np.all(res.column_status[[0, 2]] == 0) and np.all(res.column_status[1, :6] == 0)
    cen = res.lir_cen()
    assert cen.shape == (3, 3) and np.all(cen[[0, 2]] > 0) and res.peaklambda_cen().shape == (3, 3) and res.dustmass_cen().shape == (3, 3)
    # the five parameters do not depend on the derived columns being asked for
    plain = mbb.chain_reweight(target, chain, lp, burn=4, thin=2, **QS)
    assert np.array_equal(plain.mean[:, :5], res.mean[:, :5]) and np.array_equal(plain.percentiles[:, :5], res.percentiles[:, :5])


# ---------------------------------------------------------------- 9. through the stack
def _sampler_case(mbb, g_lnl, multi):
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rng = np.random.RandomState(11)
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))

    def make(flux, prior):
        lk = mbb.likelihood(response=True)
        if multi:
            lk.set_phot_multi(bands, flux, 0.1 * flux + 1.0)
        else:
            lk.set_phot(bands, flux, 0.1 * flux + 1.0)
        if prior:
            lk.set_gaussian_prior("beta", 2.0, 0.25)
        return lk
    if multi:
        ns = 3
        truths = np.column_stack([rng.uniform(8, 20, ns), rng.uniform(1.2, 2.4, ns), rng.uniform(300, 900, ns),
                                  rng.uniform(2, 4.5, ns), rng.uniform(10, 80, ns)])
        flux = one.model_flux(truths)
        p0 = truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, NW, 5)))
    else:
        truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
        flux = one.model_flux(truth)[0]
        p0 = truth * (1.0 + 0.02 * rng.normal(size=(NW, 5)))
    return make(flux, False), make(flux, True), p0, bands


ALL = RAW_FIELDS + ("target_lnprob", "log_ratio", "log_weight", "weight")


@pytest.mark.parametrize("multi", [False, True])
def test_resident_chain(mbb, g_lnl, multi):
    """9. sampler.reweight(target) and run_mcmc(storechain=False, summary=, reweight=) equal chain_reweight on the chain
    and lnprob a storechain=True run of the same seed brings back, bit for bit; a target in its own context and the run's
    own context as the target (the same density) give the same bits; the run's other eight analyses are what they are
    without reweight=."""
    lk, tg, p0, bands = _sampler_case(mbb, g_lnl, multi)
    a = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.reweight_ is None
    kw = dict(burn=5, thin=2, keep=True, **QS)
    host = mbb.chain_reweight(tg, a.chain, a.lnprobability, **kw)
    res = a.reweight(tg, **kw)
    assert _same_bits(res, host, ALL) is True and res.nsteps_used == 30 and res.nwalkers == NW
    assert res.khat.shape == ((3,) if multi else ()) and np.all(res.n_used == NW * 30)
    assert np.all(np.isfinite(res.khat)) and np.all(res.ess > 1) and np.all(res.ess < NW * 30)
    # the run's own context as the target: the identity, and the same bits as a twin likelihood in a context of its own
    own = a.reweight(lk, **kw)
    twin = _sampler_case(mbb, g_lnl, multi)[0]
    assert _same_bits(own, a.reweight(twin, **kw), ALL) is True
    assert np.all(own.n_used == NW * 30) and np.all(np.abs(own.log_ratio) <= 1e-10 * np.maximum(1.0, np.abs(own.target_lnprob)))
    skw = dict(burn=5, thin=2, derived=("peaklambda",), percentile=(68.3, 95.4))
    others = dict(summary=dict(skw), convergence=True, marginals=dict(bins=24, bins2d=6), predict=[bands[3], 70.0], draws=9,
                  goodness=True, evidence=dict(n2=256), loo=True)
    b = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b.run_mcmc(p0, NSTEPS, storechain=False, reweight=dict(target=tg, keep=True, **QS), **others)
    assert b.chain.shape[-2] == 0 and b.reweight_.burn == 5 and b.reweight_.thin == 2
    assert "peaklambda" in b.reweight_._req.derived                    # (window and derived columns default to summary='s)
    assert _same_bits(b.reweight_, host, tuple(f for f in ALL if f not in ("mean", "pct", "col_status"))) is True
    assert np.array_equal(b.reweight_.mean[..., :5], host.mean[..., :5]) and np.array_equal(b.reweight_.percentiles[..., :5, :], host.percentiles[..., :5, :])
    assert np.all(np.isfinite(b.reweight_.peaklambda_cen()))
    assert _same_bits(b.reweight(tg, **kw), host, ALL) is True
    c = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    c.run_mcmc(p0, NSTEPS, storechain=False, **others)
    assert c.reweight_ is None
    import _summary_ref as SR
    assert SR.raw_equal(b.summary, c.summary)
    for f in ("tau", "ess", "rhat", "window", "status"):
        assert np.array_equal(getattr(b.convergence_, f), getattr(c.convergence_, f), equal_nan=True), f
    for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "status"):
        assert np.array_equal(getattr(b.marginals_._raw, f), getattr(c.marginals_._raw, f), equal_nan=True), f
    for f in ("n_used", "mean", "min", "max", "pct", "status"):
        assert np.array_equal(getattr(b.predictions_._raw, f), getattr(c.predictions_._raw, f), equal_nan=True), f
    for name in ("draws_", "goodness_", "evidence_", "loo_"):
        for k, v in getattr(c, name).arrays().items():
            assert np.array_equal(getattr(b, name).arrays()[k], v, equal_nan=True), (name, k)
    # after reweight() the analyses that share the target's and the run's buffers
    assert np.array_equal(b.goodness(burn=5, thin=2).chisq_mean, c.goodness(burn=5, thin=2).chisq_mean)
    assert SR.raw_equal(b.summary, c.summary)
    b.run_mcmc(None, 3, storechain=False)
    assert b.reweight_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.reweight(tg)
    b.run_mcmc(None, 9, reweight=tg)
    assert b.reweight_.nsteps_used == 9
    assert _same_bits(b.reweight_, mbb.chain_reweight(tg, b.chain[..., -9:, :], b.lnprobability[..., -9:])) is True
    b.reset()
    assert b.reweight_ is None


def test_fitter_and_cli_reweight(mbb, g_lnl, tmp_path, capsys):
    """mbb_fitter.run(..., reweight=...) and the CLI's --reweight-prior end to end: the numbers are those of the chain
    the fit returns; without the flag nothing new is printed or written."""
    from mbb_emcee_amd import run_mbb_emcee
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    flux = one.model_flux(truth)[0]

    def fitter(prior):
        fit = mbb.mbb_fitter(nwalkers=NW, response=True, seed=3)
        fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
        if prior:
            fit.set_gaussian_prior("beta", 2.0, 0.25)
        return fit
    fit, tfit = fitter(False), fitter(True)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    fit.run(20, NSTEPS, p0, reweight=tfit)                             # (a fitter stands for its likelihood)
    assert fit.reweight is not None
    assert _same_bits(fit.reweight, mbb.chain_reweight(tfit.like, fit.sampler.chain, fit.sampler.lnprobability)) is True
    fit.run(20, 16, p0, reweight=dict(target=tfit.like, burn=2), summary=True)
    assert _same_bits(fit.reweight, mbb.chain_reweight(tfit.like, fit.sampler.chain, fit.sampler.lnprobability, burn=2)) is True
    fit.run(20, 16, p0)
    assert fit.reweight is None
    capsys.readouterr()
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", str(NW), "-b", "20", "-N", str(NSTEPS), "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--reweight-prior", "beta", "2.0", "0.25"]) == 0
    text = capsys.readouterr().out
    assert "Pareto k-hat" in text and "effective sample size" in text and "ln(Z_target / Z_run)" in text
    got = np.load(out)
    assert {"reweight_khat", "reweight_ess", "reweight_lnz_ratio", "reweight_mean", "reweight_percentiles"} <= set(got.files)
    like = mbb.likelihood(str(pf), response=True)
    like.set_gaussian_prior("beta", 2.0, 0.25)
    want = mbb.chain_reweight(like, got["chain"], got["lnprobability"], percentile=(68.3, 95.4)).arrays()
    for k, v in want.items():
        assert np.array_equal(got[k], v, equal_nan=np.asarray(v).dtype.kind == "f"), k
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == "" and not any(k.startswith("reweight_") for k in np.load(out).files)


# ---------------------------------------------------------------- 10. refusals of the C-ABI
def _native_call(like, chain, lnp, burn=0, thin=1, npct=2, nsrc=None, nw=None, nsteps=None, edit=None):
    from mbb_emcee_amd import _native, reweight
    ctx = _native.analysis_context(like)
    req = reweight._Request(like, burn=max(burn, 0), thin=max(thin, 1), nsources=chain.shape[0])
    spec = req.spec()
    spec._summary.burn, spec._summary.thin, spec._summary.npct = burn, thin, npct
    raw = reweight._Raw(chain.shape[0], 8)
    out = raw.out()
    if edit:
        edit(spec, out)
    rc = ctx.lib.mbb_chain_reweight(ctx.h, _native._d(chain), _native._d(lnp), chain.shape[0] if nsrc is None else nsrc,
                                    chain.shape[1] if nw is None else nw, chain.shape[2] if nsteps is None else nsteps,
                                    C.byref(spec), C.byref(out))
    return rc, raw, ctx


def test_native_refusals_leave_the_context_usable(mbb, world, g_lnl, g_res):
    """10. The C-ABI's refusals, each followed by a good call that gives the right answer: null arguments, wrong
    sources, a window above MBB_PW_MAX_WINDOW (an untouched block of zeros far too short for the stated shape: the
    refusal comes before any read), too many percentiles, bad burn / thin, no bands or data, no resident chain.  (A
    sharded context: tests/test_zz_gpu_processes_reweight.py.  A target on another device needs two GPUs: not run.)"""
    from mbb_emcee_amd import _native, reweight
    data, run = world
    like = RC.device_like(mbb, data, prior=(RC.PRIOR_MEAN, RC.WIDTHS["low"]))
    chain = np.ascontiguousarray(g_res["thick_walpha/chain"][None, :7, :])          # 1 x 7 x 16
    lnp = np.ascontiguousarray(_lp(run, chain[0])[None])
    rc, ref, ctx = _native_call(like, chain, lnp, burn=2)
    assert rc == 0 and ref.n_used[0] == 7 * 14

    def good():
        rc, raw, _ = _native_call(like, chain, lnp, burn=2)
        assert rc == 0
        for f in RAW_FIELDS:
            assert np.array_equal(getattr(raw, f), getattr(ref, f), equal_nan=True), f

    for kw, msg in [(dict(burn=16), "burn"), (dict(burn=-1), "burn"), (dict(thin=0), "burn"), (dict(nsteps=0), "empty chain"),
                    (dict(nw=0), "empty chain"), (dict(nsrc=0), "empty chain"), (dict(npct=9), "percentiles"),
                    (dict(npct=0), "percentiles")]:
        rc, _, _ = _native_call(like, chain, lnp, **kw)
        assert rc == -2 and msg in ctx.lib.mbb_last_error().decode(), (msg, rc, ctx.lib.mbb_last_error())
        good()
    zeros, zl = np.zeros((1, 1, 8, 5)), np.zeros((1, 1, 8))
    rc, _, _ = _native_call(like, zeros, zl, nw=1, nsteps=_native.PW_MAX_WINDOW + 1)
    assert rc == -2 and "MBB_PW_MAX_WINDOW" in ctx.lib.mbb_last_error().decode() and not zeros.any()
    good()
    rc, _, _ = _native_call(like, zeros, zl, nw=1 << 12, nsteps=1 << 12, thin=3)
    assert rc == -2 and "MBB_PW_MAX_WINDOW" in ctx.lib.mbb_last_error().decode()
    good()

    def drop(field):
        def edit(spec, out):
            setattr(out, field, None)
        return edit
    optional = ("target_lnprob", "log_ratio", "log_weight", "weight")
    for field in [f[0] for f in _native.ReweightOut._fields_]:
        rc = _native_call(like, chain, lnp, burn=2, edit=drop(field))[0]
        assert rc == (0 if field in optional else -2), field

    def no_summary(spec, out):
        spec.summary = None
    assert _native_call(like, chain, lnp, edit=no_summary)[0] == -2
    req = reweight._Request(like)
    s, out = req.spec(), reweight._Raw(1, 2).out()
    assert ctx.lib.mbb_chain_reweight(ctx.h, None, _native._d(lnp), 1, 7, 16, C.byref(s), C.byref(out)) == -2
    assert ctx.lib.mbb_chain_reweight(ctx.h, _native._d(chain), None, 1, 7, 16, C.byref(s), C.byref(out)) == -2
    assert ctx.lib.mbb_chain_reweight(ctx.h, _native._d(chain), _native._d(lnp), 1, 7, 16, None, C.byref(out)) == -2
    assert ctx.lib.mbb_chain_reweight(ctx.h, _native._d(chain), _native._d(lnp), 1, 7, 16, C.byref(s), None) == -2
    assert ctx.lib.mbb_chain_reweight(None, _native._d(chain), _native._d(lnp), 1, 7, 16, C.byref(s), C.byref(out)) == -2
    good()
    # no bands or data: MBB_ERR_STATE
    bare = _native.Context(None)
    bare.set_model(False, False, 500.0)
    assert bare.lib.mbb_chain_reweight(bare.h, _native._d(chain), _native._d(lnp), 1, 7, 16, C.byref(s), C.byref(out)) == -3
    assert "bands not set" in bare.lib.mbb_last_error().decode()
    bare.set_bands(*like.band_tables())
    assert bare.lib.mbb_chain_reweight(bare.h, _native._d(chain), _native._d(lnp), 1, 7, 16, C.byref(s), C.byref(out)) == -3
    assert "data not set" in bare.lib.mbb_last_error().decode()
    # the sampler call
    lk, tg, p0, _ = _sampler_case(mbb, g_lnl, False)
    sm = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=5)
    sctx, h = sm._handle()
    tctx = _native.analysis_context(tg)
    s8 = reweight._Request(tg).spec()
    raw8 = reweight._Raw(1, 2)
    out8 = raw8.out()
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, tctx.h, C.byref(s8), C.byref(out8)) == -3
    assert "resident" in sctx.lib.mbb_last_error().decode()
    sm.run_mcmc(p0, 8)
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, tctx.h, C.byref(s8), C.byref(out8)) == 0 and raw8.n_used[0] == NW * 8
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, None, C.byref(s8), C.byref(out8)) == -2
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, tctx.h, None, C.byref(out8)) == -2
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, tctx.h, C.byref(s8), None) == -2
    assert sctx.lib.mbb_sampler_reweight(sctx.h, None, tctx.h, C.byref(s8), C.byref(out8)) == -2
    assert sctx.lib.mbb_sampler_reweight(None, h, tctx.h, C.byref(s8), C.byref(out8)) == -2
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, bare.h, C.byref(s8), C.byref(out8)) == -3
    # a three-source target for a one-source chain
    _, tg3, _, _ = _sampler_case(mbb, g_lnl, True)
    t3 = _native.analysis_context(tg3)
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, t3.h, C.byref(s8), C.byref(out8)) == -2
    assert "sources" in sctx.lib.mbb_last_error().decode()
    again = reweight._Raw(1, 2)
    assert sctx.lib.mbb_sampler_reweight(sctx.h, h, tctx.h, C.byref(s8), C.byref(again.out())) == 0
    assert np.array_equal(again.mean, raw8.mean, equal_nan=True) and np.array_equal(again.khat, raw8.khat)
