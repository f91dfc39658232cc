"""Out-of-sample fit on the GPU (csrc/mbb_pointwise.hip.h and mbb_psis.hip.h through mbb_chain_pointwise /
mbb_sampler_pointwise / mbb_pointwise_rows and mbb_emcee_amd/loo.py) against tests/_loo_ref.py in longdouble.

Tolerances, and where they come from:
  * ll per row: against longdouble on the device's own band fluxes (goodness_rows(want_flux=True), which
    tests/test_goodness_gpu.py holds to the oracle), within gamma_(nb+4) (sum_j |L_bj| |r_j|)^2 / L_bb plus 2 eps of the
    constant (_loo_ref.ll_bound): an nb-term fma sum, the subtraction, the square, the division and the final sum;
  * the per-band tables: against _loo_ref.column in longdouble fed the device's own ll (read back through
    mbb_pointwise_rows, the same bits), within 64 x the largest distance of the float64 restatement from the longdouble
    one over this file's cases, computed here on the CPU from the reference alone; the factor covers the device's
    tree-ordered sums and an exp / log within 2 ulp that is not correctly rounded; the bound is asserted < 1e-9;
  * n_used, tail_len, status and everything said to be "the same bits": exact.
The chains are rows of the fixture chains of tests/golden/results.npz, repeated as a stretch-move chain repeats them.
The likelihoods, chains, reference and comparisons are in tests/_loo_cases.py, which tests/test_loo_seams_gpu.py shares:
that file holds the routes of several splits, partial band groups, long tails and 256 sources to the same reference."""
import ctypes as C

import numpy as np
import pytest

from conftest import parity_record
import _loo_ref as LR
from _loo_cases import (BANDS4, LD, TABLES, VARIANTS, _chain, _check_tables, _reference, _same_bits, _setup, _weights,
                        _with_budget)

pytestmark = pytest.mark.gpu

SCALES = (100.0, 1.0, 0.01)
NW, NSTEPS = 34, 64


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


# ---------------------------------------------------------------- 1. per row
ROW_CASES = [v + (c,) for c in ("bands4", "delta1", "delta2", "delta3", "cov12") for v in VARIANTS] + [VARIANTS[1] + ("cov65",)]


@pytest.mark.parametrize("name,opthin,noalpha,case", ROW_CASES)
def test_per_row_ll(mbb, oracle, g_lnl, g_pb, g_res, name, opthin, noalpha, case):
    """1. ll of every row of the fixture chain against longdouble on the device's own band fluxes, at the uncertainties
    scaled by 100, 1 and 0.01; the same rows through the chain path (a one-cell window: lppd is the entry) are the same
    bits."""
    from mbb_emcee_amd import goodness, loo
    chain = g_res[name + "/chain"]
    rows = np.ascontiguousarray(chain.reshape(-1, 5))[:128]
    for scale in SCALES:
        like = _setup(mbb, oracle, g_lnl, g_pb, chain, opthin, noalpha, case, scale)
        ll, st = loo.loo_rows(like, rows)
        assert np.all(st == 0) and ll.shape == (rows.shape[0], int(like._ndata))
        model = goodness.goodness_rows(like, rows, want_flux=True)[3]
        ref = LR.ll_rows(like._flux, model, **_weights(like))[0]
        bound = LR.ll_bound(like._flux, model, **_weights(like))
        err = np.abs((ll.astype(LD) - ref).astype(np.float64)) / bound
        print("    %s %s scale %g: ll %.4g .. %.4g, worst %.3g of its bound" % (name, case, scale, ll.min(), ll.max(), err.max()))
        parity_record("ll per row [its bound]", err.max(), 1.0)
        assert err.max() <= 1.0
        one = mbb.chain_loo(like, rows[:48].reshape(-1, 1, 1, 5))
        assert np.array_equal(one._raw.lppd, ll[:48]) and np.all(one._raw.n_used == 1)
        assert np.all(one._raw.status == (LR.TAIL_SHORT | LR.K_HIGH)) and np.all(np.isinf(one._raw.khat))


# ---------------------------------------------------------------- 2. statistics
STAT_SHAPES = [((1, 8, 64), SCALES), ((1, 5, 4), SCALES), ((1, 7, 3), SCALES), ((1, 5, 91), SCALES), ((1, 8, 57), SCALES),
               ((1, 1, 7283), (1.0,))]
WINDOWS = [dict(), dict(burn=2), dict(thin=2), dict(burn=4)]


@pytest.fixture(scope="module")
def stat_cases(mbb, oracle, g_lnl, g_pb, g_res):
    """Every statistics case of the file: (label, the device's result, the longdouble reference, the float64 one)."""
    name, opthin, noalpha = VARIANTS[1]
    base = g_res[name + "/chain"]
    cases = []

    def add(label, like, chain, **kw):
        keep = {}
        dev = mbb.chain_loo(like, chain, **kw)
        cases.append((label, dev, _reference(mbb, like, chain, dtype=LD, keep=keep, **kw),
                      _reference(mbb, like, chain, dtype=np.float64, keep=keep, **kw)))

    for shape, scales in STAT_SHAPES:
        for scale in scales:
            like = _setup(mbb, oracle, g_lnl, g_pb, base, opthin, noalpha, "bands4", scale)
            add("%s scale %g" % (shape, scale), like, _chain(g_res, name, shape, seed=shape[2]))
    like = _setup(mbb, oracle, g_lnl, g_pb, base, opthin, noalpha, "cov12", 1.0)
    add("cov12 (1, 8, 64)", like, _chain(g_res, name, (1, 8, 64), seed=5))
    like = _setup(mbb, oracle, g_lnl, g_pb, base, opthin, noalpha, "bands4", 1.0)
    for kw in WINDOWS:
        add("(3, 7, 5) %s" % kw, like, _chain(g_res, name, (3, 7, 5), seed=9), **kw)
    return cases


def test_statistics_against_longdouble(stat_cases):
    """2. The device's tables against the longdouble reference fed the device's own ll: counts, tail lengths and status
    exact, the floating-point outputs within 64 x the float64 restatement's own distance from longdouble."""
    spread = max(LR.distance(f, r) for _, _, ref, f64 in stat_cases for cr, cf in zip(ref, f64) for r, f in zip(cr, cf))
    bound = 64.0 * spread
    print("    float64 restatement vs longdouble: %.3g; bound %.3g" % (spread, bound))
    assert 0.0 < bound < 1e-9
    worst = 0.0
    for label, dev, ref, _ in stat_cases:
        w = _check_tables(dev, ref, label)
        print("    %-28s worst %.3g" % (label, w))
        worst = max(worst, w)
    parity_record("loo tables vs longdouble [max(1, |x|)]", worst, bound)
    assert worst <= bound


def test_statistics_cases_cover_the_paths(stat_cases):
    """Asserted of the cases and their uncertainty scales: S = 20, 21, 455, 456, 7283 occur with M = 4, 5, 64, 65, 257;
    some band has k-hat < 0.5, some k-hat > 0.7, and at least half of all (case, band) pairs take the smoothed path."""
    seen = {}
    khat = []
    for _, dev, _, _ in stat_cases:
        for s, m in zip(dev._raw.n_used.ravel(), dev._raw.tail_len.ravel()):
            seen[int(s)] = int(m)
        khat.append(dev._raw.khat.ravel())
    khat = np.concatenate(khat)
    for s, m in ((20, 4), (21, 5), (455, 64), (456, 65), (7283, 257), (512, 68)):
        assert seen.get(s) == m, (s, seen)
    fin = np.isfinite(khat)
    print("    k-hat: %d of %d smoothed, min %.3g max %.3g" % (fin.sum(), khat.size, khat[fin].min(), khat[fin].max()))
    assert np.any(khat[fin] < 0.5) and np.any(khat[fin] > 0.7) and 2 * fin.sum() >= khat.size


# ---------------------------------------------------------------- 3. ties
def test_ties(mbb, oracle, g_lnl, g_pb, g_res, stat_cases):
    """3. A chain in which every row stands three times, and one whose repeats straddle the cutoff: tail lengths exact
    and the tables the reference's, whose tail is a stable sort's.  What this can show of the membership: the number of
    tied entries taken into the tail, and so the ranks the others are smoothed at.  Which of several entries of equal lw
    is taken cannot show in any output: repeats of a row carry the same ll, and every output is a sum over them."""
    name, opthin, noalpha = VARIANTS[1]
    like = _setup(mbb, oracle, g_lnl, g_pb, g_res[name + "/chain"], opthin, noalpha, "bands4", 1.0)
    spread = max(LR.distance(f, r) for _, _, ref, f64 in stat_cases for cr, cf in zip(ref, f64) for r, f in zip(cr, cf))
    rows = g_res[name + "/chain"].reshape(-1, 5)[:100]
    triple = np.ascontiguousarray(np.repeat(rows, 3, axis=0).reshape(1, 4, 75, 5))
    dev = mbb.chain_loo(like, triple)
    ref = _reference(mbb, like, triple)
    assert np.all(dev._raw.n_used == 300) and np.all(dev._raw.tail_len == 52)
    assert _check_tables(dev, ref, "triples") <= 64 * spread
    # repeats of the cutoff's own row: find the cutoff entry of band 0 and plant four more copies of it
    ll = mbb.loo_rows(like, rows)[0][:, 0]
    asc = np.argsort(-ll, kind="stable")                                # ascending lw
    m = LR.tail_len(104)
    cut = rows[asc[100 - m + 1]]                                        # its five copies take places 80 .. 84 of 104
    strad = np.ascontiguousarray(np.concatenate([rows[:50], cut[None].repeat(4, 0), rows[50:]]).reshape(1, 8, 13, 5))
    dev = mbb.chain_loo(like, strad)
    ref = _reference(mbb, like, strad)
    lw = np.sort(-mbb.loo_rows(like, strad.reshape(-1, 5))[0][:, 0])
    assert lw[104 - m - 1] == lw[104 - m], "the repeats do not straddle the cutoff"
    assert _check_tables(dev, ref, "straddle") <= 64 * spread


# ---------------------------------------------------------------- 4. group independence
def test_group_independence(mbb, oracle, g_lnl, g_pb, g_res):
    """4. One band per group and all bands in one give the same bits (4 bands, and 12 with a covariance: the select
    then runs in launches of 3, 3, 3, 3 against 1 twelve times); a smaller call after a larger one; three sources of
    different scales, each its own one-source call; a [3, 300, 300] chain whose second fill chunk begins inside the
    last source."""
    name, opthin, noalpha = VARIANTS[1]
    base = g_res[name + "/chain"]
    for case in ("bands4", "cov12"):
        like = _setup(mbb, oracle, g_lnl, g_pb, base, opthin, noalpha, case, 1.0)
        chain = _chain(g_res, name, (2, 8, 40), seed=3)
        whole = mbb.chain_loo(like, chain, burn=3)
        assert np.all(whole._raw.n_used == 8 * 37)
        assert _same_bits(_with_budget(mbb, like, 0, chain, burn=3), whole), case
    like = _setup(mbb, oracle, g_lnl, g_pb, base, opthin, noalpha, "bands4", 1.0)
    small = _chain(g_res, name, (1, 6, 9), seed=4)
    before = mbb.chain_loo(like, small)
    big = _chain(g_res, name, (3, 300, 300), seed=6)
    bigres = mbb.chain_loo(like, big)
    assert _same_bits(mbb.chain_loo(like, small), before)
    assert _same_bits(_with_budget(mbb, like, 0, big), bigres)
    for src in range(3):
        alone = mbb.chain_loo(like, big[src])
        for f in TABLES:
            assert np.array_equal(getattr(alone._raw, f)[0], getattr(bigres._raw, f)[src], equal_nan=True), (src, f)
    # three sources of different scales through a three-source likelihood
    flux = np.stack([like._flux * s for s in (0.2, 1.0, 5.0)])
    unc = 0.1 * flux + 1.0
    multi = mbb.likelihood(response=True, opthin=opthin, noalpha=noalpha)
    multi.set_phot_multi(BANDS4, flux, unc)
    three = _chain(g_res, name, (3, 8, 40), seed=8)
    three[0, ..., 4] *= 0.2
    three[2, ..., 4] *= 5.0
    res = mbb.chain_loo(multi, three)
    for src in range(3):
        one = mbb.likelihood(response=True, opthin=opthin, noalpha=noalpha)
        one.set_phot(BANDS4, flux[src], unc[src])
        alone = mbb.chain_loo(one, three[src])
        for f in TABLES:
            assert np.array_equal(getattr(alone._raw, f)[0], getattr(res._raw, f)[src], equal_nan=True), (src, f)


# ---------------------------------------------------------------- 5. bad rows
def test_bad_rows(mbb, oracle, g_lnl, g_pb, g_res):
    """5. Failing and NaN rows outside the window change nothing; inside it they are left out of S, M follows, and
    the status bits say so; a source of NaN rows has NaN tables and n_used 0."""
    from mbb_emcee_amd import _native
    name, opthin, noalpha = VARIANTS[1]
    like = _setup(mbb, oracle, g_lnl, g_pb, g_res[name + "/chain"], opthin, noalpha, "bands4", 1.0)
    base = _chain(g_res, name, (3, 10, 16), seed=12)
    kw = dict(burn=4, thin=3)                                           # kept steps 4, 7, 10, 13: S = 40, M = 8
    good = mbb.chain_loo(like, base, **kw)
    assert np.all(good._raw.n_used == 40) and np.all(good._raw.tail_len == 8)
    assert np.all((good._raw.status & ~(LR.K_HIGH | LR.WAIC_VAR_HIGH | LR.TAIL_FLAT)) == 0)
    out = base.copy()
    out[1, 2, 5, 3] = -1.0
    out[2, 0, 8, 0] = np.nan
    assert _same_bits(mbb.chain_loo(like, out, **kw), good)
    ins = base.copy()
    ins[1, 2, 7, 3] = -1.0
    ins[1, 5, 4, 1] = -0.5
    for w in range(4):
        ins[1, w, 13, 0] = np.nan                                       # 6 rows gone: S = 34, M = 7
    g = mbb.chain_loo(like, ins, **kw)
    bits = sum(1 << (_native.SUM_ROW_SHIFT + r) for r in (_native.ROW_BAD_ALPHA, _native.ROW_BAD_BETA, _native.ROW_NONFINITE))
    assert np.all(g._raw.n_used[1] == 34) and np.all(g._raw.tail_len[1] == 7)
    assert np.all((g._raw.status[1] & ~(LR.K_HIGH | LR.WAIC_VAR_HIGH | LR.TAIL_FLAT)) == (bits | LR.HAS_NAN))
    for f in TABLES:
        assert np.array_equal(getattr(g._raw, f)[[0, 2]], getattr(good._raw, f)[[0, 2]], equal_nan=True), f
    ref = _reference(mbb, like, ins[1:2], **kw)
    for b, r in enumerate(ref[0]):
        assert (g._raw.status[1, b] & 0xff) == r["status"]
        assert LR.distance({k: getattr(g._raw, k)[1, b] for k in LR.FLOATS}, r) < 1e-9
    allnan = base.copy()
    allnan[2] = np.nan
    g = mbb.chain_loo(like, allnan, **kw)
    assert np.all(g._raw.n_used[2] == 0) and np.all(g._raw.tail_len[2] == 0)
    for f in ("lppd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "loo_pit"):
        assert np.all(np.isnan(getattr(g._raw, f)[2])), f
    assert np.all(np.isinf(g._raw.khat[2])) and np.all(g._raw.status[2] & LR.EMPTY) and np.all(g._raw.status[2] & LR.TAIL_SHORT)
    for f in TABLES:
        assert np.array_equal(getattr(g._raw, f)[:2], getattr(good._raw, f)[:2], equal_nan=True), f


# ---------------------------------------------------------------- 6. through the stack
def _sampler_case(mbb, g_lnl, multi):
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
    """6. sampler.loo() and run_mcmc(storechain=False, summary=, loo=) equal chain_loo on the chain a storechain=True
    run of the same seed brings back, bit for bit; the run's other seven analyses are what they are without loo=."""
    lk, p0, bands = _sampler_case(mbb, g_lnl, multi)
    a = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    a.run_mcmc(p0, NSTEPS)
    assert a.loo_ is None
    host = mbb.chain_loo(lk, a.chain, burn=5, thin=2)
    res = a.loo(burn=5, thin=2)
    assert _same_bits(res, host) and res.nsteps_used == 30 and res.nwalkers == NW
    assert res.elpd_loo.shape == ((3,) if multi else ()) and np.all(res.n_used == NW * 30)
    skw = dict(burn=5, thin=2, derived=("peaklambda",), percentile=(68.3, 95.4))
    mkw = dict(bins=24, bins2d=6)
    specs = [bands[3], 70.0]
    others = dict(summary=dict(skw), convergence=True, marginals=dict(mkw), predict=specs, draws=9, goodness=True, evidence=dict(n2=256))
    b = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    b.run_mcmc(p0, NSTEPS, storechain=False, loo=True, **others)
    assert b.chain.shape[-2] == 0 and b.loo_.burn == 5 and b.loo_.thin == 2
    assert _same_bits(b.loo_, host) and _same_bits(b.loo(burn=5, thin=2), host)
    c = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=77)
    c.run_mcmc(p0, NSTEPS, storechain=False, **others)
    assert c.loo_ is None
    import _summary_ref as SR
    assert SR.raw_equal(b.summary, c.summary)
    for f in ("tau", "ess", "rhat", "window", "status"):
        assert np.array_equal(getattr(b.convergence_, f), getattr(c.convergence_, f), equal_nan=True), f
    for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "status"):
        assert np.array_equal(getattr(b.marginals_._raw, f), getattr(c.marginals_._raw, f), equal_nan=True), f
    for f in ("n_used", "mean", "min", "max", "pct", "status"):
        assert np.array_equal(getattr(b.predictions_._raw, f), getattr(c.predictions_._raw, f), equal_nan=True), f
    for k, v in c.draws_.arrays().items():
        assert np.array_equal(b.draws_.arrays()[k], v, equal_nan=True), k
    for k, v in c.goodness_.arrays().items():
        assert np.array_equal(b.goodness_.arrays()[k], v, equal_nan=True), k
    for k, v in c.evidence_.arrays().items():
        assert np.array_equal(b.evidence_.arrays()[k], v, equal_nan=True), k
    # after loo() the goodness of fit from the resident chain, which shares the band-flux buffer
    assert np.array_equal(b.goodness(burn=5, thin=2).chisq_mean, c.goodness(burn=5, thin=2).chisq_mean)
    b.run_mcmc(None, 3, storechain=False)
    assert b.loo_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.loo()
    b.run_mcmc(None, 9, loo=True)
    assert b.loo_.nsteps_used == 9 and _same_bits(b.loo_, mbb.chain_loo(lk, b.chain[..., -9:, :]))
    b.reset()
    assert b.loo_ is None


def test_fitter_and_cli_loo(mbb, g_lnl, tmp_path, capsys):
    """mbb_fitter.run(..., loo=...) and the CLI's --loo end to end: the numbers are those of the chain the fit returns;
    without the flag nothing new is printed or written."""
    from mbb_emcee_amd import run_mbb_emcee
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    one = mbb.likelihood(response=True)
    one.set_phot(bands, np.ones(8), np.ones(8))
    flux = one.model_flux(truth)[0]
    fit = mbb.mbb_fitter(nwalkers=NW, response=True, seed=3)
    fit.like.set_phot(bands, flux, 0.1 * flux + 1.0)
    p0 = fit.generate_initial_values(truth, np.array([1.0, 0.1, 50.0, 0.2, 3.0]))
    fit.run(20, NSTEPS, p0, loo=True)
    assert fit.loo is not None and _same_bits(fit.loo, mbb.chain_loo(fit.like, fit.sampler.chain))
    fit.run(20, 16, p0, loo=dict(burn=2), summary=True)
    assert _same_bits(fit.loo, mbb.chain_loo(fit.like, fit.sampler.chain, burn=2))
    fit.run(20, 16, p0)
    assert fit.loo is None
    capsys.readouterr()
    pf = tmp_path / "phot.txt"
    with open(pf, "w") as fh:
        for b, f in zip(bands, flux):
            fh.write("%s %.8g %.8g\n" % (b, f, 0.1 * f + 1.0))
    out = tmp_path / "fit.npz"
    args = [str(pf), str(out), "-r", "-n", str(NW), "-b", "20", "-N", str(NSTEPS), "--initT", "12", "--initBeta", "1.8",
            "--initLambda0", "600", "--initAlpha", "3", "--seed", "5"]
    assert run_mbb_emcee.main(args + ["--loo"]) == 0
    text = capsys.readouterr().out
    assert "elpd_loo" in text and "Pareto k-hat per band" in text and "LOO-PIT" in text
    got = np.load(out)
    assert {"loo_elpd_loo", "loo_khat", "loo_loo_pit", "loo_elpd_loo_band", "loo_se_elpd_loo"} <= set(got.files)
    like = mbb.likelihood(str(pf), response=True)
    for k, v in mbb.chain_loo(like, got["chain"]).arrays().items():
        assert np.array_equal(got[k], v, equal_nan=True), k
    assert run_mbb_emcee.main(args) == 0
    assert capsys.readouterr().out == "" and not any(k.startswith("loo_") for k in np.load(out).files)


# ---------------------------------------------------------------- 7. refusals of the C-ABI
def _native_call(like, chain, burn=0, thin=1, nsrc=None, nw=None, nsteps=None, edit=None, nb=None):
    from mbb_emcee_amd import _native, loo
    ctx = _native.analysis_context(like)
    s = _native.PointwiseSpec()
    s.burn, s.thin = burn, thin
    raw = loo._Raw(chain.shape[0], int(like._ndata) if nb is None else nb)
    out = raw.out()
    if edit:
        edit(s, out)
    rc = ctx.lib.mbb_chain_pointwise(ctx.h, _native._d(chain), chain.shape[0] if nsrc is None else nsrc,
                                     chain.shape[1] if nw is None else nw, chain.shape[2] if nsteps is None else nsteps,
                                     C.byref(s), C.byref(out))
    return rc, raw, ctx


def test_native_refusals_leave_the_context_usable(mbb, oracle, g_lnl, g_pb, g_res):
    """7. The C-ABI's refusals, each followed by a good call that gives the right answer: bad windows, null pointers,
    a window whose tail would be longer than kTailMax (an untouched block of zeros far too short for the stated shape:
    the refusal comes before any read), 257 bands, no bands or data, no resident chain."""
    from mbb_emcee_amd import _native, loo
    like = _setup(mbb, oracle, g_lnl, g_pb, g_res["thick_walpha/chain"], False, False, "bands4")
    chain = np.ascontiguousarray(g_res["thick_walpha/chain"][None, :7, :])          # 1 x 7 x 16
    rc, ref, ctx = _native_call(like, chain, burn=2)
    assert rc == 0 and np.all(ref.n_used == 7 * 14)

    def good():
        rc, raw, _ = _native_call(like, chain, burn=2)
        assert rc == 0
        for f in TABLES:
            assert np.array_equal(getattr(raw, f), getattr(ref, f), equal_nan=True), f

    for kw, msg in [(dict(burn=16), "burn"), (dict(burn=-1), "burn"), (dict(thin=0), "burn"), (dict(nsteps=0), "empty chain"),
                    (dict(nw=0), "empty chain"), (dict(nsrc=0), "empty chain")]:
        rc, _, _ = _native_call(like, chain, **kw)
        assert rc == -2 and msg in ctx.lib.mbb_last_error().decode(), (msg, rc, ctx.lib.mbb_last_error())
        good()
    zeros = np.zeros((1, 1, 8, 5))
    rc, _, _ = _native_call(like, zeros, nw=1, nsteps=_native.PW_MAX_WINDOW + 1)
    assert rc == -2 and "tail" in ctx.lib.mbb_last_error().decode() and not zeros.any()
    good()
    rc, _, _ = _native_call(like, zeros, nw=1 << 12, nsteps=1 << 12, thin=3)
    assert rc == -2 and "tail" in ctx.lib.mbb_last_error().decode()
    good()
    with pytest.raises(ValueError, match="longer tail"):
        mbb.chain_loo(like, np.zeros((1, _native.PW_MAX_WINDOW + 1, 5)))

    def drop(field):
        def edit(spec, out):
            setattr(out, field, None)
        return edit
    for field in [f[0] for f in _native.PointwiseOut._fields_]:
        assert _native_call(like, chain, edit=drop(field))[0] == -2, field
    s, out = _native.PointwiseSpec(), loo._Raw(1, 4).out()
    s.burn, s.thin = 0, 1
    assert ctx.lib.mbb_chain_pointwise(ctx.h, None, 1, 7, 16, C.byref(s), C.byref(out)) == -2
    assert ctx.lib.mbb_chain_pointwise(ctx.h, _native._d(chain), 1, 7, 16, None, C.byref(out)) == -2
    assert ctx.lib.mbb_chain_pointwise(ctx.h, _native._d(chain), 1, 7, 16, C.byref(s), None) == -2
    good()
    p = np.ascontiguousarray(chain.reshape(-1, 5))
    n = p.shape[0]
    ll, st = np.empty((n, 4)), np.empty(n, dtype=np.int32)
    assert ctx.lib.mbb_pointwise_rows(ctx.h, _native._d(p), n, _native._d(ll), _native._i(st)) == 0
    assert ctx.lib.mbb_pointwise_rows(ctx.h, None, n, _native._d(ll), _native._i(st)) == -2
    assert ctx.lib.mbb_pointwise_rows(ctx.h, _native._d(p), 0, _native._d(ll), _native._i(st)) == -2
    assert ctx.lib.mbb_pointwise_rows(ctx.h, _native._d(p), n, None, _native._i(st)) == -2
    assert ctx.lib.mbb_pointwise_rows(ctx.h, _native._d(p), n, _native._d(ll), None) == -2
    good()
    # 257 bands
    wave = list(np.linspace(60.0, 1200.0, 257))
    wide = mbb.likelihood()
    wide.set_phot(wave, np.ones(257), np.ones(257))
    rc, _, wctx = _native_call(wide, chain)
    assert rc == -2 and "256 bands" in wctx.lib.mbb_last_error().decode()
    with pytest.raises(ValueError, match="at most 256 bands"):
        mbb.chain_loo(wide, chain)
    # no bands or data: MBB_ERR_STATE
    bare = _native.Context(None)
    bare.set_model(False, False, 500.0)
    assert bare.lib.mbb_chain_pointwise(bare.h, _native._d(chain), 1, 7, 16, C.byref(s), C.byref(out)) == -3
    assert "bands not set" in bare.lib.mbb_last_error().decode()
    assert bare.lib.mbb_pointwise_rows(bare.h, _native._d(p), n, _native._d(ll), _native._i(st)) == -3
    bare.set_bands(*like.band_tables())
    assert bare.lib.mbb_chain_pointwise(bare.h, _native._d(chain), 1, 7, 16, C.byref(s), C.byref(out)) == -3
    assert "data not set" in bare.lib.mbb_last_error().decode()
    # the sampler call
    lk, p0, _ = _sampler_case(mbb, g_lnl, False)
    sm = mbb.DeviceEnsembleSampler(NW, 5, lk, seed=5)
    sctx, h = sm._handle()
    raw8 = loo._Raw(1, 8)
    out8 = raw8.out()
    assert sctx.lib.mbb_sampler_pointwise(sctx.h, h, C.byref(s), C.byref(out8)) == -3
    assert "resident" in sctx.lib.mbb_last_error().decode()
    sm.run_mcmc(p0, 8)
    assert sctx.lib.mbb_sampler_pointwise(sctx.h, h, C.byref(s), C.byref(out8)) == 0 and raw8.n_used[0, 0] == NW * 8
    assert sctx.lib.mbb_sampler_pointwise(sctx.h, h, None, C.byref(out8)) == -2
    assert sctx.lib.mbb_sampler_pointwise(sctx.h, h, C.byref(s), None) == -2
    assert sctx.lib.mbb_sampler_pointwise(sctx.h, None, C.byref(s), C.byref(out8)) == -2
    good()
