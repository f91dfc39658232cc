"""The boundary call -- what a host-driven sampler spends its time in -- held to the oracle over the whole prior volume,
by each of the three ways it is evaluated:

  a. the general batch call        lnlike_batch (k_lnlike), what `like(pars)` gives on a fresh object;
  b. the boundary launch           likelihood.__call__'s short way with serving off: rows into the block the kernel
                                   reads, mbb_lnlike_call, one launch per call;
  c. the served call               the same short way answered by the resident kernel (k_serve, csrc/mbb_serve.hip.h),
                                   with a row's quadrature started beside its constructor (`serve_overlap` 2: samples
                                   evaluated AHEAD of the constructor from a hand-built record, a blackbody and a
                                   power-law candidate chosen between afterwards) and after it (`serve_overlap` 0).

on the 600 wide rows (T 3-200 K, beta 0-4.5, lambda0 5-3000 um, alpha 0.1-10, fnorm 0.01-1000 mJy, with the lambda_peak
prior: the second root find) and the 225-row grid of table ends (T 1-5000 K: whole bands beyond x = 48 and in the first
table rows; lambda0 1-4500 um: row 0 of C(y) and C = 1) of tests/_domain_rows.py, in all four models, diagonal and with a
full covariance; six rows no SED can be built from at the batch seams; exponents of 1e79 to 1e300; three sources at once.

Bounds: lnL against the oracle at 1e-10 max(1, |lnL|) with -inf places exact (conftest.lnl_close); everything
said to be "the same" between the ways: the same bits, NaN places included, and the same exception where one raises.
The sampler's own kernels are tests/test_domain_sampler_gpu.py's."""
import numpy as np
import pytest

from conftest import VARIANTS, lnl_close
import _domain_rows as D
from test_gpu_parity import boundary_eval
from test_domain_paths_gpu import _cov

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _rows(which):
    if which not in _CACHE:
        r = {"wide": D.wide_rows, "grid": D.grid_rows}[which]()
        r.setflags(write=False)
        _CACHE[which] = r
    return _CACHE[which]


def _like(mbb, which, opthin, noalpha, cov=False, scale=1.0):
    flux = (D.GRID_FLUX if which == "grid" else D.WIDE_FLUX) * scale
    return D.make_like(mbb, which, opthin, noalpha, cov=_cov(D.unc_of(flux)) if cov else None, scale=scale)


def general(like, pars):
    """(a) lnlike_batch, and the general path's raising (what likelihood.__call__ does with its status)."""
    from mbb_emcee_amd import _native
    lnl, st = like._sync_device().lnlike_batch(np.ascontiguousarray(pars, dtype=np.float64))
    _native.raise_for_status(st)
    return lnl


def boundary_launch(like, pars):
    """(b) likelihood.__call__ on float64 rows the short way with serving off: batches of at most a row per CU, each one
    launch of the boundary kernel.  The counters must say that the resident kernel answered none of them, and the object
    that the call went the short way (a batch with a row the reference raises for is handed on to the general path, which
    raises: nothing is asserted after it)."""
    pars = np.ascontiguousarray(pars, dtype=np.float64)
    ctx = like._sync_device()
    ctx.set_option("serve", 0)
    try:
        cus = ctx.info("cu_count")
        req0, fb0 = ctx.info("serve_requests"), ctx.info("serve_fallbacks")
        out = []
        for i in range(0, pars.shape[0], cus):
            chunk = np.ascontiguousarray(pars[i:i + cus])
            try:
                got = like(chunk)
            finally:
                assert ctx.info("serving") == 0 and ctx.info("serve_requests") == req0 and ctx.info("serve_fallbacks") == fb0
            n = chunk.shape[0]
            assert like._fast is not None and like._fast[3] >= n and (like._fast[7] is not None or n in like._fast[2])
            assert ctx.info("last_kernel_form") == 0              # (a launch of k_lnlike, not k_serve's)
            out.append(got)
    finally:
        ctx.set_option("serve", 1)
    return np.concatenate(out) if out else np.zeros(0)


def served(like, pars, overlap):
    """(c) boundary_eval's served way with the quadrature beside the constructor (overlap 2: whatever the band set's
    size) or after it (0).  Its counter assertions hold for every batch that does not raise; a batch that raises was
    served too -- one request more, no fall-back -- and the options are put back whatever happens."""
    ctx = like._sync_device()
    ctx.set_option("serve_overlap", overlap)
    req0, fb0 = ctx.info("serve_requests"), ctx.info("serve_fallbacks")
    try:
        out = boundary_eval(like, pars, "served")
        assert ctx.info("last_threads") >= 256                     # (narrower, and nothing would run ahead)
        return out
    except ValueError:
        assert ctx.info("serve_requests") == req0 + 1 and ctx.info("serve_fallbacks") == fb0
        raise
    finally:
        ctx.set_option("serve", 1); ctx.set_option("serve_after", 3); ctx.set_option("serve_budget_us", 400)
        ctx.set_option("serve_overlap", 1)


WAYS = [("the boundary launch", boundary_launch),
        ("served, quadrature beside the constructor", lambda like, pars: served(like, pars, 2)),
        ("served, quadrature after the constructor", lambda like, pars: served(like, pars, 0))]


def outcome(fn, like, pars):
    """("raised", type, message) or ("array", values)"""
    try:
        return ("array", fn(like, pars))
    except ValueError as e:
        return ("raised", type(e), str(e))


def same_outcome(a, b):
    if a[0] != b[0]:
        return False
    return np.array_equal(a[1], b[1], equal_nan=True) if a[0] == "array" else a[1:] == b[1:]


# ---------------------------------------------------------------- 1. three ways against the oracle
@pytest.mark.parametrize("which,cov", [("wide", False), ("wide", True), ("grid", False), ("grid", True)])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_three_ways_vs_oracle(mbb, oracle, name, opthin, noalpha, which, cov):
    """Every row by (a), (b) and (c): each within the project's bound of the oracle, (b) and (c) the bits of (a)."""
    like = _like(mbb, which, opthin, noalpha, cov)
    rows = _rows(which)
    orc = D.make_oracle(oracle, like)
    ref, rflux = orc(rows, nthreads=4, return_flux=True)
    assert np.all(orc.status <= 1) and not np.isnan(ref).any()
    fin = np.isfinite(ref)
    if which == "wide":
        assert fin.sum() >= 0.9 * fin.size and fin.sum() == 578
    else:
        # the far branch b = x e^-x is the models' without alpha: with the Wien-side power law x > 48 lies beyond the
        # merge point; their cold rows' PACS fluxes go down to 1e-48 of the normalisation
        assert fin.all() and (rflux.min() < 1e-30) == bool(noalpha)
    label = "%s%s" % (which, ", covariance" if cov else "")
    a = general(like, rows)
    err = lnl_close(a, ref, kind="lnL over the prior volume, general call (%s)" % label)
    print("    %s %s: general call %.3g of max(1, |lnL|), |lnL| up to %.3g" % (name, label, err, np.abs(ref[fin]).max()))
    for what, fn in WAYS:
        got = fn(like, rows)
        err = lnl_close(got, ref, kind="lnL over the prior volume, %s (%s)" % (what, label))
        print("    %s %s: %s %.3g" % (name, label, what, err))
        differ = np.flatnonzero(~((got == a) | (np.isnan(got) & np.isnan(a))))
        assert differ.size == 0, (what, differ[:5], rows[differ[:5]], got[differ[:5]], a[differ[:5]])


# ---------------------------------------------------------------- 2. rows no SED can be built from
@pytest.mark.parametrize("opened", [False, True])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_unbuildable_rows(mbb, oracle, name, opthin, noalpha, opened):
    """A NaN T, an infinite fnorm, alpha = -1, alpha = 0, T = 0 and a NaN beta at rows 0, 63, 64, 255, 256 and 605 of 606
    -- first and last row, either side of a wave and of a batch of 256 -- by (b) and (c), batch by batch as they take
    them: the outcome of (a) on the same batch, the same array with the same NaN and -inf places or, with the lower
    limits of alpha and beta opened so that the gate does not turn such rows into -inf first, the same exception.  A batch
    of good rows through the same object afterwards is served again, and right."""
    rows, keep = D.with_bad_rows()
    like = _like(mbb, "wide", opthin, noalpha)
    if opened:
        like.set_lowlim("alpha", -5.0); like.set_lowlim("beta", -5.0)
    ctx = like._sync_device()
    cus = ctx.info("cu_count")
    raised = 0
    for i in range(0, rows.shape[0], cus):
        batch = np.ascontiguousarray(rows[i:i + cus])
        want = outcome(general, like, batch)
        raised += want[0] == "raised"
        if want[0] == "array":
            # NaN where a NaN or an infinity came in, and nowhere else
            is_nan = np.zeros(batch.shape[0], dtype=bool)
            is_nan[[p - i for p, (what, col) in zip(D.BAD_AT, D.BAD) if i <= p < i + cus and what[:3] in ("NaN", "inf")]] = True
            assert np.array_equal(np.isnan(want[1]), is_nan), (name, opened, i)
        for what, fn in WAYS:
            got = outcome(fn, like, batch)
            assert same_outcome(got, want), (name, opened, i, what, got[:1] + got[1:][:2], want[:1] + want[1:][:2])
    # alpha = -1 and alpha = 0 raise where the model reads alpha and the gate lets them through, and nowhere else
    assert (raised > 0) == (opened and not noalpha), raised
    good = np.ascontiguousarray(_rows("wide")[:cus])
    want = general(like, good)
    for overlap in (2, 0):
        assert np.array_equal(served(like, good, overlap), want, equal_nan=True)      # (its counters: served, no fall-back)
    if not opened:
        lnl_close(want, D.make_oracle(oracle, like)(good, nthreads=4), kind="lnL over the prior volume, general call (wide)")


# ---------------------------------------------------------------- 3. huge exponents
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_huge_exponents(mbb, name, opthin, noalpha):
    """beta, alpha or both at 1e79, 1e80, 1e81, 1e100 and 1e300 in three good rows (_domain_rows.HUGE_BASE), a row at a
    time and all at once: (b) and (c) give the bits of (a) or raise what it raises, so none gives NaN or an infinity
    where (a) is finite.  That is not vacuous: alpha up to 1e100 leaves a finite lnprob in every model (the merge point
    moves beyond every sample and the soft wall at 20 costs a finite 3.2e200), and so does beta up to 1e100 in the
    optically thick models with lambda0 beyond the normalisation wavelength; 1e300 squared overflows the wall: -inf.
    The regression case is k_serve's record for the samples taken ahead of the constructor, which carried beta and
    alpha as they came where make_walker_k holds them at 1e80: for T 25 K, lambda0 600 um and beta 1e100 the served call
    with the quadrature beside the constructor gave NaN where the other ways give -3.156e200 (beta times a logarithm
    beyond 1e90 is more than the sample loop's exp is made for).  Both records now form their exponents through
    held_exponent (csrc/mbb_device.hip.h)."""
    rows, what = D.huge_rows()
    like = _like(mbb, "wide", opthin, noalpha)
    nfinite = 0
    for row, label in zip(rows, what):
        one = np.ascontiguousarray(row[None, :])
        want = outcome(general, like, one)
        nfinite += want[0] == "array" and bool(np.isfinite(want[1][0]))
        for way, fn in WAYS:
            got = outcome(fn, like, one)
            assert same_outcome(got, want), (name, label, way, got, want)
    print("    %s: %d of %d rows finite by the general call" % (name, nfinite, len(what)))
    # alpha alone at the four values below 1e300 in each good row; thick with lambda0 = 600 um: beta and both as well
    assert nfinite == (12 if opthin else 28), nfinite
    # and all at once, where (a) does not raise for any
    want = outcome(general, like, rows)
    for way, fn in WAYS:
        assert same_outcome(outcome(fn, like, rows), want), (name, way)


# ---------------------------------------------------------------- 4. several sources at once
@pytest.mark.parametrize("which", ["wide", "grid"])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_multi_source(mbb, oracle, name, opthin, noalpha, which):
    """[3, m, 5] rows against three sources -- the set's fluxes times 1, 0.3 and 4 --: the bits of the three single-source
    calls, and so the oracle's values."""
    base = D.GRID_FLUX if which == "grid" else D.WIDE_FLUX
    names = D.GRID_BANDS if which == "grid" else D.WIDE_BANDS
    rows = _rows(which)
    m = rows.shape[0] // 3 if which == "grid" else 192
    assert m == (75 if which == "grid" else 192)
    pars = np.ascontiguousarray(rows[:3 * m]).reshape(3, m, 5)
    flux = np.stack([base * s for s in D.SOURCE_SCALES])
    multi = D.make_like(mbb, which, opthin, noalpha)
    multi.set_phot_multi(names, flux, D.unc_of(flux))
    got = multi(pars)
    assert got.shape == (3, m) and np.array_equal(multi(pars.reshape(-1, 5)), got.ravel(), equal_nan=True)
    for g, s in enumerate(D.SOURCE_SCALES):
        single = _like(mbb, which, opthin, noalpha, scale=s)
        assert np.array_equal(got[g], general(single, pars[g]), equal_nan=True), (name, which, g)
        ref = D.make_oracle(oracle, multi, flux=flux[g])(pars[g], nthreads=4)
        lnl_close(got[g], ref, kind="lnL over the prior volume, multi-source call (%s)" % which)
