"""The out-of-sample fit on the GPU where pw_run (csrc/mbb_hip.hip) and the kernels of csrc/mbb_pointwise.hip.h leave
their simplest route, against tests/_loo_ref.py in longdouble: columns cut into several splits, band groups that are
neither one band nor all, tails of every padded length up to kTailMax, 256 sources, and several sources through one
covariance likelihood.  tests/test_loo_gpu.py holds the one-split, one-group route to the same reference.

Tolerances, by the scheme of test_loo_gpu.py's test_statistics_against_longdouble:
  * n_used, tail_len and status: exact;
  * the seven floating-point tables: against _loo_ref.column in longdouble fed the device's own ll (mbb_pointwise_rows,
    the same bits the chain path forms), by _loo_ref.distance, within 64 x the largest distance of the float64
    restatement from the longdouble one over THIS file's cases, computed from the reference alone and asserted
    0 < bound < 1e-9 (the fixture `bound`);
  * Phi: mpmath up to 20 000 entries.  Above that (and for the 256 sources of 16 400 entries each) both restatements
    take scipy.special.ndtr in float64, whose largest absolute error against mpmath on 2000 of the case's own z (evenly
    through the sorted z, both ends) is added to the bound of loo_pit alone: loo_pit is a weighted mean of Phi with
    weights that sum to 1.
Every case asserts its S, its M and a finite k-hat before anything is compared, so that none passes by a fallback.
tests/test_loo_seams_cpu.py checks the same one-band inputs without a device, on the oracle's band fluxes."""
import numpy as np
import pytest

from conftest import parity_record
import _loo_ref as LR
from _loo_cases import (NDTR_ABOVE, SEAM_DELTA1, VARIANTS, _chain, _check_tables, _columns, _groups, _ll_and_z, _ndtr_error, _same_bits,
                        _seam_nan_rows, _selects, _setup, _with_budget)

pytestmark = pytest.mark.gpu

NAME, OPTHIN, NOALPHA = VARIANTS[1]
WINDOW = dict(burn=4, thin=8)                 # of the [2, 64, 180] chains: 22 kept steps, S = 1408, M = 113
GROUP_SHAPE = (2, 64, 180)


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


@pytest.fixture(scope="module")
def like_of(mbb, oracle, g_lnl, g_pb, g_res):
    def make(case):
        return _setup(mbb, oracle, g_lnl, g_pb, g_res[NAME + "/chain"], OPTHIN, NOALPHA, case, 1.0)
    return make


def _case(label, dev, llz, ndtr=None, row_bits=0):
    """A case: the device's result and, per source, _columns of (ll, z); phi_err as the module docstring says."""
    ref, f64 = [], []
    for ll, z in llz:
        r, f = _columns(ll, z, ndtr=ndtr)
        ref.append(r)
        f64.append(f)
    used = ndtr if ndtr is not None else llz[0][0].shape[0] > NDTR_ABOVE
    phi_err = _ndtr_error(np.concatenate([z.ravel() for _, z in llz])) if used else 0.0
    return dict(label=label, dev=dev, ref=ref, f64=f64, phi_err=phi_err, row_bits=row_bits)


def _rows(chain4, src, burn=0, thin=1):
    return np.ascontiguousarray(chain4[src][:, burn::thin].reshape(-1, 5))


def _smoothed(case, S, M):
    """S, M and a finite k-hat everywhere: asserted before any comparison"""
    raw = case["dev"]._raw
    assert np.all(raw.n_used == S) and np.all(raw.tail_len == M), (case["label"], raw.n_used, raw.tail_len)
    assert np.all((raw.status & (LR.TAIL_FLAT | LR.TAIL_SHORT)) == 0) and np.all(np.isfinite(raw.khat)), case["label"]


def _hold(case, bound):
    """The case's device tables against its reference; returns the worst distance seen."""
    d, p = _check_tables(case["dev"], case["ref"], case["label"], row_bits=case["row_bits"], split_pit=True)
    print("    %-44s worst %.3g; loo_pit %.3g (Phi's error %.3g)" % (case["label"], d, p, case["phi_err"]))
    parity_record("loo seam tables vs longdouble [max(1, |x|)]", d, bound)
    parity_record("loo seam loo_pit vs longdouble", p, bound + case["phi_err"])
    assert d <= bound, (case["label"], d, bound)
    assert p <= bound + case["phi_err"], (case["label"], p, bound, case["phi_err"])
    return max(d, p)


# ---------------------------------------------------------------- the cases
def _delta1_case(mbb, like, g_res, label):
    shape, seed, nan, S, M, splits, P = SEAM_DELTA1[label]
    chain = _chain(g_res, NAME, shape, seed=seed)
    return _case(label, mbb.chain_loo(like, chain), [_ll_and_z(like, _rows(chain, 0))])


@pytest.fixture(scope="module")
def split_cases(mbb, like_of, g_res):
    """1. Split seam: one band at S = 16 384 (1 split) and 16 385 (2 splits of 8193); four response bands of one source
    of the [3, 300, 300] chain (6 splits of 15 000), whole and with burn=7, thin=3 (29 400 entries, 2 splits)."""
    like1, like4 = like_of("delta1"), like_of("bands4")
    cases = [_delta1_case(mbb, like1, g_res, "S 16384"), _delta1_case(mbb, like1, g_res, "S 16385")]
    one = np.ascontiguousarray(_chain(g_res, NAME, (3, 300, 300), seed=6)[1:2])
    for label, kw in (("bands4 S 90000", dict()), ("bands4 S 29400", dict(burn=7, thin=3))):
        cases.append(_case(label, mbb.chain_loo(like4, one, **kw), [_ll_and_z(like4, _rows(one, 0, **kw))]))
    return cases


@pytest.fixture(scope="module")
def tail_cases(mbb, like_of, g_res):
    """2. Tail sizes: one band at S = 116 508 (M = P = 1024), 116 509 (M = 1025, P = 2048), PW_MAX_WINDOW (M = P = 4096)
    and PW_MAX_WINDOW with 1000 NaN rows.  The device's ll of the largest chain is formed once for the last two: ll is
    a function of the row alone, so the NaN rows' entries are struck from it (and asserted non-finite on their own)."""
    from mbb_emcee_amd import _native, loo
    like = like_of("delta1")
    cases = [_delta1_case(mbb, like, g_res, "S 116508"), _delta1_case(mbb, like, g_res, "S 116509")]
    shape, seed = SEAM_DELTA1["S max"][:2]
    assert shape[1] * shape[2] == _native.PW_MAX_WINDOW
    chain = _chain(g_res, NAME, shape, seed=seed)
    ll, z = _ll_and_z(like, _rows(chain, 0))
    cases.append(_case("S max", mbb.chain_loo(like, chain), [(ll, z)]))
    idx = _seam_nan_rows(shape, SEAM_DELTA1["S max, 1000 NaN"][2])
    chain[0].reshape(-1, 5)[idx, 0] = np.nan
    gone, st = loo.loo_rows(like, _rows(chain, 0)[idx])
    assert not np.isfinite(gone).any() and np.all(st != 0)
    ll[idx] = np.nan
    cases.append(_case("S max, 1000 NaN", mbb.chain_loo(like, chain), [(ll, z)],
                       row_bits=1 << (_native.SUM_ROW_SHIFT + _native.ROW_NONFINITE)))
    return cases


@pytest.fixture(scope="module")
def group_cases(mbb, like_of, g_lnl, g_res):
    """3. Band groups: a two-source [2, 64, 180] chain (23 040 cells) through the one-source 12-band covariance
    likelihood at budgets of 1, 2 and 3 MB and the default; the same through a two-source set_phot_multi likelihood of
    8 response bands at 1 MB and the default.  Returns (cases, the default-budget result of each likelihood)."""
    cells = int(np.prod(GROUP_SHAPE))
    assert _groups(12, cells, 1) == [2] * 6 and _groups(12, cells, 2) == [5, 5, 2] and _groups(12, cells, 3) == [8, 4]
    assert _groups(12, cells, 16384) == [12] and _groups(8, cells, 1) == [2] * 4 and _groups(8, cells, 16384) == [8]
    assert [_selects(g) for g in (2, 5, 8, 4, 12)] == [[2], [3, 2], [3, 3, 2], [3, 1], [3, 3, 3, 3]]
    cases, whole = [], {}
    like = like_of("cov12")
    chain = _chain(g_res, NAME, GROUP_SHAPE, seed=7)
    llz = [_ll_and_z(like, _rows(chain, src, **WINDOW)) for src in range(2)]
    first = _case("cov12 default budget", mbb.chain_loo(like, chain, **WINDOW), llz)
    cases.append(first)
    whole["cov12"] = first["dev"]
    for mb in (1, 2, 3):
        cases.append(dict(first, label="cov12 budget %d MB" % mb, dev=_with_budget(mbb, like, mb, chain, **WINDOW)))
    # two sources of different brightness, each with its own data
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rows = g_res[NAME + "/chain"].reshape(-1, 5)
    unit = mbb.likelihood(response=True, opthin=OPTHIN, noalpha=NOALPHA)
    unit.set_phot(bands, np.ones(8), np.ones(8))
    model = unit.model_flux(rows[rows.shape[0] // 2])[0] * (1.0 + 0.05 * (-1.0) ** np.arange(8))
    flux = np.stack([model, 0.2 * model])
    unc = 0.1 * flux + 1.0
    multi = mbb.likelihood(response=True, opthin=OPTHIN, noalpha=NOALPHA)
    multi.set_phot_multi(bands, flux, unc)
    chain = _chain(g_res, NAME, GROUP_SHAPE, seed=8)
    chain[1, ..., 4] *= 0.2
    llz = []
    for src in range(2):
        one = mbb.likelihood(response=True, opthin=OPTHIN, noalpha=NOALPHA)
        one.set_phot(bands, flux[src], unc[src])
        llz.append(_ll_and_z(one, _rows(chain, src, **WINDOW)))
    # (the multi-source likelihood's own ll of the same rows, two equal blocks, is the same bits)
    both = mbb.loo_rows(multi, np.concatenate([_rows(chain, src, **WINDOW) for src in range(2)]))[0]
    assert np.array_equal(both, np.concatenate([llz[0][0], llz[1][0]]), equal_nan=True)
    first = _case("multi8 default budget", mbb.chain_loo(multi, chain, **WINDOW), llz)
    cases.append(first)
    whole["multi8"] = first["dev"]
    cases.append(dict(first, label="multi8 budget 1 MB", dev=_with_budget(mbb, multi, 1, chain, **WINDOW)))
    return cases, whole


MANY = (((256, 5, 5), 106, 25, 5, False), ((256, 4, 4100), 107, 16400, 385, True))


@pytest.fixture(scope="module")
def many_cases(mbb, like_of, g_res):
    """4. 256 sources of one band: [256, 5, 5] and [256, 4, 4100].  Returns (case, chain) pairs."""
    like = like_of("delta1")
    out = []
    for shape, seed, S, M, ndtr in MANY:
        chain = _chain(g_res, NAME, shape, seed=seed)
        ll, z = _ll_and_z(like, np.ascontiguousarray(chain.reshape(-1, 5)))
        ll, z = ll.reshape(shape[0], S, 1), z.reshape(shape[0], S, 1)
        out.append((_case("256 sources %s" % (shape,), mbb.chain_loo(like, chain), [(ll[s], z[s]) for s in range(shape[0])],
                          ndtr=ndtr), chain))
    return out


@pytest.fixture(scope="module")
def bound(split_cases, tail_cases, group_cases, many_cases):
    """64 x the largest distance of the float64 restatement from the longdouble one over every case of this file:
    from the reference alone."""
    cases = split_cases + tail_cases + group_cases[0] + [c for c, _ in many_cases]
    spread = max(LR.distance(f, r) for c in cases for cr, cf in zip(c["ref"], c["f64"]) for r, f in zip(cr, cf))
    print("    float64 restatement vs longdouble over %d cases: %.3g; bound %.3g" % (len(cases), spread, 64.0 * spread))
    parity_record("loo seam float64 restatement vs longdouble", spread, 1e-9 / 64.0)
    assert 0.0 < 64.0 * spread < 1e-9
    return 64.0 * spread


# ---------------------------------------------------------------- the tests
def test_split_seam(split_cases, bound):
    """1. Splits.  Until now every window held to the reference had n <= 7283 and so one split; the merge of
    k_pw_stat1's (count, sum, max, sum exp, min) partials in k_pw_begin, the sum of k_pw_stat2's part2 in k_pw_tail
    and the select's histograms merged over splits ran only where the device was compared with itself.  Here: the last
    window of one split (S = 16 384, M = 384) and the first of two (S = 16 385, per_split 8193, M = 385) in one band;
    six splits (S = 90 000, M = 900, P = 1024) and a thinned window of two (S = 29 400, M = 515) in four bands."""
    for case, (S, M) in zip(split_cases, ((16384, 384), (16385, 385), (90000, 900), (29400, 515))):
        _smoothed(case, S, M)
        _hold(case, bound)


def test_tail_sizes(tail_cases, bound):
    """2. Tail sizes.  The largest tail held to the reference was M = 257 (P = 512, 46 grid points).  Here k_pw_tail's
    gather, padding, bitonic sort and fit at M = 1024 = P, where the padding loop writes nothing (62 grid points, 8
    splits); M = 1025, P = 2048; and the last legal window, PW_MAX_WINDOW = 1 864 135 entries: M = 4096 = P = kTailMax,
    94 = kGridMax grid points, 64 = kMaxSplits splits.  Then the same n with 1000 NaN rows inside the window: the
    cutoff's rank n - M - 1 counts the -inf entries below the finite ones, S = 1 863 135, M = 4095, and the status
    carries HAS_NAN and the rows' NONFINITE bit."""
    for case, label in zip(tail_cases, ("S 116508", "S 116509", "S max", "S max, 1000 NaN")):
        S, M = SEAM_DELTA1[label][3:5]
        _smoothed(case, S, M)
        _hold(case, bound)
    assert np.all(tail_cases[3]["dev"]._raw.status & LR.HAS_NAN) and not np.any(tail_cases[2]["dev"]._raw.status & LR.HAS_NAN)


def test_band_groups(group_cases, bound):
    """3. Band groups, and several sources through one covariance likelihood.  Only pointwise_budget_mb 0 (one band per
    group) and the default (all bands in one) were run, so sel_of() and the select launch had indexed the ColState
    block with nbat = 3 and 1 alone before a reference; nbat = 2 at a source > 0 (stride src * 2 + k) and a last group
    shorter than the others never; and nsrc_data == 1 with invcov was checked for equal bits only.  Here two sources
    through the 12-band covariance likelihood in groups of 2 (nbat 2), of 5, 5, 2 (3 + 2, and a short last group) and
    of 8, 4 (3 + 3 + 2 and 3 + 1), and two sources through a two-source diagonal likelihood of 8 bands in groups of 2
    and of 8 (3 + 3 + 2): each against the reference and bit for bit the default budget's result.  The fixture
    restates pw_run's group rule and asserts these partitions."""
    cases, whole = group_cases
    for case in cases:
        _smoothed(case, 1408, 113)
        _hold(case, bound)
        assert _same_bits(case["dev"], whole[case["label"].split()[0]]), case["label"]


def test_256_sources(mbb, like_of, many_cases, bound):
    """4. Many sources.  nsrc >= 256 forces one split however long the column; no test had 256 sources.  [256, 5, 5]
    (S = 25, M = 5) and [256, 4, 4100] (n = 16 400: two splits with fewer sources), every source against the
    reference.  With M = 5 the fit's x* is the tail's first entry, which a repeated row at the cutoff makes 0: the
    reference says which sources then keep raw weights (TAIL_FLAT, asserted exactly like every status), and at least
    half of the 256 must be smoothed; at n = 16 400 all are.  Sources 0, 128 and 255 are also run alone and held to
    the same reference within the bound -- not bit for bit, because the lone call of 16 400 entries has two splits and
    so another order of its sums."""
    like = like_of("delta1")
    for (case, chain), (shape, seed, S, M, ndtr) in zip(many_cases, MANY):
        raw = case["dev"]._raw
        if S == 25:
            assert np.all(raw.n_used == S) and np.all(raw.tail_len == M) and not np.any(raw.status & LR.TAIL_SHORT)
            assert 2 * np.isfinite(raw.khat).sum() >= raw.khat.size
        else:
            _smoothed(case, S, M)
        _hold(case, bound)
        for src in (0, 128, 255):
            alone = dict(case, label="%s, source %d alone" % (case["label"], src), dev=mbb.chain_loo(like, chain[src]),
                         ref=case["ref"][src:src + 1])
            assert alone["dev"]._raw.n_used[0, 0] == S and alone["dev"]._raw.tail_len[0, 0] == M
            _hold(alone, bound)


def test_seam_cases_cover_the_paths(split_cases, tail_cases, group_cases, many_cases):
    """5. Asserted of the cases above: every (S, M) pair named occurred on the device; the padded length P took every
    power of two from 512 to 4096, with P = M at 1024 and at 4096; some band has k-hat < 0.5 and some k-hat > 0.7."""
    cases = split_cases + tail_cases + group_cases[0] + [c for c, _ in many_cases]
    seen, khat = set(), []
    for c in cases:
        raw = c["dev"]._raw
        seen |= set(zip(raw.n_used.ravel().tolist(), raw.tail_len.ravel().tolist()))
        khat.append(raw.khat.ravel())
    khat = np.concatenate(khat)
    want = {(16384, 384), (16385, 385), (90000, 900), (29400, 515), (116508, 1024), (116509, 1025), (1864135, 4096),
            (1863135, 4095), (1408, 113), (25, 5), (16400, 385)}
    assert want <= seen, want - seen
    padded = {1 << int(M - 1).bit_length() for _, M in seen}
    assert {512, 1024, 2048, 4096} <= padded and {(116508, 1024), (1864135, 4096)} <= seen, padded
    fin = np.isfinite(khat)
    print("    k-hat: %d of %d smoothed, min %.3g max %.3g" % (fin.sum(), khat.size, khat[fin].min(), khat[fin].max()))
    assert np.any(khat[fin] < 0.5) and np.any(khat[fin] > 0.7)
