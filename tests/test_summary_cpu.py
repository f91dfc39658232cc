"""Chain summaries (mbb_emcee_amd/results.py), the parts that need no GPU: the fixture made by the reference's own
mbb_results (tests/golden/summary.npz) against a plain numpy restatement, argument validation, and the C-ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import _summary_ref as SR

VARIANTS = ("thin_walpha", "thick_walpha", "thick_noalpha", "thin_noalpha")


@pytest.fixture(scope="module")
def g_sum():
    return np.load(os.path.join(GOLDEN, "summary.npz"))


@pytest.mark.parametrize("name", VARIANTS)
def test_summary_fixture_is_numpy_restatement(g_res, g_sum, name):
    """Every number the reference's mbb_results gave for the chains of results.npz is what the restatement of
    _parcen_internal / par_lowlim / par_uplim / process_fit in tests/_summary_ref.py gives, bit for bit: that guards the
    fixture, and it is the restatement that the GPU tests use at sizes the reference was not run at."""
    k = name + "/"
    chain, lnp = g_res[k + "chain"], g_res[k + "lnprobability"]
    cen, lim = g_sum["cen_percentiles"], g_sum["lim_percentiles"]
    for i in range(5):
        col = chain[:, :, i].flatten()
        for j, p in enumerate(cen):
            assert np.array_equal(SR.parcen(col, p)[0], g_sum[k + "par_cen"][i, j])
        for j, p in enumerate(lim):
            assert np.percentile(col, 100 - p) == g_sum[k + "par_lowlim"][i, j]
            assert np.percentile(col, p) == g_sum[k + "par_uplim"][i, j]
    par = int(g_sum[k + "clip_param"])
    lo, hi = [None if np.isnan(b) else float(b) for b in g_sum[k + "clip_bounds"]]
    got, n = SR.parcen(chain[:, :, par].flatten(), 68.3, lo, hi)
    assert n == int(g_sum[k + "clip_n_used"]) and 0 < n < 512
    assert np.array_equal(got, g_sum[k + "clip_par_cen"])
    for key, src in (("peaklambda_cen", "peaklambda"), ("lir_cen", "lir"), ("dustmass_cen", "dustmass")):
        assert np.array_equal(SR.parcen(g_res[k + src].flatten(), 68.3)[0], g_sum[k + key])
    pars, val, idx = SR.best_fit(chain, lnp)
    assert np.array_equal(pars, g_sum[k + "best_fit_params"]) and val == float(g_sum[k + "best_fit_lnprob"])
    assert tuple(idx) == tuple(g_sum[k + "best_fit_index"])
    assert int((lnp == lnp.max()).sum()) == int(g_sum[k + "ties_at_max"])


def test_summary_fixture_pins_the_tie_rule(g_sum):
    """The maximum of lnprob is attained more than once in fixture chains, and the tie case appended by the script has
    the best sample at three places: the reference's answer is the first in [walker][step] order."""
    assert max(int(g_sum[v + "/ties_at_max"]) for v in VARIANTS) > 1
    chain, lnp = g_sum["tiecase/chain"], g_sum["tiecase/lnprobability"]
    where = np.argwhere(lnp == lnp.max())
    assert len(where) >= 3
    assert tuple(g_sum["tiecase/best_fit_index"]) == tuple(where[0])
    pars, val, idx = SR.best_fit(chain, lnp)
    assert tuple(idx) == tuple(where[0]) and np.array_equal(pars, g_sum["tiecase/best_fit_params"])


def test_summary_fixture_regenerates_bit_for_bit(g_sum, tmp_path):
    """tests/golden/make_golden_summary.py, run again where the reference is mounted, writes the committed numbers."""
    sys.path.insert(0, GOLDEN)
    try:
        import make_golden as G
    finally:
        sys.path.remove(GOLDEN)
    if not os.path.isdir(G.REFPKG):
        pytest.skip("the reference is not mounted here")
    out = str(tmp_path / "again.npz")
    subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_summary.py"), "--out", out], check=True,
                   stdout=subprocess.PIPE, timeout=900)
    again = np.load(out)
    assert sorted(again.files) == sorted(g_sum.files)
    for key in g_sum.files:
        assert np.array_equal(again[key], g_sum[key], equal_nan=True), key


# ---------------------------------------------------------------- argument validation
class _Like(object):
    """As much of a likelihood as the validation looks at before anything reaches the device."""
    opthin, noalpha, wavenorm, data_read, nsources = False, False, 500.0, False, 1


def _chain(nw=12, nsteps=6):
    rng = np.random.RandomState(0)
    return rng.rand(nw, nsteps, 5), rng.rand(nw, nsteps)


def test_chain_summary_validates_before_the_device():
    from mbb_emcee_amd import results
    chain, lnp = _chain()
    like = _Like()
    with pytest.raises(ValueError, match="Invalid percentile"):
        results.chain_summary(like, chain, lnp, percentile=101.0)
    with pytest.raises(ValueError, match="Invalid percentile"):
        results.chain_summary(like, chain, lnp, percentiles=(-1.0,))
    with pytest.raises(ValueError, match="redshift and lumdist_mpc"):
        results.chain_summary(like, chain, lnp, derived=("lir",))
    with pytest.raises(ValueError, match="redshift and lumdist_mpc"):
        results.chain_summary(like, chain, lnp, derived=("dustmass",), redshift=2.0)
    with pytest.raises(ValueError, match="unknown derived quantity"):
        results.chain_summary(like, chain, lnp, derived=("mass",))
    with pytest.raises(ValueError, match="unknown parameter name"):
        results.chain_summary(like, chain, lnp, clip={"temperature": (1.0, 2.0)})
    with pytest.raises(ValueError, match="burn"):
        results.chain_summary(like, chain, lnp, burn=6)
    with pytest.raises(ValueError, match="thin"):
        results.chain_summary(like, chain, lnp, thin=0)
    with pytest.raises(ValueError, match="chain must be"):
        results.chain_summary(like, chain[..., :4], lnp)
    with pytest.raises(ValueError, match="lnprob must have"):
        results.chain_summary(like, chain, lnp[:, :5])
    with pytest.raises(ValueError, match="1 to 8 percentiles"):
        results.chain_summary(like, chain, lnp, percentile=(10, 20, 30, 40, 50))


def test_chain_summary_object_validates():
    """ChainSummary's queries: the reference's messages for a bad percentile or parameter, a clear error for a derived
    quantity that was not prepared or a percentile that cannot be computed any more."""
    from mbb_emcee_amd import results
    req = results._Request(list(results._pval(68.3)))
    raw = results._Raw(1, 2)
    raw.mean[:] = 1.0; raw.pct[:] = 1.0; raw.min[:] = 0.0; raw.max[:] = 2.0; raw.best[:] = 0.0
    s = results.ChainSummary(_Like(), req, raw, False, None)
    with pytest.raises(ValueError, match="percentile needs to be between 0 and 100"):
        s.par_cen(0, percentile=100.0)
    with pytest.raises(ValueError, match="percentile needs to be between 0 and 100"):
        s.par_lowlim("beta", percentile=0)
    with pytest.raises(ValueError, match="unknown parameter name"):
        s.par_cen("temperature")
    with pytest.raises(ValueError, match="invalid parameter index"):
        s.par_uplim(5)
    with pytest.raises(ValueError, match="was not asked for"):
        s.lir_cen()
    with pytest.raises(RuntimeError, match="chain was not kept"):
        s.par_cen("T", percentile=95.4)
    assert s.par_cen("T/(1+z)").shape == (3,) and s.best_fit_chisq == 0.0
    raw.status[0, 1] = 1                                   # nothing survived the clipping of beta
    with pytest.raises(Exception, match="No elements survive lower/upper limit clipping"):
        s.par_cen("beta")


def test_sharded_sampler_run_is_not_summarised():
    """A rank of a sharded run holds only its own walkers' chain: summary= is refused before anything is launched."""
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded"):
        s.run_mcmc(np.zeros((10, 5)), 4, summary=True)


def test_summary_entries_are_declared_and_bound():
    from mbb_emcee_amd import _native
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("mbb_chain_summary", "mbb_sampler_run_summary"):
        assert re.search(r"\bint %s\s*\(" % name, code) and name in _native.SIGNATURES
        assert "`%s`" % name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the binding's structures are the header's, field for field
    for struct, cls in (("mbb_summary_spec", _native.SummarySpec), ("mbb_summary_out", _native.SummaryOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                names += [re.sub(r"[\s\*]|\[.*?\]", "", n) for n in decl.split(None, 1)[1].split(",")]
        assert names == [f[0] for f in cls._fields_], (struct, names)
    assert _native.SUMMARY_COLS == int(re.search(r"#define MBB_SUMMARY_COLS (\d+)", hdr).group(1))
    assert _native.SUMMARY_MAX_PCT == int(re.search(r"#define MBB_SUMMARY_MAX_PCT (\d+)", hdr).group(1))


# ---------------------------------------------------------------- builders of tests/test_summary_derived_gpu.py
REDSHIFT, LUMDIST = 2.3, 18700.0


def test_derived_seam_shapes_put_the_seam_inside_a_source():
    """The shapes derived from the parsed kSumChunkRows: the chunk seam is strictly inside a source (and inside a
    walker), a second chunk exists, and the short last chunk is one row.  A change of the constant fails here."""
    chunk = SR.chunk_rows(ROOT)
    assert chunk == 1 << 18
    sh = SR.seam_shapes(chunk)
    assert sh["cells"] == ((64, 1, 4100), (0, 1, 3843, 3844, 3845, 4099))
    assert sh["tail"] == ((1, 1, (1 << 18) + 1), (0, (1 << 18) - 1, 1 << 18))
    assert sh["windows"] == ((3, 50, 1750, 7, 3), (1, 64, 4097, 0, 1)) and sh["resident"] == (1, 64, 4100)
    (nsrc, nw, nsteps), steps = sh["cells"]
    assert SR.cell_of(chunk, nw, nsteps) == (63, 0, 3844) and SR.cell_of(chunk - 1, nw, nsteps) == (63, 0, 3843)
    assert set(steps) >= {3843, 3844, 3845} and 0 < 3844 < nsteps - 1
    for nsrc, nw, nsteps in [sh["cells"][0], sh["tail"][0], sh["resident"]] + [w[:3] for w in sh["windows"]]:
        cells = nsrc * nw * nsteps
        assert chunk < cells < 2 * chunk                                   # two chunks, the last one short
        s, w, t = SR.cell_of(chunk, nw, nsteps)
        assert 0 < t < nsteps and (s * nw + w) * nsteps + t == chunk         # the seam is inside a walker's steps
    assert sh["tail"][0][2] - chunk == 1


def test_distinct_chain_is_distinct_and_in_the_box():
    chain, lnp = SR.distinct_chain(5, 3, 41, seed=2)
    flat = chain.reshape(-1, 5)
    assert lnp.shape == chain.shape[:-1] and np.all(flat >= SR.BOX_LO) and np.all(flat <= SR.BOX_HI)
    for k in range(5):
        assert len(np.unique(flat[:, k])) == flat.shape[0]


@pytest.mark.parametrize("shape", SR.seam_shapes(1 << 18)["windows"] + ((3, 20, 30, 5, 2),))
def test_sentinel_chain_has_its_sentinels_where_claimed(shape):
    """Sentinels sit where claimed, the in-window and out-of-window sets are disjoint and as the window says, the
    windowed reference of a parameter column is chain[:, :, burn::thin, i] flattened, and the dust mass (host numpy)
    has its per-source maximum at the in-window sentinel of largest k while every out-of-window cell is larger."""
    from mbb_emcee_amd import postprocess as pp
    nsrc, nw, nsteps, burn, thin = shape
    chunk = 1 << 18
    chain, lnp, inside, outside = SR.sentinel_chain(nsrc, nw, nsteps, burn, thin, chunk, seed=5)
    assert chain.shape == (nsrc, nw, nsteps, 5) and lnp.shape == (nsrc, nw, nsteps)
    assert inside and not (set(inside) & set(outside))
    assert bool(outside) == (thin > 1)
    assert sorted(inside.values()) == list(range(len(inside))) and sorted(outside.values()) == list(range(len(outside)))
    kept = np.zeros(nsteps, dtype=bool)
    kept[burn::thin] = True
    for (s, w, t), k in inside.items():
        assert kept[t] and chain[s, w, t, 0] == SR.SENT_T[0] + SR.SENT_T[1] * k
        assert chain[s, w, t, 4] == SR.SENT_F[0] * (1.0 + SR.SENT_F[1] * k)
    for (s, w, t), k in outside.items():
        assert not kept[t] and chain[s, w, t, 0] == SR.OUT_T[0] + SR.OUT_T[1] * k
        assert chain[s, w, t, 4] == SR.OUT_F[0] * (1.0 + SR.OUT_F[1] * k)
    cells = nsrc * nw * nsteps
    for flat in (0, chunk - 1, chunk, cells - 1):
        if flat < cells:
            assert SR.cell_of(flat, nw, nsteps) in inside or SR.cell_of(flat, nw, nsteps) in outside
    for s in range(nsrc):
        for w in (0, nw - 1):
            first, last = np.flatnonzero(kept)[[0, -1]]
            assert (s, w, first) in inside and (s, w, last) in inside
            if thin > 1:
                assert (s, w, burn - 1) in outside and (s, w, burn + 1) in outside
                assert kept[nsteps - 1] or (s, w, nsteps - 1) in outside
    # everything else is an ordinary row: inside the box, with repeats
    mask = np.ones((nsrc, nw, nsteps), dtype=bool)
    for cell in list(inside) + list(outside):
        mask[cell] = False
    rest = chain[mask]
    assert np.all(rest >= SR.BOX_LO) and np.all(rest <= SR.BOX_HI) and rest[:, 0].max() < SR.SENT_T[0]
    rep = np.all(chain[:, :, 1:] == chain[:, :, :-1], axis=-1)
    assert 0.5 < rep.mean() < 0.7                                           # 60 % of the moves are rejected
    # the window
    win = SR.windowed(chain, burn, thin)
    n = nw * len(range(burn, nsteps, thin))
    assert win.shape == (nsrc, n, 5)
    for i in range(5):
        for s in range(nsrc):
            assert np.array_equal(win[s, :, i], chain[s, :, burn::thin, i].flatten())
    assert np.array_equal(SR.windowed(lnp, burn, thin)[0], lnp[0, :, burn::thin].flatten())
    # dust mass, thick and thin: who holds the maximum
    for like in (_Like(), type("Thin", (_Like,), {"opthin": True, "noalpha": True})()):
        m = pp.dustmass(like, chain, REDSHIFT, LUMDIST)
        mw = SR.windowed(m, burn, thin)
        for s in range(nsrc):
            top = max((k, c) for c, k in inside.items() if c[0] == s)[1]
            assert mw[s].max() == m[top] and (mw[s] == m[top]).sum() == 1
            ks = sorted((k, m[c]) for c, k in inside.items() if c[0] == s)
            assert all(a[1] < b[1] for a, b in zip(ks[:-1], ks[1:]))         # each sentinel is its own value
            for c in outside:
                if c[0] == s:
                    assert m[c] > mw[s].max()
    # the reference statistics of one column, clipped, are numpy's of what survives
    col = win[0, :, 0]
    ref = SR.column_reference(col, [15.85, 84.15], lo=float(np.median(col)))
    keep = col[col >= np.median(col)]
    assert ref["n"] == keep.size and ref["mean"] == keep.mean() and ref["min"] == keep.min() and ref["max"] == keep.max()
    assert np.array_equal(ref["pct"], np.percentile(keep, [15.85, 84.15]))


def test_clip_midpoints_exist_with_their_gap():
    """Test 3's clip bounds: near the 20th and 90th percentile of every source's dust-mass column of the builder's
    chain there is an adjacent pair of the pooled sorted values more than 1e-6 apart (relative), although 60 % of the
    entries repeat their predecessor; the midpoint has entries on both sides within the source."""
    from mbb_emcee_amd import postprocess as pp
    nsrc, nw, nsteps, burn, thin = SR.seam_shapes(SR.chunk_rows(ROOT))["windows"][0]
    chain, _, _, _ = SR.sentinel_chain(nsrc, nw, nsteps, burn, thin, 1 << 18, seed=5)
    m = SR.windowed(pp.dustmass(_Like(), chain, REDSHIFT, LUMDIST), burn, thin)
    pooled = np.sort(m.reshape(-1))
    for s in range(nsrc):
        for q in (20.0, 90.0):
            near = np.percentile(m[s], q)
            bound, gap = SR.clip_midpoint(pooled, near)
            assert gap > 1e-6 and np.all(np.abs(pooled - bound) > 0.4e-6 * bound)
            below = (m[s] < bound).mean()
            assert abs(below - q / 100.0) < 0.01 and 0 < (m[s] <= bound).sum() < m.shape[1]
    with pytest.raises(AssertionError):
        SR.clip_midpoint(np.ones(50), 1.0)


def test_dustmass_closed_form_in_50_digits_is_the_host_closed_form():
    """dustmass_mp (the arbiter when device and host dust mass differ by more than 1e-13) against postprocess.dustmass
    on rows of the box: the double evaluation is within 1e-13 of it."""
    from mbb_emcee_amd import postprocess as pp
    rows = SR.box_rows(np.random.RandomState(9), 12)
    for like, kw in ((_Like(), {}), (type("Thin", (_Like,), {"opthin": True})(), {"kappa": 1.5, "kappa_wave": 250.0})):
        host = pp.dustmass(like, rows, REDSHIFT, LUMDIST, **kw)
        want = np.array([SR.dustmass_mp(r, like.opthin, like.wavenorm, REDSHIFT, LUMDIST, **kw) for r in rows])
        assert np.all(np.abs(host - want) <= 1e-13 * np.abs(want))
