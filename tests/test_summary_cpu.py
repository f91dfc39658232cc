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
