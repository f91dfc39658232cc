"""Marginals without a GPU: the numpy restatement of the definition (tests/_marginals_ref.py) against numpy.histogram
and numpy.histogram2d with samples planted on and beside every edge, ``levels`` and ``mode`` against their
definitions, the argument validation of the Python layer, and the sampler's ``marginals=`` keyword rules on a faked
device."""
import numpy as np
import pytest

import _marginals_ref as MR


def _planted(rng, n, lo, hi, nbins):
    """n random samples over a little more than [lo, hi], then every edge with its neighbours in the doubles, samples
    below and above the range, NaN and both infinities."""
    e = MR.edges(lo, hi, nbins)
    w = hi - lo
    x = np.concatenate((rng.uniform(lo - 0.05 * w, hi + 0.05 * w, n), MR.edge_values(e),
                        [lo - w, hi + w, np.nan, np.inf, -np.inf, np.nan]))
    rng.shuffle(x)
    return x


# ---------------------------------------------------------------- the definition against numpy
@pytest.mark.parametrize("nbins", [1, 2, 3, 63, 64, 4096])
def test_definition_is_numpy_histogram(nbins):
    """Edges bit for bit numpy.linspace's; counts numpy.histogram's, with a given range and with the automatic one,
    on columns of several scales and offsets; the outside and non-finite counts add up."""
    rng = np.random.RandomState(nbins)
    for case, (lo, hi) in enumerate(((0.0, 1.0), (-3.7, 11.3), (1e-3, 1.7e-3), (2.5e5, 2.5e5 + 3.0), (-1e9, 7e8), (17.0, 54.321))):
        x = _planted(rng, 3000, lo, hi, nbins)
        ref = MR.hist1d(x, nbins, (lo, hi))
        assert np.array_equal(ref["edges"].view(np.int64), np.linspace(lo, hi, nbins + 1).view(np.int64)), (case, "edges")
        fin = x[np.isfinite(x)]
        want, we = np.histogram(fin, bins=nbins, range=(lo, hi))
        assert np.array_equal(we.view(np.int64), ref["edges"].view(np.int64))
        assert np.array_equal(ref["counts"], want), (case, np.flatnonzero(ref["counts"] != want)[:8])
        assert ref["n_nonfinite"] == 4 and ref["status"] == MR.NONFINITE
        assert ref["n_below"] == (fin < lo).sum() and ref["n_above"] == (fin > hi).sum()
        assert ref["n_used"] + ref["n_below"] + ref["n_above"] + ref["n_nonfinite"] == x.size
        assert ref["n_below"] > 1 and ref["n_above"] > 1                 # (the planted neighbours of the outer edges)
        # automatic: numpy's default range over the finite samples
        auto = MR.hist1d(x, nbins)
        want, we = np.histogram(fin, bins=nbins)
        assert np.array_equal(we.view(np.int64), auto["edges"].view(np.int64)) and np.array_equal(auto["counts"], want)
        assert auto["n_below"] == 0 and auto["n_above"] == 0 and auto["n_used"] == fin.size


@pytest.mark.parametrize("nbins2", [1, 7, 100])
def test_definition_is_numpy_histogram2d(nbins2):
    rng = np.random.RandomState(100 + nbins2)
    rx, ry = (10.0, 40.0), (-0.5, 2.25)
    x, y = _planted(rng, 4000, rx[0], rx[1], nbins2), _planted(rng, 4000, ry[0], ry[1], nbins2)
    assert x.size == y.size
    fin = np.isfinite(x) & np.isfinite(y)
    H, xe, ye = MR.hist2d(x, y, nbins2, rx, ry)
    want, wx, wy = np.histogram2d(x[fin], y[fin], bins=nbins2, range=[rx, ry])
    assert np.array_equal(H, want.astype(np.int64))
    assert np.array_equal(xe.view(np.int64), wx.view(np.int64)) and np.array_equal(ye.view(np.int64), wy.view(np.int64))
    # samples inside one column's range and outside the other's exist, and are not counted
    px, py = MR.place(x, xe), MR.place(y, ye)
    assert ((px >= 0) & (py < 0)).sum() > 10 and ((px < 0) & (py >= 0)).sum() > 10
    assert H.sum() == ((px >= 0) & (py >= 0)).sum()
    # automatic ranges
    H, xe, ye = MR.hist2d(x, y, nbins2)
    want, wx, wy = np.histogram2d(x[fin], y[fin], bins=nbins2,
                                  range=[MR.auto_range(x), MR.auto_range(y)])
    assert np.array_equal(H, want.astype(np.int64))


@pytest.mark.parametrize("nbins", [1, 2, 7, 64, 4096])
def test_constant_column(nbins):
    """A fixed parameter: numpy's +-0.5 range; with an even nbins the value sits exactly on an edge and belongs to the
    bin above it."""
    for v in (2.0, 500.0, -3.25, 0.0):
        x = np.full(777, v)
        ref = MR.hist1d(x, nbins)
        want, we = np.histogram(x, bins=nbins)
        assert np.array_equal(we.view(np.int64), ref["edges"].view(np.int64)) and np.array_equal(ref["counts"], want)
        assert ref["edges"][0] == v - 0.5 and ref["edges"][-1] == v + 0.5
        assert ref["counts"].max() == 777 and ref["status"] == 0
        if nbins % 2 == 0:
            assert ref["edges"][nbins // 2] == v and ref["counts"][nbins // 2] == 777
    none = MR.hist1d(np.array([np.nan, np.inf]), nbins, (0.0, 1.0))
    assert none["status"] == MR.EMPTY | MR.NONFINITE and np.all(np.isnan(none["edges"])) and none["counts"].sum() == 0


# ---------------------------------------------------------------- levels and mode
def test_levels_against_their_definition():
    from mbb_emcee_amd.marginals import levels_of
    rng = np.random.RandomState(4)
    fr = (0.683, 0.954, 0.5, 1.0, 1e-9)
    tables = [rng.poisson(3.0, (9, 9)), rng.poisson(0.3, (7, 7)), np.full((4, 4), 5), np.zeros((3, 3), dtype=int),
              np.array([[10, 10], [10, 70]]), np.array([[1, 2], [3, 4]]), rng.randint(0, 4, (12, 12))]
    for H in tables:
        assert np.array_equal(levels_of(H, fr), MR.levels_direct(H, fr)), H
    # ties: all bins equal -- the one level holds everything; 68.3 % of [[10, 10], [10, 70]] is the peak alone
    assert np.array_equal(levels_of(np.full((4, 4), 5), (0.1, 0.9)), [5, 5])
    assert np.array_equal(levels_of(np.array([[10, 10], [10, 70]]), (0.683, 0.954)), [70, 10])
    assert np.array_equal(levels_of(np.zeros((3, 3)), (0.5,)), [0])
    with pytest.raises(ValueError, match="fraction"):
        levels_of(np.ones((2, 2)), (1.5,))


def _made(counts1, edges1, multi=False, counts2=None, pairs=()):
    """A ChainMarginals around given tables."""
    from mbb_emcee_amd import marginals
    nsrc, _, nb = counts1.shape
    req = marginals._Request(bins=nb, bins2d=0 if counts2 is None else counts2.shape[-1], pairs=list(pairs))
    raw = marginals._Raw(nsrc, req.bins, req.bins2d, len(req.pairs))
    raw.counts1[:], raw.edges1[:] = counts1, edges1
    if counts2 is not None:
        raw.counts2[:] = counts2
        raw.edges2[:] = np.linspace(0.0, 1.0, req.bins2d + 1)
    return marginals.ChainMarginals(req, raw, multi, 10, 20)


def test_mode_pdf_and_orientation():
    c = np.zeros((2, 8, 4), dtype=np.uint32)
    c[0, 0] = [1, 7, 7, 2]                                    # tied maxima: the first
    c[1, 0] = [0, 0, 0, 9]
    e = np.tile(np.array([0.0, 1.0, 2.0, 4.0, 8.0]), (2, 8, 1))
    m = _made(c, e, multi=True)
    assert np.array_equal(m.mode("T"), [1.5, 6.0])
    counts, edges = m.hist1d("T")
    assert counts.dtype == np.int64 and counts.shape == (2, 4) and edges.shape == (2, 5)
    pdf, _ = m.pdf1d(0)
    x = np.concatenate((np.full(1, 0.5), np.full(7, 1.5), np.full(7, 3.0), np.full(2, 5.0)))
    want, _ = np.histogram(x, bins=e[0, 0], density=True)
    assert np.array_equal(pdf[0], want)
    one = _made(c[:1], e[:1])
    assert one.mode("t") == 1.5 and one.hist1d("T")[0].shape == (4,)
    # 2-d: numpy.histogram2d's orientation, the transposed order transposes
    H = np.arange(9, dtype=np.uint32).reshape(1, 1, 3, 3)
    two = _made(np.zeros((1, 8, 4), dtype=np.uint32), e[:1], counts2=H, pairs=[("beta", "T")])
    assert two.pairs == [("T", "beta")]
    assert np.array_equal(two.hist2d("T", "beta")[0], H[0, 0]) and np.array_equal(two.hist2d("beta", "T")[0], H[0, 0].T)
    assert np.array_equal(two.levels("T", "beta", (0.5,)), MR.levels_direct(H[0, 0], (0.5,)))
    with pytest.raises(ValueError, match="was not asked for"):
        two.hist2d("T", "fnorm")
    with pytest.raises(ValueError, match="was not asked for"):
        two.hist1d("lir")
    assert set(two.arrays()) >= {"marginals_counts1", "marginals_edges1", "marginals_counts2", "marginals_edges2",
                                 "marginals_pairs", "marginals_n_used", "marginals_status"}
    assert "marginals_counts2" not in one.arrays() and str(one).count("range:") == 5


# ---------------------------------------------------------------- validation before the device
class _Like(object):
    """Stands where a likelihood would: touching the device is an error."""
    data_read = True

    def _sync_device(self):
        raise AssertionError("the device was touched")

    context = property(_sync_device)


def test_chain_marginals_validates_before_the_device():
    import mbb_emcee_amd
    from mbb_emcee_amd import marginals
    assert mbb_emcee_amd.chain_marginals is marginals.chain_marginals
    assert mbb_emcee_amd.ChainMarginals is marginals.ChainMarginals
    like, chain = _Like(), np.random.RandomState(0).rand(10, 20, 5)
    bad = [(dict(), "chain must be", chain[..., :4]), (dict(), "chain must be", chain[0]),
           (dict(burn=20), "burn", chain), (dict(burn=-1), "burn", chain), (dict(thin=0), "thin", chain),
           (dict(bins=0), "bins must be", chain), (dict(bins=4097), "bins must be", chain),
           (dict(bins2d=-1), "bins2d must be", chain), (dict(bins2d=101), "bins2d must be", chain),
           (dict(pairs="free"), "pairs must be", chain),
           (dict(bins2d=8, pairs=[("T", "T")]), "two different", chain),
           (dict(bins2d=8, pairs=[("T", "lir")]), "was not asked for", chain),
           (dict(bins2d=8, pairs=[("T", "nonsense")]), "unknown parameter", chain),
           (dict(bins2d=8, pairs=[("T",)]), "two column names", chain),
           (dict(pairs=[("T", "beta")]), "pairs need bins2d", chain),
           (dict(range={"T": (1.0, 1.0)}), "range of T", chain), (dict(range={"T": (2.0, 1.0)}), "range of T", chain),
           (dict(range={"beta": (0.0, np.inf)}), "range of beta", chain),
           (dict(range={"beta": (np.nan, 1.0)}), "range of beta", chain),
           (dict(range={"fnorm": (-1e308, 1e308)}), "range of fnorm", chain),
           (dict(range={"dustmass": (0.0, 1.0)}), "was not asked for", chain),
           (dict(derived=("mass",)), "unknown derived", chain),
           (dict(derived=("lir",)), "need redshift and lumdist_mpc", chain),
           (dict(derived=("dustmass",), redshift=1.0, lumdist_mpc=1e3, kappa=0.0), "kappa", chain),
           (dict(derived=("lir",), redshift=[1.0, 2.0], lumdist_mpc=1e3), "one entry per source", chain),
           (dict(peak_model="thick"), "model must be", chain)]
    for kw, msg, ch in bad:
        with pytest.raises(ValueError, match=msg):
            marginals.chain_marginals(like, ch, **kw)
    with pytest.raises(AssertionError, match="the device was touched"):     # (valid arguments do get that far)
        marginals.chain_marginals(like, chain, bins=16, bins2d=8, pairs=[("beta", "T"), ("T", "beta")], burn=4, thin=3,
                                  range={"T": (0.0, 1.0)})
    # what a request resolves to
    r = marginals._Request(bins2d=4)
    assert len(r.pairs) == 10 and r.pairs[0] == (0, 1) and r.pairs[-1] == (3, 4)
    assert marginals._Request(bins2d=0).pairs == [] and marginals._Request(bins2d=0, pairs="all").pairs == []
    r = marginals._Request(bins2d=4, pairs="all", derived=("peaklambda", "dustmass"), redshift=1.0, lumdist_mpc=1e3)
    assert r.columns == [0, 1, 2, 3, 4, 5, 7] and len(r.pairs) == 21
    r = marginals._Request(bins2d=4, pairs=[("beta", "T"), ("T", "beta"), (4, "lambda0")])
    assert r.pairs == [(0, 1), (2, 4)]
    assert marginals._Request(burn=7, thin=3).check_steps(1000) == 331
    s = r.spec()
    assert (s.nbins, s.nbins2, s.npairs) == (64, 4, 2) and (s.pairs[1][0], s.pairs[1][1]) == (2, 4)
    assert s.summary.contents.thin == 1 and s.summary.contents.npct == 1


def _bare_sampler():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary = 10, 5, _Like(), None, None

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_marginals_keyword_rules():
    """storechain=False without summary= keeps no chain on the device: marginals= says so before anything runs; so do
    bad keywords, and marginals() of a sampler that has no chain; the keywords default to the summary's."""
    s = _bare_sampler()
    p0 = np.zeros((10, 5))
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(p0, 16, storechain=False, marginals=True)
    with pytest.raises(ValueError, match="bins must be"):
        s.run_mcmc(p0, 16, marginals=dict(bins=0))
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(p0, 16, marginals=dict(burn=16))
    with pytest.raises(ValueError, match="burn leaves no step"):          # burn taken from the summary's keywords
        s.run_mcmc(p0, 16, summary=dict(burn=16), marginals=True)
    with pytest.raises(ValueError, match="was not asked for"):
        s.run_mcmc(p0, 16, summary=dict(burn=2), marginals=dict(bins2d=4, pairs=[("T", "lir")]))
    with pytest.raises(AssertionError, match="the device was touched"):   # ... and so is derived=
        s.run_mcmc(p0, 16, summary=dict(derived=("lir",), redshift=1.0, lumdist_mpc=1e3),
                   marginals=dict(bins2d=4, pairs=[("T", "lir")]))
    with pytest.raises(TypeError):
        s.run_mcmc(p0, 16, marginals=dict(nbins=2))
    assert s.marginals_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.marginals()
    s._resident = 16
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.marginals(burn=16)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.marginals(burn=15)


def test_marginals_attribute_is_reset():
    """reset() and the start of the next run -- run_mcmc or sample() -- put marginals_ back to None."""
    s = _bare_sampler()
    s._open = None
    s.marginals_ = "held"
    s.reset()
    assert s.marginals_ is None and s.convergence_ is None
    s.marginals_ = "held"
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(np.zeros((10, 5)), 4)
    assert s.marginals_ is None
    s.marginals_ = "held"
    with pytest.raises(AssertionError, match="the device was touched"):
        next(s.sample(np.zeros((10, 5)), iterations=4))
    assert s.marginals_ is None


def test_sharded_run_is_not_binned():
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.lnprobfn = _Like()
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded"):
        s.run_mcmc(np.zeros((10, 5)), 4, marginals=True)


def test_fitter_and_cli_know_marginals():
    from mbb_emcee_amd import mbb_fitter, run_mbb_emcee
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="marginals= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), marginals=True)
    assert fit.marginals is None
    a = run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz"])
    assert a.marginals == 0 and a.marginals2d == 0
    a = run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz", "--marginals", "48", "--marginals2d", "24"])
    assert (a.marginals, a.marginals2d) == (48, 24)


def test_marginals_entries_are_declared_and_bound():
    import ctypes as C
    import os
    from mbb_emcee_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_marginals", "mbb_sampler_marginals"):
        assert name in hdr and name in _native.SIGNATURES
    assert [f[0] for f in _native.MarginalsSpec._fields_] == ["nbins", "nbins2", "npairs", "pairs", "has_range", "lo", "hi",
                                                              "summary"]
    assert [f[0] for f in _native.MarginalsOut._fields_] == ["counts1", "edges1", "counts2", "edges2", "n_used", "n_below",
                                                             "n_above", "n_nonfinite", "status"]
    assert C.sizeof(_native.MarginalsSpec) == 408 and C.sizeof(_native.MarginalsOut) == 72
    for macro, value in (("MBB_MARG_MAX_BINS", _native.MARG_MAX_BINS), ("MBB_MARG_MAX_BINS2", _native.MARG_MAX_BINS2),
                         ("MBB_MARG_MAX_PAIRS", _native.MARG_MAX_PAIRS)):
        assert "#define %s %d" % (macro, value) in hdr
    assert (_native.MARG_EMPTY, _native.MARG_NONFINITE, _native.MARG_ABSENT, _native.MARG_ROW_SHIFT) == (
        _native.SUM_EMPTY, _native.SUM_HAS_NAN, _native.SUM_ABSENT, _native.SUM_ROW_SHIFT)
    src = open(os.path.join(root, "mbb_emcee_amd", "csrc", "mbb_marginals.hip.h")).read()
    assert "__dmul_rn" in src and "__dadd_rn" in src and "atomicAdd(&h[" in src
    assert "mbb_marginals.hip.h" in open(os.path.join(root, "mbb_emcee_amd", "build.py")).read()
