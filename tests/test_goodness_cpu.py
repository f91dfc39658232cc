"""CPU side of the goodness-of-fit tests (tests/test_goodness_gpu.py is the GPU side): the reference
tests/_goodness_ref.py against scipy, the HOST build of csrc/mbb_gammq.hip.h against mpmath, ``ChainGoodness``'s derived
quantities on hand-made raw results, the request's refusals, the ``goodness=`` rules of the sampler and the fitter on a
faked device, and the declarations of the new entry points.

Bound of the host build, for every order 1 <= nb <= 256 the function accepts: relative (9 + 1.5 ceil(nb/2)) eps where
the true q >= 1e-290 (_goodness_ref.horner_bound_eps), and never more than 64 eps for nb <= 64.  Where it comes from:
e^-x is m_exp(-x/2) applied twice, 2 ulp each (mbb_math.hip.h); the Horner sum has at most ceil(nb/2) steps of one
division and one fma, all terms positive, 1.5 ulp a step at the worst; three more products; erfc of the host's libm
within an ulp and its first-order correction for the rounding of sqrt, whose neglected second order is (x eps)^2.
At nb = 64: 4 + 48 + 3 + 2 = 57; at nb = 256: 4 + 192 + 3 + 2 = 201.  Every order is judged on the 70 points of
_goodness_ref.order_grid, of which at least 60 have a true q >= 1e-290 and at least one is below (asserted); the
orders of NBS also on _grid()."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _goodness_ref as GR

NBS = list(range(1, 9)) + [15, 16, 31, 32, 63, 64]


def _grid():
    """(nb, chisq) pairs: chisq from 1e-3 to 1400 and a few beyond, for every order of NBS."""
    x = np.concatenate([np.geomspace(1e-3, 1400.0, 97), [0.5, 1.0, 2.0, 1416.0, 1490.0, 1500.0, 2999.0, 3001.0]])
    nb = np.repeat(np.array(NBS, dtype=np.int32), x.size)
    return nb, np.tile(x, len(NBS))


@pytest.fixture(scope="module")
def host_q(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    so = str(tmp_path_factory.mktemp("goodness_host") / "libgoodness_host.so")
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "_goodness_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.goodness_host_q.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    lib.goodness_host_q.restype = None

    def q(nb, chisq):
        nb = np.ascontiguousarray(np.broadcast_to(nb, np.shape(chisq)), dtype=np.int32).ravel()
        x = np.ascontiguousarray(chisq, dtype=np.float64).ravel()
        out = np.empty(x.size)
        lib.goodness_host_q(nb.ctypes.data_as(C.POINTER(C.c_int)), x.ctypes.data_as(C.POINTER(C.c_double)), x.size,
                            out.ctypes.data_as(C.POINTER(C.c_double)))
        return out.reshape(np.shape(chisq))
    return q


# ---------------------------------------------------------------- the reference
def test_reference_against_scipy():
    mpmath = pytest.importorskip("mpmath")
    stats = pytest.importorskip("scipy.stats")
    nb, x = _grid()
    sf = stats.chi2.sf(x, nb)
    worst = 0.0
    for n, xi, s in zip(nb, x, sf):
        t = GR.q_mp(int(n), xi)
        if t >= GR.Q_FLOOR:
            worst = max(worst, float(abs(mpmath.mpf(float(s)) - t) / t))
        else:
            assert 0.0 <= s <= 1e-289
    print("scipy.stats.chi2.sf against mpmath: max relative error %.3g" % worst)
    assert worst <= 1e-12
    # chisq: longdouble against plain float64 on a case with an exact answer, and the quadratic form against the sum
    f, m, iv = np.array([3.0, 5.0, 9.0]), np.array([1.0, 2.0, 3.0]), np.array([0.25, 1.0, 4.0])
    assert float(GR.chisq(f, m, ivar=iv)) == 1.0 + 9.0 + 144.0
    assert float(GR.chisq(f, m, invcov=np.diag(iv))) == 154.0
    c = np.array([[2.0, 0.5, 0.0], [0.5, 1.0, 0.25], [0.0, 0.25, 3.0]])
    r = f - m
    assert abs(float(GR.chisq(f, m, invcov=c)) - r @ c @ r) <= 4 * GR.EPS * (np.abs(r) @ np.abs(c) @ np.abs(r))
    assert GR.chisq(np.tile(f, (4, 1)), np.tile(m, (4, 1)), ivar=iv).shape == (4,)
    b = GR.chisq_bound(f, m, ivar=iv)
    assert b > 0 and b < 1e-9 and GR.chisq_bound(f, m, invcov=c) > GR.chisq_bound(f, m, invcov=np.diag(np.diag(c)))


def test_reference_edges():
    mpmath = pytest.importorskip("mpmath")
    for nb in (1, 2, 7, 64):
        assert GR.q_mp(nb, 0.0) == 1 and GR.q_mp(nb, -3.0) == 1 and GR.q_mp(nb, float("inf")) == 0
        assert mpmath.isnan(GR.q_mp(nb, float("nan")))
    assert abs(float(GR.q_mp(2, 2.0)) - np.exp(-1.0)) < 1e-16
    rel, low = GR.q_errors(2, [2.0, 1e5], [np.exp(-1.0) * (1 + 1e-10), 0.0])
    assert rel.shape == (1,) and abs(rel[0] - 1e-10) < 1e-14 and np.array_equal(low, [0.0])


# ---------------------------------------------------------------- the host build of the device function
def test_host_build_edges(host_q):
    inf, nan = float("inf"), float("nan")
    for nb in (1, 2, 3, 8, 63, 64, 255, 256):
        q = host_q(nb, [0.0, -0.0, -5.0, -inf, inf, nan, 1e10, 1e300, 5e-324])
        assert np.array_equal(q[:4], np.ones(4)) and q[4] == 0.0 and np.isnan(q[5]), (nb, q)
        assert q[6] == 0.0 and q[7] == 0.0 and q[8] == 1.0, (nb, q)          # (x^j / j! never meets an e^-x of 0)
    # never a NaN, never outside [0, 1], never rising with chisq
    for nb in NBS + [255, 256]:
        x = np.concatenate([np.geomspace(1e-300, 1e12, 2000), np.linspace(1380.0, 3100.0, 500)])
        x.sort()
        q = host_q(nb, x)
        assert not np.isnan(q).any() and np.all(q >= 0) and np.all(q <= 1), nb
        big = q > 1e-280
        assert np.all(np.diff(q[big]) <= 4 * GR.EPS * q[big][:-1]), nb


def _host_bound_eps(n):
    """(9 + 1.5 ceil(nb/2)) eps, the docstring's derivation with the step count left free; never above the 64 eps the
    orders up to 64 have been held to"""
    return min(64.0, GR.horner_bound_eps(n)) if n <= 64 else GR.horner_bound_eps(n)


def test_host_build_against_mpmath(host_q):
    """Every order the function accepts, 1 .. 256: the orders of NBS on _grid(), every order on its 70 points of
    _goodness_ref.order_grid."""
    pytest.importorskip("mpmath")
    assert [_host_bound_eps(n) for n in (1, 2, 64, 65, 255, 256)] == [10.5, 10.5, 57.0, 58.5, 201.0, 201.0]
    nb, x = _grid()
    got = host_q(nb, x)
    worst, worst_of = 0.0, 0.0
    for n in NBS:
        sel = nb == n
        rel, low = GR.q_errors(n, x[sel], got[sel])
        assert np.all(low >= 0) and np.all(low <= 1e-289), (n, low)
        if rel.size:
            worst = max(worst, rel.max())
            assert rel.max() <= _host_bound_eps(n) * GR.EPS, (n, rel.max(), x[sel][np.argmax(rel)])
    for n in range(1, GR.MAX_NB + 1):
        xs, truth, big = GR.order_truth(n)
        assert big.sum() >= 60 and (~big).sum() >= 1, (n, big.sum())        # (the grid judges the function at this order)
        q = host_q(n, xs)
        rel = GR.rel_errors(truth, big, q)
        assert np.all(q[~big] >= 0) and np.all(q[~big] <= 1e-289), (n, q[~big])
        worst = max(worst, rel.max())
        worst_of = max(worst_of, rel.max() / (_host_bound_eps(n) * GR.EPS))
        assert rel.max() <= _host_bound_eps(n) * GR.EPS, (n, rel.max() / GR.EPS, xs[big][np.argmax(rel)])
    print("host build of m_gammq_half against mpmath, orders 1 .. %d: max relative error %.3g (%.1f eps), %.3f of its bound"
          % (GR.MAX_NB, worst, worst / GR.EPS, worst_of))


def test_probe_op_is_the_function(host_q):
    """The test-only probe's op for m_gammq_half (tests/_device_probe.hip, here its host build): the same bits as the
    host build above at every order, any chisq accepted, and an order that is no integer in [1, 256] refused with the
    probe's domain code before anything is evaluated."""
    import _device_probe as P
    probe = P.load_host()
    assert P.OPS["m_gammq_half"] == 5 and len(set(P.OPS.values())) == len(P.OPS) == 6
    assert os.path.join(P.CSRC, "mbb_gammq.hip.h") in P.DEPS               # (a change to the header rebuilds the probe)
    inf, nan = float("inf"), float("nan")
    x = np.concatenate([GR.order_grid(7), [0.0, -0.0, -5.0, -inf, inf, nan, 1e10, 1e300, 5e-324]])
    orders = np.arange(1, GR.MAX_NB + 1)
    got = probe.gammq(orders[:, None], x)
    assert got.shape == (GR.MAX_NB, x.size)
    assert np.array_equal(got, host_q(np.repeat(orders, x.size).reshape(got.shape), np.tile(x, (GR.MAX_NB, 1))), equal_nan=True)
    out = np.full(1, 7.0)
    for bad in (0.0, 257.0, 1.5, -1.0, nan, inf, 1e300):
        y = np.array([bad])
        assert probe.lib.probe_math(5, P._d(np.ones(1)), P._d(y), 1, P._d(out)) == -2 and out[0] == 7.0, bad
        with pytest.raises(RuntimeError, match="domain"):
            probe.gammq(bad, [1.0])
    assert probe.lib.probe_math(5, P._d(np.ones(1)), None, 1, P._d(out)) == -1                # no order given
    assert probe.lib.probe_math(6, P._d(np.ones(1)), P._d(np.ones(1)), 1, P._d(out)) == -1    # one past the last op


# ---------------------------------------------------------------- ChainGoodness on hand-made raw results
class _Like(object):
    """Stands where a likelihood would: it has data, and touching the device is an error."""
    data_read = True
    nsources = 1
    opthin = noalpha = False
    wavenorm = 500.0

    def __init__(self, nsources=1, ndata=3):
        self.nsources, self._ndata = nsources, ndata
        self._flux = np.array([10.0, 20.0, 30.0])[:ndata]
        self.data_flux_unc = np.array([1.0, 2.0, 4.0])[:ndata]
        self._flux_multi = np.arange(1, nsources + 1)[:, None] * self._flux
        self._ivar_multi = np.ones((nsources, ndata)) / self.data_flux_unc ** 2

    def _sync_device(self):
        raise AssertionError("the device was touched")

    context = property(_sync_device)


def _made(nsrc=1, multi=False, like=None):
    from mbb_emcee_amd import goodness
    like = like or _Like()
    cens, qs = goodness._quantiles(68.3, (50.0,))
    req = goodness._Request(like, qs, burn=2, thin=3)
    raw = goodness._Raw(nsrc, req.ndata, len(qs))
    for s in range(nsrc):
        raw.n_used[s] = 40
        raw.mean[s] = [7.5 + s, 0.4]
        raw.min[s] = [2.0, 0.01]
        raw.max[s] = [30.0, 0.9]
        raw.pct[s, 0] = [5.0, 11.0, 7.0]
        raw.at_mean[s] = [20.0, 1.5, 300.0, 3.0, 40.0, 4.5, 0.21]
        raw.ml[s] = [21.0, 1.6, 310.0, 3.1, 41.0, 2.0, 0.57]
        raw.ml_index[s] = [3, 8]
        raw.ml_model[s] = [9.0, 24.0, 30.0]
        raw.best[s] = [2.5, 0.47]
        raw.best_index[s] = [1, 5]
    return goodness.ChainGoodness(req, raw, multi, cens[0], 10, 4), raw


def test_derived_properties():
    g, raw = _made()
    assert g.ndata == 3 and g.n_used == 40 and g.burn == 2 and g.thin == 3 and g.nwalkers == 10 and g.nsteps_used == 4
    assert np.array_equal(g.chisq_cen(), [7.5, 11.0 - 7.5, 7.5 - 5.0])
    assert g.chisq_mean == 7.5 and g.chisq_min == 2.0 and g.ppp == 0.4 and g.chisq_at_mean == 4.5
    assert g.p_d == 3.0 and g.dic == 10.5
    params, chi, idx = g.max_likelihood
    assert np.array_equal(params, [21.0, 1.6, 310.0, 3.1, 41.0]) and chi == 2.0 and np.array_equal(idx, [3, 8])
    assert np.array_equal(g.pulls, [1.0, -2.0, 0.0])
    assert g.best_fit_chisq == 2.5 and g.best_fit_q == 0.47 and np.array_equal(g.best_index, [1, 5])
    from mbb_emcee_amd.results import _pval
    assert g.percentiles[0] == list(_pval(68.3)) + [50.0] and g.percentiles[1].shape == (2, 3)
    with pytest.raises(RuntimeError, match="made without"):
        g.chisq_cen(95.4)
    arr = g.arrays()
    assert {"goodness_dic", "goodness_p_d", "goodness_pulls", "goodness_ml_params", "goodness_mean", "goodness_status",
            "goodness_best_fit_chisq", "goodness_ml_index", "goodness_ml_model", "goodness_percentiles"} <= set(arr)
    assert all(k.startswith("goodness_") for k in arr) and set(g.arrays("g_")) == {"g_" + k[9:] for k in arr}
    text = str(g)
    assert "ChiSquare over the chain: 7.50 +3.50 -2.50 for 3 data points" in text and "p-value: 0.4000" in text
    assert "DIC: 10.50" in text and "walker 3, step 8" in text and "ChiSquare of best fit point: 2.50" in text
    # a failing SED row inside the window: chisq_cen raises as the other results' intervals do, the rest is there
    from mbb_emcee_amd import _native
    raw.status[0] = (1 << (_native.SUM_ROW_SHIFT + _native.ROW_BAD_ALPHA)) | _native.SUM_HAS_NAN
    with pytest.raises(ValueError, match="alpha must be positive"):
        g.chisq_cen()
    assert "alpha must be positive" in str(g) and g.dic == 10.5
    raw.best_index[0] = -1
    assert "best fit point" not in str(g)


def test_source_axis():
    """A multi-source result keeps its leading axis; a many-source chain through a one-source likelihood too, and its
    pulls are formed with that likelihood's one set of data."""
    g, _ = _made(3, True, _Like(3))
    assert g.chisq_cen().shape == (3, 3) and g.dic.shape == (3,) and g.pulls.shape == (3, 3) and g.status.shape == (3, 2)
    assert np.array_equal(g.p_d, [3.0, 4.0, 5.0]) and np.array_equal(g.pulls[1], [11.0, 8.0, 7.5])
    assert g.max_likelihood[0].shape == (3, 5) and g.max_likelihood[2].shape == (3, 2) and "Source 0 of 3" in str(g)
    g, _ = _made(4, True, _Like(1))
    assert g.pulls.shape == (4, 3) and np.array_equal(g.pulls[3], [1.0, -2.0, 0.0]) and g.chisq_mean.shape == (4,)


# ---------------------------------------------------------------- refusals before the device
def test_request_refusals():
    from mbb_emcee_amd import goodness, chain_goodness
    like = _Like()
    chain = np.zeros((4, 8, 5))
    for kw, msg in ((dict(burn=-1), "burn must be"), (dict(thin=0), "burn must be"), (dict(burn=8), "burn leaves no step"),
                    (dict(percentile=101.0), "Invalid percentile"), (dict(percentiles=(-1.0,)), "Invalid percentile"),
                    (dict(percentile=(68.3, 95.4, 99.7, 50.0), percentiles=(1.0,)), "1 to 8 percentiles")):
        with pytest.raises(ValueError, match=msg):
            chain_goodness(like, chain, **kw)
    with pytest.raises(ValueError, match="chain must be"):
        chain_goodness(like, np.zeros((4, 8, 4)))
    with pytest.raises(ValueError, match="the chain is empty"):
        chain_goodness(like, np.zeros((4, 0, 5)))
    with pytest.raises(ValueError, match="lnprob must have"):
        chain_goodness(like, chain, lnprob=np.zeros((4, 7)))
    # one source's lnprob beside a chain of several: the library would read nsrc times what the array holds
    with pytest.raises(ValueError, match="lnprob must have"):
        chain_goodness(_Like(3), np.zeros((3, 4, 8, 5)), lnprob=np.zeros((4, 8)))
    with pytest.raises(ValueError, match="lnprob must have"):
        chain_goodness(_Like(1), np.zeros((3, 4, 8, 5)), lnprob=np.zeros((4, 8)))
    with pytest.raises(ValueError, match="lnprob must have"):
        chain_goodness(like, chain, lnprob=np.zeros((1, 4, 8)))
    with pytest.raises(ValueError, match="2 sources, the likelihood 3"):
        chain_goodness(_Like(3), np.zeros((2, 4, 8, 5)))
    nodata = _Like()
    nodata.data_read = False
    with pytest.raises(Exception, match="Data not read"):
        chain_goodness(nodata, chain)
    with pytest.raises(Exception, match="Data not read"):
        goodness.goodness_rows(nodata, np.zeros((2, 5)))
    with pytest.raises(ValueError, match=r"pars must be \[n, 5\]"):
        goodness.goodness_rows(like, np.zeros((2, 4)))
    wide = _Like()
    wide._ndata = 257
    with pytest.raises(ValueError, match="at most 256 bands"):
        chain_goodness(wide, chain)
    # everything in order: the next thing is the device
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_goodness(like, chain, lnprob=np.zeros((4, 8)), burn=7, percentile=(68.3, 95.4))
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_goodness(_Like(1), np.zeros((6, 4, 8, 5)))                 # many sources, one set of data


# ---------------------------------------------------------------- the sampler's keyword
def _bare_sampler():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary = 10, 5, _Like(), None, None

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_goodness_keyword_rules():
    s = _bare_sampler()
    p0 = np.zeros((10, 5))
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(p0, 16, storechain=False, goodness=True)
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(p0, 16, goodness=dict(burn=16))
    with pytest.raises(ValueError, match="burn leaves no step"):          # burn taken from the summary's keywords
        s.run_mcmc(p0, 16, summary=dict(burn=16), goodness=True)
    with pytest.raises(TypeError, match="unexpected keyword"):
        s.run_mcmc(p0, 16, goodness=dict(specs=70.0))
    with pytest.raises(ValueError, match="Invalid percentile"):
        s.run_mcmc(p0, 16, goodness=dict(percentile=120.0))
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, storechain=False, summary=dict(burn=15), goodness=True)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, goodness=False)                                # (False is no request: the run itself is next)
    assert s.goodness_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.goodness()
    s._resident = 16
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.goodness(burn=16)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.goodness(burn=15)


def test_goodness_attribute_is_reset():
    s = _bare_sampler()
    s._open = None
    s.goodness_ = object()
    s.reset()
    assert s.goodness_ is None
    s.goodness_ = object()
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(np.zeros((10, 5)), 4)
    assert s.goodness_ is None
    s.goodness_ = object()
    with pytest.raises(AssertionError, match="the device was touched"):
        next(s.sample(np.zeros((10, 5)), iterations=4))
    assert s.goodness_ is None


def test_sharded_run_is_not_tested_for_goodness():
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.lnprobfn = _Like()
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded"):
        s.run_mcmc(np.zeros((10, 5)), 4, goodness=True)


def test_fitter_and_cli_know_goodness():
    import mbb_emcee_amd
    from mbb_emcee_amd import mbb_fitter, run_mbb_emcee
    assert mbb_emcee_amd.chain_goodness is mbb_emcee_amd.goodness.chain_goodness
    assert "ChainGoodness" in mbb_emcee_amd.__all__ and "chain_goodness" in mbb_emcee_amd.__all__
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="goodness= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), goodness=True)
    assert fit.goodness is None
    assert run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz"]).goodness is False
    assert run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz", "--goodness"]).goodness is True


def test_goodness_entries_are_declared_and_bound():
    from mbb_emcee_amd import _native
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_goodness", "mbb_sampler_goodness", "mbb_goodness_rows"):
        assert name in hdr and name in _native.SIGNATURES
    assert [f[0] for f in _native.GoodnessSpec._fields_] == ["npct", "burn", "thin", "pct"]
    assert [f[0] for f in _native.GoodnessOut._fields_] == ["n_used", "mean", "min", "max", "status", "pct", "at_mean", "ml",
                                                            "ml_index", "ml_model", "best", "best_index"]
    assert C.sizeof(_native.GoodnessSpec) == 16 + 8 * _native.SUMMARY_MAX_PCT and C.sizeof(_native.GoodnessOut) == 12 * 8
    # the header's structs list the same members in the same order
    import re
    for struct, cls in (("mbb_goodness_spec", _native.GoodnessSpec), ("mbb_goodness_out", _native.GoodnessOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip(" *").split("[")[0] for decl in body.split(";") if decl.strip()
                 for n in decl.strip().split(None, 1)[1].replace("*", " ").split(",") if n.strip() != "double"]
        names = [n for n in names if n]
        assert names == [f[0] for f in cls._fields_], (struct, names)
    build = open(os.path.join(ROOT, "mbb_emcee_amd", "build.py")).read()
    assert "mbb_goodness.hip.h" in build and "mbb_gammq.hip.h" in build
    src = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_gammq.hip.h")).read()
    from mbb_emcee_amd import goodness
    assert "kGammqMaxNb = %d" % goodness.MAX_BANDS in src
    # the new header stays out of the sampler's translation unit
    flow = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_flow.hip")).read()
    assert "mbb_goodness" not in flow and "mbb_gammq" not in flow
    lib = os.path.join(ROOT, "mbb_emcee_amd", "libmbb_hip.so")
    if os.path.exists(lib) and shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE).stdout.decode()
        for name in ("mbb_chain_goodness", "mbb_sampler_goodness", "mbb_goodness_rows"):
            assert " T " + name in syms
