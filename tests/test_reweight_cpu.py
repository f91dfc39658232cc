"""CPU side of the reweighting tests: the integer weighted quantile of tests/_reweight_ref.py against numpy's
inverted-CDF quantile; the two pieces of step logic of csrc/mbb_rwsteps.hip.h in their HOST build
(tests/_reweight_host.cpp) against the Python restatement; the restatement itself on a toy with a closed form;
``ChainReweight``'s arithmetic on hand-made tables; the refusals and the ``reweight=`` rules of the sampler and the fitter
on a faked device; and the inputs of tests/test_reweight_gpu.py, which are chosen in tests/_reweight_cases.py and held
here, with the oracle alone, to what that file takes them for.

Bounds.  rw_quantise in its host build against the restatement in longdouble: exp is correctly rounded to about an ulp
in glibc, so e^lw 2^32 + 1/2 computed in float64 differs from the longdouble value by at most 2^32 * 2 eps < 1e-6 of a
unit: the two floors differ by at most 1, and only where the fraction is within that of 1/2.  rw_target: the
restatement is the same float64 expression, so equality is exact.  The toy: N(0, 1) draws reweighted to N(mu, 1) have
weights w = exp(mu x - mu^2 / 2) with E w = 1 and Var w = e^(mu^2) - 1; under N(0, 1) w^2 is e^(mu^2) times the density
ratio of N(2 mu, 1), so Var(w (x - mu)) = E w^2 (x - mu)^2 = e^(mu^2) (1 + mu^2): to first order (the delta method) the
self-normalised mean has standard error sqrt(e^(mu^2) (1 + mu^2) / n), ln mean w has sqrt((e^(mu^2) - 1) / n), the
effective sample size is n / e^(mu^2), and the weighted median has 1 / (2 f) sqrt(e^(mu^2) / n) with f = 1 / sqrt(2 pi)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _loo_ref as LR
import _reweight_ref as RR
import _reweight_cases as RC

LD = LR.LD
_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_ulonglong)


# ---------------------------------------------------------------- 1. the integer quantile
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_integer_quantile_is_numpys_inverted_cdf(seed):
    rng = np.random.RandomState(seed)
    n = 200
    x = np.round(rng.standard_normal(n), 1)                  # (ties)
    u = rng.randint(0, 5, n).astype(np.int64)                # (zero weights among them)
    rep = np.repeat(x, u)
    for q in (0.0, 0.1, 15.85, 50.0, 84.15, 99.9, 100.0):
        got = RR.wquantile(x, u, q)
        assert got == np.quantile(rep, q / 100.0, method="inverted_cdf"), (q, got)
        try:
            want = np.quantile(x, q / 100.0, weights=u, method="inverted_cdf")
        except TypeError:                                   # (a numpy before 2.0 has no weights=)
            continue
        assert got == want, (q, got, want)
    # equal weights: the unweighted inverted CDF
    one = np.full(n, RR.ONE, dtype=np.int64)
    for q in (0.0, 33.3, 50.0, 100.0):
        assert RR.wquantile(x, one, q) == np.quantile(x, q / 100.0, method="inverted_cdf")
    assert np.isnan(RR.wquantile(x, np.zeros(n, dtype=np.int64), 50.0))
    assert RR.wmean(x, u, np.float64) == pytest.approx(rep.mean(), rel=1e-13)
    X = rng.standard_normal((n, 5))
    assert np.allclose(RR.wcov(X, u, np.float64), np.cov(np.repeat(X, u, axis=0).T, ddof=0), rtol=1e-12, atol=1e-15)


# ---------------------------------------------------------------- 2. the step logic in its host build
class Host(object):
    def __init__(self, tmpdir):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        if not cxx:
            raise RuntimeError("no host C++ compiler")
        so = os.path.join(str(tmpdir), "librw_host.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               os.path.join(ROOT, "tests", "_reweight_host.cpp"), "-o", so])
        L = self.lib = C.CDLL(so)
        L.rw_constants.argtypes = [_dp]
        L.rw_host_quantise.argtypes = [C.c_double]; L.rw_host_quantise.restype = C.c_ulonglong
        L.rw_host_target.argtypes = [C.c_double, C.c_ulonglong]; L.rw_host_target.restype = C.c_ulonglong
        L.rw_host_quantise_n.argtypes = [_dp, C.c_int, _up]
        L.rw_host_target_n.argtypes = [_dp, _up, C.c_int, _up]

    def quantise(self, lw):
        lw = np.ascontiguousarray(lw, dtype=np.float64)
        u = np.empty(lw.size, dtype=np.uint64)
        self.lib.rw_host_quantise_n(lw.ctypes.data_as(_dp), lw.size, u.ctypes.data_as(_up))
        return u.astype(np.int64)

    def target(self, p, U):
        p = np.ascontiguousarray(p, dtype=np.float64)
        U = np.ascontiguousarray(U, dtype=np.uint64)
        t = np.empty(p.size, dtype=np.uint64)
        self.lib.rw_host_target_n(p.ctypes.data_as(_dp), U.ctypes.data_as(_up), p.size, t.ctypes.data_as(_up))
        return t.astype(np.int64)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    try:
        return Host(tmp_path_factory.mktemp("rw_host"))
    except RuntimeError as e:
        pytest.skip(str(e))


def test_quantise_host_build(H):
    c = np.empty(2)
    H.lib.rw_constants(c.ctypes.data_as(_dp))
    assert c[0] == 2.0 ** 32 and c[1] == RR.ONE
    rng = np.random.RandomState(5)
    lw = np.concatenate([-rng.exponential(3.0, 9000), -rng.uniform(0, 30, 1000)])
    got, want = H.quantise(lw), RR.quantise(lw)
    d = np.abs(got - want)
    # the fraction of e^lw 2^32 + 1/2 as longdouble sees it: a difference needs it within 1e-6 of a whole number
    v = np.exp(lw.astype(LD)) * LD(RR.ONE) + LD(0.5)
    frac = (v - np.floor(v)).astype(np.float64)
    near = np.minimum(frac, 1.0 - frac) < 1e-6
    print("    %d of %d differ from the longdouble floor, all by 1" % (int((d > 0).sum()), lw.size))
    assert d.max() <= 1 and np.all(near[d > 0])
    assert got.min() >= 0 and got.max() <= RR.ONE
    # the ends, and what is neither a weight nor a number
    assert H.lib.rw_host_quantise(0.0) == RR.ONE and H.lib.rw_host_quantise(-np.inf) == 0
    assert H.lib.rw_host_quantise(np.nan) == 0 and H.lib.rw_host_quantise(1e-3) == RR.ONE
    assert H.lib.rw_host_quantise(-22.0) == 1 and H.lib.rw_host_quantise(-23.0) == 0      # e^-22 2^32 = 1.198, e^-23 2^32 = 0.44
    assert H.lib.rw_host_quantise(np.log(0.5)) == RR.ONE // 2


def test_target_host_build(H):
    rng = np.random.RandomState(6)
    n = 10000
    p = np.concatenate([rng.uniform(0, 100, n - 6), [0.0, 100.0, 50.0, 15.85, 84.15, 1e-300]])
    Umax = RC.CAP * RR.ONE
    assert Umax < 2 ** 53
    U = np.concatenate([rng.randint(1, 2 ** 62, n - 4, dtype=np.int64) % Umax + 1, [1, Umax, 1, Umax]]).astype(np.int64)
    U[-4:] = [1, Umax, 1, Umax]
    p[-4:] = [0.0, 0.0, 100.0, 100.0]
    got = H.target(p, U)
    want = np.array([RR.target(pp, uu) for pp, uu in zip(p, U)], dtype=np.int64)
    assert np.array_equal(got, want)
    assert np.all(got >= 1) and np.all(got <= U)
    assert list(got[-4:]) == [1, 1, 1, Umax]
    assert H.lib.rw_host_target(50.0, 0) == 0 and H.lib.rw_host_target(50.0, 1) == 1
    assert H.lib.rw_host_target(50.0, 10) == 5 and H.lib.rw_host_target(50.1, 10) == 6
    assert H.lib.rw_host_target(100.0, Umax) == Umax and H.lib.rw_host_target(0.0, Umax) == 1


# ---------------------------------------------------------------- 3. a toy with a closed form
@pytest.mark.parametrize("mu", [0.3, 1.0])
def test_gaussian_shift_toy(mu):
    """Draws of N(0, 1) reweighted to N(mu, 1): the weighted mean within five Monte-Carlo errors of mu, lnz_ratio within
    five of 0, the weighted median within five of mu's (the density at the median is 1 / sqrt(2 pi))."""
    n = 40000
    x = np.random.RandomState(17).standard_normal(n)
    lp, lq = -0.5 * x * x, -0.5 * (x - mu) ** 2
    used, zero, left = RR.classes(lp, lq)
    assert used.all()
    sc = RR.scalars(lq - lp, 0, dtype=np.float64)
    u = RR.quantise(sc["lw"].astype(np.float64))
    e2 = np.exp(mu * mu)
    se_mean = np.sqrt(e2 * (1 + mu * mu) / n)
    se_lnz = np.sqrt((e2 - 1) / n)
    mean = float(RR.wmean(x, u))
    print("    mu %g: k-hat %.2f ess %.0f mean %.4f (se %.4f) lnz_ratio %.4f (se %.4f)"
          % (mu, float(sc["khat"]), float(sc["ess"]), mean, se_mean, float(sc["lnz_ratio"]), se_lnz))
    assert abs(mean - mu) < 5 * se_mean
    assert abs(float(sc["lnz_ratio"])) < 5 * se_lnz
    assert abs(float(sc["ess"]) - n / e2) < 0.2 * n / e2
    assert abs(RR.wquantile(x, u, 50.0) - mu) < 5 * np.sqrt(2 * np.pi) * 0.5 * np.sqrt(e2 / n)
    assert float(sc["khat"]) < 0.5
    assert abs(RR.wcov(x[:, None].repeat(5, 1), u)[0, 0] - 1.0) < 0.1


def test_classes_and_degenerate_windows():
    lp = np.array([0.0, 0.0, -np.inf, np.nan, 0.0, 0.0, 1.0])
    lq = np.array([1.0, -np.inf, -np.inf, 0.0, np.nan, np.inf, -1e308])
    used, zero, left = RR.classes(lp, lq)
    assert list(used) == [True, False, False, False, False, False, True]
    assert list(zero) == [False, True, False, False, False, False, False]
    assert list(left) == [False, False, True, True, True, True, False]
    none = RR.scalars(np.empty(0), 3)
    assert none["status"] == RR.EMPTY | RR.K_HIGH | RR.TAIL_SHORT | RR.HAS_ZERO | RR.ALL_ZERO and np.isneginf(none["lnz_ratio"])
    assert np.isnan(RR.scalars(np.empty(0), 0)["lnz_ratio"])
    same = RR.scalars(np.zeros(512), 0)
    assert same["why"] == LR.FIT_FLAT and same["ess"] == 512 and same["lnz_ratio"] == 0
    assert np.all(RR.quantise(np.asarray(same["lw"], dtype=np.float64)) == RR.ONE)
    half = RR.scalars(np.zeros(100), 100)
    assert abs(float(half["lnz_ratio"]) + np.log(2.0)) < 1e-15 and half["status"] & RR.HAS_ZERO


# ---------------------------------------------------------------- 4. ChainReweight on hand-made tables
class _Like(object):
    data_read = True
    opthin = noalpha = False
    wavenorm = 500.0

    def __init__(self, nsources=1, ndata=4):
        self.nsources = nsources
        self._ndata = ndata

    def _sync_device(self):
        raise AssertionError("the device was touched")


@pytest.fixture
def no_device(monkeypatch):
    from mbb_emcee_amd import _native

    def touched(like):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_native, "analysis_context", touched)


def _made(nsrc=2, multi=True, keep=False, khat=0.3, **kw):
    from mbb_emcee_amd import reweight
    req = reweight._Request(_Like(nsrc if multi else 1), percentile=(68.3, 95.4), percentiles=(50.0,), keep=keep,
                            nsources=nsrc, **kw)
    raw = reweight._Raw(nsrc, len(req.qs), 12, keep)
    base = np.arange(nsrc * 8, dtype=np.float64).reshape(nsrc, 8)
    raw.mean[:] = 10.0 + base
    for k, q in enumerate(req.qs):
        raw.pct[:, :, k] = raw.mean + (q - 50.0) / 10.0
    raw.khat[:] = khat
    raw.ess[:] = 77.0
    raw.lnz_ratio[:] = -0.25
    raw.n_used[:] = 100; raw.n_zero[:] = 20; raw.n_left_out[:] = 0
    raw.weight_sum[:] = 100 * RR.ONE // 3
    raw.best[:] = np.arange(6.0)
    raw.best_index[:] = (3, 4)
    return reweight.ChainReweight(req, raw, multi, 10, 12)


def test_chainreweight_vocabulary():
    from mbb_emcee_amd import reweight
    r = _made()
    assert r.qs == [15.85, 84.15, 2.3, 97.7, 50.0] or np.allclose(r.qs, [15.85, 84.15, 2.3, 97.7, 50.0])
    cen = r.par_cen("beta")
    assert cen.shape == (2, 3) and np.array_equal(cen[:, 0], r._raw.mean[:, 1])
    assert np.allclose(cen[0, 1:], [(r.qs[1] - 50) / 10, (50 - r.qs[0]) / 10], rtol=1e-13)
    wide = r.par_cen(0, 95.4)
    assert np.all(wide[:, 1] > r.par_cen(0)[:, 1])
    with pytest.raises(RuntimeError, match="without the 90% interval"):
        r.par_cen(0, 90.0)
    with pytest.raises(ValueError, match="peaklambda was not asked for"):
        r.peaklambda_cen()
    with pytest.raises(ValueError, match="unknown parameter"):
        r.par_cen("gamma")
    with pytest.raises(RuntimeError, match="not kept"):
        r.weight
    best, lq, idx = r.best_fit
    assert best.shape == (2, 5) and np.array_equal(lq, [5.0, 5.0]) and idx.shape == (2, 2)
    assert r.khat.shape == (2,) and r.covariance.shape == (2, 5, 5) and r.mean.shape == (2, 8)
    assert r.percentiles.shape == (2, 8, 5) and r.nwalkers == 10 and r.nsteps_used == 12
    arrs = r.arrays()
    assert {"reweight_khat", "reweight_ess", "reweight_lnz_ratio", "reweight_n_used", "reweight_n_zero", "reweight_n_left_out",
            "reweight_tail_len", "reweight_status", "reweight_weight_sum", "reweight_mean", "reweight_percentiles",
            "reweight_covariance", "reweight_best_fit", "reweight_qs"} <= set(arrs)
    assert "reweight_weight" not in arrs and "reweight_weight" in _made(keep=True).arrays()
    assert set(_made().arrays(prefix="x_")) == {"x_" + k[9:] for k in arrs}
    text = str(r)
    assert "Source 0 of 2" in text and "Pareto k-hat: 0.30" in text and "Warning" not in text and "beta" in text
    assert "k-hat above 0.7" in str(_made(khat=0.9))
    one = _made(nsrc=1, multi=False, keep=True, derived=("peaklambda",))
    assert one.khat.shape == () and one.par_cen("T").shape == (3,) and one.weight.shape == (12,)
    assert one.peaklambda_cen().shape == (3,) and "peaklambda" in str(one)
    assert isinstance(one.best_fit[2], tuple)
    assert (reweight.ChainReweight.K_HIGH, reweight.ChainReweight.TAIL_SHORT, reweight.ChainReweight.TAIL_FLAT,
            reweight.ChainReweight.HAS_ZERO, reweight.ChainReweight.ALL_ZERO) == (16, 32, 64, 128, 65536)


def test_refusals_before_the_device(no_device):
    from mbb_emcee_amd import chain_reweight, _native
    like, chain, lnp = _Like(), np.zeros((4, 8, 5)), np.zeros((4, 8))
    for kw, msg in ((dict(burn=8), "burn leaves no step"), (dict(burn=-1), "burn must be"), (dict(thin=0), "burn must be"),
                    (dict(percentiles=tuple(range(1, 9))), "1 to 8 percentiles"), (dict(percentile=101.0), "Invalid percentile"),
                    (dict(derived=("mass",)), "unknown derived"), (dict(derived=("lir",)), "need redshift")):
        with pytest.raises(ValueError, match=msg):
            chain_reweight(like, chain, lnp, **kw)
    with pytest.raises(ValueError, match="2 sources, the likelihood 3"):
        chain_reweight(_Like(3), np.zeros((2, 4, 8, 5)), np.zeros((2, 4, 8)))
    with pytest.raises(ValueError, match="empty"):
        chain_reweight(like, np.zeros((0, 8, 5)), np.zeros((0, 8)))
    with pytest.raises(ValueError, match="lnprob must have the chain's shape"):
        chain_reweight(like, chain, np.zeros((4, 7)))
    with pytest.raises(TypeError, match="target of a reweighting"):
        chain_reweight(None, chain, lnp)
    nodata = _Like()
    nodata.data_read = False
    with pytest.raises(Exception, match="Data not read"):
        chain_reweight(nodata, chain, lnp)
    big = (_native.PW_MAX_WINDOW + 2) // 2
    with pytest.raises(ValueError, match="more than the device reweights"):
        chain_reweight(like, np.zeros((2, big, 5)), np.zeros((2, big)))
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_reweight(like, chain, lnp, burn=7, thin=2)
    with pytest.raises(AssertionError, match="the device was touched"):
        chain_reweight(_Like(1), np.zeros((6, 4, 8, 5)), np.zeros((6, 4, 8)))


# ---------------------------------------------------------------- 5. the sampler's and the fitter's keyword
def _bare_sampler():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary = 10, 5, _Like(), None, None

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_reweight_keyword_rules():
    s = _bare_sampler()
    p0, tg = np.zeros((10, 5)), _Like()
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(p0, 16, storechain=False, reweight=tg)
    with pytest.raises(ValueError, match="reweight= needs a target"):
        s.run_mcmc(p0, 16, reweight=dict(burn=2))
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(p0, 16, reweight=dict(target=tg, burn=16))
    with pytest.raises(ValueError, match="burn leaves no step"):          # burn taken from the summary's keywords
        s.run_mcmc(p0, 16, summary=dict(burn=16), reweight=tg)
    with pytest.raises(TypeError, match="unexpected keyword"):
        s.run_mcmc(p0, 16, reweight=dict(target=tg, bins=3))
    with pytest.raises(TypeError, match="target of a reweighting"):
        s.run_mcmc(p0, 16, reweight=True)
    with pytest.raises(ValueError, match="more than the device reweights"):
        s.run_mcmc(p0, 200000, reweight=tg)
    with pytest.raises(ValueError, match="1 sources, the likelihood 3"):
        s.run_mcmc(p0, 16, reweight=_Like(3))
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, storechain=False, summary=dict(burn=15), reweight=tg)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(p0, 16, reweight=False)
    assert s.reweight_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.reweight(tg)
    s._resident = 16
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.reweight(tg, burn=16)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.reweight(tg, burn=15)


def test_reweight_attribute_is_reset_and_sharded_run_refused():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = _bare_sampler()
    s._open = None
    s.reweight_ = object()
    s.reset()
    assert s.reweight_ is None
    s.reweight_ = object()
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(np.zeros((10, 5)), 4)
    assert s.reweight_ is None

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k = 10
    s.lnprobfn = _Like()
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded sampler run cannot be reweighted"):
        s.run_mcmc(np.zeros((10, 5)), 4, reweight=_Like())


def test_fitter_cli_and_bindings_know_reweight():
    import re
    import mbb_emcee_amd
    from mbb_emcee_amd import mbb_fitter, run_mbb_emcee, _native, device_sampler
    assert mbb_emcee_amd.chain_reweight is mbb_emcee_amd.reweight.chain_reweight
    assert {"ChainReweight", "chain_reweight"} <= set(mbb_emcee_amd.__all__)
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="reweight= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), reweight=_Like())
    assert fit.reweight is None
    an = device_sampler._ANALYSES["reweight"]
    assert (an.first, an.verb, an.attr, an.method) == ("target", "reweighted", "reweight_", "reweight")
    for order in (device_sampler._REQUEST_ORDER, device_sampler._SHARDED_ORDER, device_sampler._RESULT_ORDER):
        assert order[-1] == "reweight" and set(order) == set(device_sampler._ANALYSES)
    ps = run_mbb_emcee.build_parser()
    assert ps.parse_args(["phot.txt", "out.npz"]).reweight_prior is None
    a = ps.parse_args(["phot.txt", "out.npz", "--reweight-prior", "beta", "1.8", "0.2", "--reweight-prior", "T", "20", "5"])
    assert a.reweight_prior == [["beta", "1.8", "0.2"], ["T", "20", "5"]]
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_reweight", "mbb_sampler_reweight"):
        assert name in hdr and name in _native.SIGNATURES
    assert C.sizeof(_native.ReweightSpec) == 16 and C.sizeof(_native.ReweightOut) == 19 * 8
    for struct, cls in (("mbb_reweight_spec", _native.ReweightSpec), ("mbb_reweight_out", _native.ReweightOut)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip(" *") for decl in body.split(";") if decl.strip()
                 for n in decl.strip().replace("const ", "").split(None, 1)[1].replace("*", " ").split(",")]
        assert [n for n in names if n] == [f[0] for f in cls._fields_], (struct, names)
    for bit in ("K_HIGH = 16", "TAIL_SHORT = 32", "TAIL_FLAT = 64", "HAS_ZERO = 128", "ALL_ZERO = 65536"):
        assert "MBB_RW_" + bit in hdr
    assert "inverted CDF" in hdr and "no ddof correction" in hdr and "inverted CDF" in mbb_emcee_amd.reweight.__doc__
    build = open(os.path.join(ROOT, "mbb_emcee_amd", "build.py")).read()
    assert "mbb_reweight.hip.h" in build and "mbb_rwsteps.hip.h" in build
    flow = open(os.path.join(ROOT, "mbb_emcee_amd", "csrc", "mbb_flow.hip")).read()
    assert "mbb_reweight" not in flow and "mbb_rwsteps" not in flow
    lib = os.path.join(ROOT, "mbb_emcee_amd", "libmbb_hip.so")
    if os.path.exists(lib) and shutil.which("nm"):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE).stdout.decode()
        for name in ("mbb_chain_reweight", "mbb_sampler_reweight"):
            assert re.search(r" T %s$" % name, syms, flags=re.M), name


# ---------------------------------------------------------------- 6. the inputs of tests/test_reweight_gpu.py
@pytest.fixture(scope="module")
def selection(oracle, g_lnl, g_pb, g_res):
    """Per PSIS case of tests/_reweight_cases.py, with the oracle alone: (the shape, the restatement's scalars)."""
    data = RC.data_of(oracle, g_lnl, g_pb, g_res)
    run = RC.oracle_like(oracle, data)
    out = {}
    for label, (shape, seed, prior, planned) in RC.PSIS.items():
        rows = RC.chain_of(g_res, label).reshape(-1, 5)
        lp = run(rows)
        lq = lp if prior is None else RC.oracle_like(oracle, data, prior=prior)(rows)
        used, zero, left = RR.classes(lp, lq)
        out[label] = (shape, int(used.sum()), int(zero.sum()), int(left.sum()), RR.scalars((lq - lp)[used], int(zero.sum())))
    return out, data, run


def test_psis_cases_are_in_their_planned_classes(selection):
    cases = selection[0]
    seen = set()
    for label, (shape, S, nzero, nleft, sc) in cases.items():
        planned = RC.PSIS[label][3]
        print("    %-16s S %6d M %4d k-hat %6.3f: %s" % (label, S, sc["M"], float(sc["khat"]), RC.klass(sc)))
        assert S == shape[1] * shape[2] and nzero == 0 and nleft == 0, label
        assert S <= RC.CAP
        assert RC.klass(sc) == planned, (label, float(sc["khat"]), planned)
        # (not at a class's edge: the device's own lq differs from the oracle's in the last digits)
        if planned in ("low", "mid", "high"):
            assert min(abs(float(sc["khat"]) - 0.5), abs(float(sc["khat"]) - 0.7)) > 0.02, label
        seen.add(planned)
    assert seen == {"short", "flat", "low", "mid", "high"}
    assert sorted(c[1] for c in cases.values()) == [20, 21, 35, 455, 456, 512, 512, 512, 512, 7283, 16384, 16385]
    assert [cases["S 512 " + w][4]["M"] for w in ("low", "mid", "high")] == [68, 68, 68]
    assert cases["S 16384"][4]["M"] == 384 and cases["S 16385"][4]["M"] == 385 and cases["S 20"][4]["M"] == 4
    # the three widths of the prior-added test, on the S = 512 chain
    assert [RC.klass(cases["S 512 " + w][4]) for w in ("low", "mid", "high")] == ["low", "mid", "high"]


def test_limit_case_has_zero_and_used_entries(selection, oracle, g_res):
    _, data, run = selection
    rows = RC.chain_of(g_res, "S 512 low").reshape(-1, 5)
    lp = run(rows)
    used, zero, left = RR.classes(lp, RC.oracle_like(oracle, data, t_limit=RC.T_LIMIT)(rows))
    n = rows.shape[0]
    print("    T >= %g: %d used, %d zero, %d left out of %d" % (RC.T_LIMIT, used.sum(), zero.sum(), left.sum(), n))
    assert zero.sum() >= n / 10 and used.sum() >= n / 10 and left.sum() == 0
    assert np.array_equal(zero, rows[:, 0] < RC.T_LIMIT)
    used, zero, left = RR.classes(lp, RC.oracle_like(oracle, data, t_limit=RC.T_LIMIT_ALL)(rows))
    assert zero.all() and rows[:, 0].max() < RC.T_LIMIT_ALL
    # the seam chain of the sources test: two slabs of 262144 // 3 entries per source
    assert 300 * 300 > (1 << 18) // 3 and 300 * 300 <= RC.CAP
