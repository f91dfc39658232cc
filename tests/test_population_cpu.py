"""CPU side of the population tests: the step logic of csrc/mbb_popsteps.hip.h in its HOST build
(tests/_population_host.cpp) against longdouble and scipy; the restatement tests/_population_ref.py on a toy with a
closed form; pack / unpack; ``Population.sample`` on a stand-in whose likelihood is that closed form, against grid
quadrature; the refusals made in Python, the ``population=`` rules of the sampler and the fitter on a faked device, and
the stale-``Population`` error.

Bounds.  The host build's prior factor and log density are a handful of float64 operations on values of order 1 to
1e3: against longdouble they are held to 64 eps max(1, |value|) (each operation rounds once; m_log and the division
are within 2 ulp).  The record merge in any grouping is held to 1e-12 max(1, |value|) against the longdouble
restatement: 300 entries, each merge a few roundings, far below.
The toy: source n has true value m_n ~ N(2, 0.5^2) and S = 256 posterior draws x ~ N(m_n, 0.3^2) under a flat interim
prior, so that mean_j N(x_j | mu, sigma^2) estimates the integral of N(x | m_n, 0.09) N(x | mu, sigma^2), which is
N(m_n | mu, sigma^2 + 0.09).  With w_j = N(x_j | mu, sigma^2), ln mean w has the delta-method standard error
sqrt(var(w) / (S wbar^2)), and the sum over sources the root of the sum of squares.
The stand-in: with N_eff = nwalkers nsteps / tau (tau of the walkers' mean, per dimension) a chain's mean has the
standard error sd / sqrt(N_eff) and its standard deviation sqrt(mu4 - sd^4) / (2 sd sqrt(N_eff)), mu4 the fourth central
moment -- both taken from the quadrature, not from the chain."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import _population_ref as PR

LD = PR.LD
EPS = np.finfo(np.float64).eps
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return np.ascontiguousarray(a, dtype=np.int32).ctypes.data_as(_ip)


# ---------------------------------------------------------------- 1. the step logic in its host build
class Host(object):
    def __init__(self, tmpdir):
        cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
        if not cxx:
            raise RuntimeError("no host C++ compiler")
        so = os.path.join(str(tmpdir), "libpop_host.so")
        subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
                               os.path.join(ROOT, "tests", "_population_host.cpp"), "-o", so])
        L = self.lib = C.CDLL(so)
        L.pop_host_prior_factor.argtypes = [C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double]
        L.pop_host_prior_factor.restype = C.c_double
        L.pop_host_transform.argtypes = [C.c_double, C.c_int, _dp]
        L.pop_host_transform.restype = C.c_double

    def entries(self, rows, cols, transforms, prior):
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        n, d = rows.shape[0], len(cols)
        x, b = np.empty((n, d)), np.empty(n)
        f = lambda k: _d(np.ascontiguousarray(prior[k], dtype=np.float64))
        self.lib.pop_host_entries(_d(rows), n, d, _i(cols), _i(transforms), _i(prior["has_uplim"]), _i(prior["has_gprior"]),
                                  f("lowlim"), f("uplim"), f("gmean"), f("givar"), _d(x), _d(b))
        return x, b

    def prepare(self, mu, L):
        d = len(mu)
        prep = np.zeros(self.lib.pop_host_prep_len(d))
        h = np.ascontiguousarray(PR.chol_rows(mu, L))
        return (prep if self.lib.pop_host_prepare(_d(h), d, _d(prep)) else None)

    def logdens(self, prep, x, b):
        x, b = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        a = np.empty(x.shape[0])
        self.lib.pop_host_logdens(_d(prep), x.shape[1], _d(x), _d(b), x.shape[0], _d(a))
        return a

    def fold(self, prep, x, b):
        x, b = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
        d = x.shape[1]
        w = np.empty(self.lib.pop_host_words(d))
        self.lib.pop_host_fold(_d(prep), d, _d(x), _d(b), x.shape[0], _d(w))
        return w

    def merge(self, d, wa, wb):
        wa = wa.copy()
        self.lib.pop_host_merge(d, _d(wa), _d(np.ascontiguousarray(wb)))
        return wa


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    try:
        return Host(tmp_path_factory.mktemp("pop_host"))
    except RuntimeError as e:
        pytest.skip(str(e))


def _rel(got, want):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(got - want) / np.maximum(LD(1), np.abs(want))))


def test_prior_factor_host_build(H):
    """The prior factor on both sides of the upper limit and at it, with and without the Gaussian prior."""
    c = np.empty(4)
    H.lib.pop_constants(_d(c))
    assert c[0] == PR.WALL_REL_WIDTH and c[1] == PR.UNDERFLOW and c[2] == np.log(10.0) and c[3] == float(np.log(2 * PR.pi_of(LD)))
    up, low = 20.0, 0.1
    thetas = np.array([0.1, 1.5, 19.999, np.nextafter(20.0, 0), 20.0, np.nextafter(20.0, 30), 20.01, 20.4, 23.0])
    for has_up in (0, 1):
        for has_g in (0, 1):
            prior = PR.flat_prior()
            prior["has_uplim"][1], prior["uplim"][1], prior["lowlim"][1] = has_up, up, low
            prior["has_gprior"][1], prior["gmean"][1], prior["givar"][1] = has_g, 1.8, 1.0 / 0.3 ** 2
            got = np.array([H.lib.pop_host_prior_factor(t, has_up, up, low, has_g, 1.8, 1.0 / 0.3 ** 2) for t in thetas])
            want = PR.prior_factor(thetas, 1, prior, LD)
            assert _rel(got, want) <= 64 * EPS, (has_up, has_g)
            if not has_g:
                assert np.all(got[thetas <= up] == 0.0) and (not has_up or np.all(got[thetas > up] < 0.0))
    # the wall at the limit itself adds nothing; one step beyond it, next to nothing
    assert H.lib.pop_host_prior_factor(20.0, 1, 20.0, 0.1, 0, 0.0, 1.0) == 0.0
    assert -1e-25 < H.lib.pop_host_prior_factor(float(np.nextafter(20.0, 30)), 1, 20.0, 0.1, 0, 0.0, 1.0) < 0.0


def test_transform_and_entries_host_build(H):
    """log10 and its Jacobian ln(theta ln 10); whole rows: used and left-out entries, x and b against longdouble."""
    th = np.array([1e-3, 0.1, 1.0, 2.5, 10.0, 37.2, 1e4])
    jac = C.c_double()
    for t in th:
        x = H.lib.pop_host_transform(t, PR.LOG10, C.byref(jac))
        assert abs(LD(x) - np.log(LD(t)) / np.log(LD(10))) <= 8 * EPS * max(1.0, abs(x))
        assert abs(LD(jac.value) - np.log(LD(t) * np.log(LD(10)))) <= 8 * EPS * max(1.0, abs(jac.value))
        assert H.lib.pop_host_transform(t, PR.IDENTITY, C.byref(jac)) == t and jac.value == 0.0
    rng = np.random.RandomState(3)
    rows = np.column_stack([rng.uniform(5, 45, 64), rng.uniform(0.5, 22, 64), rng.uniform(100, 900, 64),
                            rng.uniform(1, 21, 64), rng.uniform(1, 80, 64)])
    rows[3, 0] = np.nan; rows[5, 1] = np.inf; rows[7, 4] = -1.0; rows[9, 4] = 0.0; rows[11, 2] = -np.inf
    prior = PR.flat_prior()
    prior.update(has_uplim=[1, 1, 0, 1, 0], uplim=[40.0, 20.0, np.inf, 20.0, np.inf], lowlim=[1, 0.1, 1, 0.1, 1e-3],
                 has_gprior=[0, 1, 0, 0, 0], gmean=[0, 1.8, 0, 0, 0], givar=[1, 4.0, 1, 1, 1])
    cols, tr = [0, 1, 4], [PR.LOG10, PR.IDENTITY, PR.LOG10]
    x, b = H.entries(rows, cols, tr, prior)
    xr, br = PR.entries(rows, cols, tr, prior, LD)
    out = np.zeros(64, dtype=bool); out[[3, 5, 7, 9]] = True          # (row 11's lambda0 is not a chosen column)
    assert np.array_equal(b == -np.inf, out) and np.array_equal(np.asarray(br == -np.inf), out)
    assert np.all(x[out] == 0.0)
    assert _rel(x[~out], xr[~out]) <= 8 * EPS and _rel(b[~out], br[~out]) <= 64 * EPS
    assert (rows[:, 0] > 40).any() and (rows[:, 1] > 20).any() and (rows[:, 0] < 40).any()


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5])
def test_forward_substitution_and_logdens_host_build(H, d):
    """a_j against scipy: L^-1 (x - mu) by solve_triangular, the density by multivariate_normal.logpdf."""
    from scipy.linalg import solve_triangular
    from scipy.stats import multivariate_normal
    rng = np.random.RandomState(10 + d)
    A = rng.standard_normal((d, d))
    cov = A @ A.T + d * np.eye(d)
    L = np.linalg.cholesky(cov)
    mu = rng.uniform(-2, 2, d)
    x = mu + rng.standard_normal((200, d)) @ L.T * 1.5
    b = rng.uniform(-3, 3, 200)
    prep = H.prepare(mu, L)
    assert prep is not None
    a = H.logdens(prep, x, b)
    z = solve_triangular(L, (x - mu).T, lower=True).T
    want = -0.5 * np.sum(z * z, axis=1) - np.sum(np.log(np.diag(L))) - 0.5 * d * np.log(2 * np.pi) + b
    assert _rel(a, want) <= 64 * EPS * d
    assert _rel(a - b, multivariate_normal(mu, cov).logpdf(x)) <= 1e-12
    assert _rel(a, PR.logdens(x.astype(LD), b.astype(LD), mu, L, LD)) <= 64 * EPS * d
    # bad candidates
    for bad in (np.nan, 0.0, -1.0, np.inf):
        Lb = L.copy(); Lb[d - 1, d - 1] = bad
        assert H.prepare(mu, Lb) is None and PR.bad_candidate(mu, Lb)
    mb = mu.copy(); mb[0] = np.nan
    assert H.prepare(mb, L) is None


@pytest.mark.parametrize("d", [1, 2, 5])
def test_record_merge_in_any_grouping(H, d):
    """The record of 300 entries, -inf ones among them, folded whole, in chunks of every kind merged left to right, as
    a tree, and with empty records on either side: always the longdouble restatement's numbers; an empty record merges
    as the identity, bit for bit."""
    rng = np.random.RandomState(20 + d)
    L = np.linalg.cholesky(np.cov(rng.standard_normal((d, 50))) + 0.1 * np.eye(d))
    mu = rng.uniform(-1, 1, d)
    x = mu + 3.0 * rng.standard_normal((300, d))
    b = rng.uniform(-40, 40, 300)
    b[[0, 17, 150, 299]] = -np.inf
    prep = H.prepare(mu, L)
    ref = PR.source(x.astype(LD), b.astype(LD), mu, L, LD)
    nd = d + d * (d + 1) // 2

    def numbers(w):
        m, s, s2 = w[:3]
        cov = np.zeros((d, d))
        cov[np.tril_indices(d)] = w[3 + d:3 + nd] / s
        cov = cov + np.tril(cov, -1).T
        return dict(lnl_src=m + np.log(s) - np.log(296.0), ess=s * s / s2, mean=w[3:3 + d], cov=cov)

    def held(w, what):
        got = numbers(w)
        for k in PR.FLOATS:
            assert _rel(got[k], ref[k]) <= 1e-12, (what, k)
    whole = H.fold(prep, x, b)
    held(whole, "whole")
    empty = H.fold(prep, x[:0], b[:0])
    assert empty[0] == -np.inf and not empty[1:].any()
    assert np.array_equal(H.merge(d, whole, empty), whole) and np.array_equal(H.merge(d, empty, whole), whole)
    assert np.array_equal(H.merge(d, empty, empty), empty)
    only_out = H.fold(prep, x[:1], b[:1])                        # (a chunk of left-out entries alone is an empty record)
    assert np.array_equal(only_out, empty)
    for cuts in ([150], [1, 2, 3], [64, 128, 192, 256], list(range(7, 300, 7)), [299]):
        parts = [H.fold(prep, xs, bs) for xs, bs in zip(np.split(x, cuts), np.split(b, cuts))]
        left = parts[0]
        for p in parts[1:]:
            left = H.merge(d, left, p)
        held(left, ("left to right", cuts[:3]))
        right = parts[-1]
        for p in parts[-2::-1]:
            right = H.merge(d, p, right)
        held(right, ("right to left", cuts[:3]))
        while len(parts) > 1:                                    # a tree
            parts = [H.merge(d, parts[i], parts[i + 1]) if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        held(parts[0], ("tree", cuts[:3]))
    # a record far below another: its weight vanishes, nothing overflows
    far = H.fold(prep, x[:10], b[:10] - 5000.0)
    assert np.array_equal(H.merge(d, whole, far)[:2], whole[:2])


# ---------------------------------------------------------------- 2. the closed-form toy
def _toy():
    rng = np.random.RandomState(20261021)
    m = rng.normal(2, 0.5, 64)
    x = m[:, None] + 0.3 * rng.standard_normal((64, 256))
    return m, x


def _toy_check(sigmas, dt):
    m, x = _toy()
    xb = [(x[n][:, None].astype(dt), np.zeros(256, dtype=dt)) for n in range(64)]
    cands = [(np.array([mu]), np.array([[sg]])) for mu in (1.6, 1.8, 2.0, 2.2, 2.4) for sg in sigmas]
    res = PR.evaluate(xb, cands, dt, moments=False)
    rows = []
    for h, (mu, L) in enumerate(cands):
        mu, sg = float(mu[0]), float(L[0, 0])
        exact = np.sum(-0.5 * (m - mu) ** 2 / (sg ** 2 + 0.09) - 0.5 * np.log(2 * np.pi * (sg ** 2 + 0.09)))
        w = np.exp(-0.5 * ((x - mu) / sg) ** 2) / (sg * np.sqrt(2 * np.pi))
        se = np.sqrt(np.sum(w.var(axis=1, ddof=1) / (256 * w.mean(axis=1) ** 2)))
        rows.append((mu, sg, float(res["lnl"][h]), exact, se, float(np.min(res["ess"][h]))))
    return rows


@pytest.mark.parametrize("dt", [np.float64, LD])
def test_toy_with_a_closed_form(dt):
    rows = _toy_check((0.5, 0.8, 1.2), dt)
    worst = 0.0
    for mu, sg, lnl, exact, se, ess in rows:
        assert ess >= 20, (mu, sg, ess)                          # first: the importance sums are well covered
        worst = max(worst, abs(lnl - exact) / se)
        assert abs(lnl - exact) <= 5 * se, (mu, sg, lnl, exact, se)
    print("    worst miss %.2f standard errors, smallest ess %.1f" % (worst, min(r[5] for r in rows)))
    # a population narrower than the per-source posteriors: one entry carries each sum, which is what ess_low warns of
    for mu, sg, lnl, exact, se, ess in _toy_check((0.2,), dt):
        assert ess < 2, (mu, sg, ess)


# ---------------------------------------------------------------- 3. pack / unpack
@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_pack_unpack(d):
    from mbb_emcee_amd import population as P
    rng = np.random.RandomState(d)
    for _ in range(20):
        u = np.concatenate([rng.uniform(-50, 50, d), rng.uniform(-2, 2, d), rng.uniform(-3, 3, d * (d - 1) // 2)])
        mu, cov = P.unpack(u, d)
        assert mu.shape == (d,) and cov.shape == (d, d) and np.array_equal(cov, cov.T)
        assert np.all(np.linalg.eigvalsh(cov) > 0)               # positive definite whatever u
        back = P.pack(mu, cov)
        assert np.allclose(back, u, rtol=1e-7, atol=1e-7)      # (Sigma's condition number stays below ~1e6 in this range)
        mu2, cov2 = P.unpack(back, d)
        assert np.allclose(mu2, mu) and np.allclose(cov2, cov, rtol=1e-9)
    A = rng.standard_normal((d, d)); cov = A @ A.T + np.eye(d); mu = rng.standard_normal(d)
    m2, c2 = P.unpack(P.pack(mu, cov), d)
    assert np.allclose(m2, mu, rtol=0, atol=0) and np.allclose(c2, cov, rtol=1e-12)
    mus, covs = P.unpack(np.stack([P.pack(mu, cov)] * 3), d)
    assert mus.shape == (3, d) and covs.shape == (3, d, d)
    with pytest.raises(ValueError):
        P.unpack(np.zeros(d + 1 + d * (d + 1) // 2), d)


# ---------------------------------------------------------------- 4. sample() on a stand-in
def _stand_in(m):
    from mbb_emcee_amd import population as P

    class StandIn(P.Population):
        def __init__(self):
            self.d, self.columns, self.nsources, self.calls, self.rows = 1, ["x"], m.size, 0, []

        def lnlike(self, mu, cov=None, chol=None):
            mu = np.atleast_2d(mu)[:, 0]
            var = (np.reshape(chol, (-1,)) ** 2 if cov is None else np.reshape(cov, (-1,))) + 0.09
            return np.sum(-0.5 * (m[None, :] - mu[:, None]) ** 2 / var[:, None] - 0.5 * np.log(2 * np.pi * var[:, None]), axis=1)

        def _sample_eval(self, mu, L):
            self.calls += 1
            self.rows.append(mu.shape[0])
            return self.lnlike(mu, chol=L), np.zeros(mu.shape[0], dtype=int)
    return StandIn()


def test_sample_on_a_stand_in_against_quadrature():
    m, _ = _toy()
    pop = _stand_in(m)
    box = np.array([[0.0, 4.0], [np.log(0.05), np.log(5.0)]])
    nw, nsteps = 16, 3000
    fit = pop.sample(nsteps=nsteps, nwalkers=nw, nburn=300, bounds=box, seed=7)
    assert fit.chain.shape == (nw, nsteps, 2) and fit.lnprob.shape == (nw, nsteps) and fit.ess_low == 0.0
    assert pop.calls == 1 + 2 * (300 + nsteps) and set(pop.rows) == {nw, nw // 2}      # one call per half-step
    tau = fit.integrated_time
    assert np.all(np.isfinite(tau)) and nsteps / tau.max() >= 50, tau
    assert 0.2 < fit.acceptance_fraction.mean() < 0.9
    # the same posterior by quadrature: flat in u = (mu, ln sigma) inside the box
    g0, g1 = np.linspace(box[0, 0], box[0, 1], 801), np.linspace(box[1, 0], box[1, 1], 801)
    G0, G1 = np.meshgrid(g0, g1, indexing="ij")
    lp = pop.lnlike(G0.reshape(-1, 1), chol=np.exp(G1).reshape(-1, 1, 1)).reshape(G0.shape)
    w = np.exp(lp - lp.max()); w /= w.sum()
    flat = fit.chain.reshape(-1, 2)
    for i, G in enumerate((G0, G1)):
        mean = np.sum(w * G); c = G - mean
        var = np.sum(w * c ** 2); sd = np.sqrt(var); mu4 = np.sum(w * c ** 4)
        neff = nw * nsteps / tau[i]
        se_mean, se_sd = sd / np.sqrt(neff), np.sqrt(mu4 - var ** 2) / (2 * sd * np.sqrt(neff))
        print("    u[%d]: mean %.4f (quadrature %.4f, se %.4f), sd %.4f (%.4f, se %.4f), tau %.1f"
              % (i, flat[:, i].mean(), mean, se_mean, flat[:, i].std(), sd, se_sd, tau[i]))
        assert abs(flat[:, i].mean() - mean) <= 5 * se_mean and abs(flat[:, i].std() - sd) <= 5 * se_sd
    # the result's summaries are of that chain
    mu_cen, sg_cen = fit.mu_cen(), fit.sigma_cen()
    assert mu_cen.shape == (1, 3) and mu_cen[0, 0] == pytest.approx(flat[:, 0].mean()) and np.all(mu_cen[0, 1:] > 0)
    assert sg_cen[0, 0] == pytest.approx(np.exp(flat[:, 1]).mean()) and fit.corr_cen().shape == (1, 1, 3)
    bmu, bcov, blp = fit.best
    assert blp == fit.lnprob.max() and blp == pytest.approx(float(pop.lnlike(bmu[None], cov=bcov[None])[0]))
    # reproducible by seed; a caller's prior replaces the box
    again = _stand_in(m).sample(nsteps=50, nwalkers=8, nburn=10, bounds=box, seed=3)
    same = _stand_in(m).sample(nsteps=50, nwalkers=8, nburn=10, bounds=box, seed=3)
    assert np.array_equal(again.chain, same.chain) and np.array_equal(again.lnprob, same.lnprob)
    tight = _stand_in(m).sample(nsteps=50, nwalkers=8, nburn=10, start=np.array([2.0, np.log(0.5)]), seed=3,
                                lnprior=lambda u: 0.0 if 1.9 < u[0] < 2.1 and -1.0 < u[1] < 0.0 else -np.inf)
    assert np.all(np.abs(tight.chain[:, :, 0] - 2.0) < 0.1)
    with pytest.raises(ValueError, match="bounds"):
        _stand_in(m).sample(bounds=np.zeros((3, 2)))


# ---------------------------------------------------------------- 5. refusals and run rules
def _like(**kw):
    from test_run_keywords_cpu import _Like
    lk = _Like()
    lk._gprior_ivar = np.ones(6)
    for k, v in kw.items():
        setattr(lk, k, v)
    return lk


def test_python_refusals():
    from mbb_emcee_amd import population as P
    R = P._Request
    req = R(_like(), ("T", "beta"), {"T": "log10"}, 3, 2)
    assert req.cols == [0, 1] and req.transform == [1, 0] and (req.burn, req.thin) == (3, 2) and req.d == 2
    s = req.spec()
    assert s.d == 2 and list(s.col)[:2] == [0, 1] and list(s.has_uplim) == [0, 1, 0, 1, 0] and s.uplim[1] == 20.0
    assert s.uplim[0] == np.inf and s.lowlim[4] == 1e-3 and req.glow[0] == 0.0 and req.glow[1] == 0.1
    assert R(_like(), "fnorm", "log10").transform == [1] and R(_like(), (4, 0), ("log10", None)).cols == [4, 0]
    with pytest.raises(ValueError, match="held fixed by the fit"):
        R(_like(), ("T", "beta"), fixed=[False, True, False, False, False])
    with pytest.raises(ValueError, match="held by the model variant \\(noalpha\\)"):
        R(_like(noalpha=True), ("T", "alpha"))
    with pytest.raises(ValueError, match="held by the model variant \\(optically thin\\)"):
        R(_like(opthin=True), ("lambda0",))
    with pytest.raises(ValueError, match="log10 of T needs a lower limit above 0"):
        R(_like(_lowlim=np.array([0.0, 0.1, 1, 0.1, 1e-3])), ("T",), "log10")
    assert R(_like(_lowlim=np.array([0.0, 0.1, 1, 0.1, 1e-3])), ("T",)).d == 1       # (the identity does not mind)
    for has in ("_has_uplim", "_has_gprior"):
        with pytest.raises(ValueError, match="peak wavelength.*not separable"):
            R(_like(**{has: [False, True, False, True, False, True]}))
    with pytest.raises(ValueError, match="given twice"):
        R(_like(), ("T", "T"))
    with pytest.raises(ValueError, match="unknown population column"):
        R(_like(), ("T", "gamma"))
    with pytest.raises(ValueError, match="unknown population column"):
        R(_like(), (0, 5))
    with pytest.raises(ValueError, match="derived column"):
        R(_like(), ("T", "lir"))
    with pytest.raises(ValueError, match="1 to 5 columns"):
        R(_like(), ())
    with pytest.raises(ValueError, match="unknown transform"):
        R(_like(), ("T",), "ln")
    with pytest.raises(ValueError, match="not chosen"):
        R(_like(), ("T",), {"beta": "log10"})
    with pytest.raises(ValueError, match="one entry per column"):
        R(_like(), ("T", "beta"), ("log10",))
    with pytest.raises(ValueError, match="burn must be"):
        R(_like(), burn=-1)
    with pytest.raises(ValueError, match="burn leaves no step"):
        R(_like(), burn=16).check_steps(16)
    with pytest.raises(TypeError, match="likelihood"):
        R(object())
    with pytest.raises(ValueError, match="chain must be"):
        P.chain_population(_like(), np.zeros((4, 4)))
    with pytest.raises(ValueError, match="empty"):
        P.chain_population(_like(), np.zeros((0, 4, 5)))


def test_run_rules_on_a_faked_device():
    """population= follows the rules of run_mcmc's other analysis keywords (tests/test_run_keywords_cpu.py)."""
    from test_run_keywords_cpu import _bare_sampler, P0, TOUCHED
    import mbb_emcee_amd as mbb

    def sampler(nranks=None):
        s = _bare_sampler(nranks)
        s.lnprobfn._gprior_ivar = np.ones(6)
        return s
    s = sampler()
    for value in (True, dict(columns=("T",))):
        with pytest.raises(ValueError) as e:
            s.run_mcmc(P0, 16, storechain=False, population=value)
        assert str(e.value) == ("population= with storechain=False needs summary= too: a run that neither stores nor "
                                "summarises its chain keeps none on the device")
    with pytest.raises(AssertionError, match=TOUCHED):           # nothing to refuse: the device is next
        s.run_mcmc(P0, 16, storechain=False, summary=True, population=True)
    with pytest.raises(ValueError) as e:
        sampler(2).run_mcmc(P0, 16, population=True)
    assert str(e.value) == ("a sharded sampler run cannot be pooled into a population on the device: a rank holds only its "
                            "own walkers' chain")
    with pytest.raises(TypeError) as e:
        s.run_mcmc(P0, 16, population=dict(bogus=1))
    assert str(e.value) == "population= got unexpected keyword(s) ['bogus']"
    # the summary's burn / thin are inherited: a burn that leaves no step is the population's refusal too
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(P0, 16, summary=dict(burn=16), population=True)
    with pytest.raises(AssertionError, match=TOUCHED):
        s.run_mcmc(P0, 16, summary=dict(burn=16), population=dict(burn=2))
    thin = sampler()
    thin.lnprobfn.opthin = True
    with pytest.raises(ValueError, match="held by the model variant"):
        thin.run_mcmc(P0, 16, population=dict(columns=("lambda0",)))
    # population_ is cleared with the others
    s = sampler()
    s.population_ = object()
    with pytest.raises(AssertionError, match=TOUCHED):
        s.run_mcmc(P0, 16)
    assert s.population_ is None
    s.population_ = object()
    s._open = None; s._chain = None
    mbb.DeviceEnsembleSampler.reset(s)
    assert s.population_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.population()
    # the fitter: population= needs the device sampler, and passes its fixed parameters on
    fit = mbb.mbb_fitter.__new__(mbb.mbb_fitter)
    fit.sampler = object()
    with pytest.raises(ValueError, match='population= needs sampler="device"'):
        fit.run(5, 5, P0, population=True)
    with pytest.raises(ValueError, match='needs sampler="device"'):
        fit.population()
    fit.sampler, fit._fixed = s, [False, True, False, False, False]
    s._resident = 16
    with pytest.raises(ValueError, match="beta is held fixed by the fit"):
        fit.population(columns=("T", "beta"))
    assert fit.population_ is None


def test_stale_population_raises():
    """A Population whose block a later build of the same context replaced raises RuntimeError, never a number."""
    from mbb_emcee_amd import population as P

    class Lib(object):
        def __init__(self):
            self.current = 0

        def mbb_population_eval(self, h, serial, rows, H, moments, out):
            return 0 if serial == self.current else -3

        def mbb_last_error(self):
            return b"no population block of this serial in the context"

    class Ctx(object):
        h = 1
        lib = Lib()
    ctx = Ctx()

    def build():
        ctx.lib.current += 1
        raw = P._BuildRaw(2)
        raw.serial[0] = ctx.lib.current
        return P.Population(ctx, P._Request(_like(), ("T",)), raw, True, 4, 8)
    first = build()
    assert np.isnan(first.lnlike([20.0], cov=[[4.0]]))            # (the faked library fills nothing in)
    second = build()
    with pytest.raises(RuntimeError, match="a later build replaced it"):
        first.lnlike([20.0], cov=[[4.0]])
    with pytest.raises(RuntimeError, match="a later build replaced it"):
        first.evaluate([20.0], cov=[[4.0]])
    with pytest.raises(RuntimeError, match="a later build replaced it"):
        first.source_means()
    assert np.isnan(second.lnlike([20.0], cov=[[4.0]]))
    second._closed = True
    with pytest.raises(RuntimeError, match="closed"):
        second.lnlike([20.0], cov=[[4.0]])
    # shapes follow the inputs
    third = build()
    ev = third.evaluate([[20.0], [21.0]], cov=[[4.0]], moments=True)
    assert ev.lnl.shape == (2,) and ev.lnl_source.shape == (2, 2) and ev.mean.shape == (2, 2, 1) and ev.covariance.shape == (2, 2, 1, 1)
    assert ev.mass_below.shape == (2, 1) and ev.mass_below[0, 0] == pytest.approx(1.0342e-21, rel=1e-3)       # Phi(-9.5)
    one = third.evaluate([20.0], chol=[[2.0]])
    assert np.ndim(one.lnl) == 0 and one.lnl_source.shape == (2,) and one.mean is None and one.mass_below.shape == (1,)
    with pytest.raises(ValueError, match="one of the two"):
        third.evaluate([20.0])
    with pytest.raises(ValueError, match="1 values per candidate"):
        third.evaluate([20.0, 1.0], cov=np.eye(2))
