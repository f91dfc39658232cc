"""Posterior draws without a GPU: the reference pick of tests/_draws_ref.py against its definition (inside the window,
the smallest and largest populations, even's spacing, uniformity), ``ChainDraws.choice()``'s tuple against the
reference's rules (results.py:803-893) on hand-made results, the argument validation of the Python layer, and the
``draws=`` keyword rules of the sampler and the fitter on a faked device."""
import numpy as np
import pytest

import _draws_ref as DR
from mbb_emcee_amd import draws as _draws_module              # noqa: F401 -- (no draws, no tests: the reference alone proves nothing)


# ---------------------------------------------------------------- the reference pick
def test_reference_philox_known_answers():
    """Random123's known answers for Philox4x32-10; the vectorised form equals the scalar one."""
    assert DR.philox4x32((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert DR.philox4x32((0xffffffff,) * 4, (0xffffffff,) * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert DR.philox4x32((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == (
        0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    seed = 0x123456789abcdef0
    u = DR.philox_u64(5, 2, seed)
    for i in range(5):
        c = DR.philox4x32((i, 2, DR.STREAM, 1), (seed & DR.MASK32, seed >> 32))
        assert u[i] == c[0] | (c[1] << 32)


@pytest.mark.parametrize("how", ["random", "even"])
def test_picks_are_always_inside_the_window(how):
    for nw, nsteps, burn, thin in ((7, 5, 0, 1), (7, 5, 2, 3), (7, 5, 4, 1), (7, 5, 0, 100), (1, 1, 0, 1), (3, 64, 63, 7)):
        steps = list(range(burn, nsteps, thin))
        idx = DR.indices(2, nw, nsteps, burn, thin, 500, how, seed=9)
        assert idx.shape == (2, 500, 2)
        assert idx[..., 0].min() >= 0 and idx[..., 0].max() < nw
        assert set(idx[..., 1].ravel().tolist()) <= set(steps)
        if how == "random" and nw * len(steps) > 1:
            assert not np.array_equal(idx[0], idx[1])                      # (the source is in the counter)


def test_smallest_and_largest_population():
    assert DR.picks(100, 1, "random", seed=3) == [0] * 100 and DR.picks(100, 1, "even") == [0] * 100
    N = 2 ** 32 - 1
    j = DR.picks(4096, N, "random", seed=3)
    assert 0 <= min(j) and max(j) < N and max(j) > N - N // 512 and min(j) < N // 512 and len(set(j)) == 4096
    u = DR.philox_u64(4096, 0, 3)
    assert j == [(x * N) // 2 ** 64 for x in u]
    e = DR.picks(4096, N, "even")
    assert e[0] == 0 and e[-1] == (4095 * N) // 4096 < N and len(set(e)) == 4096


def test_even_spacing_and_no_repeats():
    for N in (1, 2, 12, 35, 1000, 2 ** 31 - 1):
        for n in (1, 2, 7, 12, 35, 64, 1000):
            j = DR.picks(n, N, "even")
            assert j[0] == 0 and all(0 <= x < N for x in j) and j == sorted(j)
            gaps = set(b - a for a, b in zip(j, j[1:]))
            assert gaps <= {N // n, N // n + 1}, (N, n, gaps)                 # spread as evenly as integers allow
            if n <= N:
                assert len(set(j)) == n
            else:
                assert set(j) == set(range(N))                                # every cell, repeated


def test_random_picks_are_uniform():
    """60 000 picks over 12 cells, seed 20: chi-square with 11 degrees of freedom against uniform, at the 1 % level
    (24.72) -- a fixed seed, so a fixed number; and with replacement: far more draws than cells."""
    j = np.array(DR.picks(60000, 12, "random", seed=20))
    counts = np.bincount(j, minlength=12)
    assert counts.size == 12 and counts.sum() == 60000
    chi2 = float(((counts - 5000.0) ** 2 / 5000.0).sum())
    print("chi-square of 60000 picks over 12 cells: %.3f" % chi2)
    assert chi2 < 24.72
    # another source, another seed: other picks
    assert DR.picks(64, 12, "random", seed=20, src=1) != DR.picks(64, 12, "random", seed=20)
    assert DR.picks(64, 12, "random", seed=21) != DR.picks(64, 12, "random", seed=20)


def test_reference_gather_reads_planted_cells():
    chain, lnp = DR.planted_chain(3, 7, 5, scale=[1.0, 1e-3, 250.0])
    idx = DR.indices(3, 7, 5, 2, 3, 40, "random", seed=1)
    rows, l = DR.gather(chain, lnp, idx)
    sc = np.array([1.0, 1e-3, 250.0])
    for s in range(3):
        assert np.array_equal(rows[s, :, 0], sc[s] * (1000.0 * s + idx[s, :, 0] + idx[s, :, 1] / 1024.0))
        assert np.array_equal(l[s], -(s + idx[s, :, 0] / 64.0 + idx[s, :, 1] / 65536.0))
    assert np.all(np.isnan(DR.gather(chain, None, idx)[1]))


# ---------------------------------------------------------------- choice() on hand-made results
def _made(nsrc, n, derived=(), multi=False):
    from mbb_emcee_amd import draws
    req = draws._Request(n, derived=derived, redshift=1.0, lumdist_mpc=1e3, nsources=nsrc)
    raw = draws._Raw(nsrc, n, req.derived)
    raw.rows[:] = np.arange(nsrc * n * 5, dtype=np.float64).reshape(nsrc, n, 5)
    raw.lnprob[:] = -np.arange(nsrc * n, dtype=np.float64).reshape(nsrc, n)
    raw.index[:] = np.arange(nsrc * n * 2).reshape(nsrc, n, 2)
    for k, d in enumerate(raw.derived):
        raw.derived[d][:] = 100.0 * (k + 1) + np.arange(nsrc * n).reshape(nsrc, n)
    return draws.ChainDraws(None, req, raw, multi, 10, 20)


def test_choice_tuple_follows_the_reference():
    all3 = ("peaklambda", "lir", "dustmass")
    d = _made(1, 6, all3)
    assert d.params.shape == (6, 5) and d.lnprob.shape == (6,) and d.index.shape == (6, 2) and d.status.shape == (8,)
    t = d.choice()
    assert isinstance(t, tuple) and len(t) == 1 and t[0].shape == (6, 5)
    t = d.choice(getpeaklambda=True, getlir=True, getdustmass=True)
    assert [x.shape for x in t] == [(6, 5), (6,), (6,), (6,)]
    assert t[1][0] == 100.0 and t[2][0] == 200.0 and t[3][0] == 300.0          # in that order
    t = d.choice(getdustmass=True, getpeaklambda=True)
    assert len(t) == 3 and t[1][0] == 100.0 and t[2][0] == 300.0
    # n == 1: a 5-vector and floats
    one = _made(1, 1, all3)
    t = one.choice(getpeaklambda=True, getlir=True, getdustmass=True)
    assert t[0].shape == (5,) and [type(x) for x in t[1:]] == [float] * 3 and t[1:] == (100.0, 200.0, 300.0)
    # the reference's exceptions for what was not computed
    some = _made(1, 4, ("lir",))
    for kw, msg in ((dict(getpeaklambda=True), "Peak lambda not computed"), (dict(getdustmass=True), "Dustmass not computed")):
        with pytest.raises(Exception, match=msg):
            some.choice(**kw)
    assert len(some.choice(getlir=True)) == 2 and some.lir.shape == (4,)
    with pytest.raises(Exception, match="Peak lambda not computed"):
        some.peaklambda
    with pytest.raises(Exception, match="Dustmass not computed"):
        some.dustmass
    with pytest.raises(Exception, match="LIR not computed"):
        _made(1, 4).lir
    # a source axis in front
    m = _made(3, 6, all3, multi=True)
    assert m.params.shape == (3, 6, 5) and m.lir.shape == (3, 6) and m.status.shape == (3, 8)
    assert [x.shape for x in m.choice(getlir=True)] == [(3, 6, 5), (3, 6)]
    assert [x.shape for x in _made(3, 1, all3, multi=True).choice(getlir=True)] == [(3, 5), (3,)]
    # the results are copies
    d.params[0, 0] = -1.0
    assert d.params[0, 0] == 0.0
    keys = set(m.arrays())
    assert keys == {"draws_params", "draws_lnprob", "draws_index", "draws_status", "draws_peaklambda", "draws_lir",
                    "draws_dustmass"}
    assert set(_made(1, 2).arrays(prefix="x_")) == {"x_params", "x_lnprob", "x_index", "x_status"}
    text = str(m)
    assert text.startswith("Source 0 of 3") and "6 random draws from 20 steps of 10 walkers" in text
    assert text.count("mean:") == 8
    assert "np.random.seed" in type(d).choice.__doc__


# ---------------------------------------------------------------- validation before the device
class _Like(object):
    """Stands where a likelihood would: touching the device is an error."""
    data_read = True

    def _sync_device(self):
        raise AssertionError("the device was touched")

    context = property(_sync_device)


def test_chain_draws_validates_before_the_device():
    import mbb_emcee_amd
    from mbb_emcee_amd import draws, _native
    assert mbb_emcee_amd.chain_draws is draws.chain_draws and mbb_emcee_amd.ChainDraws is draws.ChainDraws
    assert mbb_emcee_amd.draw_indices is draws.draw_indices
    like, chain = _Like(), np.random.RandomState(0).rand(10, 20, 5)
    bad = [(dict(), "chain must be", chain[..., :4]), (dict(), "chain must be", chain[0]),
           (dict(n=0), "n must be", chain), (dict(n=-3), "n must be", chain),
           (dict(n=_native.DRAWS_MAX + 1), "draws per source", chain),
           (dict(how="all"), "how must be", chain), (dict(seed=-1), "seed must be", chain),
           (dict(seed=2 ** 64), "seed must be", chain),
           (dict(burn=20), "burn", chain), (dict(burn=-1), "burn", chain), (dict(thin=0), "thin", chain),
           (dict(lnprob=np.zeros((10, 19))), "lnprob must have", chain),
           (dict(derived=("mass",)), "unknown derived", chain),
           (dict(derived=("lir",)), "need redshift and lumdist_mpc", chain),
           (dict(derived=("dustmass",), redshift=1.0, lumdist_mpc=1e3, kappa=0.0), "kappa", chain),
           (dict(derived=("lir",), redshift=[1.0, 2.0], lumdist_mpc=1e3), "one entry per source", chain),
           (dict(derived=("lir",), redshift=1.0, lumdist_mpc=1e3, lir_range=(0.0, 10.0)), "wavelengths", chain),
           (dict(peak_model="thick"), "model must be", chain)]
    for kw, msg, ch in bad:
        with pytest.raises(ValueError, match=msg):
            draws.chain_draws(like, ch, **kw)
    with pytest.raises(ValueError, match="2\\^31 - 1 draws per call"):
        draws._Request(_native.DRAWS_MAX, nsources=128)
    with pytest.raises(AssertionError, match="the device was touched"):     # (valid arguments do get that far)
        draws.chain_draws(like, chain, lnprob=np.zeros((10, 20)), n=100, how="even", seed=2 ** 64 - 1, burn=4, thin=3)
    for kw, msg in ((dict(n=0), "n must be"), (dict(n=4, how="odd"), "how must be"), (dict(n=4, burn=20), "burn leaves"),
                    (dict(n=4, thin=0), "thin"), (dict(n=4, nsources=0), "empty")):
        with pytest.raises(ValueError, match=msg):
            draws.draw_indices(10, 20, like=like, **kw)
    with pytest.raises(AssertionError, match="the device was touched"):
        draws.draw_indices(10, 20, 4, like=like)
    # what a request resolves to
    r = draws._Request(7, "even", 2 ** 63 + 5, burn=7, thin=3, derived=("dustmass", "peaklambda"), redshift=1.0,
                       lumdist_mpc=1e3)
    assert r.check_steps(1000) == 331
    s = r.spec()
    assert (s.n, s.how, s.seed) == (7, _native.DRAWS_EVEN, 2 ** 63 + 5)
    assert (s.summary.contents.burn, s.summary.contents.thin, s.summary.contents.derived) == (7, 3, 5)
    raw = draws._Raw(2, 7, r.derived)
    o = raw.out()
    assert bool(o.derived[0]) and not bool(o.derived[1]) and bool(o.derived[2])
    assert list(raw.derived) == ["peaklambda", "dustmass"]


def _bare_sampler():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary, s.seed = 10, 5, _Like(), None, None, 5

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_draws_keyword_rules():
    """storechain=False without summary= keeps no chain on the device: draws= says so before anything runs; so do bad
    keywords, and draws() of a sampler that has no chain; the keywords default to the summary's."""
    s = _bare_sampler()
    p0 = np.zeros((10, 5))
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(p0, 16, storechain=False, draws=10)
    with pytest.raises(ValueError, match="n must be"):
        s.run_mcmc(p0, 16, draws=dict(n=0))
    with pytest.raises(ValueError, match="how must be"):
        s.run_mcmc(p0, 16, draws=dict(n=4, how="best"))
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(p0, 16, draws=dict(n=4, burn=16))
    with pytest.raises(ValueError, match="burn leaves no step"):          # burn taken from the summary's keywords
        s.run_mcmc(p0, 16, summary=dict(burn=16), draws=4)
    with pytest.raises(ValueError, match="need redshift"):
        s.run_mcmc(p0, 16, summary=dict(burn=2), draws=dict(n=4, derived=("lir",)))
    with pytest.raises(AssertionError, match="the device was touched"):   # ... and so are derived= and its settings
        s.run_mcmc(p0, 16, summary=dict(derived=("lir",), redshift=1.0, lumdist_mpc=1e3), draws=4)
    with pytest.raises(TypeError):
        s.run_mcmc(p0, 16, draws=dict(n=4, nsamples=2))
    assert s.draws_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.draws(5)
    s._resident = 16
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.draws(5, burn=16)
    with pytest.raises(ValueError, match="n must be"):
        s.draws(0)
    with pytest.raises(AssertionError, match="the device was touched"):
        s.draws(5, burn=15)


def test_draws_attribute_is_reset():
    """reset() and the start of the next run -- run_mcmc or sample() -- put draws_ back to None."""
    s = _bare_sampler()
    s._open = None
    s.draws_ = "held"
    s.reset()
    assert s.draws_ is None
    s.draws_ = "held"
    with pytest.raises(AssertionError, match="the device was touched"):
        s.run_mcmc(np.zeros((10, 5)), 4)
    assert s.draws_ is None
    s.draws_ = "held"
    with pytest.raises(AssertionError, match="the device was touched"):
        next(s.sample(np.zeros((10, 5)), iterations=4))
    assert s.draws_ is None


def test_sharded_run_is_not_drawn_from():
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.lnprobfn, s.seed = _Like(), 5
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded sampler run cannot be drawn from"):
        s.run_mcmc(np.zeros((10, 5)), 4, draws=3)


def test_fitter_and_cli_know_draws():
    from mbb_emcee_amd import mbb_fitter, run_mbb_emcee
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="draws= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), draws=5)
    assert fit.draws is None
    a = run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz"])
    assert a.draws == 0
    a = run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz", "--draws", "48"])
    assert a.draws == 48


def test_draws_entries_are_declared_and_bound():
    import ctypes as C
    import os
    from mbb_emcee_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_draws", "mbb_sampler_draws", "mbb_draw_indices"):
        assert name in hdr and name in _native.SIGNATURES
    assert [f[0] for f in _native.DrawsSpec._fields_] == ["n", "how", "seed", "summary"]
    assert [f[0] for f in _native.DrawsOut._fields_] == ["rows", "lnprob", "index", "derived", "status"]
    assert C.sizeof(_native.DrawsSpec) == 24 and C.sizeof(_native.DrawsOut) == 56
    assert "#define MBB_DRAWS_MAX (1 << 24)" in hdr and _native.DRAWS_MAX == 1 << 24
    assert "MBB_DRAWS_RANDOM = 0, MBB_DRAWS_EVEN = 1" in hdr and (_native.DRAWS_RANDOM, _native.DRAWS_EVEN) == (0, 1)
    src = open(os.path.join(root, "mbb_emcee_amd", "csrc", "mbb_draws.hip.h")).read()
    assert "philox4x32(" in src and "0x44524157u" in src and "mbbc::sample_" in src
    assert "mbb_draws.hip.h" in open(os.path.join(root, "mbb_emcee_amd", "build.py")).read()
