"""The device sampler held to emcee's calling contract (the docstrings of DeviceEnsembleSampler.run_mcmc, sample and
reset), on the 8-band cfg2 likelihood with 16 walkers.

The oracle is the trajectory (tests/_sampler_model.py): a step's Philox key is its number in the sampler's life, so one
``run_mcmc(p0, 240)`` of a fresh sampler with the same seed gives every position and log-probability that any
interleaving of calls may show, and the same trajectory made one step per call gives every acceptance count.  Every
comparison with it is bit-for-bit equality.  The only toleranced check is lnl_close where a walker starts
at -inf; the diagnostics comparison is the bitwise one of tests/test_diagnostics_gpu.py for the same two paths.
tests/test_sampler_contract_cpu.py holds what the program seeds cover, and the model itself, without a GPU."""
import gc

import numpy as np
import pytest

from conftest import lnl_close
import _sampler_model as M

pytestmark = pytest.mark.gpu

NW, T = 16, 240


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


@pytest.fixture(scope="module")
def like(mbb, g_lnl):
    like = mbb.likelihood(response=True)
    like.set_phot([str(b) for b in g_lnl["cfg2/bands"]], g_lnl["cfg2/thick_walpha/flux"], g_lnl["cfg2/thick_walpha/unc"])
    return like


@pytest.fixture(scope="module")
def p0():
    rng = np.random.RandomState(8)
    return np.array([12.0, 1.8, 600.0, 3.0, 40.0]) * (1.0 + 0.02 * rng.normal(size=(NW, 5)))


@pytest.fixture(scope="module")
def multi(mbb, g_lnl):
    """Three sources on the same bands: fluxes by model_flux of three truths, and the starting ensembles."""
    bands = [str(b) for b in g_lnl["cfg2/bands"]]
    rng = np.random.RandomState(9)
    ns = 3
    truths = np.column_stack([rng.uniform(8, 20, ns), rng.uniform(1.2, 2.4, ns), rng.uniform(300, 900, ns),
                              rng.uniform(2, 4.5, ns), rng.uniform(10, 80, ns)])
    single = mbb.likelihood(response=True)
    single.set_phot(bands, np.ones(8), np.ones(8))
    flux = single.model_flux(truths)
    like3 = mbb.likelihood(response=True)
    like3.set_phot_multi(bands, flux, 0.1 * flux + 1.0)
    return like3, truths[:, None, :] * (1.0 + 0.02 * rng.normal(size=(ns, NW, 5)))


def _trajectory(mbb, like, p0, seed, nsteps=T):
    """(p0, lnp0, ref_chain, ref_lnp, acc_true) of the sampler with this seed: one run, and the counts one step per call."""
    ref = mbb.DeviceEnsembleSampler(NW, 5, like, seed=seed)
    ref.run_mcmc(p0, nsteps)
    one = mbb.DeviceEnsembleSampler(NW, 5, like, seed=seed)
    _, lnp0, _ = one.run_mcmc(p0, 0)
    acc = np.empty(ref.lnprobability.shape)
    pos = None
    for t in range(nsteps):
        pos, lnp, _ = one.run_mcmc(None, 1, storechain=False)
        acc[..., t] = one.naccepted
    # (the two references are one trajectory, and a walker moves if and only if its count does)
    assert np.array_equal(pos, ref.chain[..., -1, :]) and np.array_equal(lnp, ref.lnprobability[..., -1])
    assert np.array_equal(acc[..., -1], ref.naccepted) and np.all(np.diff(acc, axis=-1) >= 0)
    from mbb_emcee_amd.device_sampler import accepted_by_step
    assert np.array_equal(accepted_by_step(p0, ref.chain), acc)
    return p0, lnp0.copy(), ref.chain, ref.lnprobability, acc


# ------------------------------------------------------------------------------------------------- 1, 2: programs
@pytest.mark.parametrize("seed", range(24))
def test_programs_single_source(mbb, like, p0, seed):
    """1. Program `seed` of run_mcmc, sample (whole, left by break, kept and overtaken) and reset calls, 200 to 240 steps
    of the sampler's life: after every call and at every step handed out, chain, lnprobability, flatchain.shape,
    iterations, naccepted, acceptance_fraction and the returned state are the reference trajectory's, bit for bit."""
    traj = _trajectory(mbb, like, p0, seed)
    s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=seed)
    assert M.run_program(s, M.Model(*traj), M.program(seed), "seed %d" % seed) > 50


@pytest.mark.parametrize("seed", range(12))
def test_programs_three_sources(mbb, multi, seed):
    """2. The same on three sources: every array carries the leading (3, 16)."""
    like3, p03 = multi
    traj = _trajectory(mbb, like3, p03, seed)
    assert traj[2].shape == (3, NW, T, 5) and traj[4].shape == (3, NW, T)
    s = mbb.DeviceEnsembleSampler(NW, 5, like3, seed=seed)
    assert M.run_program(s, M.Model(*traj), M.program(seed), "seed %d" % seed) > 50
    assert s.naccepted.shape == (3, NW)


# ------------------------------------------------------------------------------------- 3: the review's case, literally
def test_run_mcmc_overtakes_a_suspended_generator(mbb, like, p0):
    """3. ``g = s.sample(p0, iterations=100, chunk=10); next(g); s.run_mcmc(None, 5)``: the device made ten steps for the
    generator, the run goes on from there and the sampler shows all fifteen; collecting g changes nothing; a second such
    generator raises RuntimeError when resumed."""
    _, _, ref, ref_lnp, acc = _trajectory(mbb, like, p0, 21, 40)
    s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=21)
    g = s.sample(p0, iterations=100, chunk=10)
    next(g)
    assert s.iterations == 1 and s.chain.shape == (NW, 1, 5)
    pos, lnp, _ = s.run_mcmc(None, 5)

    def fifteen():
        assert s.iterations == 15 and s.chain.shape == (NW, 15, 5)
        assert np.array_equal(s.chain, ref[:, :15]) and np.array_equal(s.lnprobability, ref_lnp[:, :15])
        assert np.array_equal(s.naccepted, acc[:, 14])
        assert np.array_equal(s.acceptance_fraction, acc[:, 14] / 15)
    fifteen()
    assert np.array_equal(pos, ref[:, 14]) and np.array_equal(lnp, ref_lnp[:, 14])
    del g
    gc.collect()
    fifteen()
    g = s.sample(None, iterations=100, chunk=10)
    pos, lnp, _ = next(g)
    assert np.array_equal(pos, ref[:, 15]) and s.iterations == 16
    s.run_mcmc(None, 5)
    with pytest.raises(RuntimeError):
        next(g)
    assert s.iterations == 30 and np.array_equal(s.chain, ref[:, :30]) and np.array_equal(s.naccepted, acc[:, 29])


# ------------------------------------------------------------------------------------------------------ 4: lnprob0
def test_lnprob0_as_the_sampler_reports_it_changes_nothing(mbb, like, p0):
    """4a, 4f. lnprob0 equal to the log-probabilities the sampler itself reports for p0 (a 0-step run): the chain is
    bitwise that of the run without it, by run_mcmc and by sample(), where it applies to the first chunk only."""
    a = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    a.run_mcmc(p0, 60)
    z = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    pos, l0, _ = z.run_mcmc(p0, 0)
    assert np.array_equal(pos, p0) and l0.shape == (NW,) and np.all(np.isfinite(l0))
    lnl_close(l0, like(p0))
    b = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    b.run_mcmc(p0, 60, lnprob0=l0)
    assert np.array_equal(b.chain, a.chain) and np.array_equal(b.lnprobability, a.lnprobability)
    assert np.array_equal(b.naccepted, a.naccepted)
    c = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    n = 0
    for pos, lnp, _ in c.sample(p0, lnprob0=l0, iterations=60, chunk=7):
        assert np.array_equal(pos, a.chain[:, n]) and np.array_equal(lnp, a.lnprobability[:, n])
        n += 1
    assert n == 60 and np.array_equal(c.chain, a.chain) and np.array_equal(c.lnprobability, a.lnprobability)
    assert np.array_equal(c.naccepted, a.naccepted)


def test_lnprob0_is_taken_as_given(mbb, like, p0):
    """4b. lnprob0[w] = 1e300 for one walker: it never moves in 60 steps and its lnprobability is 1e300 throughout;
    every other walker moves."""
    z = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    _, l0, _ = z.run_mcmc(p0, 0)
    l0 = l0.copy()
    w = 5
    l0[w] = 1e300
    s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    pos, lnp, _ = s.run_mcmc(p0, 60, lnprob0=l0)
    assert np.all(s.chain[w] == p0[w]) and np.all(s.lnprobability[w] == 1e300) and s.naccepted[w] == 0
    assert np.array_equal(pos[w], p0[w]) and lnp[w] == 1e300
    assert np.all(np.delete(s.naccepted, w) > 0)
    assert np.all(np.isfinite(np.delete(s.lnprobability, w, axis=0)))


@pytest.mark.parametrize("given", [False, True])
def test_a_walker_that_starts_at_minus_infinity(mbb, like, p0, given):
    """4c. One walker starts below the lower limit of T (T = 0.5), with lnprob0 None and with the -inf given: the run
    succeeds, the walker's lnprobability is -inf exactly until its first move, which comes within 60 steps (a proposal
    lands above the limit with probability about 0.38 per step), and from then on it is the likelihood of the chain.
    Four seeds, so that the walker's first move is not the first step in all of them."""
    w = 11
    start = p0.copy()
    start[w, 0] = 0.5
    l0 = None
    if given:
        good = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3).run_mcmc(p0, 0)[1]
        l0 = good.copy()
        l0[w] = -np.inf
    firsts = []
    for seed in (17, 18, 19, 20):
        s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=seed)
        pos, lnp, _ = s.run_mcmc(start, 60, lnprob0=l0)
        moved = np.flatnonzero(np.any(s.chain[w] != start[w], axis=-1))
        assert moved.size > 0, "the walker has not moved in 60 steps (seed %d)" % seed
        first = moved[0]
        firsts.append(int(first))
        assert np.all(np.isneginf(s.lnprobability[w, :first])) and np.all(s.chain[w, :first] == start[w])
        assert np.all(np.isfinite(s.lnprobability[w, first:])) and np.all(s.chain[w, first:, 0] >= 1.0)
        assert s.naccepted[w] >= 1 and np.all(np.isfinite(lnp))
        for t in sorted(set((0, int(first), 59))):
            lnl_close(like(np.ascontiguousarray(s.chain[:, t, :])), s.lnprobability[:, t])
        lnl_close(like(np.ascontiguousarray(s.chain[w, first:])), s.lnprobability[w, first:])
    print("    first move of the walker at steps %r" % firsts)
    assert max(firsts) > 0, "the -inf stretch of the chain was empty at every seed: nothing of it was checked"


def test_lnprob0_refusals(mbb, like, p0, multi):
    """4d, 4e. NaN in lnprob0 and every wrong shape -- (nw - 1,), (nw, 1), (nw + 1,), and (nw,) for three sources -- are a
    ValueError raised in Python, before the native side reads nsources * nw doubles from the array; the sampler then
    still runs from a valid state."""
    ref = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    _, good, _ = ref.run_mcmc(p0, 0)
    ref.run_mcmc(None, 10)
    s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    nan = good.copy()
    nan[2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        s.run_mcmc(p0, 10, lnprob0=nan)
    for bad in (good[:NW - 1], good[:, None], np.r_[good, good[0]]):
        with pytest.raises(ValueError, match="lnprob0 must have shape"):
            s.run_mcmc(p0, 10, lnprob0=bad)
        with pytest.raises(ValueError, match="lnprob0 must have shape"):
            next(s.sample(p0, lnprob0=bad, iterations=10))
    assert s.iterations == 0 and s.chain.shape == (NW, 0, 5)
    with pytest.raises(ValueError):
        s.run_mcmc(None, 1)                              # (nothing of the refused calls became a state)
    s.run_mcmc(p0, 10, lnprob0=good)
    assert np.array_equal(s.chain, ref.chain)
    like3, p03 = multi
    s3 = mbb.DeviceEnsembleSampler(NW, 5, like3, seed=3)
    with pytest.raises(ValueError, match="lnprob0 must have shape"):
        s3.run_mcmc(p03, 10, lnprob0=good)
    with pytest.raises(ValueError, match="lnprob0 must have shape"):
        s3.run_mcmc(p03, 10, lnprob0=np.zeros(3 * NW))
    _, good3, _ = s3.run_mcmc(p03, 0)
    assert good3.shape == (3, NW)
    s3.run_mcmc(p03, 10, lnprob0=good3)
    r3 = mbb.DeviceEnsembleSampler(NW, 5, like3, seed=3)
    r3.run_mcmc(p03, 10)
    assert np.array_equal(s3.chain, r3.chain)


# ----------------------------------------------------------------------------------------------------------- 5: C7
def test_convergence_after_sample_is_of_the_whole_run_or_refused(mbb, like, p0):
    """5. After sample(iterations=40, chunk=64) the run was one chunk and is resident: convergence() equals
    chain_diagnostics of s.chain field by field, bit for bit as tests/test_diagnostics_gpu.py compares the same two paths.
    After sample(iterations=40, chunk=16) it raises: the resident chunk would be 8 of the 40 steps.  summary and
    convergence_ are None either way."""
    s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=77)
    for _ in s.sample(p0, iterations=40, chunk=64):
        pass
    assert s.summary is None and s.convergence_ is None and s.chain.shape == (NW, 40, 5)
    for kw in (dict(), dict(burn=5, nacf=8, method="walkers")):
        got, host = s.convergence(**kw), mbb.chain_diagnostics(like, s.chain, **kw)
        assert got.nsteps_used == 40 - kw.get("burn", 0) == host.nsteps_used and got.nwalkers == NW
        for f in ("tau", "ess", "rhat", "window", "status", "converged"):
            assert np.array_equal(getattr(got, f), getattr(host, f), equal_nan=True), f
        assert (got.acf is None) == (host.acf is None)
        assert got.acf is None or np.array_equal(got.acf, host.acf, equal_nan=True)
    b = mbb.DeviceEnsembleSampler(NW, 5, like, seed=77)
    for _ in b.sample(p0, iterations=40, chunk=16):
        pass
    assert b.summary is None and b.convergence_ is None and np.array_equal(b.chain, s.chain)
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        b.convergence()


# ----------------------------------------------------------------------------------------------------------- 6: C6
def test_sample_refuses_at_the_first_next(mbb, like, p0):
    """6. What run_mcmc refuses -- the shape of p0, NaN or inf in it, p0 None without a state -- sample() refuses at the
    first next(); the sampler then runs as if nothing had been asked."""
    s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    nan, inf = p0.copy(), p0.copy()
    nan[3, 0], inf[3, 1] = np.nan, np.inf
    for bad, msg in ((p0[:NW - 1], "shape"), (p0[None], "shape"), (nan, "NaN"), (inf, "infinite"), (None, "pos0=None")):
        g = s.sample(bad, iterations=5, chunk=2)
        with pytest.raises(ValueError, match=msg):
            next(g)
        with pytest.raises(ValueError, match=msg):
            s.run_mcmc(bad, 5)
    assert s.iterations == 0 and s.chain.shape == (NW, 0, 5) and not s.naccepted.any()
    ref = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
    ref.run_mcmc(p0, 5)
    for _ in s.sample(p0, iterations=5, chunk=2):
        pass
    assert np.array_equal(s.chain, ref.chain) and np.array_equal(s.naccepted, ref.naccepted)
