"""The device sampler's calling contract, the parts that need no GPU: the reconstruction of per-step acceptance counts,
what the committed program seeds of tests/test_sampler_contract_gpu.py cover, the model and the runner of
tests/_sampler_model.py against a numpy stand-in, DeviceEnsembleSampler's own Python (run_mcmc, sample, reset) on a
faked device, and lnprob0 on the host EnsembleSampler."""
import gc

import numpy as np
import pytest

import _sampler_model as M
from _targets import G5

SEEDS, SEEDS_MULTI, T = range(24), range(12), 240


# ----------------------------------------------------------------------------------------------- accepted_by_step
def _abs():
    from mbb_emcee_amd.device_sampler import accepted_by_step
    return accepted_by_step


def test_accepted_by_step_known_arrays():
    f = _abs()
    cur = np.array([[1.0, 2, 3, 4, 5], [6.0, 7, 8, 9, 10]])
    steps = np.empty((2, 4, 5))
    ulp = np.array([0, 0, 0, 0, np.spacing(5.0)])
    steps[0] = [cur[0], cur[0] + ulp, cur[0] + ulp, cur[0]]                                      # stays, moves, stays, moves
    steps[1] = [cur[1] * 2, cur[1] * 2, cur[1] * 2, cur[1] * 2]                                  # moves, then never again
    got = f(cur, steps)
    assert got.shape == (2, 4) and np.array_equal(got, [[0, 1, 1, 2], [1, 1, 1, 1]])
    # one changed column is a move; the counts are cumulative and never decrease
    one = steps.copy()
    one[0, 3] = one[0, 2]
    one[0, 3, 0] = -1.0
    assert np.array_equal(f(cur, one), [[0, 1, 1, 2], [1, 1, 1, 1]])
    # a run of no steps, and of one
    assert f(cur, steps[:, :0]).shape == (2, 0)
    assert np.array_equal(f(cur, steps[:, :1]), [[0], [1]])


@pytest.mark.parametrize("lead", [(16,), (3, 16)])
def test_accepted_by_step_is_the_truth_and_masks_other_ranks_rows(lead):
    """Against the moves of a made-up trajectory, one source and three; on a chain with zeros in the rows of the other
    ranks' walkers -- as a rank of a run sharded with the one-hop exchange holds it -- those rows never count, with the
    mask given as booleans or as indices."""
    f = _abs()
    p0, _, chain, _, acc = M.toy_trajectory(lead, 50, 3)
    got = f(p0, chain)
    assert np.array_equal(got, acc) and np.all(np.diff(got, axis=-1) >= 0) and got[..., -1].max() > 10
    # continued from the middle
    assert np.array_equal(f(chain[..., 19, :], chain[..., 20:, :]), acc[..., 20:] - acc[..., 19:20])
    from mbb_emcee_amd.device_sampler import _own_rows
    for rank, nranks in ((0, 2), (1, 2), (3, 4)):
        own = _own_rows(16, rank, nranks)
        per = 8 // nranks
        assert np.array_equal(np.flatnonzero(own), np.r_[rank * per:(rank + 1) * per, 8 + rank * per:8 + (rank + 1) * per])
        sharded = np.where(own[:, None, None], chain, 0.0)
        want = np.where(own[:, None], acc, 0.0)
        for mask in (own, np.flatnonzero(own)):
            got = f(p0, sharded, mask)
            assert np.array_equal(got, want) and np.all(np.diff(got, axis=-1) >= 0)
        # without the mask the zero rows count as moved at the first step: what the mask is for
        assert np.all(f(p0, sharded)[..., ~own, :] == 1)


# ------------------------------------------------------------------------------------------- the committed programs
def test_program_seeds_cover_what_the_gpu_tests_claim(capsys):
    """The programs of seeds 0..23 (the single-source GPU test; the three-source one runs 0..11) cannot pass vacuously.
    Observed over 0..23: B 82, K-resumed 48, K-closed 37, Z 88, storechain=False 129, chunk 1 / 3 / 7 / k / k+5
    88 / 74 / 67 / 52 / 57, sample onto a stored chain 293, state given with lnprob0 106, R 112, S 171, life steps 200..222;
    over 0..11: B 43, K-resumed 27, K-closed 19, Z 40, storechain=False 77, the chunk kinds 41 / 35 / 43 / 26 / 29."""
    for seeds in (SEEDS, SEEDS_MULTI):
        progs = [M.program(s) for s in seeds]
        c = M.coverage(progs)
        with capsys.disabled():
            print("\n    program seeds 0..%d: %s" % (len(progs) - 1, ", ".join("%s %d" % kv for kv in sorted(c.items()))))
        for what in ("B", "K-resumed", "K-closed", "Z", "storechain=False"):
            assert c.get(what, 0) >= 10, (what, c)
        for ck in M.CHUNK_KINDS:
            assert c.get("chunk " + ck, 0) >= 10, (ck, c)
        assert c.get("onto a stored chain", 0) >= 5 and c.get("state and lnprob0 given", 0) >= 5
        assert 200 <= c["life min"] and c["life max"] <= T
    for ops in (M.program(s) for s in SEEDS):
        assert ops[0].kind != "Z"
        for op in M.flat_ops(ops):
            assert 0 <= op.k <= M.KMAX and (op.kind not in "BK" or 1 <= op.j <= op.k)
            assert op.kind in "RZ" or op.chunk in (1, 3, 7, op.k, op.k + 5)
            assert (op.nxt is not None) == (op.kind == "K") and (op.nxt is None or op.nxt.kind in "RSBZ")
    assert M.program(5) == M.program(5) and M.program(5) != M.program(6)


# ------------------------------------------------------------------------------- the model against the stand-in
@pytest.mark.parametrize("lead", [(16,), (3, 16)])
def test_model_and_runner_against_the_stand_in(lead):
    """The written contract as a numpy sampler satisfies the model on every program: a bug in model, runner or generator
    is met here first."""
    checks = 0
    for seed in SEEDS:
        traj = M.toy_trajectory(lead, T, 100 + seed)
        checks += M.run_program(M.StandIn(traj), M.Model(*traj), M.program(seed), "seed %d" % seed)
    assert checks > 2000


def test_model_notices_a_sampler_that_does_not_retire_its_generator():
    """The sampler before the contract's fourth clause -- a suspended generator is not retired by the next call, and
    its end overwrites what that call did -- fails every program that keeps a generator."""
    seen = 0
    for seed in SEEDS:
        ops = M.program(seed)
        # (a kept generator whose next call makes no step and which is then closed shows nothing either way)
        if not any(op.kind == "K" and (op.fate == "resume" or op.nxt.used > 0) for op in ops):
            continue
        seen += 1
        traj = M.toy_trajectory((16,), T, 100 + seed)
        with pytest.raises(AssertionError, match="the contract says|differs from the reference|must raise RuntimeError"):
            M.run_program(M.StandIn(traj, retire=False), M.Model(*traj), ops, "seed %d" % seed)
    assert seen >= 20


def test_model_notices_a_wrong_cell():
    traj = M.toy_trajectory((16,), T, 1)
    m = M.Model(*traj)
    s = M.StandIn(traj)
    s.run_mcmc(traj[0], 7)
    m.run(7, True)
    m.check(s)
    for name in ("_chain", "_lnprob", "naccepted"):
        a = getattr(s, name).copy()
        keep, flat = a.copy(), a.reshape(-1)
        flat[-1] = np.nextafter(flat[-1], np.inf)
        setattr(s, name, a)
        with pytest.raises(AssertionError, match="differs from the reference"):
            m.check(s)
        setattr(s, name, keep)
    s.iterations += 1
    with pytest.raises(AssertionError, match="iterations"):
        m.check(s)


# ------------------------------------------------------------ DeviceEnsembleSampler's own Python on a faked device
def _device_sampler(traj, seed=1, **kw):
    from mbb_emcee_amd.device_sampler import DeviceEnsembleSampler
    dev = M.FakeDevice(traj, **kw)
    return DeviceEnsembleSampler(traj[0].shape[-2], 5, dev, seed=seed), dev


@pytest.mark.parametrize("lead", [(16,), (3, 16)])
def test_device_sampler_python_layer_satisfies_the_model(lead):
    for seed in SEEDS:
        traj = M.toy_trajectory(lead, T, 200 + seed)
        s, _ = _device_sampler(traj)
        M.run_program(s, M.Model(*traj), M.program(seed), "seed %d" % seed)


def test_kept_generator_is_retired_by_run_mcmc():
    """The case of the review, on the faked device: a generator suspended inside its chunk, then run_mcmc(None, 5)."""
    traj = M.toy_trajectory((16,), 40, 9)
    p0, _, chain, lnp, acc = traj
    s, _ = _device_sampler(traj)
    g = s.sample(p0, iterations=30, chunk=10)
    next(g)
    assert s.iterations == 1 and s.chain.shape == (16, 1, 5)
    s.run_mcmc(None, 5)

    def whole():
        assert s.iterations == 15 and np.array_equal(s.chain, chain[:, :15]) and np.array_equal(s.lnprobability, lnp[:, :15])
        assert np.array_equal(s.naccepted, acc[:, 14])
    whole()
    del g
    gc.collect()
    whole()
    g = s.sample(None, iterations=30, chunk=10)
    next(g)
    s.reset()
    with pytest.raises(RuntimeError, match="retired"):
        next(g)
    assert s.iterations == 0 and s.chain.shape == (16, 0, 5) and not s.naccepted.any()
    with pytest.raises(StopIteration):
        next(g)


def test_lnprob0_shape_and_nan_are_refused_before_any_native_call():
    """lnprob0 must have the ensemble's leading shape: the native side reads nsources * nw doubles from whatever it is
    handed.  Refused in Python, with no mbb_sampler_set_state made; the sampler then still runs from a valid state."""
    for lead, bad_shapes in (((16,), [(15,), (16, 1), (17,), (), (1, 16)]), ((3, 16), [(16,), (48,), (3, 15), (3, 16, 1)])):
        traj = M.toy_trajectory(lead, 20, 4)
        p0, lnp0 = traj[0], traj[1]
        s, dev = _device_sampler(traj)
        for shape in bad_shapes:
            for call in (lambda l: s.run_mcmc(p0, 3, lnprob0=l), lambda l: next(s.sample(p0, lnprob0=l, iterations=3))):
                with pytest.raises(ValueError, match="lnprob0 must have shape"):
                    call(np.zeros(shape))
        nan = lnp0.copy()
        nan[..., 3] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            s.run_mcmc(p0, 3, lnprob0=nan)
        assert "set_state" not in dev.calls and "run" not in dev.calls
        assert s.iterations == 0 and s.chain.shape == lead + (0, 5)
        s.run_mcmc(p0, 3, lnprob0=lnp0)
        assert dev.calls.count("set_state") == 1 and np.array_equal(s.chain, traj[2][..., :3, :])


def test_sample_refuses_at_the_first_next_what_run_mcmc_refuses():
    traj = M.toy_trajectory((16,), 20, 4)
    p0 = traj[0]
    s, dev = _device_sampler(traj)
    for bad, msg in ((p0[:15], "shape"), (p0[None], "shape"), (np.where(np.arange(16)[:, None] == 2, np.nan, p0), "NaN"),
                     (np.where(np.arange(16)[:, None] == 2, np.inf, p0), "infinite"), (None, "pos0=None")):
        for n in (5, 0):
            g = s.sample(bad, iterations=n)              # (making the generator refuses nothing)
            with pytest.raises(ValueError, match=msg):
                next(g)
            with pytest.raises(ValueError, match=msg):
                s.run_mcmc(bad, n)
    assert "run" not in dev.calls and s.iterations == 0 and s.chain.shape == (16, 0, 5)
    assert len(list(s.sample(p0, iterations=0))) == 0    # no steps, and the state is set as run_mcmc(p0, 0) sets it
    s.run_mcmc(None, 2)
    assert np.array_equal(s.chain, traj[2][:, :2])


def test_what_is_resident_after_sample():
    """After a sample(), convergence() may describe the whole of it or nothing: the sampler counts a chain resident
    only where the run was one chunk."""
    traj = M.toy_trajectory((16,), 200, 4)
    for n, chunk, want in ((40, 64, 40), (40, 40, 40), (40, 16, 0), (100, 64, 0), (65, 64, 0)):
        s, _ = _device_sampler(traj)
        for _ in s.sample(traj[0], iterations=n, chunk=chunk):
            assert s._resident in (0, want)
        assert s._resident == want and s.summary is None and s.convergence_ is None, (n, chunk)
        if not want:
            with pytest.raises(ValueError, match="no chain of this sampler is resident"):
                s.convergence()
    # left inside the first of several chunks, and retired there
    s, _ = _device_sampler(traj)
    for _ in s.sample(traj[0], iterations=40, chunk=16):
        break
    assert s._resident == 0 and s.iterations == 16
    g = s.sample(None, iterations=40, chunk=16)
    next(g)
    s.run_mcmc(None, 0, storechain=False)
    assert s._resident == 0 and s.iterations == 32


@pytest.mark.parametrize("rank,nranks", [(0, 2), (1, 2), (2, 3)])
def test_per_step_naccepted_on_a_sharded_rank_counts_its_own_rows(rank, nranks):
    """sample() on a rank of a run sharded with the one-hop exchange (faked: the chain and the counts hold the rank's own
    rows, zeros elsewhere): at every step naccepted is the truth in the rank's rows and 0 in the others."""
    nw = 24
    traj = M.toy_trajectory((nw,), 30, 6)
    p0, _, chain, _, acc = traj
    s, dev = _device_sampler(traj, rank=rank, nranks=nranks)
    own = dev.own
    assert own.sum() == nw // nranks
    s.run_mcmc(p0, 4)
    n = 4
    for pos, lnp, _ in s.sample(None, iterations=7, chunk=3):
        n += 1
        assert np.array_equal(s.naccepted[own], acc[own, n - 1]) and not s.naccepted[~own].any(), n
        assert np.array_equal(pos[own], chain[own, n - 1]) and s.iterations == n
    assert n == 11 and acc[~own, 10].min() > 0


# ------------------------------------------------------------------------------------- the host EnsembleSampler
def _host(seed=5):
    from mbb_emcee_amd.ensemble import EnsembleSampler
    tgt = G5()
    rng = np.random.RandomState(2)
    return EnsembleSampler(16, 5, tgt.lnp, vectorize=True, seed=seed), tgt, tgt.draw(rng, (16,))


def test_host_sampler_lnprob0():
    s, tgt, p0 = _host()
    s.run_mcmc(p0, 30)
    a, _, _ = _host()
    a.run_mcmc(p0, 30, lnprob0=tgt.lnp(p0))
    assert np.array_equal(a.chain, s.chain) and np.array_equal(a.lnprobability, s.lnprobability)
    # taken as given: a walker at 1e300 never moves
    b, _, _ = _host()
    l0 = tgt.lnp(p0)
    l0[4] = 1e300
    b.run_mcmc(p0, 60, lnprob0=l0)
    assert np.all(b.chain[4] == p0[4]) and np.all(b.lnprobability[4] == 1e300) and b.naccepted[4] == 0
    assert np.all(np.delete(b.naccepted, 4) > 0)
    # ... and one at -inf leaves at its first finite proposal
    c, _, _ = _host()
    l0 = tgt.lnp(p0)
    l0[4] = -np.inf
    c.run_mcmc(p0, 60, lnprob0=l0)
    first = np.flatnonzero(np.any(c.chain[4] != p0[4], axis=-1))[0]
    assert np.all(np.isneginf(c.lnprobability[4, :first])) and np.allclose(c.lnprobability[4, first:], tgt.lnp(c.chain[4, first:]), rtol=1e-13, atol=0)     # (a sum of five squares, evaluated twice)


def test_host_sampler_lnprob0_refusals():
    s, tgt, p0 = _host()
    good = tgt.lnp(p0)
    for bad in (good[:15], good[:, None], np.r_[good, 0.0], np.float64(1.0), np.tile(good, (3, 1))):
        with pytest.raises(ValueError, match="lnprob0 must have shape"):
            s.run_mcmc(p0, 2, lnprob0=bad)
        with pytest.raises(ValueError, match="lnprob0 must have shape"):
            next(s.sample(p0, lnprob0=bad, iterations=2))
    nan = good.copy()
    nan[7] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        s.run_mcmc(p0, 2, lnprob0=nan)
    assert s.iterations == 0 and s.chain.shape == (16, 0, 5)
    s.run_mcmc(p0, 2, lnprob0=good)
    assert s.chain.shape == (16, 2, 5)
