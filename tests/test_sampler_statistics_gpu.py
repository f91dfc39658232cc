"""The device sampler (and the host sampler through the fit driver) held to distributions that are known exactly.

The targets (tests/_targets.py: G5, five independent Gaussians; W5, G5 with a hard wall through beta and a soft wall
through alpha) are made on the product with its own knobs: Gaussian priors on all five parameters, limits for the
walls, photometry with uncertainties of 1e12 mJy so that the data term is constant.  Every test first ASSERTS that the
likelihood is the target (differences of log density to 1e-9 absolute), then runs the moment battery
(_targets.Battery): ensembles started from exact independent draws are stationary under a correct sampler, so each
of the 25 / 18 / 12 / 7 statistics (five / four / three / two free columns: three per column, one per pair) has
expectation 0 at every step, and over R independent ensembles t = mean / (std / sqrt(R)).

Bound: every |t| <= 5, fixed seeds, no statistic left out -- a condition (a correct sampler crosses it with
probability ~1e-3 over the whole file, at the chosen seeds never again), checked on the numpy reference in
tests/test_sampler_statistics_cpu.py, which also shows that a 2 % error of the variance fails it (max |t| 14).
Beside the moments: the mean acceptance fraction against the numpy reference's for the same target, walkers, scale and
free columns within 5 combined standard errors; no walker of W5 below the hard wall; fixed columns bit for bit;
lnprob of the final state is like(pos).

Then the draw itself through the test-only probe: Philox4x32-10 against Random123's known answers and a numpy replica,
and stretch_draw's ranges, laws and independence.

Rank deficiency that is not axis-aligned (walkers on a tilted plane) is out of scope: the exponent counts columns."""
import numpy as np
import pytest

import _stretch_ref as ref
from _targets import G5, W5, WAVE, FLUX, UNC, PARAMS, Battery
from conftest import lnl_close, parity_record

pytestmark = pytest.mark.gpu

BOUND = Battery.BOUND
NSTAT = {5: 25, 4: 18, 3: 12, 2: 7}
FIXED_SETS = {"alpha": (3,), "lambda0_alpha": (2, 3), "lambda0_alpha_fnorm": (2, 3, 4)}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _target(name):
    return G5() if name == "G5" else W5()


def _make_like(mbb, target, R=None, opthin=False, noalpha=False):
    like = mbb.likelihood(response=False, opthin=opthin, noalpha=noalpha)
    if R:
        like.set_phot_multi(WAVE, np.tile(FLUX, (R, 1)), np.tile(UNC, (R, 1)))
    else:
        like.set_phot(WAVE, FLUX, UNC)
    target.apply(like)
    return like


def _assert_target(like, target, fixed=()):
    """like(p) - like(p_ref) is the target's log-density difference to 1e-9 absolute on >= 1000 draws, on rows mirrored
    below the hard wall (-inf on both sides) and on rows well above the soft wall; with every source of a multi-source
    likelihood."""
    R = getattr(like, "nsources", 1)
    m = max(8, -(-1400 // R))
    p = target.draw(np.random.RandomState(3), (R, m))
    p[:, 1::8, 1] = 2.0 * target.mu0[1] - p[:, 1::8, 1]
    p[:, 2::8, 3] = target.mu0[3] + np.abs(p[:, 2::8, 3] - target.mu0[3])
    for k in fixed:
        p[..., k] = target.mu0[k]
    got = np.asarray(like(p if R > 1 else p[0])).reshape(R, m)
    want = target.lnp(p)
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert fin[0, 0] and np.all(np.isfinite(got[fin]))
    err = np.abs((got[fin] - got[0, 0]) - (want[fin] - want[0, 0])).max()
    parity_record("target vs likelihood (abs)", err, 1e-9)
    assert err <= 1e-9, (target.name, err)
    if target.hard is not None and target.hard not in fixed:
        assert np.isneginf(want).sum() >= 50


def _check_t(what, bat, nfree):
    t = bat.t()
    worst = int(np.argmax(np.abs(t)))
    var = {n: round(float(v), 4) for n, v in bat.excess().items() if n.startswith("var ")}
    print("%s: %d statistics, max |t| %.2f (%s); variance / exact - 1: %s" % (what, len(t), np.abs(t).max(), bat.names[worst], var))
    parity_record("sampler moment t", np.abs(t).max(), BOUND)
    assert len(t) == NSTAT[nfree]
    assert np.abs(t).max() <= BOUND, (what, dict(zip(bat.names, np.round(t, 2))), var)


def _check_acceptance(what, acc, target, nw, a, free, seed=99):
    """acc [R]: each ensemble's acceptance fraction; against the numpy reference from exact draws, 256 ensembles x 200 steps"""
    _, _, racc, _ = ref.run_battery(target, 256, nw, 10, 20, seed, a=a, free=free)
    se = np.hypot(acc.std(ddof=1) / np.sqrt(len(acc)), racc.std(ddof=1) / np.sqrt(len(racc)))
    print("%s: acceptance %.4f, reference %.4f, combined standard error %.4f" % (what, acc.mean(), racc.mean(), se))
    parity_record("acceptance fraction vs reference / standard error", abs(acc.mean() - racc.mean()) / se, 5.0)
    assert abs(acc.mean() - racc.mean()) <= 5.0 * se, (what, acc.mean(), racc.mean(), se)


def _check_state(target, fixed, pos):
    for k in fixed:
        assert np.all(pos[..., k] == target.mu0[k]), "fixed column %d moved" % k          # bit for bit
    if target.hard is not None and target.hard not in fixed:
        assert pos[..., target.hard].min() >= target.mu0[target.hard], "a walker below the hard wall"


def _multi_battery(mbb, target, R, nw, nchunk, every, seed, a=2.0, fixed=(), opthin=False, noalpha=False, p0=None,
                   burn_chunks=0, what=""):
    """R sources with the same (uninformative) photometry = R independent ensembles of nw walkers in one launch."""
    free = [k for k in range(5) if k not in fixed]
    like = _make_like(mbb, target, R, opthin, noalpha)
    _assert_target(like, target, fixed)
    p = target.draw(np.random.RandomState(seed), (R, nw)) if p0 is None else np.array(p0, dtype=np.float64)
    for k in fixed:
        p[..., k] = target.mu0[k]
    s = mbb.DeviceEnsembleSampler(nw, 5, like, a=a, seed=seed)
    bat = Battery(target, free)
    nacc0 = np.zeros((R, nw))
    for ch in range(nchunk):
        pos, lnp, _ = s.run_mcmc(p if ch == 0 else None, every, storechain=False)
        assert pos.shape == (R, nw, 5)
        _check_state(target, fixed, pos)
        if ch >= burn_chunks:
            bat.add(pos)
        elif ch == burn_chunks - 1:
            nacc0 = np.array(s.naccepted, dtype=np.float64)
    lnl_close(lnp, like(pos))
    assert s.iterations == nchunk * every
    what = "%s multi-source %s, %d x %d walkers, a = %g, fixed %s" % (what, target.name, R, nw, a, fixed)
    _check_t(what, bat, len(free))
    acc = ((s.naccepted - nacc0) / ((nchunk - burn_chunks) * every)).mean(axis=1)
    _check_acceptance(what, acc, target, nw, a, free)
    return bat


# ---- all five columns free -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,nw", [(256, 64), (1024, 10), (256, 26)])
@pytest.mark.parametrize("tname", ["G5", "W5"])
def test_multi_source_moments(mbb, tname, R, nw):
    """Multi-source runs, 100 chunks of 20 steps: 256 x 64 walkers (the volume; rows of different sources must be
    independent streams), 1024 x 10 (the smallest ensemble there is) and 256 x 26 (halves of 13: the partner index and
    the halves at small and odd sizes).  25 statistics each."""
    _multi_battery(mbb, _target(tname), R, nw, 100, 20, seed=1000 + R + nw)


def test_multi_source_other_stretch_scale(mbb):
    """a = 1.3 on G5: the z law and the exponent for a scale other than 2.  25 statistics."""
    _multi_battery(mbb, G5(), 256, 64, 100, 20, seed=13, a=1.3)


BURN = 1000


def test_multi_source_converges_from_a_tight_ball(mbb):
    """Convergence, not only stationarity: G5 from a ball of 2 % scatter about the mean (a quarter to four tenths of
    the target's widths), 256 x 64 walkers, BURN steps of burn-in, then 50 chunks of 20 steps; 25 statistics.
    BURN is twice the smallest multiple of 500 steps at which the numpy reference from the same kind of ball passes at
    |t| <= 3 for two seeds.  The reference's max |t| after B steps of burn-in, seeds 1 and 2:
    B = 500: 1.95, 2.38; 1000: 1.54, 2.30; 1500: 1.95, 2.76; 2000: 1.68, 1.92 -- so 500, and BURN = 1000.
    The acceptance fraction is that of the steps after the burn-in."""
    rng = np.random.RandomState(101)
    p0 = G5().mu0 * (1.0 + 0.02 * rng.normal(size=(256, 64, 5)))
    _multi_battery(mbb, G5(), 256, 64, BURN // 20 + 50, 20, seed=14, p0=p0, burn_chunks=BURN // 20, what="from a tight ball:")


def test_single_source_default_form_moments(mbb):
    """The product's default one-launch form: one likelihood, 64 samplers of 250 walkers with seeds 1..64 (independence
    across seeds), G5 and W5, 50 chunks of 20 steps each; 25 statistics.  The plan for 250 walkers -- 125 movers, two
    workgroups each, on 256 CUs, one walker per workgroup -- is form 7 (k_flowm)."""
    R, nw, nchunk, every = 64, 250, 50, 20
    for target in (G5(), W5()):
        like = _make_like(mbb, target)
        _assert_target(like, target)
        rng = np.random.RandomState(15)
        samplers = [mbb.DeviceEnsembleSampler(nw, 5, like, seed=r + 1) for r in range(R)]
        state = target.draw(rng, (R, nw))
        bat = Battery(target)
        for ch in range(nchunk):
            for r, s in enumerate(samplers):
                pos, lnp, _ = s.run_mcmc(state[r] if ch == 0 else None, every, storechain=False)
                assert like.context.info("last_kernel_form") == 7
                state[r] = pos
            _check_state(target, (), state)
            bat.add(state)
        lnl_close(lnp, like(pos))
        what = "single source %s, 64 samplers x 250 walkers" % target.name
        _check_t(what, bat, 5)
        acc = np.array([s.acceptance_fraction.mean() for s in samplers])
        _check_acceptance(what, acc, target, nw, 2.0, list(range(5)))


# ---- fixed columns ---------------------------------------------------------------------------------------------------
def _model_of(fixed):
    """(opthin, noalpha): lambda0 and alpha fixed is the thin model without alpha, as the README's example and the
    command line's --noalpha fix what the model does not use; otherwise the thick model with alpha"""
    return (True, True) if tuple(fixed) == (2, 3) else (False, False)


@pytest.mark.parametrize("fname", list(FIXED_SETS))
@pytest.mark.parametrize("tname", ["G5", "W5"])
def test_multi_source_moments_with_fixed_columns(mbb, tname, fname):
    """DeviceEnsembleSampler, multi-source, with columns held fixed by zero initial scatter: 256 x 64 walkers, 50 chunks of
    20 steps; 18 / 12 / 7 statistics over the free columns; the fixed columns stay bit for bit.  With the exponent
    dim - 1 = 4 whatever the ensemble spans the variances are 22 % / 56 % / 110 % high (measured on the device before the
    fix: see DESIGN.md) and every "var" statistic fails by tens of standard errors."""
    fixed = FIXED_SETS[fname]
    opthin, noalpha = _model_of(fixed)
    _multi_battery(mbb, _target(tname), 256, 64, 50, 20, seed=21 + len(fixed), fixed=fixed, opthin=opthin, noalpha=noalpha)


@pytest.mark.parametrize("kind", ["device", "native"])
@pytest.mark.parametrize("fname", list(FIXED_SETS))
@pytest.mark.parametrize("tname", ["G5", "W5"])
def test_fitter_moments_with_fixed_parameters(mbb, tname, fname, kind):
    """The way a user fixes a parameter: mbb_fitter.fix_param + generate_initial_values (a Gaussian ball of the target's
    own widths, redrawn inside the limits: exact draws of the free columns), sampler="device" and sampler="native".
    64 ensembles of 64 walkers one after another on one fitter (the device sampler's key counts the steps of its life,
    the host sampler's generator goes on: independent streams), 20 chunks of 20 steps each; 18 / 12 / 7 statistics."""
    R, nw, nchunk, every = 64, 64, 20, 20
    target, fixed = _target(tname), FIXED_SETS[fname]
    free = [k for k in range(5) if k not in fixed]
    opthin, noalpha = _model_of(fixed)
    fit = mbb.mbb_fitter(nwalkers=nw, opthin=opthin, noalpha=noalpha, seed=31 + len(fixed), sampler=kind)
    fit.set_data(WAVE, FLUX, UNC)
    target.apply(fit.like)
    _assert_target(fit.like, target, fixed)
    for k in fixed:
        fit.fix_param(PARAMS[k])
    states = np.empty((nchunk, R, nw, 5))
    acc = np.empty(R)
    for r in range(R):
        p0 = fit.generate_initial_values(target.mu0, target.sd)
        assert all(np.all(p0[:, k] == target.mu0[k]) for k in fixed)
        fit.sampler.reset()
        for ch in range(nchunk):
            pos, lnp, _ = fit.sampler.run_mcmc(p0 if ch == 0 else None, every, storechain=False)[:3]
            states[ch, r] = pos
        acc[r] = np.mean(fit.sampler.acceptance_fraction)
    lnl_close(lnp, fit.like(pos))
    bat = Battery(target, free)
    for ch in range(nchunk):
        _check_state(target, fixed, states[ch])
        bat.add(states[ch])
    what = "mbb_fitter(sampler=%r) %s, fixed %s" % (kind, target.name, fixed)
    _check_t(what, bat, len(free))
    _check_acceptance(what, acc, target, nw, 2.0, free)


def test_sources_must_agree_on_the_fixed_columns(mbb):
    """One exponent per run: a multi-source p0 whose sources differ in how many columns are constant is refused."""
    g = G5()
    like = _make_like(mbb, g, 4)
    p0 = g.draw(np.random.RandomState(5), (4, 16))
    p0[2, :, 3] = 3.0
    s = mbb.DeviceEnsembleSampler(16, 5, like, seed=1)
    with pytest.raises(ValueError):
        s.run_mcmc(p0, 2)
    p0[:, :, 3] = 3.0
    pos, _, _ = s.run_mcmc(p0, 2)
    assert np.all(pos[..., 3] == 3.0)


def parent_chain(mbb, g_lnl, lookahead):
    """The run whose results tests/golden/sampler_chain_parent.npz keeps: cfg2's likelihood (eight passbands, thick model with
    alpha), 250 walkers, seed 77, 60 stored steps and 20 unstored ones."""
    like = mbb.likelihood(response=True)
    like.set_phot([str(b) for b in g_lnl["cfg2/bands"]], g_lnl["cfg2/thick_walpha/flux"], g_lnl["cfg2/thick_walpha/unc"])
    like.context.set_option("lookahead_sampler", lookahead)
    p0 = np.array([12.0, 1.8, 600.0, 3.0, 40.0]) * (1.0 + 0.02 * np.random.RandomState(4).normal(size=(250, 5)))
    s = mbb.DeviceEnsembleSampler(250, 5, like, seed=77)
    s.run_mcmc(p0, 60)
    pos, lnp, _ = s.run_mcmc(None, 20, storechain=False)
    form = like.context.info("last_kernel_form")
    like.context.set_option("lookahead_sampler", 1)
    return {"pos": pos, "lnprob": lnp, "chain_every_10": s.chain[:, 9::10, :].copy(),
            "lnprob_every_10": s.lnprobability[:, 9::10].copy(), "naccepted": np.array(s.naccepted, dtype=np.float64)}, form


def test_chain_with_five_free_columns_is_the_parents(mbb, g_lnl):
    """With five free columns the exponent is 4.0 as before and the chain of a given seed is bit for bit what the
    commit before the exponent became a launch argument computed (tests/golden/sampler_chain_parent.npz, made by
    tests/golden/make_golden_sampler_chain.py with that commit's build): one-launch form and launch train."""
    import os
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_chain_parent.npz"))
    for look, form_want in ((1, 7), (0, 1)):
        got, form = parent_chain(mbb, g_lnl, look)
        assert form == form_want
        for k in got:
            assert np.array_equal(got[k], want[k]), (look, k)


# ---- the draw itself -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    import _device_probe
    return _device_probe.load()


def _philox_np(ctr, key):
    """numpy Philox4x32-10 (Salmon et al. 2011), vectorised: ctr[n, 4], key[n, 2] uint32"""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = key[:, 0].astype(np.uint64), key[:, 1].astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M, p1 >> np.uint64(32), p1 & M
        c = [(hi1 ^ c[1] ^ k0) & M, lo1, (hi0 ^ c[3] ^ k1) & M, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, axis=1).astype(np.uint32)


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_device_philox_known_answers(probe):
    """philox4x32 on the device against Random123's published known-answer vectors and, bit for bit, against the numpy
    replica on 1e5 random counters and keys."""
    ctr = np.array([k[0] for k in KAT], dtype=np.uint32)
    key = np.array([k[1] for k in KAT], dtype=np.uint32)
    want = np.array([k[2] for k in KAT], dtype=np.uint32)
    assert np.array_equal(_philox_np(ctr, key), want)
    assert np.array_equal(probe.philox(ctr, key), want)
    rng = np.random.RandomState(7)
    ctr = rng.randint(0, 1 << 32, size=(100000, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.randint(0, 1 << 32, size=(100000, 2), dtype=np.uint64).astype(np.uint32)
    ctr[:16, 0] = np.arange(16); ctr[:16, 1:] = 0                    # (counters as the sampler forms them)
    assert np.array_equal(probe.philox(ctr, key), _philox_np(ctr, key))


GOLD = 0x9E3779B97F4A7C15


def _step_keys(seed, steps):
    """the key of step t (0-based) of a sampler's life: seed + GOLD (t + 1) mod 2^64"""
    return np.array([(seed + GOLD * (int(t) + 1)) & 0xFFFFFFFFFFFFFFFF for t in steps], dtype=np.uint64)


def _draw_inputs():
    """(row, half, key) [n], n = 2^22 + ...: the grid rows x halves x steps x seeds that the correlation tests walk, and
    rows up to 2^31 - 1.  Layout: [seed 2][step 64][half 2][row 16384] then 2^18 scattered rows."""
    rows = np.concatenate([np.arange(16320), np.int64(2 ** 31 - 1) - np.arange(64)[::-1]]).astype(np.int64)
    assert rows.size == 16384
    keys = np.stack([_step_keys(1234567, range(64)), _step_keys(1234568, range(64))])          # seeds that differ by 1
    row = np.broadcast_to(rows, (2, 64, 2, 16384))
    half = np.broadcast_to(np.arange(2)[:, None], (2, 64, 2, 16384))
    key = np.broadcast_to(keys[:, :, None, None], (2, 64, 2, 16384))
    rng = np.random.RandomState(8)
    srow = rng.randint(0, 2 ** 31, size=1 << 18)
    skey = _step_keys(77, rng.randint(0, 10 ** 6, size=1 << 18))
    shalf = rng.randint(0, 2, size=1 << 18)
    return (np.concatenate([row.ravel(), srow]), np.concatenate([half.ravel(), shalf]),
            np.concatenate([key.ravel(), skey]), (2, 64, 2, 16384))


def _ks_p(u):
    """two-sided Kolmogorov-Smirnov p value of u against the uniform on (0, 1)"""
    from scipy import stats
    return stats.kstest(u, "uniform").pvalue


@pytest.mark.parametrize("a", [2.0, 1.3])
def test_device_stretch_draw_ranges_laws_and_independence(probe, a):
    """stretch_draw on 4.46e6 (row, half, key) triples -- rows up to 2^31 - 1, keys as step_key forms them for 64
    consecutive steps and for seeds that differ by 1 -- for c_count in {1, 5, 13, 125, 2048}:
    1/a <= zz < a, 0 < u3 < 1 strictly (its log is taken), 0 <= pj < c_count;
    zz against its law G(z) = (sqrt(a z) - 1) / (a - 1) and u3 against the uniform by Kolmogorov-Smirnov, pj by chi-square
    over the c_count cells: p >= 1e-6 each (a condition: twelve tests per scale, fixed inputs);
    the three draws of a row, the same draw in neighbouring rows, in the two halves, in consecutive steps and under
    neighbouring seeds uncorrelated: |r| sqrt(n) <= 5 (a condition: r sqrt(n) is a standard normal for independent
    draws; 33 correlations per scale)."""
    from scipy import stats
    row, half, key, grid = _draw_inputs()
    n = row.size
    assert n >= 4000000
    for c_count in (1, 5, 13, 125, 2048):
        zz, pj, u3 = probe.stretch_draw(row, half, key, a, c_count)
        assert zz.min() >= 1.0 / a and zz.max() < a
        assert u3.min() > 0.0 and u3.max() < 1.0
        assert pj.min() >= 0 and pj.max() < c_count
        if c_count > 1:
            cnt = np.bincount(pj, minlength=c_count)
            p = stats.chisquare(cnt).pvalue
            print("a = %g, c_count %d: chi-square p of pj %.3g" % (a, c_count, p))
            assert p >= 1e-6, (c_count, p)
    # (the last call: c_count = 2048)
    uz = (np.sqrt(a * zz) - 1.0) / (a - 1.0)                       # G(z): uniform when zz follows its law
    uj = (pj + 0.5) / 2048.0
    for name, u in (("zz", uz), ("u3", u3)):
        p = _ks_p(u)
        print("a = %g: Kolmogorov-Smirnov p of %s %.3g" % (a, name, p))
        assert p >= 1e-6, (name, p)
    # and in a part of the inputs (one seed, one half, the first 8 steps), so that a defect of single steps is not averaged out
    ngrid = int(np.prod(grid))
    G = {"zz": uz[:ngrid].reshape(grid), "pj": uj[:ngrid].reshape(grid), "u3": u3[:ngrid].reshape(grid)}
    for name in ("zz", "u3"):
        p = _ks_p(G[name][0, :8, 0].ravel())
        assert p >= 1e-6, (name, p)

    def corr(x, y, what):
        x, y = x.ravel(), y.ravel()
        r = np.corrcoef(x, y)[0, 1] * np.sqrt(x.size)
        parity_record("stretch draw correlation |r| sqrt(n)", abs(r), 5.0)
        assert abs(r) <= 5.0, (what, r)
        return r

    names = list(G)
    worst = 0.0
    for i, x in enumerate(names):
        for y in names[i:]:
            if x != y:
                worst = max(worst, abs(corr(G[x], G[y], "%s and %s of a row" % (x, y))))           # 3
            # the same or another draw in neighbouring rows / the two halves / consecutive steps / neighbouring seeds
            for what, u, v in (("neighbouring rows", G[x][..., :-1], G[y][..., 1:]),
                               ("the two halves", G[x][:, :, 0], G[y][:, :, 1]),
                               ("consecutive steps", G[x][:, :-1], G[y][:, 1:]),
                               ("seeds that differ by 1", G[x][0], G[y][1]),
                               ("second half of this step, first of the next", G[x][:, :-1, 1], G[y][:, 1:, 0])):
                worst = max(worst, abs(corr(u, v, "%s of a row, %s in %s" % (x, y, what))))       # 6 x 5
    print("a = %g: largest |r| sqrt(n) of the correlations %.2f" % (a, worst))

