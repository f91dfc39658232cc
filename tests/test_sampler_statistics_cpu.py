"""The stretch move held to distributions that are known exactly -- the half that needs no GPU.

tests/_targets.py has the analytic targets (G5, W5), their exact moments and the moment battery; tests/_stretch_ref.py
the plain numpy stretch move that is the yardstick.  Here:

  * the yardstick itself: the targets' draws have the targets' moments; the numpy reference passes the battery at
    |t| <= 5 for two seeds and FAILS it with the exponent 3.9 (a 2 % error of the variance), and with the exponent
    dim - 1 = 4 on an ensemble with fixed columns (the defect the reference implementation has: +22 %, +56 %, +110 %);
  * the target is what the likelihood computes, through the CPU oracle;
  * the host `EnsembleSampler` on a Python lnprob of the targets: all five columns free and with one, two and three
    columns held fixed by zero initial scatter (the exponent is the number of columns the ensemble spans, less one).

Bound: every |t| <= 5 with fixed seeds, no statistic left out (Battery's docstring says why that is a condition and
not a measurement).  Rank deficiency that is not axis-aligned (walkers on a tilted plane) is out of scope."""
import numpy as np
import pytest

import _stretch_ref as ref
from _targets import G5, W5, WAVE, FLUX, UNC, Battery
from conftest import parity_record

BOUND = Battery.BOUND
FIXED_SETS = [(), (3,), (2, 3), (2, 3, 4)]             # nothing; alpha; lambda0, alpha; lambda0, alpha, fnorm
NSTAT = {5: 25, 4: 18, 3: 12, 2: 7}


def _report(what, t, names):
    worst = int(np.argmax(np.abs(t)))
    print("%s: %d statistics, max |t| %.2f (%s)" % (what, len(t), np.abs(t).max(), names[worst]))
    parity_record("sampler moment t", np.abs(t).max(), BOUND)


def test_targets_draws_have_the_exact_moments():
    """The yardstick's own consistency: quadrature moments against the closed forms where there are any (Gaussian:
    sd^2, 3 sd^4; half-normal: mean sd sqrt(2/pi), variance sd^2 (1 - 2/pi)), and 4e6 exact draws against the
    quadrature moments (each |t| <= 5: 15 statistics per target)."""
    g, w = G5(), W5()
    mu, var, m4 = g.moments()
    assert np.all(np.abs(mu - g.mu0) <= 1e-12 * g.sd)
    np.testing.assert_allclose(var, g.sd ** 2, rtol=1e-12)
    np.testing.assert_allclose(m4, 3.0 * g.sd ** 4, rtol=1e-12)
    mu, var, m4 = w.moments()
    np.testing.assert_allclose(mu[1], 1.8 + 0.15 * np.sqrt(2.0 / np.pi), rtol=1e-12)
    np.testing.assert_allclose(var[1], 0.15 ** 2 * (1.0 - 2.0 / np.pi), rtol=1e-12)
    s = w.s_up                                             # two half-normals, widths 1 and s, masses 1 : s
    m1 = (s * s - 1.0) * np.sqrt(2.0 / np.pi) / (1.0 + s)
    np.testing.assert_allclose(mu[3], 3.0 + 0.2 * m1, rtol=1e-12)
    np.testing.assert_allclose(var[3], 0.2 ** 2 * ((1.0 + s ** 3) / (1.0 + s) - m1 * m1), rtol=1e-12)
    for tg in (g, w):
        mu, var, m4 = tg.moments()
        x = tg.draw(np.random.RandomState(11), (4000000,))
        d = x - mu
        for k, stat in enumerate((d, d * d / var - 1.0, d ** 4 / m4 - 1.0)):
            t = stat.mean(axis=0) / (stat.std(axis=0, ddof=1) / np.sqrt(len(x)))
            assert np.abs(t).max() <= BOUND, (tg.name, k, t)
        if tg.hard is not None:
            assert x[:, tg.hard].min() >= tg.mu0[tg.hard]


@pytest.mark.parametrize("seed", [1, 2])
def test_reference_passes_the_battery(seed):
    """The numpy reference on W5, R = 256 ensembles of 64 walkers, 100 chunks of 20 steps from exact draws: all 25
    |t| <= 5 (observed when written: 2.2 and 1.8), no walker below the hard wall."""
    t, names, acc, p = ref.run_battery(W5(), 256, 64, 100, 20, seed)
    _report("reference, W5, seed %d" % seed, t, names)
    assert len(t) == 25 and np.abs(t).max() <= BOUND, dict(zip(names, np.round(t, 2)))
    assert p[..., 1].min() >= 1.8
    assert 0.3 < acc.mean() < 0.7


def test_battery_sees_a_two_percent_error_of_the_variance():
    """The battery's power: the same run with the exponent 3.9 in place of 4 fails (observed: max |t| about 15)."""
    t, names, _, _ = ref.run_battery(W5(), 256, 64, 100, 20, 4, zpow=3.9)
    print("reference with z^3.9: max |t| %.1f" % np.abs(t).max())
    assert np.abs(t).max() > 2 * BOUND


@pytest.mark.parametrize("fixed", FIXED_SETS[1:])
def test_reference_with_fixed_columns_needs_the_smaller_exponent(fixed):
    """Columns held fixed by zero scatter: with z^(free - 1) the reference passes, with z^(dim - 1) = z^4 -- what the
    reference implementation and this package's samplers used -- the variances of the free columns come out 22 %, 56 %
    and 110 % too large (one, two, three fixed columns)."""
    free = [k for k in range(5) if k not in fixed]
    t, names, _, p = ref.run_battery(G5(), 256, 64, 40, 20, 5, free=free)
    _report("reference, G5, fixed %s" % (fixed,), t, names)
    assert len(t) == NSTAT[len(free)] and np.abs(t).max() <= BOUND, dict(zip(names, np.round(t, 2)))
    assert all(np.all(p[..., k] == G5().mu0[k]) for k in fixed)
    t4, names, _, _ = ref.run_battery(G5(), 256, 64, 40, 20, 5, free=free, zpow=4.0)
    iv = [i for i, n in enumerate(names) if n.startswith("var ")]
    print("reference with z^4 and %d fixed: max |t| %.1f" % (len(fixed), np.abs(t4).max()))
    assert np.abs(t4[iv]).min() > 2 * BOUND


def test_target_is_what_the_oracle_computes(oracle):
    """like(p) - like(p_ref) is the analytic log-density difference to 1e-9 absolute on 1000 draws of each target and
    on rows below the hard wall (-inf both): no term of the data, of the default limits or of lambda0's automatic
    upper limit has crept in."""
    for tg in (G5(), W5()):
        like = oracle.OracleLikelihood(FLUX, UNC, wave=WAVE, **tg.oracle_kwargs())
        p = tg.draw(np.random.RandomState(3), (1000,))
        # (and rows mirrored about the centre in beta or in alpha: below the hard wall, and well above the soft one)
        m1, m3 = p[:200].copy(), p[:200].copy()
        m1[:, 1] = 2.0 * tg.mu0[1] - m1[:, 1]
        m3[:, 3] = tg.mu0[3] + np.abs(m3[:, 3] - tg.mu0[3])
        p = np.concatenate([p, m1, m3])
        got, want = like(p), tg.lnp(p)
        assert np.all(like.status[np.isfinite(want)] == 0)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        fin = np.isfinite(want)
        err = np.abs((got[fin] - got[0]) - (want[fin] - want[0]))
        parity_record("target vs likelihood (abs)", err.max(), 1e-9)
        assert err.max() <= 1e-9, (tg.name, err.max())
        if tg.hard is not None:
            assert np.isneginf(want).sum() > 50


# ---- the host sampler --------------------------------------------------------------------------------------------
R_HOST, NW_HOST, CHUNKS_HOST, EVERY_HOST = 64, 32, 40, 10


def _host_battery(target, fixed, seed0, a=2.0):
    """R_HOST independent host samplers (seeds seed0 + r) of NW_HOST walkers on the Python lnprob of the target, each
    from exact draws, CHUNKS_HOST chunks of EVERY_HOST unstored steps -> (battery, acceptance per ensemble)."""
    from mbb_emcee_amd.ensemble import EnsembleSampler
    free = [k for k in range(5) if k not in fixed]
    bat = Battery(target, free)
    rng = np.random.RandomState(1000 + seed0)
    state = np.empty((R_HOST, NW_HOST, 5))
    samplers = []
    for r in range(R_HOST):
        s = EnsembleSampler(NW_HOST, 5, target.lnp, a=a, vectorize=True, seed=seed0 + r)
        p0 = target.draw(rng, (NW_HOST,))
        for k in fixed:
            p0[:, k] = target.mu0[k]
        samplers.append(s)
        state[r] = p0
    first = True
    for ch in range(CHUNKS_HOST):
        for r, s in enumerate(samplers):
            pos, lnp, _ = s.run_mcmc(state[r] if first else None, EVERY_HOST, storechain=False)
            state[r] = pos
            if ch == CHUNKS_HOST - 1:
                assert np.array_equal(lnp, target.lnp(pos))           # lnprob of the final state is the target's
        first = False
        bat.add(state)
    for k in fixed:
        assert np.all(state[..., k] == target.mu0[k])                  # bit for bit
    if target.hard is not None and target.hard in free:
        assert state[..., target.hard].min() >= target.mu0[target.hard]
    acc = np.array([s.acceptance_fraction.mean() for s in samplers])
    assert all(s.iterations == CHUNKS_HOST * EVERY_HOST for s in samplers)
    return bat, acc


@pytest.mark.parametrize("fixed", FIXED_SETS, ids=lambda f: "fixed" + "".join(map(str, f)) if f else "free")
@pytest.mark.parametrize("tname", ["G5", "W5"])
def test_host_sampler_moments(tname, fixed):
    """The host EnsembleSampler, 64 ensembles x 32 walkers x 400 steps from exact draws: 25 / 18 / 12 / 7 statistics with
    0 / 1 / 2 / 3 columns fixed, every |t| <= 5; fixed columns stay bit for bit; nobody below the hard wall; the mean
    acceptance fraction is the numpy reference's for the same target, walkers and exponent within 5 combined standard
    errors.  (Before the exponent followed the number of free columns the variances of the fixed cases were 22 %, 56 % and
    110 % high: t of several tens.)"""
    target = G5() if tname == "G5" else W5()
    bat, acc = _host_battery(target, fixed, seed0=17 + 100 * len(fixed))
    t = bat.t()
    _report("host sampler, %s, fixed %s" % (tname, fixed), t, bat.names)
    ex = bat.excess()
    print("   variance / exact - 1:", {n: round(v, 4) for n, v in ex.items() if n.startswith("var ")})
    assert len(t) == NSTAT[5 - len(fixed)]
    assert np.abs(t).max() <= BOUND, dict(zip(bat.names, np.round(t, 2)))
    _, _, racc, _ = ref.run_battery(target, 256, NW_HOST, 10, 20, 99, free=bat.free)
    se = np.hypot(acc.std(ddof=1) / np.sqrt(len(acc)), racc.std(ddof=1) / np.sqrt(len(racc)))
    print("   acceptance %.4f, reference %.4f, combined standard error %.4f" % (acc.mean(), racc.mean(), se))
    parity_record("acceptance fraction vs reference / standard error", abs(acc.mean() - racc.mean()) / se, 5.0)
    assert abs(acc.mean() - racc.mean()) <= 5.0 * se


def test_host_sampler_other_stretch_scale():
    """a = 1.3 on G5: the z law and the exponent for a scale other than 2."""
    bat, acc = _host_battery(G5(), (), seed0=901, a=1.3)
    t = bat.t()
    _report("host sampler, G5, a = 1.3", t, bat.names)
    assert len(t) == 25 and np.abs(t).max() <= BOUND, dict(zip(bat.names, np.round(t, 2)))
    _, _, racc, _ = ref.run_battery(G5(), 256, NW_HOST, 10, 20, 98, a=1.3)
    se = np.hypot(acc.std(ddof=1) / np.sqrt(len(acc)), racc.std(ddof=1) / np.sqrt(len(racc)))
    assert abs(acc.mean() - racc.mean()) <= 5.0 * se, (acc.mean(), racc.mean(), se)


def test_host_sampler_exponent_follows_the_starting_ensemble():
    """The exponent is decided where the state is set: the number of columns of p0 that are not constant over the
    walkers, less one; continuing a run keeps it."""
    from mbb_emcee_amd.ensemble import EnsembleSampler
    g = G5()
    for fixed in FIXED_SETS:
        s = EnsembleSampler(16, 5, g.lnp, vectorize=True, seed=1)
        p0 = g.draw(np.random.RandomState(2), (16,))
        for k in fixed:
            p0[:, k] = g.mu0[k]
        s.run_mcmc(p0, 2)
        assert s._zpow == 4.0 - len(fixed)
        s.run_mcmc(None, 2)
        assert s._zpow == 4.0 - len(fixed)
