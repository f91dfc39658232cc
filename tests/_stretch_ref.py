"""The stretch move of Goodman & Weare (2010) as emcee 2 makes it, in plain numpy: the yardstick of the sampler
statistics tests.  It shares nothing with the code under test -- numpy's own generator (no Philox), no likelihood
of the package -- and is vectorised over R independent ensembles:

    p [R, nw, d], lnp [R, nw] are moved in place; lnprob(q[..., d]) -> [...] is any callable.

Per half-step every walker s of one half draws z with density g(z) ~ 1/sqrt(z) on [1/a, a] and a partner c from the
other half, proposes q = c - z (c - s) and accepts with probability min(1, z^zpow p(q) / p(s)).  The exponent is an
argument: the correct one is (dimension of the space the walkers span) - 1, and the tests also run wrong ones."""
import numpy as np


def stretch_move(lnprob, p, lnp, nsteps, rng, a=2.0, zpow=4.0):
    """nsteps full steps in place; returns the accepted moves per ensemble, [R]."""
    R, nw = p.shape[:2]
    half = nw // 2
    nacc = np.zeros(R)
    for _ in range(int(nsteps)):
        for S, C in ((slice(0, half), slice(half, nw)), (slice(half, nw), slice(0, half))):
            s, c, ls = p[:, S], p[:, C], lnp[:, S]                  # (views)
            ns, nc = s.shape[1], c.shape[1]
            zz = ((a - 1.0) * rng.random_sample((R, ns)) + 1.0) ** 2 / a
            partner = np.take_along_axis(c, rng.randint(nc, size=(R, ns))[:, :, None], axis=1)
            q = partner - zz[:, :, None] * (partner - s)
            new = lnprob(q)
            with np.errstate(invalid="ignore"):
                ok = zpow * np.log(zz) + new - ls > np.log(rng.random_sample((R, ns)))
            s[ok] = q[ok]
            ls[ok] = new[ok]
            nacc += ok.sum(axis=1)
    return nacc


def run_battery(target, R, nw, nchunk, every, seed, a=2.0, zpow=None, free=None, p0=None, burn_chunks=0):
    """The moment battery (tests/_targets.py, `Battery`) on this reference: R ensembles of nw walkers from exact draws of
    the target (or from p0 [R, nw, 5]), nchunk chunks of `every` steps, the first burn_chunks of them not counted.
    -> (t values, names, acceptance fraction per ensemble, final p)"""
    from _targets import Battery
    rng = np.random.RandomState(seed)
    free = list(range(5)) if free is None else list(free)
    p = target.draw(rng, (R, nw)) if p0 is None else np.array(p0, dtype=np.float64)
    for k in range(5):
        if k not in free:
            p[..., k] = target.mu0[k]
    lnp = target.lnp(p)
    bat = Battery(target, free)
    nacc = np.zeros(R)
    for ch in range(nchunk):
        nacc += stretch_move(target.lnp, p, lnp, every, rng, a=a, zpow=len(free) - 1.0 if zpow is None else zpow)
        if ch >= burn_chunks:
            bat.add(p)
    return bat.t(), bat.names, nacc / (nw * nchunk * every), p
