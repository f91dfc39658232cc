"""Analytic targets for the sampler statistics tests, with their exact moments, exact draws, and the moment battery.

A target is a product over the five parameters (T, beta, lambda0, alpha, fnorm) of one-dimensional densities that the
product's own knobs can make: a Gaussian prior on every parameter (`set_gaussian_prior`), optionally a hard lower wall
through the middle of one column (`set_lowlim`: below it the likelihood is -inf) and a soft upper wall through the
middle of another (`set_uplim`: above it the likelihood adds -0.5 (x - uplim)^2 / w^2, w = 0.02 (uplim - lowlim), so the
density there is the narrower Gaussian of width 1 / sqrt(1 / sd^2 + 1 / w^2)).  With photometry whose uncertainties are
enormous the data term is constant and the likelihood IS the target; the tests assert that before they use it.

    G5   five independent Gaussians of very different widths, every limit more than six sigma away
    W5   G5 with the hard wall at beta = 1.8 and the soft wall at alpha = 3.0

Moments by one-dimensional quadrature split at the wall (scipy quad, epsrel 1e-13); draws exact by construction."""
import numpy as np

PARAMS = ("T", "beta", "lambda0", "alpha", "fnorm")
LOWLIM = np.array([1.0, 0.1, 1.0, 0.1, 1e-3])            # the likelihood's default lower limits


class Target(object):
    def __init__(self, name, mu0, sd, hard=None, soft=None):
        self.name = name
        self.mu0, self.sd = np.array(mu0, dtype=np.float64), np.array(sd, dtype=np.float64)
        self.hard, self.soft = hard, soft                 # column of the wall; the wall is at mu0[column]
        assert hard is None or soft is None or hard != soft
        self.w = 0.02 * (self.mu0[soft] - LOWLIM[soft]) if soft is not None else None
        # width above the soft wall, in units of the column's sd
        self.s_up = 1.0 / np.sqrt(1.0 + (self.sd[soft] / self.w) ** 2) if soft is not None else None
        self._mom = None

    # ---- the density
    def lnp(self, p):
        """log density up to a constant, p[..., 5]"""
        p = np.asarray(p, dtype=np.float64)
        x = (p - self.mu0) / self.sd
        l = -0.5 * (x * x).sum(axis=-1)
        if self.soft is not None:
            d = p[..., self.soft] - self.mu0[self.soft]
            l = l - np.where(d > 0, 0.5 * d * d / self.w ** 2, 0.0)
        if self.hard is not None:
            l = np.where(p[..., self.hard] < self.mu0[self.hard], -np.inf, l)
        return l

    def _density_1d(self, k):
        """(density of x = (p - mu0) / sd of column k, its break points)"""
        if k == self.hard:
            return (lambda x: np.exp(-0.5 * x * x)), (0.0, 1.0, np.inf)
        if k == self.soft:
            r2 = (self.sd[k] / self.w) ** 2
            return (lambda x: np.exp(-0.5 * x * x * (1.0 + (x > 0) * r2))), (-np.inf, 0.0, np.inf)
        return (lambda x: np.exp(-0.5 * x * x)), (-np.inf, 0.0, np.inf)

    def moments(self):
        """exact (mean, variance, fourth central moment) of every column"""
        if self._mom is None:
            from scipy.integrate import quad
            mu, var, m4 = np.zeros(5), np.zeros(5), np.zeros(5)
            for k in range(5):
                dens, pts = self._density_1d(k)

                def integral(g):
                    return sum(quad(lambda x: g(x) * dens(x), lo, hi, epsabs=0, epsrel=1e-13)[0]
                               for lo, hi in zip(pts[:-1], pts[1:]))
                norm = integral(lambda x: 1.0)
                m = integral(lambda x: x) / norm
                mu[k] = self.mu0[k] + self.sd[k] * m
                var[k] = self.sd[k] ** 2 * integral(lambda x: (x - m) ** 2) / norm
                m4[k] = self.sd[k] ** 4 * integral(lambda x: (x - m) ** 4) / norm
            self._mom = (mu, var, m4)
        return self._mom

    def draw(self, rng, shape):
        """exact independent draws, shape + (5,)"""
        shape = tuple(shape)
        x = rng.normal(size=shape + (5,))
        if self.hard is not None:
            x[..., self.hard] = np.abs(x[..., self.hard])
        if self.soft is not None:
            # the mass below the wall to the mass above it is 1 : s_up (two half-normals of equal height at the wall)
            below = rng.random_sample(shape) < 1.0 / (1.0 + self.s_up)
            h = np.abs(rng.normal(size=shape))
            x[..., self.soft] = np.where(below, -h, self.s_up * h)
        return self.mu0 + self.sd * x

    # ---- the same thing on the product
    def apply(self, like):
        """set this target's priors and walls on a likelihood (or an mbb_fitter, which forwards the calls)"""
        for k, name in enumerate(PARAMS):
            like.set_gaussian_prior(name, self.mu0[k], self.sd[k])
        if self.hard is not None:
            like.set_lowlim(PARAMS[self.hard], self.mu0[self.hard])
        if self.soft is not None:
            like.set_uplim(PARAMS[self.soft], self.mu0[self.soft])

    def oracle_kwargs(self):
        """the limits and priors `apply` + `set_phot(WAVE, ...)` leave on a likelihood, as oracle.OracleLikelihood's keywords"""
        lowlim = LOWLIM.copy()
        has_uplim, uplim = [0, 1, 1, 1, 0, 0], [np.inf, 20.0, 3.0 * WAVE.max(), 20.0, np.inf, np.inf]
        if self.hard is not None:
            lowlim[self.hard] = self.mu0[self.hard]
        if self.soft is not None:
            has_uplim[self.soft], uplim[self.soft] = 1, self.mu0[self.soft]
        return dict(lowlim=lowlim, has_uplim=has_uplim, uplim=uplim, has_gprior=[1] * 5 + [0],
                    gprior_mean=list(self.mu0) + [0.0], gprior_sigma=list(self.sd) + [1.0])


# Photometry that says nothing: a handful of plain wavelengths (no passband integration: an evaluation costs next to
# nothing), uncertainties of 1e12 mJy -- the data term is below 1e-19 for any SED of the targets.  (set_phot gives
# lambda0 a soft upper limit at 3 x 850 um, beta and alpha have theirs at 20: tens of sigma from the targets.)
WAVE = np.array([100.0, 160.0, 250.0, 350.0, 500.0, 850.0])
FLUX = np.full(6, 10.0)
UNC = np.full(6, 1e12)

_MU = (30.0, 1.8, 600.0, 3.0, 40.0)
_SD = (2.0, 0.15, 30.0, 0.2, 3.0)


def G5():
    return Target("G5", _MU, _SD)


def W5():
    return Target("W5", _MU, _SD, hard=1, soft=3)


class Battery(object):
    """The moment battery.  After every chunk of steps `add(p)` takes, per ensemble, the walker averages of
    (x - mu), (x - mu)^2 / var - 1, (x - mu)^4 / m4 - 1 for each free column and (x_a - mu_a)(x_b - mu_b) / (sd_a sd_b) for
    each pair of free columns -- mu, var, m4 the EXACT values: 3 f + f (f - 1) / 2 statistics for f free columns (25, 18, 12,
    7 for f = 5, 4, 3, 2).  An ensemble started from exact draws is stationary under a correct sampler, so each
    statistic's expectation is 0 at every step whatever the autocorrelation; the R ensembles are independent, and
    t = mean / (std / sqrt(R)) over them is a standard normal to good accuracy for R >= 64."""

    BOUND = 5.0

    def __init__(self, target, free=None):
        self.free = list(range(5)) if free is None else list(free)
        mu, var, m4 = target.moments()
        f = self.free
        self.mu, self.var, self.m4 = mu[f], var[f], m4[f]
        self.pairs = [(i, j) for i in range(len(f)) for j in range(i + 1, len(f))]
        self.names = (["mean " + PARAMS[k] for k in f] + ["var " + PARAMS[k] for k in f] + ["m4 " + PARAMS[k] for k in f] +
                      ["cov %s,%s" % (PARAMS[f[i]], PARAMS[f[j]]) for i, j in self.pairs])
        self.sum, self.n = None, 0

    def add(self, p):
        """p [R, nw, 5]: the ensembles as they stand"""
        d = np.asarray(p, dtype=np.float64)[..., self.free] - self.mu
        sd = np.sqrt(self.var)
        st = [d.mean(axis=1), (d * d / self.var).mean(axis=1) - 1.0, (d ** 4 / self.m4).mean(axis=1) - 1.0]
        if self.pairs:
            st.append(np.stack([(d[..., i] * d[..., j]).mean(axis=1) / (sd[i] * sd[j]) for i, j in self.pairs], axis=-1))
        s = np.concatenate(st, axis=-1)
        self.sum = s if self.sum is None else self.sum + s
        self.n += 1

    def means(self):
        """[R, nstat]: every ensemble's time average of every statistic"""
        return self.sum / self.n

    def t(self):
        m = self.means()
        return m.mean(axis=0) / (m.std(axis=0, ddof=1) / np.sqrt(m.shape[0]))

    def excess(self):
        """mean over ensembles of each statistic (e.g. variance / exact - 1), by name"""
        return dict(zip(self.names, self.means().mean(axis=0)))
