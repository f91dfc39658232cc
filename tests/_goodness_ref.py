"""Reference of the goodness-of-fit analysis (csrc/mbb_goodness.hip.h) for its tests: chisq in numpy's longdouble from
given band fluxes, and the chi-square tail probability Q(nb/2, chisq/2) from mpmath at 50 digits.
tests/test_goodness_cpu.py holds both to scipy.stats.chi2.sf; tests/test_goodness_gpu.py holds the device to them."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
Q_FLOOR = 1e-290           # below this true value q is only asked to be in [0, 1e-289]


def chisq(flux, model, ivar=None, invcov=None):
    """sum_b (f_b - m_b)^2 ivar_b, or r^T C^-1 r, in longdouble; model [..., nb] -> [...]"""
    r = np.asarray(flux, dtype=LD) - np.asarray(model, dtype=LD)
    if invcov is None:
        return (r * r * np.asarray(ivar, dtype=LD)).sum(axis=-1)
    return np.einsum("...i,ij,...j->...", r, np.asarray(invcov, dtype=LD), r)


def chisq_bound(flux, model, ivar=None, invcov=None):
    """The bound on |chisq - reference| for a device whose band fluxes are within 1e-12 of `model`, each:
    with A = diag(ivar) or |C^-1| elementwise and r = f - m,
        2e-12 |r|^T A |m| + 1e-24 |m|^T A |m| + (2 nb + 4) eps |r|^T A |r|
    -- the flux error propagated to first and second order, then the rounding of the subtraction, the products and an
    nb-term sum."""
    m = np.abs(np.asarray(model, dtype=LD))
    r = np.abs(np.asarray(flux, dtype=LD) - np.asarray(model, dtype=LD))
    nb = m.shape[-1]
    A = np.diag(np.asarray(ivar, dtype=LD)) if invcov is None else np.abs(np.asarray(invcov, dtype=LD))
    q = lambda x, y: np.einsum("...i,ij,...j->...", x, A, y)            # noqa: E731
    return (2e-12 * q(r, m) + 1e-24 * q(m, m) + (2 * nb + 4) * EPS * q(r, r)).astype(np.float64)


def q_mp(nb, chisq_value):
    """Q(nb/2, chisq/2) as an mpmath number at 50 digits; the edge values of the definition."""
    import mpmath
    x = float(chisq_value)
    if x != x:
        return mpmath.nan
    if x <= 0:
        return mpmath.mpf(1)
    if x == float("inf"):
        return mpmath.mpf(0)
    with mpmath.workdps(50):
        return mpmath.gammainc(mpmath.mpf(nb) / 2, mpmath.mpf(x) / 2, mpmath.inf, regularized=True)


MAX_NB = 256               # kGammqMaxNb: the orders m_gammq_half accepts are 1 .. MAX_NB
_ORDER_TRUTH = {}


def order_grid(nb):
    """The 70 chisq values order nb is judged on: sixty from 1e-3 to 2999, seven around the order's own mean nb (where
    q falls from 1 to 0 for a large order), and the edge of the range (from chisq = 3000 on the function returns 0)."""
    x = np.unique(np.concatenate([np.geomspace(1e-3, 2999.0, 60), nb * np.array([0.25, 0.5, 0.9, 1.0, 1.1, 2.0, 4.0]),
                                  [1416.0, 1490.0, 2999.0, 3001.0]]))
    assert x.size == 70, (nb, x.size)
    return x


def order_truth(nb):
    """(order_grid(nb), [q_mp(nb, x) for x in it], which of them are >= Q_FLOOR), computed once per session"""
    if nb not in _ORDER_TRUTH:
        x = order_grid(nb)
        t = [q_mp(nb, v) for v in x]
        _ORDER_TRUTH[nb] = (x, t, np.array([v >= Q_FLOOR for v in t]))
    return _ORDER_TRUTH[nb]


def horner_bound_eps(nb):
    """The derived bound on the relative error of m_gammq_half where no library function enters (even nb on the device;
    every nb on the host, whose erfc is the host libm's within an ulp), in units of eps: m_exp twice at 2 ulp each,
    ceil(nb/2) Horner steps of one IEEE division and one fma at 1.5 ulp a step at the worst, three products, and two
    for erfc and its first-order correction: 4 + 1.5 ceil(nb/2) + 3 + 2."""
    return 9.0 + 1.5 * ((nb + 1) // 2)


def rel_errors(truth, big, got):
    """relative errors of got against the mpmath numbers truth, where big"""
    import mpmath
    with mpmath.workdps(50):
        return np.array([float(abs(mpmath.mpf(float(g)) - t) / t) for g, t, b in zip(got, truth, big) if b])


def q_errors(nb, chisq_values, got):
    """(relative errors of `got` where the true q >= Q_FLOOR, the values of `got` where it is below), against mpmath
    at the very doubles chisq_values."""
    import mpmath
    rel, low = [], []
    for x, g in zip(np.ravel(chisq_values), np.ravel(got)):
        t = q_mp(nb, x)
        if t >= Q_FLOOR:
            with mpmath.workdps(50):
                rel.append(float(abs(mpmath.mpf(float(g)) - t) / t))
        else:
            low.append(float(g))
    return np.array(rel), np.array(low)
