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
