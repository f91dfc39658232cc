"""Plain numpy restatement of what the reference's mbb_results makes of a chain (reference mbb_emcee/results.py),
for the summary tests: tests/test_summary_cpu.py holds it to tests/golden/summary.npz (the reference's own output)
bit for bit, and tests/test_summary_gpu.py uses it at sizes the reference was not run at."""
import numpy as np

EPS = np.finfo(np.float64).eps


def parcen(array, percentile, lowlim=None, uplim=None):
    """_parcen_internal (results.py:314-369): [mean, upper - mean, mean - lower], and the surviving count."""
    pcnt = float(percentile)
    if pcnt < 0 or pcnt > 100:
        raise ValueError("Invalid percentile {:f}".format(pcnt))
    pval = 0.5 * (100 - pcnt)
    a = np.asarray(array, dtype=np.float64)
    if lowlim is not None or uplim is not None:
        if lowlim is None:
            cond = (a <= float(uplim)).nonzero()[0]
        elif uplim is None:
            cond = (a >= float(lowlim)).nonzero()[0]
        else:
            cond = np.logical_and(a >= float(lowlim), a <= float(uplim)).nonzero()[0]
        if len(cond) == 0:
            raise Exception("No elements survive lower/upper limit clipping")
        if len(cond) != len(a):
            a = a[cond]
    mn = a.mean() if lowlim is None and uplim is None else np.mean(a)
    perc = np.percentile(a, [pval, 100 - pval])
    return np.array([mn, perc[1] - mn, mn - perc[0]]), len(a)


def best_fit(chain, lnprob):
    """process_fit (results.py:160-165): the first maximum of lnprobability in [walker][step] order."""
    idx = np.unravel_index(lnprob.argmax(), lnprob.shape)
    return chain[idx[0], idx[1], :], lnprob[idx[0], idx[1]], idx


def bracket(sorted_a, q):
    """The two order statistics numpy's linear percentile q interpolates between."""
    n = sorted_a.shape[-1]
    vi = (n - 1) * (q / 100.0)
    lo = int(np.floor(vi))
    lo, hi = (n - 1, n - 1) if vi >= n - 1 else ((0, 0) if vi < 0 else (lo, lo + 1))
    return sorted_a[..., lo], sorted_a[..., hi]


def ulps_off(got, want, lo, hi):
    """|got - want| in units of the spacing of the larger bracketing value (the rounding of the interpolation)."""
    scale = np.spacing(np.maximum(np.maximum(np.abs(lo), np.abs(hi)), np.finfo(np.float64).tiny))
    return np.abs(np.asarray(got) - np.asarray(want)) / scale
