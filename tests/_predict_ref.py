"""Plain numpy restatement of the predicted-flux analysis (mbb_results._predict_flux and predflux_cen, reference
mbb_emcee/results.py:895-985) for the prediction tests: the oracle's SED at a spec's quadrature samples, summed with
the weights, then numpy's mean and percentile of the column.  tests/test_predict_cpu.py holds it to the columns the
reference itself made (tests/golden/results.npz, predict/*); tests/test_predict_gpu.py uses its statistics at sizes the
reference was not run at."""
import numpy as np

import _summary_ref as SR

UM_TO_GHZ = 299792458e-3

EMPTY, HAS_NAN, ROW_SHIFT = 1, 2, 8


def wave_samples(wave):
    """The one quadrature sample of a wavelength [um]: (frequency [GHz], weight 1)."""
    return np.array([UM_TO_GHZ / float(wave)]), np.ones(1)


def band_samples(wave, sedmult, normfac):
    """A passband's quadrature samples from the reference-made tables (conftest.golden_bands): response.py:572-576 sums
    f_nu(freq) * sedmult and multiplies by normfac."""
    return UM_TO_GHZ / np.asarray(wave, dtype=np.float64), np.asarray(sedmult, dtype=np.float64) * float(normfac)


def column(O, chain, samples, opthin, noalpha, wavenorm=500.0):
    """The predicted flux of every chain entry: sum_i f_nu(freq_i) weight_i with the oracle's SED."""
    freq, weight = samples
    c = np.asarray(chain, dtype=np.float64).reshape(-1, 5)
    out = np.array([(O.OracleSED(*p, wavenorm=wavenorm, opthin=opthin, noalpha=noalpha).f_nu(freq) * weight).sum() for p in c])
    return out.reshape(np.shape(chain)[:-1])


def windowed_column(col, burn=0, thin=1):
    """A [nw, nsteps] column's kept steps, flattened in [nw][nkept] order: what _parcen_internal is given."""
    return np.ascontiguousarray(np.asarray(col)[:, burn::thin]).reshape(-1)


def stats(col1d, qs, lo=None, hi=None):
    """numpy's count, min, max, mean and percentiles of a 1-d column, clipped as _parcen_internal clips."""
    return SR.column_reference(col1d, qs, lo, hi)


def predflux_cen(col1d, percentile=68.3, lowlim=None, uplim=None):
    """[mean, upper - mean, mean - lower] as _parcen_internal forms it (results.py:314-369)."""
    return SR.parcen(col1d, percentile, lowlim, uplim)[0]
