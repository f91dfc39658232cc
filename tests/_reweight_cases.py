"""What the reweighting tests share (tests/test_reweight_cpu.py, tests/test_reweight_gpu.py): the run's likelihood and
the targets of every case, the chains (tests/_loo_cases._chain's, rows of the fixture chains), and the restatement of a
whole call from the device's own per-entry arrays.  tests/test_reweight_cpu.py chooses nothing: it asserts, with the
oracle alone, that the inputs named here are what the GPU file takes them for."""
import numpy as np

import _loo_ref as LR
import _reweight_ref as RR
from _loo_cases import _chain, _data

LD = LR.LD
RUN = ("thick_walpha", False, False)           # the run's model: name in tests/golden/results.npz, opthin, noalpha
CASE = "bands4"
PRIOR_MEAN = 3.0                                # the target's Gaussian prior on beta, beyond the chain's largest (2.52)
WIDTHS = {"low": 1.0, "mid": 0.28, "high": 0.2}  # ... at three widths: k-hat < 0.5, in [0.5, 0.7], > 0.7 on the S = 512 chain
T_LIMIT = 14.0                                  # the limit case: the target's lower limit on T, near the chain's median
T_LIMIT_ALL = 25.0                              # ... and above every entry (the chain's largest T is 20.1)
CAP = 1864135

# label -> ([1, nw, nsteps] of the chain, _chain's seed, (prior mean, sigma) or None for the identity, the class planned)
PSIS = {
    "S 20": ((1, 5, 4), 4, (3.0, 0.2), "short"),
    "S 21": ((1, 7, 3), 3, (4.0, 0.2), "mid"),
    "S 35": ((1, 7, 5), 5, (3.0, 0.3), "low"),
    "S 455": ((1, 5, 91), 91, (3.0, 0.2), "high"),
    "S 456": ((1, 8, 57), 57, (3.0, 0.5), "low"),
    "S 512 low": ((1, 8, 64), 64, (PRIOR_MEAN, WIDTHS["low"]), "low"),
    "S 512 mid": ((1, 8, 64), 64, (PRIOR_MEAN, WIDTHS["mid"]), "mid"),
    "S 512 high": ((1, 8, 64), 64, (PRIOR_MEAN, WIDTHS["high"]), "high"),
    "S 512 identity": ((1, 8, 64), 64, None, "flat"),
    "S 7283": ((1, 1, 7283), 7283, (3.0, 0.2), "high"),
    "S 16384": ((1, 128, 128), 128, (4.0, 0.2), "high"),
    "S 16385": ((1, 113, 145), 145, (4.0, 0.3), "high"),
}


def klass(sc):
    """The class of a _reweight_ref.scalars() result: short, flat, low, mid or high"""
    if sc["why"] == LR.FIT_SHORT:
        return "short"
    if sc["why"] == LR.FIT_FLAT:
        return "flat"
    k = float(sc["khat"])
    return "low" if k < 0.5 else ("mid" if k <= 0.7 else "high")


def chain_of(g_res, label):
    shape, seed = PSIS[label][:2]
    return _chain(g_res, RUN[0], shape, seed=seed)


def data_of(oracle, g_lnl, g_pb, g_res, case=CASE):
    """_loo_cases._data of the run's model: (oracle band keywords, set_phot's first argument, flux, unc, cov)"""
    return _data(oracle, g_lnl, g_pb, g_res[RUN[0] + "/chain"], RUN[1], RUN[2], case, 1.0)


def oracle_like(oracle, data, prior=None, t_limit=None, opthin=RUN[1], noalpha=RUN[2]):
    """The oracle's likelihood on _data's photometry with the reference's default limits, a Gaussian prior (mean, sigma)
    on beta and / or a lower limit on T besides."""
    okw, first, flux, unc, cov = data
    kw = dict(opthin=opthin, noalpha=noalpha)
    if prior is not None:
        kw.update(has_gprior=[0, 1, 0, 0, 0, 0], gprior_mean=[0, prior[0], 0, 0, 0, 0], gprior_sigma=[1, prior[1], 1, 1, 1, 1])
    if t_limit is not None:
        kw.update(lowlim=[t_limit, 0.1, 1, 0.1, 1e-3])
    return oracle.OracleLikelihood(flux, unc, cov=cov, **okw, **kw)


def device_like(mbb, data, prior=None, t_limit=None, opthin=RUN[1], noalpha=RUN[2], keep=None, multi=None):
    """A likelihood of this package on _data's photometry (a new object every time: limits and priors are set on it);
    keep: the bands kept, as indices; multi: scales, one source each."""
    okw, first, flux, unc, cov = data
    like = mbb.likelihood(response="bands" in okw, opthin=opthin, noalpha=noalpha)
    idx = list(range(len(first))) if keep is None else list(keep)
    first, flux, unc = [first[i] for i in idx], flux[idx], unc[idx]
    if multi is not None:
        like.set_phot_multi(first, np.array([flux * s for s in multi]), np.array([unc * s for s in multi]))
    else:
        like.set_phot(first, flux, unc)
        if cov is not None:
            like.set_cov(cov[np.ix_(idx, idx)])
    if prior is not None:
        like.set_gaussian_prior("beta", prior[0], prior[1])
    if t_limit is not None:
        like.set_lowlim("t", t_limit)
    return like


def restate(lp, res, src, dtype=LD, smooth=True):
    """_reweight_ref.scalars of source src of a kept device result (its own log_ratio), the counts and the masks:
    (scalars dict, used, zero, left out)."""
    raw = res._raw
    used, zero, left = RR.classes(np.asarray(lp).ravel(), raw.target_lnprob[src])
    sc = RR.scalars(raw.log_ratio[src][used], int(zero.sum()), dtype=dtype, smooth=smooth)
    return sc, used, zero, left


def device_scalars(res, src, used):
    raw = res._raw
    return dict(lw=raw.log_weight[src][used], khat=raw.khat[src], ess=raw.ess[src], lnz_ratio=raw.lnz_ratio[src])


def check_quantiles(res, src, columns, slots, label=""):
    """Every weighted quantile of source src against the integer restatement from the device's own weights: exact.
    columns [n, 8] (NaN where not asked for), slots the column slots to check."""
    raw = res._raw
    u = raw.weight[src]
    for slot in slots:
        x = columns[:, slot]
        for k, q in enumerate(res.qs):
            want = RR.wquantile(x, u, q)
            got = raw.pct[src, slot, k]
            assert got == want or (np.isnan(got) and np.isnan(want)), (label, src, slot, q, got, want)
