#!/usr/bin/env python3
"""Command-line fit: photometry file in, chain out.

A compact harness with the reference CLI's main flags and defaults
(reference mbb_emcee/run_mbb_emcee.py:66-193: 250 walkers, 50 burn-in and 250
main steps, initial values (10, 2, 2500, 4, 40) with scatter (2, 0.2, 100, 0.3,
5)).  The reference's results object / HDF5 output and the cosmology-dependent
quantities are out of scope: the chain is written as a NumPy .npz.

    python -m mbb_emcee_amd.run_mbb_emcee phot.txt out.npz --opthin -v
"""
from __future__ import print_function

import argparse

import numpy as np

from . import mbb_fitter, postprocess

NAMES = ["T", "Beta", "Lambda0", "Alpha", "Fnorm"]


def build_parser():
    p = argparse.ArgumentParser(description="Fit a modified blackbody to photometry with an "
                                            "ensemble MCMC running on an MI355X.")
    p.add_argument("photfile", help="text file: wavelength [um] (or passband name with "
                                    "--response), flux [mJy], uncertainty [mJy]")
    p.add_argument("outfile", help="output .npz")
    p.add_argument("-b", "--burn", type=int, default=50)
    p.add_argument("-n", "--nwalkers", type=int, default=250)
    p.add_argument("-N", "--nsteps", type=int, default=250)
    p.add_argument("--noalpha", action="store_true")
    p.add_argument("--opthin", action="store_true")
    p.add_argument("-r", "--response", action="store_true")
    p.add_argument("--responsefile", default=None)
    p.add_argument("--responsedir", default=None)
    p.add_argument("-w", "--wavenorm", type=float, default=500.0)
    p.add_argument("-t", "--threads", type=int, default=1, help="accepted and ignored")
    p.add_argument("--sampler", choices=["device", "native"], default="device")
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--get_peaklambda", action="store_true")
    p.add_argument("--summary", action="store_true",
                   help="summarise the chain on the device (means, 68.3%% and 95.4%% intervals, covariance, best fit; "
                        "with --get_peaklambda the peak wavelength too): printed, and added to the .npz")
    p.add_argument("--convergence", action="store_true",
                   help="diagnose the chain on the device (autocorrelation time, effective sample size, split R-hat "
                        "per parameter; needs --sampler device): printed, and added to the .npz as convergence_*")
    p.add_argument("--marginals", type=int, default=0, metavar="NBINS",
                   help="bin the chain on the device (a histogram of NBINS bins per parameter, with --get_peaklambda of "
                        "the peak wavelength too; needs --sampler device): printed, and added to the .npz as marginals_*")
    p.add_argument("--marginals2d", type=int, default=0, metavar="NBINS2",
                   help="with --marginals: also the 2-d histograms of all pairs of columns, NBINS2 bins per axis")
    p.add_argument("--predict", default=None, metavar="SPEC[,SPEC...]",
                   help="predict fluxes from the chain on the device: each SPEC a wavelength in um or, with --response, "
                        "the name of a passband of the wheel (needs --sampler device): mean and 68.3%% interval printed, "
                        "and added to the .npz as predict_*")
    p.add_argument("--goodness", action="store_true",
                   help="goodness of fit from the chain on the device (needs --sampler device): chisq of every entry "
                        "against the data, the posterior predictive p-value, DIC and the maximum-likelihood entry "
                        "printed, and added to the .npz as goodness_*")
    p.add_argument("--loo", action="store_true",
                   help="WAIC and PSIS leave-one-band-out cross-validation from the chain on the device (needs --sampler "
                        "device): elpd_loo, the Pareto k-hat and the LOO-PIT of every band printed, and added to the "
                        ".npz as loo_*")
    p.add_argument("--evidence", type=int, nargs="?", const=-1, default=None, metavar="N2",
                   help="the evidence ln Z of the fit, bridge-sampled from the chain on the device with N2 proposal draws "
                        "(default: as many as posterior samples; needs --sampler device): printed, and added to the "
                        ".npz as evidence_*")
    p.add_argument("--reweight-prior", dest="reweight_prior", nargs=3, action="append", default=None,
                   metavar=("NAME", "MEAN", "SIGMA"),
                   help="reweight the chain on the device under the same fit with a Gaussian prior MEAN, SIGMA on parameter "
                        "NAME set in addition (repeatable; needs --sampler device): Pareto k-hat, effective sample size, "
                        "ln(Z_target / Z_run) and the weighted means and intervals printed, and added to the .npz as "
                        "reweight_*")
    p.add_argument("--map-init", dest="map_init", type=int, nargs="?", const=8, default=0, metavar="NSTART",
                   help="find the maximum of the posterior on the device first, from NSTART (default 8) points of the "
                        "initial ball: the optimum with its Laplace errors is printed and added to the .npz as map_*, and "
                        "the walkers start from a ball around it no wider than the Laplace errors")
    p.add_argument("--draws", type=int, default=0, metavar="N",
                   help="draw N cells of the chain on the device (parameters, lnprob, walker and step; with "
                        "--get_peaklambda the peak wavelength too; needs --sampler device): printed, and added to the "
                        ".npz as draws_*")
    p.add_argument("-v", "--verbose", action="store_true")
    for nm, dflt in zip(NAMES, (10.0, 2.0, 2500.0, 4.0, 40.0)):
        p.add_argument("--init" + nm, type=float, default=dflt)
        p.add_argument("--fix" + nm, action="store_true")
        p.add_argument("--low" + nm, type=float, default=None)
        p.add_argument("--up" + nm, type=float, default=None)
        p.add_argument("--prior" + nm, type=float, nargs=2, default=None, metavar=("MEAN", "SIGMA"))
    p.add_argument("--upLambdaPeak", type=float, default=None)
    p.add_argument("--priorLambdaPeak", type=float, nargs=2, default=None)
    return p


def parse_predict(text):
    """--predict's list: what reads as a number is a wavelength in um, anything else a passband name."""
    specs = []
    for tok in (t.strip() for t in text.split(",")):
        if not tok:
            raise ValueError("--predict: empty spec in {!r}".format(text))
        try:
            specs.append(float(tok))
        except ValueError:
            specs.append(tok)
    return specs


def make_fitter(a, more_priors=()):
    """The fitter the arguments describe, with the Gaussian priors (name, mean, sigma) of more_priors set in addition."""
    fit = mbb_fitter(nwalkers=a.nwalkers, photfile=a.photfile, wavenorm=a.wavenorm,
                     noalpha=a.noalpha, opthin=a.opthin, nthreads=a.threads, response=a.response,
                     responsefile=a.responsefile, responsedir=a.responsedir, sampler=a.sampler,
                     seed=a.seed)
    unused = {"Lambda0": a.opthin, "Alpha": a.noalpha}
    for nm in NAMES:                                  # run_mbb_emcee.py:226-283
        if getattr(a, "fix" + nm) or (nm == "Alpha" and a.noalpha):
            fit.fix_param(nm.lower())
        if unused.get(nm):
            continue
        if getattr(a, "low" + nm) is not None:
            fit.set_lowlim(nm.lower(), getattr(a, "low" + nm))
        if getattr(a, "up" + nm) is not None:
            fit.set_uplim(nm.lower(), getattr(a, "up" + nm))
        pr = getattr(a, "prior" + nm)
        if pr is not None:
            fit.set_gaussian_prior(nm.lower(), pr[0], pr[1])
    if a.upLambdaPeak is not None:
        fit.set_uplim("lambda_peak", a.upLambdaPeak)
    if a.priorLambdaPeak is not None:
        fit.set_gaussian_prior("lambda_peak", a.priorLambdaPeak[0], a.priorLambdaPeak[1])
    for nm, mean, sigma in more_priors:
        fit.set_gaussian_prior(nm.lower(), mean, sigma)
    return fit


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.nwalkers <= 0:
        raise ValueError("Invalid (non-positive) nwalkers: %d" % a.nwalkers)
    fit = make_fitter(a)
    target = None
    if a.reweight_prior:
        target = make_fitter(a, [(nm, float(mean), float(sigma)) for nm, mean, sigma in a.reweight_prior])

    p0init = np.array([getattr(a, "init" + nm) for nm in NAMES])
    initsigma = np.array([2, 0.2, 100, 0.3, 5.0])
    mapfit = None
    if a.map_init:
        mapfit = fit.find_map(p0init, initsigma, nstart=a.map_init)
        print(mapfit)
        p0 = fit.map_initial_values(mapfit, initsigma)
    else:
        p0 = fit.generate_initial_values(p0init, initsigma)   # :285-291
    summary = None
    if a.summary:
        summary = dict(percentile=(68.3, 95.4), derived=("peaklambda",) if a.get_peaklambda else ())
    extra = dict(convergence=True) if a.convergence else {}
    if a.marginals2d and not a.marginals:
        raise ValueError("--marginals2d needs --marginals")
    if a.marginals:
        extra["marginals"] = dict(bins=a.marginals, bins2d=a.marginals2d, pairs="all",
                                  derived=("peaklambda",) if a.get_peaklambda else ())
    if a.predict:
        extra["predict"] = parse_predict(a.predict)
    if a.goodness:
        extra["goodness"] = True
    if a.loo:
        extra["loo"] = True
    if a.evidence is not None:
        extra["evidence"] = dict(n2=None if a.evidence < 0 else a.evidence)
    if target is not None:
        extra["reweight"] = dict(target=target, percentile=(68.3, 95.4),
                                 derived=("peaklambda",) if a.get_peaklambda else ())
    if a.draws:
        extra["draws"] = dict(n=a.draws, derived=("peaklambda",) if a.get_peaklambda else ())
    fit.run(a.burn, a.nsteps, p0, verbose=a.verbose, summary=summary, **extra)
    chain, lnp = fit.sampler.chain, fit.sampler.lnprobability
    out = dict(chain=chain, lnprobability=lnp, acceptance_fraction=fit.sampler.acceptance_fraction,
               parnames=np.array(NAMES), noalpha=a.noalpha, opthin=a.opthin, wavenorm=a.wavenorm,
               data_wave=fit.like.data_wave, data_flux=fit.like.data_flux,
               data_flux_unc=fit.like.data_flux_unc)
    if mapfit is not None:
        out.update(mapfit.arrays())
    if a.get_peaklambda:
        out["peaklambda"] = postprocess.peak_wavelength(fit.like, chain)
    if a.summary:
        out.update(fit.summary.arrays())
        print(fit.summary)
    if a.convergence:
        out.update(fit.convergence.arrays())
        print(fit.convergence)
    if a.marginals:
        out.update(fit.marginals.arrays())
        print(fit.marginals)
    if a.predict:
        out.update(fit.predictions.arrays())
        print(fit.predictions)
    if a.goodness:
        out.update(fit.goodness.arrays())
        print(fit.goodness)
    if a.loo:
        out.update(fit.loo.arrays())
        print(fit.loo)
    if a.evidence is not None:
        out.update(fit.evidence.arrays())
        print(fit.evidence)
    if target is not None:
        out.update(fit.reweight.arrays())
        print(fit.reweight)
    if a.draws:
        out.update(fit.draws.arrays())
        print(fit.draws)
    np.savez_compressed(a.outfile, **out)
    if a.verbose:
        flat = chain.reshape(-1, 5)
        print("Fit results (median, +/- 68.3%):")
        for i, nm in enumerate(NAMES):
            if (i == 2 and a.opthin) or (i == 3 and a.noalpha):
                continue
            lo, med, hi = np.percentile(flat[:, i], [15.85, 50.0, 84.15])
            print("  {:8s} {:10.4g} +{:.3g} -{:.3g}".format(nm, med, hi - med, med - lo))
        best = np.unravel_index(np.argmax(lnp), lnp.shape)
        print("  best lnP {:.3f} at".format(lnp[best]), chain[best])
        print("Saved", a.outfile)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
