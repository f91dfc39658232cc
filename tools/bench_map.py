"""Measures the MAP fit (optimize.map_fit, csrc/mbb_map.hip.h) at the catalogue shape of bench.py's cfg5: 1000 sources
through the fit's eight bands, eight starts per source.

    python tools/bench_map.py [--sources 1000] [--nstart 8] [--host-sources 16] [--burnin] [--out profiles/r22/map.json]
    python tools/bench_map.py --save cat.npz ; python tools/bench_map.py --host-from cat.npz --host-threads 16

The second form is the host way in full: the first run saves the catalogue, the starts and the device's optima, the second
(no GPU needed) runs scipy on every source in --host-threads processes and reports its wall time and the gaps.

1. against the host way: wall time of map_fit (best of five), bytes back, and scipy.optimize.least_squares on the oracle's
   residuals for --host-sources of the same sources and starts (one thread; the figure for all sources is that times
   sources / host-sources -- divide by the threads you have), with the gap between the two optima;
2. --burnin: against the burn-in it replaces -- the median split R-hat of a 250-step main chain after nburn in
   {25, 50, 100, 250} steps from the one shared ball and from map_initial_values, the price of a step re-measured in the
   same process, and the price of the MAP call in steps.
Kernel time comes from a `rocprofv3 --kernel-trace --stats -- python tools/bench_map.py` run of its own."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BANDS = ["PACS_70um", "PACS_100um", "PACS_160um", "SPIRE_250um", "SPIRE_350um", "SPIRE_500um", "SCUBA2_850um",
         "Bolocam_1.1mm"]
TRUTH = np.array([12.0, 1.8, 150.0, 3.0, 40.0])


def catalogue(nsrc, seed=5):
    """nsrc thin-with-alpha sources: T, beta, alpha scattered by factors, fnorm over three decades"""
    import mbb_emcee_amd as mbb
    rng = np.random.default_rng(seed)
    truth = np.tile(TRUTH, (nsrc, 1))
    truth[:, 0] *= np.exp(rng.normal(0, 0.25, nsrc))
    truth[:, 1] *= 1.0 + 0.15 * rng.uniform(-1, 1, nsrc)
    truth[:, 3] *= 1.0 + 0.15 * rng.uniform(-1, 1, nsrc)
    truth[:, 4] *= 10.0 ** rng.uniform(-1, 2, nsrc)
    like = mbb.likelihood(response=True, opthin=True, device=0)
    like.set_phot(BANDS, np.ones(8), np.ones(8))
    m = like.model_flux(truth)
    unc = 0.05 * m + 0.005 * m.max(axis=1, keepdims=True)
    like.set_phot_multi(BANDS, m + unc * rng.standard_normal(m.shape), unc)
    return like, truth


def _host_one(args):
    """scipy.optimize.least_squares on the oracle's residuals from every start of one source: (best lnP, lnP of the
    device's optimum), both by the oracle"""
    flux, ivar, starts, params, has_uplim, uplim, bands = args
    import _map_ref as MR
    from oracle import oracle as O
    s = MR.settings("thin_walpha", 5)
    s["has_uplim"], s["uplim"] = has_uplim, uplim
    orc = O.OracleLikelihood(flux, 1.0 / np.sqrt(ivar), bands=bands, opthin=True, has_uplim=has_uplim, uplim=uplim)
    best = max(MR.ref_search(O, orc, s, x0)[1] for x0 in starts)
    return best, float(orc(params)[0])


def host_way(a):
    import multiprocessing
    import mbb_emcee_amd as mbb
    from oracle import oracle as O
    O.build()
    c = np.load(a.host_from)
    like = mbb.likelihood(response=True, opthin=True)
    like.set_phot(BANDS, np.ones(8), np.ones(8))                      # (the band tables only: no device is touched)
    bands = [(r.wavelength, r._sedmult, r._normfac) for r in like._responses]
    n = c["flux"].shape[0]
    jobs = [(c["flux"][k], c["ivar"][k], c["starts"][k], c["params"][k], c["has_uplim"], c["uplim"], bands) for k in range(n)]
    t0 = time.perf_counter()
    with multiprocessing.Pool(a.host_threads) as pool:
        res = pool.map(_host_one, jobs, chunksize=4)
    wall = time.perf_counter() - t0
    best, dev = np.array(res).T
    gap = (best - dev) / np.maximum(1.0, np.abs(best))
    out = {"sources": n, "nstart": int(c["starts"].shape[1]), "processes": a.host_threads, "wall_s": wall,
           "gap_over_max1_lnp": {"max": float(gap.max()), "min": float(gap.min()), "median": float(np.median(gap))},
           "sources_where_the_device_is_worse_by_more_than_1e-10": int((gap > 1e-10).sum()),
           "sources_where_scipy_is_worse_by_more_than_1e-10": int((gap < -1e-10).sum())}
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--nstart", type=int, default=8)
    ap.add_argument("--host-sources", type=int, default=16)
    ap.add_argument("--burnin", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--save", default=None, help="save the catalogue, the starts and the device's optima for --host-from")
    ap.add_argument("--host-from", default=None, help="the host way on a saved catalogue: no GPU is touched")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--lib", default=None, help="another build of the library (an A/B of the kernel's workgroup size)")
    a = ap.parse_args()
    if a.lib:
        from mbb_emcee_amd import _native
        _native.LIB_PATH = os.path.abspath(a.lib)
    if a.host_from:
        return host_way(a)
    import mbb_emcee_amd as mbb
    from mbb_emcee_amd import optimize
    like, truth = catalogue(a.sources)
    rng = np.random.default_rng(9)
    starts = truth[:, None, :] * (1.0 + 0.25 * rng.uniform(-1, 1, (a.sources, a.nstart, 5)))
    starts = np.maximum(starts, like._lowlim)
    optimize.map_fit(like, starts)                     # (first call: buffers, module load)
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        mf = optimize.map_fit(like, starts)
        walls.append(time.perf_counter() - t0)
    raw = mf._raw
    back = sum(x.nbytes for x in (raw.params, raw.lnprob, raw.chisq, raw.q, raw.model_flux, raw.cov, raw.niter, raw.nfev,
                                  raw.start_index, raw.status, raw.lnprob_all, raw.params_all, raw.status_all))
    res = {"shape": {"sources": a.sources, "bands": 8, "nstart": a.nstart, "model": "thin with alpha"},
           "map_fit_wall_s": {"best": min(walls), "all": walls}, "bytes_back": int(back),
           "niter_median": float(np.median(mf.niter)), "nfev_median": float(np.median(mf.nfev)),
           "status_counts": {n: int(sum(n in s for s in mf.status_names())) for n in
                             ("CONVERGED_F", "CONVERGED_X", "MAXITER", "START_INVALID", "COV_SINGULAR")}}
    if a.save:
        np.savez(a.save, flux=like._flux_multi, ivar=like._ivar_multi, starts=starts, params=mf.params, lnprob=mf.lnprob,
                 has_uplim=np.array([int(b) for b in like._has_uplim]), uplim=np.array(like._uplim))
    print("map_fit: %d sources x %d starts in %.4f s (best of 5), %d bytes back, median %g iterations"
          % (a.sources, a.nstart, min(walls), back, np.median(mf.niter)), flush=True)
    if a.host_sources > 0:
        try:
            import _map_ref as MR
            from oracle import oracle as O
            O.build()
            n = min(a.host_sources, a.sources)
            s = MR.settings("thin_walpha", 5)
            s["has_uplim"], s["uplim"] = np.array([int(b) for b in like._has_uplim]), np.array(like._uplim)
            bands = [(r.wavelength, r._sedmult, r._normfac) for r in like._responses]
            t0, gaps = time.perf_counter(), []
            for k in range(n):
                orc = O.OracleLikelihood(like._flux_multi[k], 1.0 / np.sqrt(like._ivar_multi[k]), bands=bands, opthin=True,
                                         has_uplim=s["has_uplim"], uplim=s["uplim"])
                best = max(MR.ref_search(O, orc, s, x0)[1] for x0 in starts[k])
                gaps.append((best - orc(mf.params[k])[0]) / max(1.0, abs(best)))
            host = time.perf_counter() - t0
            res["host_scipy"] = {"sources": n, "wall_s_one_thread": host, "extrapolated_all_sources_one_thread_s":
                                 host * a.sources / n, "gap_over_max1_lnp": {"max": float(np.max(gaps)), "min": float(np.min(gaps))}}
            print("scipy on the oracle: %d sources in %.2f s on one thread (%.1f s for all); gap max %.2e min %.2e"
                  % (n, host, host * a.sources / n, np.max(gaps), np.min(gaps)), flush=True)
        except ImportError as e:
            res["host_scipy"] = {"error": str(e)}
    if a.burnin:
        fit = mbb.mbb_fitter(nwalkers=250, response=True, opthin=True, seed=1)
        fit.like = like
        fit.sampler = mbb.DeviceEnsembleSampler(250, 5, like, seed=1)
        initsigma = np.array([2, 0.2, 0.0, 0.3, 5.0])
        fit.fix_param("lambda0")
        shared = np.broadcast_to(fit.generate_initial_values(TRUTH, initsigma), (a.sources, 250, 5)).copy()
        mapped = fit.map_initial_values(mf, initsigma)
        fit.run(25, 250, mapped)                       # (the first run: the sampler's set-up, not timed)
        t0 = time.perf_counter()
        fit.run(25, 250, mapped)
        step_s = (time.perf_counter() - t0) / 275
        out = {}
        for tag, p0 in (("shared_ball", shared), ("map_initial_values", mapped)):
            out[tag] = {}
            for nburn in (25, 50, 100, 250):
                fit.run(nburn, 250, p0, convergence=True)
                out[tag][str(nburn)] = float(np.nanmedian(fit.convergence.rhat[:, [0, 1, 3, 4]]))
        res["burnin"] = {"median_split_rhat": out, "step_s": step_s, "map_fit_in_steps": min(walls) / step_s}
        print(json.dumps(res["burnin"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
