#!/usr/bin/env python3
"""Golden fixtures for the chain summaries (mbb_emcee_amd/results.py) from the *reference itself*.

TEST INFRASTRUCTURE.  Runs only where the reference is mounted (see make_golden.py).  It imports
make_golden_results.py for its shims and its chain maker, rebuilds for each of the four 32 x 16 chains of
results.npz the reference's own `mbb_fitter` holding that chain, and lets the reference's `mbb_results`
(results.py) summarise it:

  par_cen         (results.py:397-431 -> _parcen_internal :314-369) for the five parameters at 68.3 and 95.4
  par_cen clipped one per variant, lower / upper / both bounds inside the chain's range; the surviving count
  par_lowlim, par_uplim (:433-493) at 68.3 and 95
  peaklambda_cen, lir_cen, dustmass_cen (:507-532, :600-625, :699-724) at 68.3
  best_fit        (:160-165) parameters, lnprob, (walker, step)

The chains repeat steps exactly (rejected moves), so ties in lnprob are the rule; `ties_at_max` records how
often each variant's maximum is attained.  So that the tie rule (the smallest flat index wins) is pinned whatever
those chains happen to hold, a case of its own is appended: `tiecase/` is the thick_walpha chain with its best
sample copied to one place before and one place behind it.

Writes only numbers to tests/golden/summary.npz (a few KB).

Usage:  python tests/golden/make_golden_summary.py [--out other.npz]      (about a minute: scipy quad per entry)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G                    # noqa: E402
import make_golden_results as R            # noqa: E402

CEN_PCT = [68.3, 95.4]
LIM_PCT = [68.3, 95.0]
VARIANTS = (("thin_walpha", True, False), ("thick_walpha", False, False),
            ("thick_noalpha", False, True), ("thin_noalpha", True, True))
# the clipped par_cen of each variant: parameter, (percentile of the column the lower bound sits at or None, upper)
CLIPS = {"thin_walpha": (0, (20.0, 85.0)), "thick_walpha": (2, (30.0, None)),
         "thick_noalpha": (1, (None, 70.0)), "thin_noalpha": (4, (10.0, 60.0))}


def round3(x):
    return float("%.3g" % x)


def main(argv):
    outpath = os.path.join(HERE, "summary.npz")
    if "--out" in argv:
        outpath = argv[argv.index("--out") + 1]
    if not os.path.isdir(G.REFPKG):
        raise SystemExit("reference not mounted at %s" % G.REF)
    g = np.load(os.path.join(HERE, "results.npz"))
    G.build_fnu()
    mb, rs, lk = G.install_shim()
    G.kat_gate(mb, rs)
    fitmod, resmod = R.install_results_shim()
    out = {"cen_percentiles": np.array(CEN_PCT), "lim_percentiles": np.array(LIM_PCT)}
    any_tie = False
    for seed, (nm, opthin, noalpha) in enumerate(VARIANTS):
        k = nm + "/"
        chain = g[k + "chain"]
        assert np.array_equal(chain, R.make_chain(20260404 + seed))          # the chains of results.npz, as made there
        fit = fitmod.mbb_fitter(nwalkers=R.NWALK, response=True, noalpha=noalpha, opthin=opthin)
        flux = g[k + "data_flux"]
        fit.like.set_phot(R.BANDS, flux, 0.1 * flux + 1.0)
        fit.sampler.chain = chain
        fit.sampler.lnprobability = g[k + "lnprobability"]
        res = resmod.mbb_results(fit=fit, redshift=R.REDSHIFT, lumdist=R.LUMDIST_MPC)
        res.compute_peaklambda()
        res.compute_lir()
        res.compute_dustmass()
        assert np.array_equal(np.asarray(res.lir, dtype=np.float64), g[k + "lir"])
        out[k + "par_cen"] = np.array([[res.par_cen(i, percentile=p) for p in CEN_PCT] for i in range(5)])
        par, (plo, phi) = CLIPS[nm]
        col = chain[:, :, par].flatten()
        lo = None if plo is None else round3(np.percentile(col, plo))
        hi = None if phi is None else round3(np.percentile(col, phi))
        keep = np.ones(col.size, dtype=bool)
        if lo is not None:
            keep &= col >= lo
        if hi is not None:
            keep &= col <= hi
        assert 0 < keep.sum() < col.size
        out[k + "clip_param"] = par
        out[k + "clip_bounds"] = np.array([np.nan if lo is None else lo, np.nan if hi is None else hi])
        out[k + "clip_n_used"] = int(keep.sum())
        out[k + "clip_par_cen"] = res.par_cen(par, percentile=68.3, lowlim=lo, uplim=hi)
        out[k + "par_lowlim"] = np.array([[res.par_lowlim(i, percentile=p) for p in LIM_PCT] for i in range(5)])
        out[k + "par_uplim"] = np.array([[res.par_uplim(i, percentile=p) for p in LIM_PCT] for i in range(5)])
        out[k + "peaklambda_cen"] = res.peaklambda_cen()
        out[k + "lir_cen"] = res.lir_cen()
        out[k + "dustmass_cen"] = res.dustmass_cen()
        bf = res.best_fit
        out[k + "best_fit_params"] = np.array(bf[0], dtype=np.float64)
        out[k + "best_fit_lnprob"] = float(bf[1])
        out[k + "best_fit_index"] = np.array(bf[2], dtype=np.int64)
        lnp = fit.sampler.lnprobability
        ties = int((lnp == lnp.max()).sum())
        out[k + "ties_at_max"] = ties
        any_tie |= ties > 1
        print("  %s: T %.3f +%.3f -%.3f; clipped n %d of %d; best lnP %.3f at %s, attained %d time(s)"
              % ((nm,) + tuple(out[k + "par_cen"][0, 0]) + (keep.sum(), col.size, bf[1], tuple(bf[2]), ties)))
        if nm == "thick_walpha":
            # the tie case: the best sample copied before and behind itself in [walker][step] order
            w, t = bf[2]
            c2, l2 = chain.copy(), np.array(lnp, copy=True)
            first = (max(int(w) - 3, 0), 5) if w > 0 else (0, 0)
            last = (min(int(w) + 2, R.NWALK - 1), 11)
            assert first < (w, t) < last
            for pos in (first, last):
                c2[pos] = chain[w, t]
                l2[pos] = lnp[w, t]
            fit.sampler.chain, fit.sampler.lnprobability = c2, l2
            res2 = resmod.mbb_results(fit=fit, redshift=R.REDSHIFT, lumdist=R.LUMDIST_MPC)
            assert tuple(res2.best_fit[2]) == first and int((l2 == l2.max()).sum()) >= 3
            out["tiecase/chain"], out["tiecase/lnprobability"] = c2, l2
            out["tiecase/best_fit_params"] = np.array(res2.best_fit[0], dtype=np.float64)
            out["tiecase/best_fit_lnprob"] = float(res2.best_fit[1])
            out["tiecase/best_fit_index"] = np.array(res2.best_fit[2], dtype=np.int64)
            out["tiecase/par_cen"] = np.array([[res2.par_cen(i, percentile=p) for p in CEN_PCT] for i in range(5)])
            any_tie = True
    assert any_tie
    np.savez_compressed(outpath, **out)
    print("  %s %d B" % (os.path.basename(outpath), os.path.getsize(outpath)))


if __name__ == "__main__":
    main(sys.argv[1:])
