#!/usr/bin/env python3
"""The evidence's time on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands):

  (e) run_mcmc(storechain=False, summary=...), then sampler.evidence(): proposal fit, N2 = N1 = 31 250 draws per source,
      their likelihood, the whole bridge iteration and neff from the device diagnostics, nothing but the results back;
  (h) the host way: run_mcmc with the chain stored and brought back, then per source the reference implementation
      (tests/_evidence_ref.py: moments and lnq in numpy, the longdouble bridge) on 16 threads at most, the proposal draws
      by numpy and their lnprob by like() in slabs of sources.

In one process, warmed up; (e) `--runs` times (default nine) alternated with (h) while `--host-runs` (default three: it
takes many times as long) last; walls with their spread and the bytes each way brings back, as one JSON object
(profiles/r23/evidence.json), rewritten after every run.  Both ways work on the same chain (same seed); the host's
draws are numpy's, so the two lnz differ by their errors: the largest difference in units of the combined error is
reported.  `--only-device` runs (e) twice, for a kernel trace of its own; `--shape NS NW NSTEPS` rehearses at another size."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mbb_emcee_amd as mbb                    # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
SLAB = 8                                       # sources per like() call of way (h)


def arg(name, default, n=1):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    vals = sys.argv[i + 1:i + 1 + n]
    return vals[0] if n == 1 else vals


def main():
    ns, nw, nsteps = [int(v) for v in arg("--shape", (1000, 250, 250), 3)]
    runs, host_runs = int(arg("--runs", 9)), int(arg("--host-runs", 3))
    out_path = arg("--out", None)
    like, _, p0 = setup(ns, nw)
    free = [i for i in range(5) if not (i == 2 and like.opthin) and not (i == 3 and like.noalpha)]

    def way_e():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        e = s.evidence()
        t2 = time.perf_counter()
        r = s.summary._raw
        nbytes = sum(getattr(r, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best", "best_index"))
        nbytes += sum(v.nbytes for v in vars(e._raw).values() if isinstance(v, np.ndarray))
        return t2 - t0, t1 - t0, t2 - t1, e, nbytes

    def way_h():
        import _evidence_ref as ER
        import _diag_ref as DR
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        chain, lp = s.chain, s.lnprobability
        fit, post = ER.window(nsteps)
        n1 = nw * len(post)
        lnz, err = np.full(ns, np.nan), np.full(ns, np.nan)
        rng = np.random.default_rng(5)

        def prepare(g):
            x = chain[g][:, fit].reshape(-1, 5)
            mu = x.mean(axis=0)
            L = np.linalg.cholesky(np.cov(x[:, free].T))
            prop = np.tile(mu, (n1, 1))
            prop[:, free] += rng.standard_normal((n1, len(free))) @ L.T
            return mu, L, prop

        def finish(args):
            g, mu, L, prop, lnp = args
            xp = chain[g][:, post].reshape(-1, 5)
            l1 = lp[g][:, post].reshape(-1) - ER.lnq(xp, mu, L, free, np.float64)
            with np.errstate(invalid="ignore"):
                l2 = lnp - ER.lnq(prop, mu, L, free, np.float64)
            ess = DR.diagnostics_ref(chain[g][:, post], 0)["ess"][free]
            r = ER.ref_bridge(l1, l2, neff=np.nanmin(ess) if np.isfinite(ess).any() else None, tol=1e-10)
            lnz[g], err[g] = r["lnz"], r["err"]
        with ThreadPoolExecutor(THREADS) as ex:
            for g0 in range(0, ns, SLAB):
                gs = list(range(g0, min(ns, g0 + SLAB)))
                prep = [prepare(g) for g in gs]
                # like() of a catalogue takes nsources equal blocks: the slab's sources through a likelihood of their own
                lnp = slab_lnprob(like, gs, np.array([p[2] for p in prep]))
                list(ex.map(finish, [(g, prep[k][0], prep[k][1], prep[k][2], lnp[k]) for k, g in enumerate(gs)]))
                if g0 % (25 * SLAB) == 0:
                    print("  host way: source %d of %d" % (g0, ns), flush=True)
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, t2 - t1, (lnz, err), chain.nbytes + lp.nbytes

    if "--only-device" in sys.argv:
        way_e(); way_e()
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps}, "host_threads": THREADS, "runs_asked": runs,
           "host_runs_asked": host_runs, "n1": nw * (nsteps - nsteps // 2), "n2": nw * (nsteps - nsteps // 2)}
    we = way_e()
    out["warmup_wall_s"] = {"e": we[0]}
    print("warm-up: e %.2f s (evidence %.3f s)" % (we[0], we[2]), flush=True)
    e, h, res = [], [], {}

    def write():
        for k, rows, part in (("e_device_evidence", e, "evidence_s"), ("h_stored_chain_reference_on_the_host", h, "host_s")):
            if rows:
                w = [x[0] for x in rows]
                res.setdefault(k, {}).update({"wall_s": w, "run_mcmc_s": [x[1] for x in rows], part: [x[2] for x in rows],
                                              "median_s": float(np.median(w)), "spread_s": float(max(w) - min(w)),
                                              part.replace("_s", "_median_s"): float(np.median([x[2] for x in rows]))})
        out["runs_done"], out["host_runs_done"], out["results"] = len(e), len(h), res
        if out_path:
            with open(out_path + ".tmp", "w") as fh:
                json.dump(out, fh, indent=1)
            os.replace(out_path + ".tmp", out_path)

    for i in range(runs):
        re_ = way_e()
        e.append(re_[:3])
        ev = re_[3]
        res.setdefault("e_device_evidence", {}).update(
            bytes_back=int(re_[4]), converged=int(np.sum(ev.status & 1 != 0)), niter_max=int(ev.niter.max()),
            lnz_err_median=float(np.nanmedian(ev.lnz_err)), lnz_err_max=float(np.nanmax(ev.lnz_err)),
            neff_median=float(np.median(ev.neff)))
        print("run %d: e %.3f s (evidence %.3f)" % (len(e), re_[0], re_[2]), flush=True)
        if i < host_runs:
            rh = way_h()
            h.append(rh[:3])
            lnz, err = rh[3]
            res.setdefault("h_stored_chain_reference_on_the_host", {})["bytes_back"] = int(rh[4])
            res["max_lnz_difference_in_combined_errors"] = float(np.nanmax(np.abs(lnz - ev.lnz) / np.hypot(err, ev.lnz_err)))
            print("host %d: %.2f s (reference %.2f)" % (len(h), rh[0], rh[2]), flush=True)
        write()
    print(json.dumps(out))


_SLAB_LIKE = {}


def slab_lnprob(like, gs, rows):
    """lnprob [len(gs), n] of rows [len(gs), n, 5], source g's rows against source g's data"""
    key = len(gs)
    flux, ivar = np.asarray(like._flux_multi)[gs], np.asarray(like._ivar_multi)[gs]
    if key not in _SLAB_LIKE:
        from bench import BANDS
        lk = mbb.likelihood(response=True, opthin=like.opthin, noalpha=like.noalpha, wavenorm=like.wavenorm)
        _SLAB_LIKE[key] = (lk, list(BANDS))
    lk, bands = _SLAB_LIKE[key]
    lk.set_phot_multi(bands, flux, 1.0 / np.sqrt(ivar))
    for i in range(5):
        lk.set_lowlim(i, like._lowlim[i])
    for i in range(6):
        if like._has_uplim[i]:
            lk.set_uplim(i, like._uplim[i])
        if like._has_gprior[i]:
            lk.set_gaussian_prior(i, like._gprior_mean[i], like._gprior_sigma[i])
    return lk(rows.reshape(-1, 5)).reshape(len(gs), -1)


if __name__ == "__main__":
    main()
