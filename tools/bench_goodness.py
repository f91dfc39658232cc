#!/usr/bin/env python3
"""The goodness of fit's time on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands):

  (g) run_mcmc(storechain=False, summary=...), then sampler.goodness();
  (p) the same run, then sampler.predictions(the fit's own eight bands): the same band sums without the chisq, the
      cost the goodness of fit has to stay at or under;
  (h) the host way: run_mcmc with the chain stored, like.model_flux of every chain entry (in slabs of sources), chisq
      and scipy.special.gammaincc per entry and numpy's mean and percentiles per source (16 threads at most).

In one process, warmed up; (g) and (p) alternated `--runs` times each (default nine), (h) `--host-runs` times (default
two: it takes twenty times as long); walls with their spread and the bytes each way brings back, as one JSON object
(profiles/r21/goodness.json), rewritten after every pair so that a run cut short leaves what it measured.  All ways work
on the same chain (same seed) and their numbers are compared.  `--only-device` runs (g) twice, for a kernel trace of
its own; `--shape NS NW NSTEPS` rehearses at another size."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbb_emcee_amd as mbb                    # noqa: E402
from bench import BANDS                        # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
QS = [15.85, 84.15]
SLAB = 40                                      # sources per like.model_flux call of way (h)


def arg(name, default, n=1):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    vals = sys.argv[i + 1:i + 1 + n]
    return vals[0] if n == 1 else vals


def main():
    ns, nw, nsteps = [int(v) for v in arg("--shape", (1000, 250, 250), 3)]
    runs, host_runs = int(arg("--runs", 9)), int(arg("--host-runs", 2))
    out_path = arg("--out", None)
    like, _, p0 = setup(ns, nw)
    nb = len(BANDS)
    flux, ivar = np.asarray(like._flux_multi), np.asarray(like._ivar_multi)

    def summary_bytes(s):
        r = s.summary._raw
        return sum(getattr(r, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best", "best_index"))

    def way_g():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        g = s.goodness(percentile=68.3)
        t2 = time.perf_counter()
        nbytes = summary_bytes(s) + sum(v.nbytes for v in vars(g._raw).values())
        return t2 - t0, t1 - t0, t2 - t1, g._raw, nbytes

    def way_p():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        p = s.predictions(list(BANDS), percentile=68.3, keep=False)
        t2 = time.perf_counter()
        nbytes = summary_bytes(s) + sum(getattr(p._raw, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status"))
        return t2 - t0, t1 - t0, t2 - t1, p._raw, nbytes

    def way_h():
        from scipy.special import gammaincc
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        chain = s.chain
        mean, pct, ppp = np.empty(ns), np.empty((ns, 2)), np.empty(ns)

        def one(args):
            g, table = args                                       # table [nw * nsteps, nb]
            r = flux[g] - table
            chi = (r * r * ivar[g]).sum(axis=1)
            mean[g], pct[g], ppp[g] = chi.mean(), np.percentile(chi, QS), gammaincc(0.5 * nb, 0.5 * chi).mean()
        with ThreadPoolExecutor(THREADS) as ex:
            for g0 in range(0, ns, SLAB):
                g1 = min(ns, g0 + SLAB)
                # (a one-source likelihood's model fluxes: the bands are the fit's, the data is not looked at)
                table = one_like.model_flux(chain[g0:g1].reshape(-1, 5)).reshape(g1 - g0, nw * nsteps, nb)
                list(ex.map(one, [(g0 + k, table[k]) for k in range(g1 - g0)]))
        t2 = time.perf_counter()
        nbytes = s.chain.nbytes + s.lnprobability.nbytes + ns * nw * nsteps * nb * 8
        return t2 - t0, t1 - t0, t2 - t1, (mean, pct, ppp), nbytes

    one_like = mbb.likelihood(response=True)
    one_like.set_phot(list(BANDS), np.ones(nb), np.ones(nb))
    for i in range(5):                                              # (the fit's lower limits would turn rows into NaN fluxes)
        one_like.set_lowlim(i, -np.inf)
    if "--only-device" in sys.argv:
        way_g(); way_g()
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": nb}, "host_threads": THREADS,
           "runs_asked": runs, "host_runs_asked": host_runs}
    wg = way_g(); wp = way_p()
    out["warmup_wall_s"] = {"g": wg[0], "p": wp[0]}
    print("warm-up: g %.2f s (goodness %.3f s), p %.2f s (predictions %.3f s)" % (wg[0], wg[2], wp[0], wp[2]), flush=True)
    g, p, h = [], [], []
    res = {}

    def write():
        for k, rows, part in (("g_device_goodness", g, "goodness_s"), ("p_device_predictions_of_the_8_bands", p, "predictions_s"),
                              ("h_stored_chain_model_flux_numpy_scipy", h, "host_s")):
            if rows:
                w = [x[0] for x in rows]
                res.setdefault(k, {}).update({"wall_s": w, "run_mcmc_s": [x[1] for x in rows], part: [x[2] for x in rows],
                                              "median_s": float(np.median(w)), "spread_s": float(max(w) - min(w)),
                                              part.replace("_s", "_median_s"): float(np.median([x[2] for x in rows]))})
        out["runs_done"], out["host_runs_done"], out["results"] = len(g), len(h), res
        if out_path:
            with open(out_path + ".tmp", "w") as fh:
                json.dump(out, fh, indent=1)
            os.replace(out_path + ".tmp", out_path)

    for _ in range(runs):
        rg = way_g(); rp = way_p()
        g.append(rg[:3]); p.append(rp[:3])
        res.setdefault("g_device_goodness", {})["bytes_back"] = int(rg[4])
        res.setdefault("p_device_predictions_of_the_8_bands", {})["bytes_back"] = int(rp[4])
        print("pair %d: g %.3f s (goodness %.3f), p %.3f s (predictions %.3f)" % (len(g), rg[0], rg[2], rp[0], rp[2]), flush=True)
        write()
    for _ in range(host_runs):
        rh = way_h()
        h.append(rh[:3])
        mean, pct, ppp = rh[3]
        res.setdefault("h_stored_chain_model_flux_numpy_scipy", {})["bytes_back"] = int(rh[4])
        raw = rg[3]
        res["max_rel_diff_mean_chisq"] = float((np.abs(mean - raw.mean[:, 0]) / np.abs(mean)).max())
        res["max_rel_diff_percentiles"] = float((np.abs(pct - raw.pct[:, 0, :2]) / np.abs(pct)).max())
        res["max_abs_diff_ppp"] = float(np.abs(ppp - raw.mean[:, 1]).max())
        print("host %d: %.2f s (model_flux, numpy and scipy %.2f)" % (len(h), rh[0], rh[2]), flush=True)
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
