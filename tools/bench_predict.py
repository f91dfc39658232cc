#!/usr/bin/env python3
"""The predictions' time on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands): predflux_cen of the fit's
eight bands and of 32 wavelengths log-spaced over 20-2000 um, 40 specs,

  (a) run_mcmc with the chain stored, then postprocess.predict_flux of every chain entry (in slabs of sources: the
      whole table of 62.5 M rows x 40 specs would be 20 GB) and numpy's mean and percentile of every (source, spec)
      column on the host (16 threads at most);
  (b) run_mcmc(storechain=False, summary=...), then sampler.predictions(specs).

In one process, warmed up, alternated, `--runs` times each (default nine); walls with their spread and the bytes each
way brings back, as one JSON object (profiles/r19/predict.json), rewritten after every pair of runs so that a run cut
short leaves what it measured.  Both ways predict from the same chain (same seed) and their numbers are compared.
`--budget-s S` stops the alternation once S seconds have gone by (the number of runs made is recorded).
`--only-device` runs (b) twice, for a kernel trace of its own (rocprofv3 --kernel-trace --stats --
python tools/bench_predict.py --only-device); `--shape NS NW NSTEPS` rehearses at another size."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbb_emcee_amd as mbb                    # noqa: E402
from mbb_emcee_amd import postprocess          # noqa: E402
from bench import BANDS                        # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
QS = [15.85, 84.15]
SLAB = 40                                      # sources per postprocess.predict_flux call of way (a)


def arg(name, default, n=1):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    vals = sys.argv[i + 1:i + 1 + n]
    return vals[0] if n == 1 else vals


def main():
    ns, nw, nsteps = [int(v) for v in arg("--shape", (1000, 250, 250), 3)]
    runs = int(arg("--runs", 9))
    out_path = arg("--out", None)
    budget = float(arg("--budget-s", 1e9))
    t_start = time.perf_counter()
    specs = list(BANDS) + [float(w) for w in np.geomspace(20.0, 2000.0, 32)]
    like, _, p0 = setup(ns, nw)

    def host_stats(chain):
        """mean and the two percentiles of every (source, spec) column: [ns, nspec], [ns, nspec, 2]"""
        mean, pct = np.empty((ns, len(specs))), np.empty((ns, len(specs), 2))

        def one(args):
            g, table = args                                       # table [nw, nsteps, nspec]
            for i in range(len(specs)):
                col = np.ascontiguousarray(table[..., i]).ravel()
                mean[g, i] = col.mean()
                pct[g, i] = np.percentile(col, QS)
        with ThreadPoolExecutor(THREADS) as ex:
            for g0 in range(0, ns, SLAB):
                table = postprocess.predict_flux(like, chain[g0:g0 + SLAB], specs)
                list(ex.map(one, [(g0 + k, table[k]) for k in range(table.shape[0])]))
        return mean, pct

    def way_a():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        mean, pct = host_stats(s.chain)
        t2 = time.perf_counter()
        # (the chain and lnprob of the run, and the flux table of every slab)
        nbytes = s.chain.nbytes + s.lnprobability.nbytes + ns * nw * nsteps * len(specs) * 8
        return t2 - t0, t1 - t0, t2 - t1, (mean, pct), nbytes

    def way_b():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        p = s.predictions(specs, percentile=68.3, keep=False)
        t2 = time.perf_counter()
        r = s.summary._raw
        nbytes = sum(getattr(r, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best",
                                                    "best_index"))
        nbytes += sum(getattr(p._raw, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status"))
        return t2 - t0, t1 - t0, t2 - t1, (p._raw.mean, p._raw.pct), nbytes

    if "--only-device" in sys.argv:
        way_b(); way_b()
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": 8}, "specs": [str(s) for s in specs],
           "host_threads": THREADS, "runs_asked": runs}
    wb = way_b()                                                   # warm-up of both
    print("warm-up: b %.2f s (predictions %.2f s)" % (wb[0], wb[2]), flush=True)
    wa = way_a()
    out["warmup_wall_s"] = {"a": wa[0], "b": wb[0]}
    print("warm-up: a %.2f s, b %.2f s (predictions %.2f s)" % (wa[0], wb[0], wb[2]), flush=True)
    a, b = [], []
    for _ in range(runs):
        if time.perf_counter() - t_start > budget:
            break
        ra = way_a(); rb = way_b()
        a.append(ra[:3]); b.append(rb[:3])
        # band columns differ per entry at the 1e-12 level (another summation order): relative difference of the results
        scale = np.abs(ra[3][0]).max(axis=0)
        res = {"a_stored_chain_predict_flux_numpy": {"wall_s": [x[0] for x in a], "run_mcmc_s": [x[1] for x in a],
                                                     "predict_flux_and_numpy_s": [x[2] for x in a], "bytes_back": int(ra[4])},
               "b_device_predictions": {"wall_s": [x[0] for x in b], "run_mcmc_summary_s": [x[1] for x in b],
                                        "predictions_s": [x[2] for x in b], "bytes_back": int(rb[4])},
               "max_rel_diff_mean": float((np.abs(ra[3][0] - rb[3][0]) / scale).max()),
               "max_rel_diff_percentiles": float((np.abs(ra[3][1] - rb[3][1]) / scale[:, None]).max())}
        for k in ("a_stored_chain_predict_flux_numpy", "b_device_predictions"):
            w = res[k]["wall_s"]
            res[k]["median_s"], res[k]["spread_s"] = float(np.median(w)), float(max(w) - min(w))
        res["b_device_predictions"]["predictions_median_s"] = float(np.median(res["b_device_predictions"]["predictions_s"]))
        res["a_stored_chain_predict_flux_numpy"]["host_median_s"] = float(
            np.median(res["a_stored_chain_predict_flux_numpy"]["predict_flux_and_numpy_s"]))
        out["runs_done"] = len(a)
        print("pair %d: a %.2f s (host %.2f), b %.2f s (predictions %.2f)" % (len(a), ra[0], ra[2], rb[0], rb[2]), flush=True)
        out["results"] = res
        if out_path:
            with open(out_path + ".tmp", "w") as fh:
                json.dump(out, fh, indent=1)
            os.replace(out_path + ".tmp", out_path)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
