#!/usr/bin/env python3
"""The chain summary's time claim on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands):

  (a) run_mcmc with the chain stored, then numpy mean + percentile of the five parameters per source on the host
      (16 threads at most): what a user had to do before the device summary existed;
  (b) run_mcmc(storechain=False, summary=...) for the same five columns.

Both in one process, warmed up, alternated, three times each; walls with their spread and the bytes each way brings
back, as one JSON object (profiles/r07/summary.json).  `--single` measures the single-source 250 x 250 case the same
way; `--only-summary` runs (b) once after a warm-up, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/bench_summary.py --only-summary)."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbb_emcee_amd as mbb                    # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

QS = [15.85, 84.15]
THREADS = min(16, os.cpu_count() or 1)


def host_summary(chain):
    """mean and the 68.3 % interval of the five parameters of every source, numpy on the host."""
    ns = chain.shape[0]
    flat = chain.reshape(ns, -1, 5)

    def one(g):
        cols = np.ascontiguousarray(flat[g].T)
        return cols.mean(axis=1), np.percentile(cols, QS, axis=1)
    with ThreadPoolExecutor(THREADS) as ex:
        res = list(ex.map(one, range(ns)))
    return np.array([r[0] for r in res]), np.array([r[1] for r in res])


def main():
    single = "--single" in sys.argv
    ns, nw, nsteps = (1, 250, 250) if single else (1000, 250, 250)
    if single:
        from bench import BANDS
        truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
        like = mbb.likelihood(response=True)
        like.set_phot(BANDS, np.ones(8), np.ones(8))
        flux = like.model_flux(truth)[0]
        like.set_phot(BANDS, flux, 0.1 * flux + 1.0)
        p0 = truth * (1.0 + 0.02 * np.random.RandomState(1).normal(size=(nw, 5)))
    else:
        like, _, p0 = setup(ns, nw)
    kw = dict(percentile=68.3)

    def way_a():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        ch = s.chain if not single else s.chain[None]
        mean, pct = host_summary(ch)
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, t2 - t1, mean, pct, s.chain.nbytes + s.lnprobability.nbytes

    def way_b():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=kw)
        t1 = time.perf_counter()
        r = s.summary._raw
        nbytes = sum(getattr(r, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best", "best_index"))
        return t1 - t0, s.summary.mean.reshape(ns, 8)[:, :5], np.moveaxis(s.summary.percentiles[1].reshape(ns, 8, 2)[:, :5], 2, 1), nbytes

    if "--only-summary" in sys.argv:
        way_b(); way_b()
        return
    way_b(); way_a()                                             # warm-up of both
    a, b = [], []
    for _ in range(3):
        ra = way_a(); rb = way_b()
        a.append(ra[:3]); b.append(rb[0])
    # the two ways agree (same seed, same chain)
    assert np.allclose(rb[1], ra[3], rtol=1e-12) and np.allclose(rb[2], ra[4], rtol=1e-12, atol=0)
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": 8}, "host_threads": THREADS,
           "a_stored_chain_then_numpy": {"wall_s": [x[0] for x in a], "run_mcmc_s": [x[1] for x in a],
                                         "numpy_s": [x[2] for x in a], "bytes_back": int(ra[5])},
           "b_device_summary": {"wall_s": b, "bytes_back": int(rb[3])}}
    for k in ("a_stored_chain_then_numpy", "b_device_summary"):
        w = out[k]["wall_s"]
        out[k]["median_s"], out[k]["spread_s"] = float(np.median(w)), float(max(w) - min(w))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
