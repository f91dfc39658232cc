#!/usr/bin/env python3
"""The marginals' time claim on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands):

  (a) run_mcmc with the chain stored, then numpy.histogram of the five parameters of every source on the host (16
      threads at most), and with "2d" also numpy.histogram2d of the ten parameter pairs;
  (b) run_mcmc(storechain=False, summary=..., marginals=...).

Two table sets -- "1d": five 1-D tables of 64 bins; "2d": those and the ten 32 x 32 pairs --, in one process, warmed
up, alternated, nine times each (`--runs N`: N times); walls with their spread and the bytes each way brings back, as one JSON object
(profiles/r16/marginals.json).  Both ways bin the same chain (same seed) and the counts are compared.  `--single`
measures the single-source 250 x 250 case the same way; `--only-device` runs (b) twice per set after a warm-up, for a
kernel trace of its own (rocprofv3 --kernel-trace --stats -- python tools/bench_marginals.py --only-device)."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbb_emcee_amd as mbb                    # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
PAIRS = [(a, b) for a in range(5) for b in range(a + 1, 5)]
SETS = {"1d": dict(bins=64, bins2d=0), "2d": dict(bins=64, bins2d=32)}
RUNS = 9


def host_tables(chain, bins, bins2d):
    """numpy's tables of a stored chain [nsrc, nw, nsteps, 5]: counts1 [nsrc, 5, bins], counts2 [nsrc, 10, b2, b2]."""
    def one(g):
        cols = [np.ascontiguousarray(chain[g, :, :, k]).ravel() for k in range(5)]
        c1 = [np.histogram(x, bins=bins)[0] for x in cols]
        c2 = [np.histogram2d(cols[a], cols[b], bins=bins2d)[0] for a, b in PAIRS] if bins2d else []
        return c1, c2
    with ThreadPoolExecutor(THREADS) as ex:
        res = list(ex.map(one, range(chain.shape[0])))
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

    def way_a(kw):
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        c1, c2 = host_tables(s.chain if not single else s.chain[None], kw["bins"], kw["bins2d"])
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, t2 - t1, (c1, c2), s.chain.nbytes + s.lnprobability.nbytes

    def way_b(kw):
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        m = s.marginals(**kw)
        t2 = time.perf_counter()
        r = s.summary._raw
        nbytes = sum(getattr(r, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best",
                                                    "best_index"))
        nbytes += sum(getattr(m._raw, f).nbytes for f in ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below",
                                                          "n_above", "n_nonfinite", "status"))
        return t2 - t0, t1 - t0, t2 - t1, (m._raw.counts1[:, :5], m._raw.counts2), nbytes

    runs = int(sys.argv[sys.argv.index("--runs") + 1]) if "--runs" in sys.argv else RUNS
    if "--only-device" in sys.argv:
        for kw in SETS.values():
            way_b(kw); way_b(kw)
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": 8}, "host_threads": THREADS, "runs": runs}
    for name, kw in SETS.items():
        way_b(kw); way_a(kw)                                     # warm-up of both
        a, b = [], []
        for _ in range(runs):
            ra = way_a(kw); rb = way_b(kw)
            a.append(ra[:3]); b.append(rb[:3])
        same = bool(np.array_equal(ra[3][0], rb[3][0]) and (not kw["bins2d"] or np.array_equal(ra[3][1], rb[3][1])))
        res = {"a_stored_chain_then_numpy": {"wall_s": [x[0] for x in a], "run_mcmc_s": [x[1] for x in a],
                                             "numpy_histograms_s": [x[2] for x in a], "bytes_back": int(ra[4])},
               "b_device_marginals": {"wall_s": [x[0] for x in b], "run_mcmc_summary_s": [x[1] for x in b],
                                      "marginals_s": [x[2] for x in b], "bytes_back": int(rb[4])},
               "counts_equal_numpys": same}
        for k in ("a_stored_chain_then_numpy", "b_device_marginals"):
            w = res[k]["wall_s"]
            res[k]["median_s"], res[k]["spread_s"] = float(np.median(w)), float(max(w) - min(w))
        res["b_device_marginals"]["marginals_median_s"] = float(np.median(res["b_device_marginals"]["marginals_s"]))
        res["a_stored_chain_then_numpy"]["numpy_median_s"] = float(np.median(res["a_stored_chain_then_numpy"]["numpy_histograms_s"]))
        out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
