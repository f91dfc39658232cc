#!/usr/bin/env python3
"""The reweighting's time on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands); the target is the same fit
with a Gaussian prior on beta:

  (d) run_mcmc(storechain=False, summary=...), then sampler.reweight(target): the weights and the weighted statistics
      per source on the device, nothing but the tables back;
  (h) the host way: run_mcmc with the chain and its lnprob stored and brought back, the target's lnprob of every row by
      target(rows), then tests/_reweight_ref.py in float64 per source on 16 threads at most (PSIS, the integer weights,
      the weighted mean and two quantiles of the five parameters).

In one process, warmed up; (d) `--runs` times (default nine), (h) `--host-runs` times (default one: it takes many times
as long) after the first of them; walls with their spread and the bytes each way brings back, as one JSON object
(profiles/r32/reweight.json), rewritten after every run.  `--only-device` runs (d) twice, for a kernel trace of its
own; `--shape NS NW NSTEPS` rehearses at another size."""
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
from bench import BANDS                        # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
PRIOR = (2.0, 0.3)


def arg(name, default, n=1):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    vals = sys.argv[i + 1:i + 1 + n]
    return vals[0] if n == 1 else vals


def nbytes_of(raw):
    return sum(v.nbytes for v in vars(raw).values() if isinstance(v, np.ndarray))


def main():
    ns, nw, nsteps = [int(v) for v in arg("--shape", (1000, 250, 250), 3)]
    runs, host_runs = int(arg("--runs", 9)), int(arg("--host-runs", 1))
    out_path = arg("--out", None)
    like, _, p0 = setup(ns, nw)
    target = mbb.likelihood(response=True)
    target.set_phot_multi(BANDS, np.asarray(like._flux_multi), 1.0 / np.sqrt(np.asarray(like._ivar_multi)))
    target.set_gaussian_prior("beta", *PRIOR)

    def device():
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        res = s.reweight(target)
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, t2 - t1, res, nbytes_of(s.summary._raw) + nbytes_of(res._raw)

    def way_h():
        import _reweight_ref as RR
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        chain, lp = s.chain, s.lnprobability
        # (a tenth of the walkers at a time: the rows of a call are nsources equal blocks)
        cuts = np.linspace(0, nw, 11).astype(int)
        lq = np.concatenate([target(np.ascontiguousarray(chain[:, a:b]).reshape(ns, -1, 5)).reshape(ns, b - a, nsteps)
                             for a, b in zip(cuts[:-1], cuts[1:]) if b > a], axis=1).reshape(ns, -1)
        t2 = time.perf_counter()
        lp = lp.reshape(ns, -1)
        khat, lnz, mean = np.full(ns, np.nan), np.full(ns, np.nan), np.full((ns, 5), np.nan)
        pct = np.full((ns, 5, 2), np.nan)

        def one(g):
            used, zero, left = RR.classes(lp[g], lq[g])
            sc = RR.scalars((lq[g] - lp[g])[used], int(zero.sum()), dtype=np.float64)
            u = np.zeros(lp[g].size, dtype=np.int64)
            u[used] = RR.quantise(np.asarray(sc["lw"], dtype=np.float64))
            rows = chain[g].reshape(-1, 5)
            khat[g], lnz[g] = sc["khat"], sc["lnz_ratio"]
            for k in range(5):
                mean[g, k] = RR.wmean(rows[:, k], u, np.float64)
                pct[g, k] = [RR.wquantile(rows[:, k], u, q) for q in (15.85, 84.15)]
        with ThreadPoolExecutor(THREADS) as ex:
            list(ex.map(one, range(ns)))
        t3 = time.perf_counter()
        return t3 - t0, t1 - t0, t2 - t1, t3 - t2, (khat, lnz, mean, pct), chain.nbytes + s.lnprobability.nbytes + lq.nbytes

    if "--only-device" in sys.argv:
        device(); device()
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": int(like._ndata)}, "host_threads": THREADS,
           "target": "the same fit with a Gaussian prior on beta, mean %g sigma %g" % PRIOR,
           "runs_asked": runs, "host_runs_asked": host_runs}
    w = device()
    out["warmup_wall_s"] = w[0]
    print("warm-up: %.2f s (reweight %.3f s)" % (w[0], w[2]), flush=True)
    rows, hrows, res = [], [], {}

    def write():
        if rows:
            wl = [x[0] for x in rows]
            res.setdefault("d_device_reweight", {}).update(
                wall_s=wl, run_mcmc_s=[x[1] for x in rows], reweight_s=[x[2] for x in rows], median_s=float(np.median(wl)),
                spread_s=float(max(wl) - min(wl)), reweight_median_s=float(np.median([x[2] for x in rows])))
        if hrows:
            res["h_stored_chain_target_rows_reference_on_the_host"].update(
                wall_s=[x[0] for x in hrows], run_mcmc_s=[x[1] for x in hrows], target_rows_s=[x[2] for x in hrows],
                host_s=[x[3] for x in hrows], median_s=float(np.median([x[0] for x in hrows])))
        out["runs_done"], out["host_runs_done"], out["results"] = len(rows), len(hrows), res
        if out_path:
            with open(out_path + ".tmp", "w") as fh:
                json.dump(out, fh, indent=1)
            os.replace(out_path + ".tmp", out_path)

    for i in range(runs):
        rd = device()
        rows.append(rd[:3])
        raw = rd[3]._raw
        fin = np.isfinite(raw.khat)
        res.setdefault("d_device_reweight", {}).update(
            bytes_back=int(rd[4]), khat_median=float(np.median(raw.khat[fin])), khat_above_0p7=int(np.sum(raw.khat > 0.7)),
            fallbacks=int(np.sum(~fin)), tail_len=int(raw.tail_len.max()), ess_median=float(np.median(raw.ess)),
            lnz_ratio_median=float(np.median(raw.lnz_ratio)))
        print("run %d: %.3f s (run_mcmc %.3f, reweight %.3f)" % (i + 1, rd[0], rd[1], rd[2]), flush=True)
        if i < host_runs:
            rh = way_h()
            hrows.append(rh[:4])
            khat, lnz, mean, pct = rh[4]
            lo, hi = raw.pct[:, :5, 0], raw.pct[:, :5, 1]
            res.setdefault("h_stored_chain_target_rows_reference_on_the_host", {}).update(
                bytes_back=int(rh[5]),
                max_abs_diff_khat=float(np.nanmax(np.abs(khat - raw.khat))), max_abs_diff_lnz_ratio=float(np.nanmax(np.abs(lnz - raw.lnz_ratio))),
                max_rel_diff_mean=float(np.nanmax(np.abs(mean - raw.mean[:, :5]) / np.abs(mean))),
                quantiles_equal=int(np.sum((pct[..., 0] == lo) & (pct[..., 1] == hi))), quantiles_compared=int(lo.size))
            print("host %d: %.2f s (target(rows) %.2f, reference %.2f)" % (len(hrows), rh[0], rh[2], rh[3]), flush=True)
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
