#!/usr/bin/env python3
"""The out-of-sample fit's time on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands):

  (l) run_mcmc(storechain=False, summary=...), then sampler.loo(): WAIC and PSIS-LOO per source and band on the device,
      nothing but the tables back;
  (g) the same run, then sampler.goodness(): the analysis that needs the same band-flux fill and nothing of the new
      kernels -- the difference of the two analysis times is what the new kernels cost;
  (h) the host way: run_mcmc with the chain stored and brought back, the log-likelihood blob ll [rows, bands] through
      loo_rows (what an emcee user stores per sample), then tests/_loo_ref.py in float64 per (source, band) on 16
      threads at most, Phi by scipy.

In one process, warmed up; (l) and (g) alternated `--runs` times (default nine), (h) `--host-runs` times (default one: it
takes many times as long); walls with their spread and the bytes each way brings back, as one JSON object
(profiles/r25/loo.json), rewritten after every run.  `--budget-mb N` sets pointwise_budget_mb (0: one band per group,
which refills the band fluxes for every band); `--only-device` runs (l) twice, for a kernel trace of its own;
`--shape NS NW NSTEPS` rehearses at another size."""
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
from mbb_emcee_amd import _native              # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
TABLES = ("n_used", "tail_len", "status", "lppd", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "khat", "loo_pit")


def arg(name, default, n=1):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    vals = sys.argv[i + 1:i + 1 + n]
    return vals[0] if n == 1 else vals


def summary_bytes(s):
    r = s.summary._raw
    return sum(getattr(r, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best", "best_index"))


def main():
    ns, nw, nsteps = [int(v) for v in arg("--shape", (1000, 250, 250), 3)]
    runs, host_runs = int(arg("--runs", 9)), int(arg("--host-runs", 1))
    budget = arg("--budget-mb", None)
    out_path = arg("--out", None)
    like, _, p0 = setup(ns, nw)
    if budget is not None:
        _native.analysis_context(like).set_option("pointwise_budget_mb", int(budget))

    def device(which):
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        res = s.loo() if which == "l" else s.goodness()
        t2 = time.perf_counter()
        nbytes = summary_bytes(s) + sum(v.nbytes for v in vars(res._raw).values() if isinstance(v, np.ndarray))
        return t2 - t0, t1 - t0, t2 - t1, res, nbytes

    def way_h():
        import _loo_ref as LR
        from scipy.special import ndtr
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        chain = s.chain
        ll, _ = mbb.loo_rows(like, chain.reshape(-1, 5))
        ll = ll.reshape(ns, nw * nsteps, -1)
        t2 = time.perf_counter()
        nb = ll.shape[-1]
        elpd = np.full((ns, nb), np.nan)
        lam = np.asarray(like._ivar_multi)

        def one(g):
            for b in range(nb):
                v = ll[g, :, b]
                # |z| from ll; its sign is not in the blob, and Phi's cost does not depend on it
                z = np.sqrt(np.maximum(0.0, -2.0 * (v - 0.5 * (np.log(lam[g, b]) - np.log(2 * np.pi)))))
                elpd[g, b] = LR.column(v, z, dtype=np.float64, phi=ndtr(z))["elpd_loo"]
        with ThreadPoolExecutor(THREADS) as ex:
            list(ex.map(one, range(ns)))
        t3 = time.perf_counter()
        return t3 - t0, t1 - t0, t2 - t1, t3 - t2, elpd, chain.nbytes + ll.nbytes

    if "--only-device" in sys.argv:
        device("l"); device("l")
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": int(like._ndata)}, "host_threads": THREADS,
           "runs_asked": runs, "host_runs_asked": host_runs, "pointwise_budget_mb": budget}
    wl, wg = device("l"), device("g")
    out["warmup_wall_s"] = {"l": wl[0], "g": wg[0]}
    print("warm-up: l %.2f s (loo %.3f s), g %.2f s (goodness %.3f s)" % (wl[0], wl[2], wg[0], wg[2]), flush=True)
    rows = {"l": [], "g": [], "h": []}
    res = {}

    def write():
        for k, name, part in (("l", "l_device_loo", "loo_s"), ("g", "g_device_goodness", "goodness_s")):
            if rows[k]:
                w = [x[0] for x in rows[k]]
                res.setdefault(name, {}).update({"wall_s": w, "run_mcmc_s": [x[1] for x in rows[k]], part: [x[2] for x in rows[k]],
                                                 "median_s": float(np.median(w)), "spread_s": float(max(w) - min(w)),
                                                 part.replace("_s", "_median_s"): float(np.median([x[2] for x in rows[k]]))})
        if rows["l"] and rows["g"]:
            res["loo_minus_goodness_median_s"] = res["l_device_loo"]["loo_median_s"] - res["g_device_goodness"]["goodness_median_s"]
        if rows["h"]:
            res["h_stored_chain_blob_reference_on_the_host"].update(
                {"wall_s": [x[0] for x in rows["h"]], "run_mcmc_s": [x[1] for x in rows["h"]], "blob_s": [x[2] for x in rows["h"]],
                 "host_s": [x[3] for x in rows["h"]], "median_s": float(np.median([x[0] for x in rows["h"]]))})
        out["runs_done"], out["host_runs_done"], out["results"] = len(rows["l"]), len(rows["h"]), res
        if out_path:
            with open(out_path + ".tmp", "w") as fh:
                json.dump(out, fh, indent=1)
            os.replace(out_path + ".tmp", out_path)

    for i in range(runs):
        rl = device("l")
        rows["l"].append(rl[:3])
        lo = rl[3]
        kh = lo._raw.khat
        res.setdefault("l_device_loo", {}).update(
            bytes_back=int(rl[4]), khat_median=float(np.median(kh[np.isfinite(kh)])), khat_above_0p7=int(np.sum(kh > 0.7)),
            fallbacks=int(np.sum(~np.isfinite(kh))), tail_len=int(lo._raw.tail_len.max()))
        rg = device("g")
        rows["g"].append(rg[:3])
        res.setdefault("g_device_goodness", {})["bytes_back"] = int(rg[4])
        print("run %d: l %.3f s (loo %.3f), g %.3f s (goodness %.3f)" % (i + 1, rl[0], rl[2], rg[0], rg[2]), flush=True)
        if i < host_runs:
            rh = way_h()
            rows["h"].append(rh[:4])
            res.setdefault("h_stored_chain_blob_reference_on_the_host", {})["bytes_back"] = int(rh[5])
            res["max_abs_diff_elpd_loo_band"] = float(np.nanmax(np.abs(rh[4] - lo._raw.elpd_loo)))
            print("host %d: %.2f s (blob %.2f, reference %.2f)" % (len(rows["h"]), rh[0], rh[2], rh[3]), flush=True)
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
