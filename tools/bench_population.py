#!/usr/bin/env python3
"""The population hyper-likelihood's time on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands), columns T
and beta:

  (d) run_mcmc(storechain=False, summary=...), sampler.population() (the block is built on the device), then one
      evaluate() of H = 1, 16 and 64 candidates with and without moments, and a 200-step sample() of 32 walkers (400
      device calls of 16 candidates); nothing but the tables comes back;
  (h) the host way: run_mcmc with the chain stored and brought back, then tests/_population_ref.py in float64 per source
      on 16 threads at most for the same 16 candidates.

In one process, warmed up; (d) `--runs` times (default nine), (h) `--host-runs` times (default one) after the first of
them; walls with their spread and the bytes each way brings back, as one JSON object (profiles/r33/population.json),
rewritten after every run.  `--only-device` runs the build and the evaluations twice, for a kernel trace of its own;
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
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)
COLUMNS = ("T", "beta")
HS = (1, 16, 64)


def arg(name, default, n=1):
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    vals = sys.argv[i + 1:i + 1 + n]
    return vals[0] if n == 1 else vals


def candidates(truths, H):
    """H candidates about the catalogue's true T and beta."""
    rng = np.random.RandomState(1)
    t = truths[:, :2]
    mu = t.mean(axis=0) + 0.2 * t.std(axis=0) * rng.standard_normal((H, 2))
    L = np.zeros((H, 2, 2))
    L[:, 0, 0], L[:, 1, 1] = t[:, 0].std() * rng.uniform(0.7, 1.5, H), t[:, 1].std() * rng.uniform(0.7, 1.5, H)
    L[:, 1, 0] = 0.2 * t[:, 1].std() * rng.standard_normal(H)
    return mu, L


def main():
    ns, nw, nsteps = [int(v) for v in arg("--shape", (1000, 250, 250), 3)]
    runs, host_runs = int(arg("--runs", 9)), int(arg("--host-runs", 1))
    sample_steps = int(arg("--sample-steps", 200))
    out_path = arg("--out", None)
    like, truths, p0 = setup(ns, nw)
    cands = {H: candidates(truths, H) for H in HS}

    def device(sample=True):
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        pop = s.population(columns=COLUMNS)
        t2 = time.perf_counter()
        ev, evals, back = {}, {}, {}
        for H in HS:
            for moments in (False, True):
                ta = time.perf_counter()
                e = pop.evaluate(cands[H][0], chol=cands[H][1], moments=moments)
                evals["H%d%s" % (H, "_moments" if moments else "")] = time.perf_counter() - ta
                back["H%d%s" % (H, "_moments" if moments else "")] = int(sum(
                    np.asarray(v).nbytes for v in (e.lnl, e.lnl_source, e.ess, e.mean, e.covariance, e.status, e.n_sources_used)
                    if v is not None))
                ev[(H, moments)] = e
        fit, t_sample = None, None
        if sample:
            ta = time.perf_counter()
            fit = pop.sample(nsteps=sample_steps, nwalkers=32, nburn=0, seed=4)
            t_sample = time.perf_counter() - ta
        return dict(wall=t2 - t0, run=t1 - t0, build=t2 - t1, evals=evals, sample=t_sample, back=back, ev=ev, fit=fit, pop=pop)

    def way_h():
        import _population_ref as PR
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        chain = s.chain
        prior = PR.like_prior(like)
        mu, L = cands[16]
        cl = [(mu[h], L[h]) for h in range(16)]
        lnl_src = np.full((16, ns), np.nan)

        def one(g):
            xb = [PR.entries(PR.window(chain[g]), [0, 1], [0, 0], prior, np.float64)]
            lnl_src[:, g] = PR.evaluate(xb, cl, np.float64, moments=False)["lnl_src"][:, 0]
        with ThreadPoolExecutor(THREADS) as ex:
            list(ex.map(one, range(ns)))
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, t2 - t1, lnl_src, chain.nbytes

    if "--only-device" in sys.argv:
        device(sample=False); device(sample=False)
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": int(like._ndata), "columns": list(COLUMNS),
                     "entries_per_source": nw * nsteps, "block_bytes": ns * nw * nsteps * 3 * 8},
           "host_threads": THREADS, "sample": "%d steps of 32 walkers: %d device calls of 16 candidates" % (sample_steps, 2 * sample_steps + 1),
           "runs_asked": runs, "host_runs_asked": host_runs}
    w = device()
    out["warmup_wall_s"] = w["wall"]
    print("warm-up: %.2f s (build %.3f s)" % (w["wall"], w["build"]), flush=True)
    rows, hrows, res = [], [], {}

    def med(v):
        return float(np.median(v))

    def write():
        if rows:
            d = res.setdefault("d_device_population", {})
            d.update(run_summary_build_s=[r["wall"] for r in rows], run_mcmc_s=[r["run"] for r in rows],
                     build_s=[r["build"] for r in rows], median_s=med([r["wall"] for r in rows]),
                     spread_s=float(max(r["wall"] for r in rows) - min(r["wall"] for r in rows)),
                     build_median_s=med([r["build"] for r in rows]), sample_s=[r["sample"] for r in rows],
                     sample_median_s=med([r["sample"] for r in rows]),
                     evaluate_median_s={k: med([r["evals"][k] for r in rows]) for k in rows[0]["evals"]},
                     evaluate_s={k: [r["evals"][k] for r in rows] for k in rows[0]["evals"]})
        if hrows:
            res["h_stored_chain_reference_on_the_host"].update(
                wall_s=[x[0] for x in hrows], run_mcmc_s=[x[1] for x in hrows], reference_16_candidates_s=[x[2] for x in hrows])
        out["runs_done"], out["host_runs_done"], out["results"] = len(rows), len(hrows), res
        if out_path:
            with open(out_path + ".tmp", "w") as fh:
                json.dump(out, fh, indent=1)
            os.replace(out_path + ".tmp", out_path)

    for i in range(runs):
        r = device()
        rows.append({k: r[k] for k in ("wall", "run", "build", "evals", "sample")})
        e, fit = r["ev"][(16, False)], r["fit"]
        res.setdefault("d_device_population", {}).update(
            bytes_back_evaluate=r["back"], bytes_back_build=int(sum(v.nbytes for v in vars(r["pop"]._raw).values())),
            ess_median_H16=float(np.nanmedian(e.ess)), lnl_H16=[float(v) for v in e.lnl],
            sample_acceptance=float(fit.acceptance_fraction.mean()), sample_ess_low=fit.ess_low,
            sample_mu=fit.mu_cen().tolist(), sample_sigma=fit.sigma_cen().tolist(), sample_corr_T_beta=fit.corr_cen()[1, 0].tolist())
        print("run %d: %.3f s (run_mcmc %.3f, build %.4f; evaluate H16 %.4f, H64 moments %.4f; sample %.2f)"
              % (i + 1, r["wall"], r["run"], r["build"], r["evals"]["H16"], r["evals"]["H64_moments"], r["sample"]), flush=True)
        if i < host_runs:
            rh = way_h()
            hrows.append(rh[:3])
            res.setdefault("h_stored_chain_reference_on_the_host", {}).update(
                bytes_back=int(rh[4]),
                max_abs_diff_lnl_src=float(np.nanmax(np.abs(rh[3] - e.lnl_source) / np.maximum(1.0, np.abs(rh[3])))))
            print("host %d: %.2f s (run_mcmc and the chain home %.2f, reference %.2f)" % (len(hrows), rh[0], rh[1], rh[2]), flush=True)
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
