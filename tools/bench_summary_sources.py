#!/usr/bin/env python3
"""What a redshift per source costs the device summary, on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands):
run_mcmc(storechain=False, summary=dict(derived=("lir", "dustmass"), ...)) in three configurations,

  parent_scalar   another tree's build (--parent DIR, a checkout of the parent commit built in place), one redshift;
  scalar          this tree, one redshift and distance for the whole call (the kernels the parent has);
  sources         this tree, an array of 1000 redshifts and distances (the per-source kernels).

A library cannot be loaded twice, so every measurement is a process of its own (`--one NAME`: a warm-up run, then
--runs timed ones, one JSON line); the driver starts them one after the other, alternating the three configurations
--rounds times, and writes walls with their spread as one JSON object (profiles/r15/summary_per_source.json).
`--one NAME --trace` does the warm-up and a single run, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/bench_summary_sources.py --one sources --trace)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_LIMIT_S = 300


def one(name, tree, ns, runs):
    tree = os.path.abspath(tree)
    sys.path.insert(0, tree)
    import mbb_emcee_amd as mbb
    from tools.bench_cfg5 import setup
    assert os.path.dirname(os.path.dirname(os.path.abspath(mbb.__file__))) == os.path.abspath(tree)
    nw, nsteps = 250, 250
    like, _, p0 = setup(ns, nw)
    if name == "sources":
        z = 0.5 + 3.0 * np.random.RandomState(2).rand(ns)
        d = 3000.0 + 30000.0 * np.random.RandomState(3).rand(ns)
    else:
        z, d = 2.3, 18700.0
    kw = dict(percentile=68.3, derived=("lir", "dustmass"), redshift=z, lumdist_mpc=d)
    walls = []
    for i in range(1 + runs):
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=kw)
        walls.append(time.perf_counter() - t0)
    flagged = int(np.count_nonzero(s.summary.status[:, 6:]))          # (a walker's failing row flags its source's column)
    print(json.dumps({"config": name, "sources": ns, "warmup_s": walls[0], "wall_s": walls[1:],
                      "lir_mean_source0": float(s.summary.mean[0, 6]), "flagged_columns": flagged}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", choices=("parent_scalar", "scalar", "sources"))
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--sources", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.tree, a.sources, 1 if a.trace else a.runs)
    configs = ([("parent_scalar", os.path.abspath(a.parent))] if a.parent else []) + [("scalar", HERE), ("sources", HERE)]
    res = {name: {"wall_s": [], "warmup_s": []} for name, _ in configs}
    for _ in range(a.rounds):
        for name, tree in configs:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--tree", tree, "--sources", str(a.sources),
                   "--runs", str(a.runs)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=STEP_LIMIT_S, cwd=tree)
            if p.returncode != 0:                              # nothing more is started on the GPU after a failure
                sys.exit("%s failed with status %d" % (name, p.returncode))
            r = json.loads(p.stdout.decode().strip().splitlines()[-1])
            res[name]["wall_s"] += r["wall_s"]
            res[name]["warmup_s"].append(r["warmup_s"])
            res[name]["lir_mean_source0"], res[name]["flagged_columns"] = r["lir_mean_source0"], r["flagged_columns"]
            print(name, r["wall_s"], flush=True)
    for v in res.values():
        w = v["wall_s"]
        v["median_s"], v["spread_s"], v["min_s"] = float(np.median(w)), float(max(w) - min(w)), float(min(w))
    out = {"shape": {"sources": a.sources, "walkers": 250, "steps": 250, "bands": 8},
           "what": "run_mcmc(storechain=False, summary=dict(derived=('lir', 'dustmass'), ...)): host wall of the call",
           "runs_per_config": a.rounds * a.runs, "processes_per_config": a.rounds, **res}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
