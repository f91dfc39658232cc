#!/usr/bin/env python3
"""The draws' time on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands): 100 draws per source with peak
wavelength, L_IR and dust mass, one redshift per source,

  (a) run_mcmc with the chain stored, then numpy indexing at the same picks (draw_indices) and postprocess on the drawn
      rows on the host;
  (b) run_mcmc(storechain=False, summary=True), then sampler.draws(100, derived=all three, redshift per source).

In one process, warmed up, alternated, nine times each; walls with their spread and the bytes each way brings back, as
one JSON object (profiles/r20/draws.json; `--out PATH`, default draws.json beside the working directory), rewritten
after every pair of runs.  Both ways draw from the same chain (same seed) and their rows and values are compared.
`--only-device` makes one run and three draws calls, for a kernel trace of its own (rocprofv3 --kernel-trace --stats --
python tools/bench_draws.py --only-device)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mbb_emcee_amd as mbb                                   # noqa: E402
from mbb_emcee_amd import postprocess as pp                   # noqa: E402
from tools.bench_cfg5 import setup                            # noqa: E402

NS, NW, NSTEPS, N, RUNS = 1000, 250, 250, 100, 9
DERIVED = ("peaklambda", "lir", "dustmass")


def main():
    like, truths, p0 = setup(NS, NW)
    rng = np.random.RandomState(3)
    z = rng.uniform(0.5, 4.0, NS)
    dl = 3000.0 + 9000.0 * z
    out = {"shape": {"sources": NS, "walkers": NW, "steps": NSTEPS, "bands": 8}, "draws_per_source": N,
           "derived": list(DERIVED), "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")), "runs_asked": RUNS}
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else "draws.json"
    if "--only-device" in sys.argv:
        s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
        s.run_mcmc(p0, NSTEPS, storechain=False, summary=True)
        for _ in range(3):
            d = s.draws(N, derived=DERIVED, redshift=z, lumdist_mpc=dl)
        print("draws:", d.params.shape)
        return

    def leg_a():
        t0 = time.perf_counter()
        s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
        s.run_mcmc(p0, NSTEPS)
        t1 = time.perf_counter()
        idx = mbb.draw_indices(NW, NSTEPS, N, seed=3, nsources=NS, like=like)
        src = np.arange(NS)[:, None]
        rows = np.ascontiguousarray(s.chain[src, idx[..., 0], idx[..., 1]])
        lnp = s.lnprobability[src, idx[..., 0], idx[..., 1]]
        peak = pp.peak_wavelength(like, rows)
        lir = np.empty((NS, N))
        dust = np.empty((NS, N))
        for g in range(NS):
            lir[g] = pp.lir(like, rows[g], z[g], dl[g])
            dust[g] = pp.dustmass(like, rows[g], z[g], dl[g])
        t2 = time.perf_counter()
        back = s.chain.nbytes + s.lnprobability.nbytes + idx.nbytes + peak.nbytes + lir.nbytes
        return (t2 - t0, t1 - t0, t2 - t1, back), dict(rows=rows, lnp=lnp, peak=peak, lir=lir, dust=dust, idx=idx)

    def leg_b():
        t0 = time.perf_counter()
        s = mbb.DeviceEnsembleSampler(NW, 5, like, seed=3)
        s.run_mcmc(p0, NSTEPS, storechain=False, summary=True)
        t1 = time.perf_counter()
        d = s.draws(N, derived=DERIVED, redshift=z, lumdist_mpc=dl)
        t2 = time.perf_counter()
        r = d._raw
        back = (r.rows.nbytes + r.lnprob.nbytes + r.index.nbytes + r.status.nbytes + sum(v.nbytes for v in r.derived.values()))
        sm = s.summary._raw
        back_summary = sum(v.nbytes for v in vars(sm).values() if isinstance(v, np.ndarray))
        return (t2 - t0, t1 - t0, t2 - t1, back, back_summary), d

    t0 = time.perf_counter(); leg_a(); ta = time.perf_counter() - t0
    t0 = time.perf_counter(); leg_b(); tb = time.perf_counter() - t0
    out["warmup_wall_s"] = {"a": ta, "b": tb}
    A, B = [], []
    for k in range(RUNS):
        ra, va = leg_a()
        rb, d = leg_b()
        A.append(ra); B.append(rb)
        if k == 0:
            assert np.array_equal(d.index, va["idx"]) and np.array_equal(d.params, va["rows"]) and np.array_equal(d.lnprob, va["lnp"])
            rel = lambda g, w: float(np.max(np.abs(g - w) / np.abs(w)))
            out["draws_equal_host_picks"] = True
            out["max_rel_diff"] = {"peaklambda": rel(d.peaklambda, va["peak"]), "lir": rel(d.lir, va["lir"]),
                                   "dustmass": rel(d.dustmass, va["dust"])}
        out["runs_done"] = k + 1
        med = lambda v: float(np.median(v))
        spread = lambda v: float(np.max(v) - np.min(v))
        out["results"] = {
            "a_stored_chain_numpy_postprocess": {
                "wall_s": [r[0] for r in A], "run_mcmc_s": [r[1] for r in A], "index_and_postprocess_s": [r[2] for r in A],
                "bytes_back": int(A[0][3]), "median_s": med([r[0] for r in A]), "spread_s": spread([r[0] for r in A]),
                "host_median_s": med([r[2] for r in A]), "host_spread_s": spread([r[2] for r in A])},
            "b_device_draws": {
                "wall_s": [r[0] for r in B], "run_mcmc_summary_s": [r[1] for r in B], "draws_s": [r[2] for r in B],
                "bytes_back": int(B[0][3]), "bytes_back_with_summary": int(B[0][3] + B[0][4]),
                "median_s": med([r[0] for r in B]), "spread_s": spread([r[0] for r in B]),
                "draws_median_s": med([r[2] for r in B]), "draws_spread_s": spread([r[2] for r in B])}}
        json.dump(out, open(path, "w"), indent=1)
        print("run %d: a %.3f s (host part %.3f), b %.3f s (draws %.4f)" % (k, ra[0], ra[2], rb[0], rb[2]), flush=True)
    print(json.dumps(out["results"]["b_device_draws"]))


if __name__ == "__main__":
    main()
