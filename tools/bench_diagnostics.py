#!/usr/bin/env python3
"""The chain diagnostics' time claim on cfg5's shape (1000 sources x 250 walkers, 250 steps, 8 bands):

  (a) run_mcmc with the chain stored, then the autocorrelation time of every source on the host (16 threads at
      most) -- what get_autocorr_time() does for source 0, done for every source ("mean": integrated_time of the
      ensemble-mean series; "walkers": every walker's FFT autocorrelation function, averaged and windowed);
  (b) run_mcmc(storechain=False, summary=..., convergence=...).

Both methods, in one process, warmed up, alternated, three times each; walls with their spread and the bytes each way
brings back, as one JSON object (profiles/r14/diagnostics.json).  `--single` measures the single-source 250 x 250
case the same way; `--only-device` runs (b) once per method after a warm-up, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/bench_diagnostics.py --only-device)."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mbb_emcee_amd as mbb                    # noqa: E402
from mbb_emcee_amd.ensemble import integrated_time   # noqa: E402
from tools.bench_cfg5 import setup             # noqa: E402

THREADS = min(16, os.cpu_count() or 1)


def walkers_time(x, c=5.0):
    """emcee 3's estimator for x [nw, n]"""
    nw, n = x.shape
    nfft = 1 << (2 * n - 1).bit_length()
    y = x - x.mean(axis=1, keepdims=True)
    f = np.fft.rfft(y, nfft, axis=1)
    acf = np.fft.irfft(f * np.conjugate(f), axis=1)[:, :n]
    rho = (acf / acf[:, :1]).mean(axis=0)
    taus = 2.0 * np.cumsum(rho) - 1.0
    win = np.arange(n) >= c * taus
    return taus[np.argmax(win) if win.any() else n - 1]


def host_times(chain, method):
    """tau [nsrc, 5] of a stored chain [nsrc, nw, nsteps, 5], numpy on the host."""
    def one(g):
        if method == "mean":
            m = chain[g].mean(axis=0)
            return [integrated_time(m[:, i]) for i in range(5)]
        return [walkers_time(chain[g, :, :, i]) for i in range(5)]
    with ThreadPoolExecutor(THREADS) as ex:
        return np.array(list(ex.map(one, range(chain.shape[0]))))


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

    def way_a(method):
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps)
        t1 = time.perf_counter()
        tau = host_times(s.chain if not single else s.chain[None], method)
        t2 = time.perf_counter()
        return t2 - t0, t1 - t0, t2 - t1, tau, s.chain.nbytes + s.lnprobability.nbytes

    def way_b(method):
        s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=3)
        t0 = time.perf_counter()
        s.run_mcmc(p0, nsteps, storechain=False, summary=dict(percentile=68.3))
        t1 = time.perf_counter()
        d = s.convergence(method=method)
        t2 = time.perf_counter()
        r = s.summary._raw
        nbytes = sum(getattr(r, f).nbytes for f in ("n_used", "mean", "min", "max", "pct", "status", "cov", "best",
                                                    "best_index"))
        nbytes += sum(a.nbytes for a in (d.tau, d.ess, d.rhat, d.window, d.status))
        return t2 - t0, t1 - t0, t2 - t1, d.tau.reshape(ns, 5), nbytes

    methods = ("mean", "walkers")
    if "--only-device" in sys.argv:
        for m in methods:
            way_b(m); way_b(m)
        return
    out = {"shape": {"sources": ns, "walkers": nw, "steps": nsteps, "bands": 8}, "host_threads": THREADS}
    for m in methods:
        way_b(m); way_a(m)                                       # warm-up of both
        a, b = [], []
        for _ in range(3):
            ra = way_a(m); rb = way_b(m)
            a.append(ra[:3]); b.append(rb[:3])
        # the two ways agree (same seed, same chain; the host's FFT rounds differently, and a window decision that
        # is marginal under it may fall the other way: counted, not asserted)
        with np.errstate(invalid="ignore"):
            close = np.isclose(rb[3], ra[3], rtol=1e-6, equal_nan=True)
        res = {"a_stored_chain_then_host": {"wall_s": [x[0] for x in a], "run_mcmc_s": [x[1] for x in a],
                                            "host_autocorr_s": [x[2] for x in a], "bytes_back": int(ra[4])},
               "b_device_diagnostics": {"wall_s": [x[0] for x in b], "run_mcmc_summary_s": [x[1] for x in b],
                                        "convergence_s": [x[2] for x in b], "bytes_back": int(rb[4])},
               "tau_entries": int(close.size), "tau_entries_that_differ": int((~close).sum()),
               "tau_median": float(np.nanmedian(rb[3]))}
        for k in ("a_stored_chain_then_host", "b_device_diagnostics"):
            w = res[k]["wall_s"]
            res[k]["median_s"], res[k]["spread_s"] = float(np.median(w)), float(max(w) - min(w))
        out[m] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
