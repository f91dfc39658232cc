"""Worker of test_sharded_contexts_are_refused (tests/test_zz_gpu_processes_reweight.py): two ranks as processes on ONE
GPU with a communicator over tests/rccl_standin/ (MBB_RCCL_LIB), as tests/_map_rank_worker.py.  A context that is one
rank of a sharded run is refused by mbb_chain_reweight as the target, and by mbb_sampler_reweight as the target and as the
owner of the chain, with MBB_ERR_STATE and nothing written.  Once the communicator is gone the same contexts reweight
as any other."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    from _filecomm import FileComm
    side = FileComm()
    rank, world = side.rank, side.world
    assert os.environ.get("MBB_RCCL_LIB", "").endswith("librccl_standin.so")
    import mbb_emcee_amd as mbb
    from mbb_emcee_amd import _native, reweight
    from mbb_emcee_amd.parallel import RcclComm
    truth = np.array([12.0, 1.8, 600.0, 3.0, 40.0])
    wave = [100.0, 250.0, 500.0, 850.0]
    nw, nsteps = 12, 10

    def make(prior):
        lk = mbb.likelihood(device=0)
        lk.set_phot(wave, np.ones(4), np.ones(4))
        flux = lk.model_flux(truth)[0]
        lk.set_phot(wave, flux, 0.1 * flux + 1.0)
        if prior:
            lk.set_gaussian_prior("beta", 2.0, 0.3)
        return lk

    like, other = make(False), make(True)
    p0 = truth * (1.0 + 0.02 * np.random.RandomState(3).normal(size=(nw, 5)))
    sm = mbb.DeviceEnsembleSampler(nw, 5, like, seed=9)
    sm.run_mcmc(p0, nsteps)
    so = mbb.DeviceEnsembleSampler(nw, 5, other, seed=9)
    so.run_mcmc(p0, nsteps)
    before = sm.reweight(other)
    ctx = like._sync_device()
    octx = other._sync_device()
    uid = side.allgather_bytes(ctx.comm_unique_id() if rank == 0 else b"")[0]
    comm = RcclComm(ctx, rank, world, uid)
    assert ctx.info("nranks") == world

    def call(entry, *args):
        req = reweight._Request(other)
        raw = reweight._Raw(1, len(req.qs))
        spec, out = req.spec(), raw.out()
        rc = entry(*(args + (C.byref(spec), C.byref(out))))
        assert np.all(np.isnan(raw.mean)) and np.all(raw.n_used == 0) or rc == 0        # nothing was written
        return rc, ctx.lib.mbb_last_error().decode()

    chain, lnp = np.ascontiguousarray(sm.chain[None]), np.ascontiguousarray(sm.lnprobability[None])
    # the sharded context as the target of a host chain
    rc, msg = call(ctx.lib.mbb_chain_reweight, ctx.h, _native._d(chain), _native._d(lnp), 1, nw, nsteps)
    assert rc == -3 and "sharded" in msg and "reweight" in msg, (rc, msg)
    # ... as the target of another context's resident chain
    rc, msg = call(ctx.lib.mbb_sampler_reweight, octx.h, so._handle()[1], ctx.h)
    assert rc == -3 and "sharded" in msg and "reweight" in msg, (rc, msg)
    # ... and as the owner of the chain
    rc, msg = call(ctx.lib.mbb_sampler_reweight, ctx.h, sm._handle()[1], octx.h)
    assert rc == -3 and "sharded" in msg, (rc, msg)
    side.barrier()
    comm.close()
    side.barrier()
    after = sm.reweight(other)
    for f in ("khat", "ess", "lnz_ratio", "mean", "pct", "cov", "best", "n_used", "status", "weight_sum"):
        assert np.array_equal(getattr(after._raw, f), getattr(before._raw, f), equal_nan=True), f
    print("REWEIGHT_RANKS_OK %d" % rank)


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        try:
            open(os.path.join(os.environ["MBB_TEST_RDZV_DIR"], "abort"), "w").close()
        except Exception:
            pass
        raise
