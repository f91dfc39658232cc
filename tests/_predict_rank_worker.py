"""Worker of test_sharded_run_is_refused_by_the_library (tests/test_predict_gpu.py): two ranks as processes on ONE GPU
with a communicator over tests/rccl_standin/ (MBB_RCCL_LIB), as tests/_rccl_worker.py.  A sharded sampler run leaves
each rank only its own walkers' chain: mbb_sampler_predict refuses it with MBB_ERR_STATE, as mbb_sampler_diagnostics
and mbb_sampler_marginals do, and so does the Python layer before it gets there."""
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
    from mbb_emcee_amd import _native, predict
    from mbb_emcee_amd.parallel import RcclComm
    g = np.load(os.path.join(ROOT, "tests", "golden", "lnlike.npz"))
    bands = [str(b) for b in g["cfg2/bands"]]
    like = mbb.likelihood(response=True, device=0)
    like.set_phot(bands, g["cfg2/thick_walpha/flux"], g["cfg2/thick_walpha/unc"])
    ctx = like._sync_device()
    uid = side.allgather_bytes(ctx.comm_unique_id() if rank == 0 else b"")[0]
    comm = RcclComm(ctx, rank, world, uid)
    assert ctx.info("nranks") == world
    nw = 24 * world
    rng = np.random.RandomState(3)                                # the same on every rank
    p0 = np.array([12.0, 1.8, 600.0, 3.0, 40.0]) * (1.0 + 0.02 * rng.normal(size=(nw, 5)))
    smp = mbb.DeviceEnsembleSampler(nw, 5, like, seed=21)
    for kw in (dict(predict=[70.0]), dict(predict=dict(specs="SCUBA2_450um"), summary=True)):
        try:
            smp.run_mcmc(p0, 4, **kw)
            raise AssertionError("predict= of a sharded run must be refused")
        except ValueError as e:
            assert "sharded" in str(e), str(e)
    smp.run_mcmc(p0, 6)
    req = predict._Request(like, [70.0, "SCUBA2_450um"], [16.0, 84.0])
    raw = predict._Raw(1, 2, 2)
    spec, out = req.spec(), raw.out()
    _, h = smp._handle()
    rc = ctx.lib.mbb_sampler_predict(ctx.h, h, C.byref(spec), C.byref(out))
    msg = ctx.lib.mbb_last_error().decode()
    assert rc == -3 and "sharded" in msg and "predicted from" in msg, (rc, msg)
    try:
        smp.predictions(70.0)
        raise AssertionError("predictions() of a sharded run must be refused")
    except ValueError as e:
        assert "no chain of this sampler is resident" in str(e), str(e)
    # the host chain every rank ends with can be predicted from as any other
    assert mbb.chain_predictions(like, smp.chain, [70.0, "SCUBA2_450um"]).n_used[0] == nw * 6
    del smp
    import gc
    gc.collect()
    side.barrier()
    comm.close()
    side.barrier()
    print("PREDICT_RANKS_OK %d" % rank)


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        try:
            open(os.path.join(os.environ["MBB_TEST_RDZV_DIR"], "abort"), "w").close()
        except Exception:
            pass
        raise
