"""Worker of test_sharded_context_is_refused (tests/test_map_gpu.py): two ranks as processes on ONE GPU with a
communicator over tests/rccl_standin/ (MBB_RCCL_LIB), as tests/_predict_rank_worker.py.  A context that is one rank of a
sharded run is refused by mbb_map_fit with MBB_ERR_STATE: every rank would repeat the whole search.  Once the
communicator is gone the same context fits as any other."""
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
    from mbb_emcee_amd import _native, optimize
    from mbb_emcee_amd.parallel import RcclComm
    g = np.load(os.path.join(ROOT, "tests", "golden", "map.npz"))
    name = "thin_walpha_s5"
    like = mbb.likelihood(response=True, opthin=True, device=0)
    like.set_phot([str(b) for b in g["bands"]], g[name + "/flux"], g[name + "/unc"])
    like.set_uplim(2, 2550.0)
    starts = g[name + "/starts"][:2]
    ctx = like._sync_device()
    before = optimize.map_fit(like, starts[None], squeeze=True)
    uid = side.allgather_bytes(ctx.comm_unique_id() if rank == 0 else b"")[0]
    comm = RcclComm(ctx, rank, world, uid)
    assert ctx.info("nranks") == world
    req = optimize._Request(like, starts[None])
    raw = optimize._Raw(1, 2, 6)
    spec, out = req.spec(), raw.out()
    rc = ctx.lib.mbb_map_fit(ctx.h, C.byref(spec), C.byref(out))
    msg = ctx.lib.mbb_last_error().decode()
    assert rc == -3 and "sharded" in msg and "map fit" in msg, (rc, msg)
    assert np.all(np.isnan(raw.params))                              # nothing was written
    try:
        optimize.map_fit(like, starts[None])
        raise AssertionError("map_fit on a sharded context must be refused")
    except _native.NativeError as e:
        assert "sharded" in str(e), str(e)
    side.barrier()
    comm.close()
    side.barrier()
    after = optimize.map_fit(like, starts[None], squeeze=True)
    assert np.array_equal(after.params_all, before.params_all) and np.array_equal(after.lnprob_all, before.lnprob_all)
    print("MAP_RANKS_OK %d" % rank)


if __name__ == "__main__":
    try:
        main()
    except BaseException:
        try:
            open(os.path.join(os.environ["MBB_TEST_RDZV_DIR"], "abort"), "w").close()
        except Exception:
            pass
        raise
