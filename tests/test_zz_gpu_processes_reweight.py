"""The reweighting's refusal of sharded contexts, which takes two processes: collected last, with the other process tests
(tests/conftest.py sorts by this file's name)."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_sharded_contexts_are_refused():
    """Two ranks as processes on this GPU with a communicator over tests/rccl_standin/: mbb_chain_reweight and
    mbb_sampler_reweight answer MBB_ERR_STATE for a sharded target and for a sharded owner of the chain, write nothing,
    and reweight again once the communicator is gone (tests/_reweight_rank_worker.py).  The refusal of a target on
    ANOTHER device needs two GPUs and is not run here: its check is one comparison of the two contexts' device numbers
    ahead of every other in mbb_sampler_reweight."""
    from _filecomm import launch
    d = os.path.join(ROOT, "tests", "rccl_standin")
    so, src = os.path.join(d, "librccl_standin.so"), os.path.join(d, "rccl_standin.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-shared", "-fPIC", "-o", so, src, "-lrt"])
    ok, text = launch(os.path.join(ROOT, "tests", "_reweight_rank_worker.py"), 2, extra_env={"MBB_RCCL_LIB": so}, timeout=300.0)
    assert ok and "REWEIGHT_RANKS_OK 0" in text and "REWEIGHT_RANKS_OK 1" in text, text[-6000:]
