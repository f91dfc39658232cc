"""tests/golden/sampler_chain_parent.npz: what the device sampler made of a fixed seed BEFORE the exponent of z in the accept
test became a launch argument (the commit "Test device math, SED constructor and per-sample f_nu at high precision").
Run on an MI355X with that commit's library built and this file and tests/test_sampler_statistics_gpu.py copied into
its tree:

    python tests/golden/make_golden_sampler_chain.py [OUT.npz]

The run is tests/test_sampler_statistics_gpu.py's parent_chain; the one-launch form and the launch train must agree
before anything is written."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

if __name__ == "__main__":
    import mbb_emcee_amd as mbb
    from test_sampler_statistics_gpu import parent_chain
    g_lnl = np.load(os.path.join(HERE, "lnlike.npz"))
    a, fa = parent_chain(mbb, g_lnl, 1)
    b, fb = parent_chain(mbb, g_lnl, 0)
    assert (fa, fb) == (7, 1), (fa, fb)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "sampler_chain_parent.npz")
    np.savez_compressed(out, **a)
    print("wrote", out, {k: v.shape for k, v in a.items()})
