"""Writes tests/golden/map.npz: the cases of the MAP-fit tests with their reference optima (data only).

    python tests/make_golden_map.py

Per case of tests/_map_ref.py ``case_specs``: the data (flux, unc), the starts, the settings, the reference optimum
(theta_ref, lnp_ref: the best of scipy.optimize.least_squares from every start, lnP by the oracle), the reference Laplace
covariance cov_ref and its own disagreement between two difference steps (cov_dis).  Needs scipy; the tests that read the
file do not."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _map_ref as MR          # noqa: E402


def make():
    from oracle import oracle as O
    O.build()
    g_pb = np.load(os.path.join(HERE, "golden", "passbands.npz"))
    out = {"bands": np.array(MR.BANDS), "truth": MR.TRUTH, "names": np.array(sorted(MR.case_specs()))}
    for name, (s, nstart) in sorted(MR.case_specs().items()):
        flux, unc = MR.make_data(O, g_pb, s)
        like = MR.oracle_like(O, g_pb, s, flux, unc)
        starts = MR.make_starts(s, nstart)
        best = None
        for x0 in starts:
            p, lnp = MR.ref_search(O, like, s, x0)
            if np.isfinite(lnp) and (best is None or lnp > best[1]):
                best = (p, lnp)
        cov, dis = MR.ref_cov(O, like, s, best[0])
        r = MR.residuals(O, like, s, best[0])
        print("%-18s lnP %.12g  theta %s  cov disagreement %.2e  r^T r + 2 lnP %.1e" %
              (name, best[1], np.array2string(best[0], precision=7), dis, r @ r + 2 * best[1]))
        out.update({name + "/flux": flux, name + "/unc": unc, name + "/starts": starts,
                    name + "/model": np.array([int(s["opthin"]), int(s["noalpha"])]),
                    name + "/lowlim": s["lowlim"], name + "/has_uplim": s["has_uplim"], name + "/uplim": s["uplim"],
                    name + "/has_gprior": s["has_gprior"], name + "/gmean": s["gmean"], name + "/gsigma": s["gsigma"],
                    name + "/theta_ref": best[0], name + "/lnp_ref": np.array(best[1]),
                    name + "/cov_ref": cov, name + "/cov_dis": np.array(dis)})
    np.savez(os.path.join(HERE, "golden", "map.npz"), **out)


if __name__ == "__main__":
    make()
