"""Writes tests/golden/evidence.npz: the cases of the evidence tests with their exact ln Z (data only).

    python tests/make_golden_evidence.py

A thin model without alpha at four plain wavelengths (tests/_evidence_ref.py ``case_settings``):
  (a) fnorm alone free: the posterior is Gaussian in fnorm, ln Z = -chisq_min / 2 + ln(2 pi / sum s_b^2 ivar_b) / 2 in
      longdouble, s_b the oracle's band fluxes at fnorm = 1;
  (b) T and fnorm free: scipy.integrate.dblquad of the oracle's P at epsrel 1e-10;
  (c) as (b) with a lower limit on T one posterior sigma below the posterior mean.
Needs scipy; the tests that read the file do not."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _evidence_ref as ER          # noqa: E402


def make():
    from oracle import oracle as O
    O.build()
    g = ER.make_cases(O)
    for k in sorted(g):
        print("%-16s %s" % (k, np.array2string(np.asarray(g[k]), precision=12)))
    np.savez(os.path.join(HERE, "golden", "evidence.npz"), **g)


if __name__ == "__main__":
    make()
