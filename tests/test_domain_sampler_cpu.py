"""What tests/test_domain_sampler_gpu.py relies on, asserted with the oracle alone (no GPU).  The GPU tests start the device
sampler from ensembles that span the prior volume and hold every move to the oracle; that says something only if the
ensembles really move, really leave the neighbourhood of a fit, and leave few moves too close to their threshold to be
decided.  Here the stretch move is run on the host with the device's own draws (tests/_domain_rows.py: emulate) and the
ORACLE as the likelihood, seed 77 over 8 steps:

  * the frozen ensembles are what they are said to be: `wide250` / `wide576` the first 250 / 576 wide rows whose oracle
    lnprob -- limits and the lambda_peak prior included -- is finite, in every model; `grid224` finite everywhere;
  * no proposal of the emulation is a row the oracle cannot build (the device sampler would stop the run for one);
  * the ensembles move: accepted moves counted per model, the exact figures beside the assertions;
  * the chains leave the starting box: the ranges reached, per ensemble over the four models;
  * fewer than 1 % of the moves are within 2e-10 (max(1, |new|) + max(1, |old|)) of their threshold.
The exponent of z in the accept test is the number of columns the ensemble spans, less one (the library's rule for
columns that are constant over the ensemble): 4 on the wide ensembles, 2 on the grid's, whose alpha and fnorm are one
value each.
"""
import numpy as np
import pytest

from conftest import VARIANTS
import _domain_rows as D

NSTEPS = D.STEPS[0]
_CACHE = {}


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def oracle_like(mbb, oracle, which, opthin, noalpha):
    """The oracle's likelihood of the wide set (default limits, the lambda_peak prior) or of the grid set (lambda0's
    upper limit at 5000 um): what the GPU tests hold the device to."""
    return D.make_oracle(oracle, D.make_like(mbb, which, opthin, noalpha))


def _emulation(mbb, oracle, name, opthin, noalpha):
    key = (name, opthin, noalpha)
    if key not in _CACHE:
        orc = oracle_like(mbb, oracle, name[:4], opthin, noalpha)
        seen = []

        def lnprob(rows):
            out = orc(rows, nthreads=4)
            seen.append(orc.status.copy())
            return out
        res = D.emulate(lnprob, D.ensemble(name), D.SEED, NSTEPS)
        _CACHE[key] = res + (np.concatenate(seen),)
    return _CACHE[key]


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_the_wide_ensembles_are_the_first_finite_rows(mbb, oracle, name, opthin, noalpha):
    orc = oracle_like(mbb, oracle, "wide", opthin, noalpha)
    rows = D.wide_rows()
    lnp = orc(rows, nthreads=4)
    assert not np.isnan(lnp).any() and np.all(orc.status <= 1)
    fin = np.isfinite(lnp)
    assert np.array_equal(fin, ~(rows < D.LOWLIM).any(axis=1))
    assert fin.sum() == 578                                  # of 600: at least 90 %, and at least 576
    for n in (250, 576):
        assert np.array_equal(D.ensemble("wide%d" % n), rows[np.flatnonzero(fin)[:n]])
    grid = oracle_like(mbb, oracle, "grid", opthin, noalpha)
    lnp = grid(D.ensemble("grid224"), nthreads=4)
    assert np.all(np.isfinite(lnp)) and np.all(grid.status == 0)
    assert D.zpow_of(D.ensemble("wide250")) == 4.0 and D.zpow_of(D.ensemble("grid224")) == 2.0


def test_the_huge_rows_are_fifteen_of_each_good_row():
    rows, what = D.huge_rows()
    assert rows.shape == (45, 5) and len(set(what)) == 45
    assert sorted(set(rows[:, 1]) | set(rows[:, 3])) == sorted({1.7, 2.2} | set(D.HUGE))


# accepted moves of the oracle emulation, seed 77, 8 steps: of 2000 on wide250, of 1792 on grid224
ACCEPTED = {("wide250", "thin_noalpha"): 445, ("wide250", "thin_walpha"): 453,
            ("wide250", "thick_noalpha"): 526, ("wide250", "thick_walpha"): 526,
            ("grid224", "thin_noalpha"): 511, ("grid224", "thin_walpha"): 485,
            ("grid224", "thick_noalpha"): 598, ("grid224", "thick_walpha"): 576}
UNDECIDABLE_MAX = 0.01


@pytest.mark.parametrize("ens", ["wide250", "grid224"])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_the_ensembles_move_and_few_moves_are_undecidable(mbb, oracle, name, opthin, noalpha, ens):
    chain, lnp, moved, decid, status = _emulation(mbb, oracle, ens, opthin, noalpha)
    assert np.all(status <= 1)                       # every proposal is a row the oracle builds, or one below a limit
    assert np.all(np.isfinite(lnp))
    nacc, nmoves = int(moved.sum()), moved.size
    share = 1.0 - decid.mean()
    print("    %s %s: accepted %d of %d moves, %d undecidable (%.3g %%), |lnprob| up to %.3g"
          % (ens, name, nacc, nmoves, (~decid).sum(), 100 * share, np.abs(lnp).max()))
    assert nmoves == {"wide250": 2000, "grid224": 1792}[ens]
    assert nacc == ACCEPTED[(ens, name)]
    assert nacc >= 400                               # (the GPU test's floor is 300)
    assert share < UNDECIDABLE_MAX


@pytest.mark.parametrize("ens", ["wide250", "grid224"])
def test_the_chains_leave_the_starting_box(mbb, oracle, ens):
    """Over the four models: the ranges the chains reach in 8 steps, against the box the ensemble starts in."""
    p0 = D.ensemble(ens)
    lo, hi = p0.min(axis=0), p0.max(axis=0)
    clo, chi = np.full(5, np.inf), np.full(5, -np.inf)
    for name, opthin, noalpha in VARIANTS:
        chain = _emulation(mbb, oracle, ens, opthin, noalpha)[0]
        clo = np.minimum(clo, chain.reshape(-1, 5).min(axis=0))
        chi = np.maximum(chi, chain.reshape(-1, 5).max(axis=0))
        left = (chain < lo).any(axis=(0, 1)) | (chain > hi).any(axis=(0, 1))
        print("    %s %s: left the starting box in columns %s" % (ens, name, np.flatnonzero(left)))
        # (a column that is one value over the ensemble -- the grid's alpha and fnorm -- stays that value exactly)
        const = lo == hi
        assert np.all(left[:3]) and np.all(left[3:] | const[3:]), (name, left)
        assert np.all(chain[:, :, const] == lo[const])
    print("    %s: T %.3g-%.3g K, beta %.3g-%.3g, lambda0 %.3g-%.3g um, alpha %.3g-%.3g, fnorm %.3g-%.3g"
          % ((ens,) + tuple(np.column_stack([clo, chi]).ravel())))
    want = REACHED[ens]
    np.testing.assert_allclose(np.column_stack([clo, chi]), want, rtol=5e-3)


# the ranges reached (min, max per column: T, beta, lambda0, alpha, fnorm), to three digits
REACHED = {"wide250": [[2.39, 468.0], [0.121, 14.1], [1.82, 3810.0], [0.1, 17.9], [0.00804, 1150.0]],
           "grid224": [[1.0, 11800.0], [0.101, 9.68], [1.0, 15000.0], [2.5, 2.5], [40.0, 40.0]]}
