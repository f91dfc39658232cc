"""The device sampler's forms -- the plain launch train, form 7 (k_flowm) and form 9 (k_flowa with one, three and seven
walkers of each half per workgroup), each of which runs the SED constructor under its own setting and works lnprob out
in-kernel -- held to the oracle over the whole prior volume.  Every other test of them starts from a ball of a few
percent around a good fit; here the ensembles ARE the prior volume (tests/_domain_rows.py: ensemble): `wide250`, the
first 250 wide rows with a finite lnprob (T 3-200 K, beta 0.1-4.5, lambda0 5-3000 um, alpha 0.1-10, fnorm 0.01-1000 mJy;
250 walkers is the most form 7 takes), `wide576` (plain train and form 9 only) and `grid224`, the grid of table ends
(T 1-5000 K, lambda0 1-4500 um).  Seed 77; 8 stored steps, 3 unstored, 2 stored.  Held:

  1. every look-ahead form gives the plain train's chain, lnprobability, states and counts bit for bit, and really ran
     (last_kernel_form, no fall-back);
  2. every stored lnprobability is the oracle's lnprob of the stored position, at 1e-10 max(1, |lnprob|);
  3. every move is a legal one: the position after a step is the one before it exactly, or the stretch move's proposal --
     restated in numpy from the device's own previous positions and its Philox draws -- within relative 1e-13 (the
     bound of test_device_sampler_matches_host_emulation);
  4. the accept rule, wherever the oracle can decide it: with m = (d - 1) ln z + new - old - ln u and |m| beyond
     2e-10 (max(1, |new|) + max(1, |old|)), the walker moved iff m > 0; a proposal at -inf was rejected; fewer than 1 %
     of the moves are undecidable.  d is the number of columns the ensemble spans (4 ln z on the wide ensembles, 2 ln z
     on the grid's, whose alpha and fnorm are one value each: the library's rule for fixed columns);
  5. the test is not vacuous: at least 300 moves were accepted in the first 8 steps and the chain left the box it started
     in, in T, beta and alpha -- alpha where the ensemble spans it: the grid's one value stays that value exactly
     (tests/test_domain_sampler_cpu.py has the oracle emulation's figures: 445-598 accepted; the device made the very
     same numbers of moves, model by model).
No trajectory is compared with a host emulation: with |lnprob| up to 1e15 one decision within rounding of its threshold
would fork the chain with no bug behind it.  The boundary call is tests/test_domain_boundary_gpu.py's."""
import numpy as np
import pytest

from conftest import VARIANTS, lnl_close, parity_record, rec_allclose
import _domain_rows as D
from test_gpu_parity import _sampler_forms
from test_domain_paths_gpu import _cov

pytestmark = pytest.mark.gpu

ACCEPTED_FLOOR = 300
UNDECIDABLE_MAX = 0.01


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _form_of(opts):
    if not opts.get("lookahead_sampler"):
        return 1
    return 9 if opts.get("resident_sampler") == 2 else 7


def _forms_for(nw):
    """The forms an ensemble of nw walkers can take: form 7 up to 250 walkers; form 9 with W walkers of each half per
    workgroup while the workgroups fit the device (256 CUs: W = 1 up to 512 walkers)."""
    forms = _sampler_forms(None)
    if nw <= 250:
        return forms
    return [f for f in forms if _form_of(f[1]) == 1 or f[1].get("resident_walkers", 1) >= 3]


def _run(mbb, make, opts, p0):
    """One sampler of a fresh likelihood under the form's options: 8 stored steps, 3 unstored, 2 stored."""
    like = make()
    ctx = like.context
    for o, v in opts.items():
        ctx.set_option(o, v)
    nw = p0.shape[0]
    s = mbb.DeviceEnsembleSampler(nw, 5, like, seed=D.SEED)
    forms = []
    a = s.run_mcmc(p0, D.STEPS[0])
    forms.append(ctx.info("last_kernel_form"))
    nacc_a = s.naccepted.copy()
    b = s.run_mcmc(None, D.STEPS[1], storechain=False)
    forms.append(ctx.info("last_kernel_form"))
    c = s.run_mcmc(None, D.STEPS[2])
    forms.append(ctx.info("last_kernel_form"))
    assert forms == [_form_of(opts)] * 3 and ctx.info("flow_fallbacks") == 0, (forms, ctx.info("flow_fallbacks"))
    if _form_of(opts) == 9 and "resident_walkers" in opts:
        assert ctx.info("last_wpb") == opts["resident_walkers"]
    assert s.chain.shape == (nw, D.STEPS[0] + D.STEPS[2], 5)
    return dict(a_pos=a[0], a_lnp=a[1], b_pos=b[0], b_lnp=b[1], c_pos=c[0], c_lnp=c[1], chain=s.chain.copy(),
                lnp=s.lnprobability.copy(), nacc_a=nacc_a, nacc=s.naccepted.copy())


def _hold(orc, p0, r, label):
    """2. to 5. on one run's results."""
    nw = p0.shape[0]
    chain, lnp = r["chain"], r["lnp"]
    n0, n2 = D.STEPS[0], D.STEPS[2]
    nst = n0 + n2
    zpow = D.zpow_of(p0)

    def oracle(rows):
        out = orc(np.ascontiguousarray(rows), nthreads=4)
        assert np.all(orc.status <= 1), rows[orc.status > 1][:3]      # (the device stops a run for such a proposal)
        return out
    # 2. the stored lnprob is the oracle's
    ref = oracle(chain.reshape(-1, 5)).reshape(nw, nst)
    assert np.all(np.isfinite(ref))
    err = lnl_close(lnp, ref, kind="lnprob of the device sampler over the prior volume")
    ref_p0, ref_b = oracle(p0), oracle(r["b_pos"])
    lnl_close(r["b_lnp"], ref_b, kind="lnprob of the device sampler over the prior volume")
    assert np.array_equal(r["a_pos"], chain[:, n0 - 1]) and np.array_equal(r["a_lnp"], lnp[:, n0 - 1])
    assert np.array_equal(r["c_pos"], chain[:, -1]) and np.array_equal(r["c_lnp"], lnp[:, -1])
    # 3., 4.: step by step from the device's own positions
    nmoved = nundec = nmoves = 0
    worst = 0.0
    moved_all = np.zeros((nw, nst), dtype=bool)
    for t in range(nst):
        if t == 0:
            prev, old, step_no = p0, ref_p0, 1
        elif t == n0:
            prev, old, step_no = r["b_pos"], ref_b, n0 + D.STEPS[1] + 1
        else:
            prev, old, step_no = chain[:, t - 1], ref[:, t - 1], (t + 1 if t < n0 else t + D.STEPS[1] + 1)
        now = chain[:, t]
        q, z, lnu = D.proposals(prev, now[:nw // 2], D.SEED, step_no)
        moved = (now != prev).any(axis=1)
        moved_all[:, t] = moved
        if moved.any():
            rel = np.abs(now[moved] - q[moved]) / np.abs(q[moved])
            worst = max(worst, rel.max())
            rec_allclose(now[moved], q[moved], rtol=1e-13, kind="a move of the device sampler vs the proposal restated")
        stay = ~moved
        if t:                                       # (a walker that stays keeps its lnprob to the bit)
            assert np.array_equal(lnp[stay, t], (r["b_lnp"] if t == n0 else lnp[:, t - 1])[stay])
        new = np.where(moved, ref[:, t], np.nan)
        if stay.any():
            new[stay] = oracle(q[stay])
        assert not np.isnan(new).any()
        assert not (moved & np.isneginf(new)).any()
        m, decidable = D.accept_margin(zpow, z, lnu, new, old)
        wrong = decidable & (moved != (m > 0))
        assert not wrong.any(), (label, t, np.flatnonzero(wrong)[:5], m[wrong][:5], new[wrong][:5], old[wrong][:5])
        nmoves += nw
        nmoved += int(moved.sum())
        nundec += int((~decidable).sum())
    share = nundec / float(nmoves)
    first = int(moved_all[:, :n0].sum())
    print("    %s: lnprob %.3g of max(1, |lnprob|), |lnprob| up to %.3g; %d of %d moves made, %d in the first %d steps; "
          "worst move %.3g from its proposal; %d undecidable (%.3g %%)"
          % (label, err, np.abs(ref).max(), nmoved, nmoves, first, n0, worst, nundec, 100 * share))
    parity_record("undecidable moves of the device sampler (share)", share, UNDECIDABLE_MAX)
    assert share < UNDECIDABLE_MAX
    # 5. not vacuous
    assert np.array_equal(r["nacc_a"], moved_all[:, :n0].sum(axis=1))
    assert first >= ACCEPTED_FLOOR, first
    lo, hi = p0.min(axis=0), p0.max(axis=0)
    left = (chain < lo).any(axis=(0, 1)) | (chain > hi).any(axis=(0, 1))
    const = lo == hi
    assert np.all(left[[0, 1]]) and (left[3] or const[3]), (label, left)
    assert np.all(chain[:, :, const] == lo[const])


def _check(mbb, oracle, ens, opthin, noalpha, cov=False):
    which = ens[:4]
    p0 = D.ensemble(ens)
    p0.setflags(write=False)

    def make():
        flux = D.GRID_FLUX if which == "grid" else D.WIDE_FLUX
        return D.make_like(mbb, which, opthin, noalpha, cov=_cov(D.unc_of(flux)) if cov else None)
    forms = _forms_for(p0.shape[0])
    res = [_run(mbb, make, opts, p0) for _, opts in forms]
    # 1. the forms agree bit for bit
    for (form, _), r in zip(forms[1:], res[1:]):
        for key in res[0]:
            assert np.array_equal(res[0][key], r[key]), (ens, form, key)
    _hold(D.make_oracle(oracle, make()), p0, res[0], "%s%s" % (ens, ", covariance" if cov else ""))


@pytest.mark.parametrize("ens", ["wide250", "grid224"])
@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_sampler_forms_over_the_prior_volume(mbb, oracle, name, opthin, noalpha, ens):
    """All five forms from the form-7-sized ensembles."""
    _check(mbb, oracle, ens, opthin, noalpha)


@pytest.mark.parametrize("name,opthin,noalpha", VARIANTS)
def test_resident_form_from_576_wide_rows(mbb, oracle, name, opthin, noalpha):
    """The plain train and form 9 with three and seven walkers of each half per workgroup from nearly every finite
    wide row."""
    _check(mbb, oracle, "wide576", opthin, noalpha)


def test_sampler_forms_with_a_full_covariance(mbb, oracle):
    """All five forms on the thick model with alpha, the data's covariance full."""
    _check(mbb, oracle, "wide250", False, False, cov=True)
