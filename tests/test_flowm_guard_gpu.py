"""Sampler form 7 (k_flowm) held bitwise to the plain launch train (form 1) where its sharded lag guard can go wrong: the
completion counters are done[2][ring][shards], a workgroup arrives on the counter of its number mod the shards, the accept
test's wave asks every non-empty shard for the workgroups that arrive on it, a launch uses one of the two sets and clears
every shard of the other for the sampler's next launch (mbb_flow_index.h: fm_shard, fm_shard_wgs, fm_done_word).  A
mistake there does not give wrong numbers: a guard that never opens ends in a bounded give-up (error 9) and a silent redo
as a launch train, which passes every bitwise check; one that opens too early lets a slot be overwritten under a reader,
who then waits for a check word that never comes -- the same end.  So every case also asserts that every launch was form
7's, that no fall-back was counted and that no RuntimeWarning was raised.
Needs an MI355X: `pytest -m gpu`.

Shapes: ensembles of 2 walkers (two workgroups: shards 2 and 3 are empty), 4 (one workgroup per shard), 18 (uneven shards:
5, 5, 4, 4 workgroups), 34, and the bench's 250 once; runs of 1, 2 and 5 steps (shorter than the lag, and the ring of eight counters per
shard not yet wrapped) and of 40 (ten rounds of the ring); each run is followed on the same sampler by launches of 3 and of 40
steps -- the two sets of counters alternate, and each launch finds every shard of its set as the launch before cleared it;
one case whose first run on the sampler is the plain train, so that the counters form 7 finds are the host's clear; the
four-band set (a workgroup of fewer than 16 waves) once.  Compared after every launch: positions, ln p, and the accepted
moves per walker (exactly); at the end the chain and its ln p.

A guard that is too LENIENT shows in none of that: under the GPU's own timing no workgroup runs four half-steps ahead of
another, the guard never binds, and a reader that ignores a shard or a clear that leaves a shard's old totals behind
passes every bitwise check (profiles/r13/form7.txt, item d).  Two things hold it all the same, through the sampler's
flow_counters() hook.  After every form 7 launch the counters are read back: in the set the launch used every (ring slot,
shard) holds exactly the workgroups that arrive on the shard times the half-steps of the launch that fall on the slot,
and every counter of the other set is zero -- a clear that covers shard 0 only, arrivals on another line than the reader
asks, a set used twice all fail there.  And one case per ensemble pre-loads the set about to be used so that every shard
but the last non-empty one is satisfied for good and the last one never is (it starts at -1: its total stays one short):
a reader that asks every shard takes the bounded give-up -- a fall-back is counted, the warning raised, the run redone as
a train with the same chain --, one that ignores the last shard runs through as form 7 and the case fails."""
import warnings

import numpy as np
import pytest

from test_flowm_arbitration_gpu import PLAIN, FORM7, _sampler, _eight, _four, _start

pytestmark = pytest.mark.gpu

FOLLOW = (3, 40)                          # the launches that follow a case's first run on the same sampler


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _shard_wgs(grid, s, shards):
    return (grid - s + shards - 1) // shards if grid > s else 0


def _check_counters(s, nw, nsteps, used):
    """What a form 7 launch of nsteps steps leaves in the counters; returns the set the next launch uses."""
    c, nxt = s.flow_counters()
    _, ring, shards = c.shape
    assert used in (None, nxt ^ 1), (used, nxt)                     # (the sets alternate)
    used = nxt ^ 1
    want = np.array([[_shard_wgs(nw, sh, shards) * len(range(slot, 2 * nsteps, ring)) for sh in range(shards)] for slot in range(ring)],
                    dtype=np.uint64)
    assert np.array_equal(c[used], want), (nw, nsteps, c[used].tolist(), want.tolist())
    assert not c[used ^ 1].any(), (nw, nsteps, c[used ^ 1].tolist())    # (cleared, every shard, for the next launch)
    return nxt


def _launches(mbb, like, plan, nw, p0, seed):
    """plan: [(options, steps), ...] on one sampler.  Returns what every launch left, the forms, the fall-backs counted."""
    ctx = like.context
    fallbacks = ctx.info("flow_fallbacks")
    out, forms = [], []
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        s, nxt = None, None
        for opts, nsteps in plan:
            for o, v in opts.items():
                ctx.set_option(o, v)
            if s is None:
                s = _sampler(mbb, nw, like, seed)
                pos, lnp, _ = s.run_mcmc(p0, nsteps)
            else:
                pos, lnp, _ = s.run_mcmc(None, nsteps)
            forms.append(ctx.info("last_kernel_form"))
            out.append((pos.copy(), lnp.copy(), s.naccepted.copy()))
            if forms[-1] == 7:
                nxt = _check_counters(s, nw, nsteps, nxt)
        out.append((s.chain.copy(), s.lnprobability.copy(), s.naccepted.copy()))
    return out, forms, ctx.info("flow_fallbacks") - fallbacks


def _held(mbb, g_lnl, make, nw, seed, steps, first_plain=0):
    p0 = _start(nw, seed)
    lead = [(PLAIN, first_plain)] if first_plain else []
    ref, forms, _ = _launches(mbb, make(mbb, g_lnl), lead + [(PLAIN, n) for n in steps], nw, p0, seed)
    assert set(forms) == {1}
    got, forms, grew = _launches(mbb, make(mbb, g_lnl), lead + [(FORM7, n) for n in steps], nw, p0, seed)
    assert forms == [1] * len(lead) + [7] * len(steps) and grew == 0, (forms, grew)
    for k, (x, y) in enumerate(zip(ref, got)):
        for a, b in zip(x, y):
            assert np.array_equal(a, b, equal_nan=True), (nw, steps, k)
    total = sum(steps) + first_plain
    assert ref[-1][0].shape == (nw, total, 5) and np.isfinite(ref[-1][1]).all()
    assert ref[-1][2].sum() > 0 or total < 3          # (moves were accepted: the counts compared are not all zero)
    return ref


@pytest.mark.parametrize("nsteps", (1, 2, 5, 40))
@pytest.mark.parametrize("nw", (4, 18, 34))
def test_form7_equals_the_launch_train_with_the_sharded_guard(mbb, g_lnl, nw, nsteps):
    _held(mbb, g_lnl, _eight, nw, 71 + nw, (nsteps,) + FOLLOW)


def test_two_walkers_leave_shards_empty(mbb, g_lnl):
    _held(mbb, g_lnl, _eight, 2, 73, (40,) + FOLLOW)


def test_the_bench_ensemble(mbb, g_lnl):
    _held(mbb, g_lnl, _eight, 250, 77, (40,) + FOLLOW)


def test_after_a_plain_launch_train_the_host_clears_every_shard(mbb, g_lnl):
    _held(mbb, g_lnl, _eight, 18, 79, (5,) + FOLLOW, first_plain=3)


def test_four_bands_fewer_than_16_waves(mbb, g_lnl):
    _held(mbb, g_lnl, _four, 18, 83, (5,) + FOLLOW)


@pytest.mark.parametrize("nw", (2, 4, 18, 34))
def test_a_reader_that_asks_every_shard_gives_up_when_the_last_one_is_short(mbb, g_lnl, nw):
    """The set about to be used pre-loaded: every shard but the last non-empty one far past anything asked, the last one at
    -1, so that its total is one short of what is asked for ever.  The kernel's reader must not get through."""
    seed, steps = 87 + nw, 40
    p0 = _start(nw, seed)
    ref, forms, _ = _launches(mbb, _eight(mbb, g_lnl), [(PLAIN, 5), (PLAIN, steps), (PLAIN, 3)], nw, p0, seed)
    like = _eight(mbb, g_lnl)
    ctx = like.context
    for o, v in FORM7.items():
        ctx.set_option(o, v)
    s = _sampler(mbb, nw, like, seed)
    s.run_mcmc(p0, 5)
    assert ctx.info("last_kernel_form") == 7
    c, nxt = s.flow_counters()
    _, ring, shards = c.shape
    last = min(nw, shards) - 1
    assert _shard_wgs(nw, last, shards) > 0 and not c[nxt].any()
    c[nxt, :, :last] = np.uint64(1) << np.uint64(62)
    c[nxt, :, last] = np.uint64(0xFFFFFFFFFFFFFFFF)
    c2, _ = s.flow_counters(store=c)
    assert np.array_equal(c2, c)
    fallbacks = ctx.info("flow_fallbacks")
    ctx.set_option("flow_spin_log2", 12)                    # (a give-up within milliseconds)
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            pos, lnp, _ = s.run_mcmc(None, steps)
    finally:
        ctx.set_option("flow_spin_log2", 0)
    assert ctx.info("flow_fallbacks") - fallbacks == 1, "the reader got through a guard whose last shard was never satisfied"
    assert any(issubclass(w.category, RuntimeWarning) for w in seen)
    assert np.array_equal(pos, ref[1][0]) and np.array_equal(lnp, ref[1][1]) and np.array_equal(s.naccepted, ref[1][2])
    # ... and the next launch is form 7's again, on counters the host has cleared
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        pos, lnp, _ = s.run_mcmc(None, 3)
    assert ctx.info("last_kernel_form") == 7 and ctx.info("flow_fallbacks") - fallbacks == 1
    _check_counters(s, nw, 3, None)
    assert np.array_equal(pos, ref[2][0]) and np.array_equal(lnp, ref[2][1])
    assert np.array_equal(s.chain, ref[-1][0]) and np.array_equal(s.lnprobability, ref[-1][1])
