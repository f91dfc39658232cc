"""One context across every seam at which the host library remakes a buffer, twice, against fresh contexts.

Every device and pinned block of a context or a sampler is an owner that is remade through one grow()
(mbb_emcee_amd/csrc/mbb_owned.h).  What a call computes must not depend on what the context's buffers went through
before it: here one context is driven over every growth seam -- boundary blocks, model fluxes, SED scratch, SED
outputs, the chain store, the analyses' work buffers, a second sampler -- and every array that comes back is compared,
bit for bit, with the same call on a context that has done nothing else.  The analyses that reduce columns share one
set of work buffers (StatWork, mbb_hip.hip): a second test runs them one after the other over one resident chain."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240917
NW = 8


@pytest.fixture(scope="module")
def mbb():
    import mbb_emcee_amd
    return mbb_emcee_amd


def _sampler(ctx):
    h = C.c_void_p()
    from mbb_emcee_amd import _native
    _native._check(ctx.lib.mbb_sampler_create(ctx.h, NW, SEED, C.byref(h)))
    return h


def _run(ctx, h, p0, nsteps, store=True):
    """set_state(p0), then nsteps steps: the stored chain, its lnprob, the final state and the acceptance counts."""
    from mbb_emcee_amd import _native
    _d = _native._d
    p0 = np.ascontiguousarray(p0)
    _native._check(ctx.lib.mbb_sampler_set_state(ctx.h, h, _d(p0), None))
    chain, lnp = np.empty((NW, nsteps, 5)), np.empty((NW, nsteps))
    pos, lnprob, nacc = np.empty((NW, 5)), np.empty(NW), np.empty(NW)
    _native.check_arg(ctx.lib.mbb_sampler_run(ctx.h, h, nsteps, 2.0, _d(chain) if store else None, _d(lnp) if store else None,
                                              _d(pos), _d(lnprob), _d(nacc)), ctx)
    out = {"pos": pos, "lnprob": lnprob, "nacc": nacc}
    if store:
        out.update(chain=chain, chain_lnprob=lnp)
    return out


def _raw_arrays(raw):
    return {k: v for k, v in sorted(vars(raw).items()) if isinstance(v, np.ndarray)}


def _summary(ctx, h):
    from mbb_emcee_amd import _native, results
    req = results._Request([15.85, 50.0, 84.15])
    raw = results._Raw(1, len(req.qs))
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_sampler_run_summary(ctx.h, h, 0, 2.0, C.byref(spec), C.byref(out), None, None, None, None,
                                                      None), ctx)
    return _raw_arrays(raw)


def _convergence(ctx, h):
    from mbb_emcee_amd import _native, diagnostics
    req = diagnostics._Request(0, 5.0, 50.0, "mean", 4)
    raw = diagnostics._Raw(1, req.nacf)
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_sampler_diagnostics(ctx.h, h, C.byref(spec), C.byref(out)), ctx)
    return _raw_arrays(raw)


def _marginals(ctx, h):
    from mbb_emcee_amd import _native, marginals
    req = marginals._Request(bins=16, bins2d=8, nsources=1)
    raw = marginals._Raw(1, req.bins, req.bins2d, len(req.pairs))
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_sampler_marginals(ctx.h, h, C.byref(spec), C.byref(out)), ctx)
    return _raw_arrays(raw)


def _generation(ctx):
    return int(C.cast(ctx.lib.mbb_boundary_generation(ctx.h), C.POINTER(C.c_uint64))[0])


def _buffers(ctx, nmax):
    _, rows, lnl, st, _, _ = ctx.boundary_views(nmax)
    return rows.ctypes.data, lnl.ctypes.data, st.ctypes.data


def test_one_context_across_every_growth_seam_equals_fresh_contexts(mbb):
    import bench
    helper = mbb.likelihood(response=True)
    helper.set_phot(bench.BANDS, np.ones(8), np.ones(8))
    flux = helper.model_flux(bench.TRUTH)[0]
    helper.context.close()
    rows = np.ascontiguousarray(bench.walkers(1)[:300])          # the bench's ball around its truth: every row valid
    p0 = rows[:NW]
    grid4 = np.array([300.0, 600.0, 1200.0, 2400.0])
    grid16 = np.geomspace(100.0, 6000.0, 16)

    def make():
        like = mbb.likelihood(response=True)
        like.set_phot(bench.BANDS, flux, 0.1 * flux + 1.0)
        return like, like._sync_device()

    def named(prefix, arrays):
        return {"%s.%s" % (prefix, k): v for k, v in arrays.items()}

    # every call of the lifecycle, by name: what it runs on a context (state: the samplers it has made)
    def boundary(n):
        def call(like, ctx, st):
            lnl, status, mflux = ctx.lnlike_batch(rows[:n], want_flux=True)
            return {"call": np.array(like(rows[:n])), "lnl": lnl, "status": status, "model_flux": mflux}
        return call

    def prologue(n):
        return lambda like, ctx, st: dict(zip(("out", "status"), ctx.sed_prologue(rows[:n], False, False, 500.0, want_peak=True)))

    def sed_eval(n, grid):
        return lambda like, ctx, st: dict(zip(("out", "status"), ctx.sed_eval(rows[:n], False, False, 500.0, grid)))

    def run(nsteps, which="s1"):
        def call(like, ctx, st):
            if which not in st:
                st[which] = _sampler(ctx)
            return _run(ctx, st[which], p0, nsteps)
        return call

    def second_sampler(like, ctx, st):
        from mbb_emcee_amd import _native
        _native._check(ctx.lib.mbb_sampler_destroy(ctx.h, st.pop("s1")))
        return run(4, "s2")(like, ctx, st)

    steps = [
        ("boundary200a", boundary(200)), ("boundary300", boundary(300)), ("boundary200b", boundary(200)),
        ("prologue60", prologue(60)), ("eval60x4", sed_eval(60, grid4)), ("prologue70", prologue(70)), ("eval70x4", sed_eval(70, grid4)),
        ("eval60x16", sed_eval(60, grid16)), ("eval70x16", sed_eval(70, grid16)),
        ("run4", run(4)), ("run8", run(8)),
        ("summary", lambda like, ctx, st: _summary(ctx, st["s1"])),
        ("convergence", lambda like, ctx, st: _convergence(ctx, st["s1"])),
        ("marginals", lambda like, ctx, st: _marginals(ctx, st["s1"])),
        ("second_sampler", second_sampler),
    ]
    # what a fresh context has to have done before a call can be made on it at all (no buffer the call uses is made by it
    # at another size: the sampler's life is 4 steps old, nothing of them stored; the analysed chain is the 8-step run's)
    def unstored4(like, ctx, st):
        st["s1"] = _sampler(ctx)
        _run(ctx, st["s1"], p0, 4, store=False)

    def resident8(like, ctx, st):
        unstored4(like, ctx, st)
        _run(ctx, st["s1"], p0, 8)

    before = {"run8": unstored4, "summary": resident8, "convergence": resident8, "marginals": resident8,
              "second_sampler": lambda like, ctx, st: st.update(s1=_sampler(ctx))}

    def close(ctx, st):
        from mbb_emcee_amd import _native
        for h in st.values():
            _native._check(ctx.lib.mbb_sampler_destroy(ctx.h, h))
        ctx.close()

    fresh = {}
    for name, call in steps:
        like, ctx = make()
        st = {}
        if name in before:
            before[name](like, ctx, st)
        fresh.update(named(name, call(like, ctx, st)))
        close(ctx, st)
    assert len(fresh) >= 45 and all(isinstance(v, np.ndarray) and v.size for v in fresh.values())

    lives = []
    for life in range(3):
        like, ctx = make()
        st, got, bumps = {}, {}, []
        gen = _generation(ctx)
        held = None
        for name, call in steps:
            got.update(named(name, call(like, ctx, st)))
            if _generation(ctx) != gen:
                assert _generation(ctx) == gen + 1, name
                gen += 1
                bumps.append(name)
            if name == "boundary200b":
                held = _buffers(ctx, 512)
                assert _buffers(ctx, 300) == held                     # the same capacity: the same blocks
        # the boundary blocks were made at 256 rows and remade at 512: the generation says so there and nowhere else
        assert bumps == ["boundary200a", "boundary300"], bumps
        assert _buffers(ctx, 512) == held and _generation(ctx) == gen
        close(ctx, st)
        assert sorted(got) == sorted(fresh)
        differ = [k for k in sorted(got) if got[k].tobytes() != fresh[k].tobytes() or got[k].shape != fresh[k].shape]
        assert not differ, (life, differ)
        lives.append(got)
    for life in (1, 2):
        differ = [k for k in sorted(lives[0]) if lives[life][k].tobytes() != lives[0][k].tobytes()]
        assert not differ, (life, differ)


# ---- the analyses that share the column-statistics buffers, one after the other on one context
BANDS3 = ["A_delta_100um", "SPIRE_250um", "B_delta_850um"]        # one sample, a passband of many, one sample
QS3 = [15.85, 50.0, 84.15]
NSTEPS = 48


def _analysis_calls(like, ctx, h):
    """name -> a call that runs one analysis of the chain resident with sampler h and returns the arrays the library
    filled, in the order the shared buffers are to go through them."""
    from mbb_emcee_amd import _native, evidence, goodness, loo, predict, results

    def analyse(entry, req, raw):
        spec, out = req.spec(), raw.out()
        _native.check_arg(getattr(ctx.lib, "mbb_sampler_" + entry)(ctx.h, h, C.byref(spec), C.byref(out)), ctx)
        return _raw_arrays(raw)

    def summary(**kw):
        def call():
            req = results._Request(QS3, **kw)
            raw = results._Raw(1, len(req.qs))
            spec, out = req.spec(), raw.out()
            _native.check_arg(ctx.lib.mbb_sampler_run_summary(ctx.h, h, 0, 2.0, C.byref(spec), C.byref(out), None, None, None,
                                                              None, None), ctx)
            return _raw_arrays(raw)
        return call

    def predicted(specs):
        def call():
            req = predict._Request(like, specs, QS3)
            return analyse("predict", req, predict._Raw(1, len(req.keys), len(req.qs)))
        return call

    def good():
        req = goodness._Request(like, QS3)
        return analyse("goodness", req, goodness._Raw(1, req.ndata, len(req.qs)))

    def pointwise():
        req = loo._Request(like)
        return analyse("pointwise", req, loo._Raw(1, req.ndata))

    def bridged():
        req = evidence._Request(like, 64, seed=SEED)
        nkept, nfit = req.check_steps(NSTEPS)
        req.set_neff(None, 1)
        return analyse("evidence", req, evidence._Raw(1, NW * (nkept - nfit), 64, False))

    return [
        ("summary_a", summary()),
        ("predict3", predicted([70.0, "SPIRE_250um", 500.0])),
        ("goodness_a", good),
        ("loo", pointwise),
        ("summary_derived", summary(derived=("peaklambda", "lir", "dustmass"), redshift=1.0, lumdist_mpc=6000.0)),
        ("goodness_b", good),
        # (more specs than mbbp::kGroup = 3: two groups, the shared buffers reused within one call)
        ("predict5", predicted([70.0, "SPIRE_250um", 500.0, "B_delta_850um", 1100.0])),
        ("evidence", bridged),
        ("summary_b", summary()),
    ]


def test_analyses_sharing_work_buffers_equal_fresh_contexts(mbb):
    """Summary, predictions, goodness of fit, WAIC / PSIS-LOO and evidence of one resident chain (8 walkers x 48 steps;
    3 bands, one of them a passband of many samples), in an order that takes the shared column-statistics buffers from
    every analysis to every other: each array of each result is the same bytes (NaNs by bit pattern) as from the same
    call on a context that has run the chain and nothing else, and the first and the last summary are the same bytes."""
    import bench
    from mbb_emcee_amd import _native
    helper = mbb.likelihood(response=True)
    helper.set_phot(BANDS3, np.ones(3), np.ones(3))
    flux = helper.model_flux(bench.TRUTH)[0]
    helper.context.close()
    p0 = np.ascontiguousarray(bench.walkers(1)[:NW])

    def make():
        like = mbb.likelihood(response=True)
        like.set_phot(BANDS3, flux, 0.1 * flux + 1.0)
        ctx = like._sync_device()
        h = _sampler(ctx)
        return like, ctx, h, _run(ctx, h, p0, NSTEPS)["chain"]

    def close(ctx, h):
        _native._check(ctx.lib.mbb_sampler_destroy(ctx.h, h))
        ctx.close()

    like, ctx, h, chain = make()
    calls = _analysis_calls(like, ctx, h)
    names = [name for name, _ in calls]
    got = {name: call() for name, call in calls}
    close(ctx, h)
    assert all(arrays and all(v.size for v in arrays.values()) for arrays in got.values())
    assert sum(len(arrays) for arrays in got.values()) >= 70

    def differing(a, b):
        assert sorted(a) == sorted(b)
        return [k for k in sorted(a) if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]

    for name in names:
        like, ctx, h, again = make()
        assert again.tobytes() == chain.tobytes()                        # the same chain: the runs are seeded
        fresh = dict(_analysis_calls(like, ctx, h))[name]()
        close(ctx, h)
        assert not differing(got[name], fresh), (name, differing(got[name], fresh))
    assert not differing(got["summary_a"], got["summary_b"])
    assert not differing(got["goodness_a"], got["goodness_b"])
    # (the calls did something: every summary saw all the samples, the predictions of one spec agree across the calls)
    assert np.all(got["summary_a"]["n_used"][:, :5] == NW * NSTEPS)
    assert got["predict5"]["mean"][0, :3].tobytes() == got["predict3"]["mean"].tobytes()
