"""A redshift and a luminosity distance per source in a chain summary (mbb_summary_spec's src_redshift /
src_lumdist_mpc), the parts that need no GPU: shapes are refused before anything native is called, the request keeps
its arrays through with_ (so that on-demand percentiles see the same per-source values), a scalar request leaves both
pointers NULL, arrays() names what was used, and the header and the binding agree on the two new fields."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


class _Like(object):
    """As much of a likelihood as the validation looks at: it has no context, so reaching the device raises
    AttributeError, not ValueError."""
    opthin, noalpha, wavenorm, data_read, nsources = False, False, 500.0, False, 1


def _chain(shape):
    rng = np.random.RandomState(0)
    return rng.rand(*(shape + (5,))), rng.rand(*shape)


DER = ("lir", "dustmass")


@pytest.mark.parametrize("z, d, what", [
    (np.arange(4) + 0.5, 1000.0, "redshift"),                          # wrong length for three sources
    (1.0, np.full(2, 1000.0), "lumdist_mpc"),
    (np.ones((3, 1)), np.full(3, 1000.0), "redshift"),                 # two-dimensional
    (np.ones(3), np.full((1, 3), 1000.0), "lumdist_mpc"),
    (np.ones(0), np.full(3, 1000.0), "redshift"),
])
def test_wrong_shapes_are_refused_before_the_device(z, d, what):
    from mbb_emcee_amd import results
    chain, lnp = _chain((3, 12, 6))
    with pytest.raises(ValueError, match=what + " must be a number or a 1-d array with one entry per source"):
        results.chain_summary(_Like(), chain, lnp, derived=DER, redshift=z, lumdist_mpc=d)
    with pytest.raises(AttributeError):                                # (the right shapes do go on to the device)
        results.chain_summary(_Like(), chain, lnp, derived=DER, redshift=np.ones(3), lumdist_mpc=1000.0)


def test_single_source_takes_length_one_only():
    from mbb_emcee_amd import results
    chain, lnp = _chain((12, 6))
    for z, d in ((np.ones(3), 1000.0), (1.0, np.full(3, 1000.0)), (np.ones((1, 1)), 1000.0)):
        with pytest.raises(ValueError, match="one entry per source"):
            results.chain_summary(_Like(), chain, lnp, derived=DER, redshift=z, lumdist_mpc=d)
    req = results._Request([50.0], derived=DER, redshift=np.array([1.5]), lumdist_mpc=np.array([900.0]))
    assert req.nsources == 1 and req.src_redshift.shape == (1,) and req.src_lumdist_mpc[0] == 900.0
    req = results._Request([50.0], derived=DER, redshift=np.float64(1.5), lumdist_mpc=np.array(900.0))   # 0-d: numbers
    assert req.src_redshift is None and (req.redshift, req.lumdist_mpc) == (1.5, 900.0)


def test_sampler_refuses_wrong_shapes_before_the_run():
    """run_mcmc(summary=...) and so mbb_fitter.run(summary=...): the request learns the sampler's number of sources."""
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 1 if name == "nranks" else 0

    class Like3(_Like):
        nsources = 3

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s._handle = lambda: (Ctx(), None)                                  # (no library behind it: a native call raises)
    s.lnprobfn = Like3()
    with pytest.raises(ValueError, match="one entry per source \\(3\\)"):
        s.run_mcmc(np.zeros((3, 10, 5)), 4, summary=dict(derived=DER, redshift=np.ones(4), lumdist_mpc=1000.0))
    req = s._summary_request(dict(derived=DER, redshift=np.ones(3), lumdist_mpc=1000.0), 4)
    assert req.nsources == 3 and np.array_equal(req.src_lumdist_mpc, np.full(3, 1000.0))


def _addr(p):
    return C.cast(p, C.c_void_p).value


def test_request_keeps_its_arrays_and_a_scalar_request_has_none():
    from mbb_emcee_amd import results
    z, d = np.array([0.5, np.nan, 1.25]), np.array([100.0, 200.0, 300.0])
    req = results._Request([15.85, 84.15], derived=DER, redshift=z, lumdist_mpc=d, nsources=3)
    z[0] = 9.0                                                         # the request holds copies, read-only
    assert req.src_redshift[0] == 0.5 and not req.src_redshift.flags.writeable
    again = req.with_([2.3, 97.7], 6, 1.0, None)
    assert again.src_redshift is req.src_redshift and again.src_lumdist_mpc is req.src_lumdist_mpc
    assert again.qs == [2.3, 97.7] and again.clip == {6: (1.0, None)} and again.nsources == 3
    for r in (req, again):
        s = r.spec()
        assert _addr(s.src_redshift) == req.src_redshift.ctypes.data
        assert _addr(s.src_lumdist_mpc) == req.src_lumdist_mpc.ctypes.data
        assert np.array_equal(np.ctypeslib.as_array(s.src_redshift, (3,)), [0.5, np.nan, 1.25], equal_nan=True)
    # a scalar beside an array is broadcast
    mixed = results._Request([50.0], derived=DER, redshift=2.0, lumdist_mpc=d, nsources=3)
    assert np.array_equal(mixed.src_redshift, np.full(3, 2.0)) and np.array_equal(mixed.src_lumdist_mpc, d)
    # scalars: both pointers NULL, the numbers where they always were
    s = results._Request([50.0], derived=DER, redshift=2.0, lumdist_mpc=1000.0, nsources=3).spec()
    assert _addr(s.src_redshift) is None and _addr(s.src_lumdist_mpc) is None
    assert (s.redshift, s.lumdist_mpc) == (2.0, 1000.0)
    s = results._Request([50.0]).spec()
    assert _addr(s.src_redshift) is None and _addr(s.src_lumdist_mpc) is None


def _summary(req, nsrc, multi):
    from mbb_emcee_amd import results
    raw = results._Raw(nsrc, len(req.qs))
    for f in ("mean", "min", "max", "pct", "cov", "best"):
        getattr(raw, f)[:] = 1.0
    return results.ChainSummary(_Like(), req, raw, multi, None), raw


def test_arrays_name_the_redshift_and_distance_only_when_used():
    from mbb_emcee_amd import results
    base = set(_summary(results._Request([50.0]), 1, False)[0].arrays())
    assert "summary_mean" in base and not any("redshift" in k or "lumdist" in k for k in base)
    s, _ = _summary(results._Request([50.0], derived=("peaklambda",), redshift=1.0, lumdist_mpc=10.0), 1, False)
    assert set(s.arrays()) == base
    s, _ = _summary(results._Request([50.0], derived=("lir",), redshift=1.0, lumdist_mpc=10.0), 1, False)
    a = s.arrays()
    assert set(a) == base | {"summary_redshift", "summary_lumdist_mpc"}
    assert a["summary_redshift"].shape == () and float(a["summary_redshift"]) == 1.0
    s, _ = _summary(results._Request([50.0], derived=("lir",), redshift=np.array([1.5]), lumdist_mpc=10.0), 1, False)
    a = s.arrays()
    assert a["summary_redshift"].shape == () and float(a["summary_redshift"]) == 1.5 and float(a["summary_lumdist_mpc"]) == 10.0
    s, _ = _summary(results._Request([50.0], derived=("dustmass",), redshift=1.0, lumdist_mpc=10.0, nsources=3), 3, True)
    a = s.arrays(prefix="x_")
    assert np.array_equal(a["x_redshift"], np.full(3, 1.0)) and np.array_equal(a["x_lumdist_mpc"], np.full(3, 10.0))
    z = np.array([0.5, np.nan, 2.0])
    s, _ = _summary(results._Request([50.0], derived=DER, redshift=z, lumdist_mpc=10.0, nsources=3), 3, True)
    a = s.arrays()
    assert np.array_equal(a["summary_redshift"], z, equal_nan=True) and np.array_equal(a["summary_lumdist_mpc"], np.full(3, 10.0))
    a["summary_redshift"][0] = 7.0                                     # a copy: the request's array is not touched
    assert s._req.src_redshift[0] == 0.5


def test_cen_does_not_raise_for_an_unknown_source():
    """A clip drops the NaNs of an unknown source, so its column is empty: that is not the reference's "No elements
    survive"; an empty column of a source with a redshift still is."""
    from mbb_emcee_amd import results, _native
    z = np.array([0.5, np.nan, 2.0])
    req = results._Request(list(results._pval(68.3)), derived=DER, redshift=z, lumdist_mpc=10.0, nsources=3,
                           clip={"lir": (0.5, None)})
    s, raw = _summary(req, 3, True)
    raw.status[1, 6] = _native.SUM_EMPTY
    raw.mean[1, 6] = raw.pct[1, 6] = np.nan
    got = s.lir_cen(lowlim=0.5)
    assert got.shape == (3, 3) and np.all(np.isnan(got[1])) and np.all(np.isfinite(got[[0, 2]]))
    raw.status[2, 6] = _native.SUM_EMPTY
    with pytest.raises(Exception, match="No elements survive"):
        s.lir_cen(lowlim=0.5)


def test_header_and_binding_agree_on_the_new_fields():
    from mbb_emcee_amd import _native
    hdr = open(os.path.join(ROOT, "include", "mbb_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct mbb_summary_spec \{(.*?)\} mbb_summary_spec;", code, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-1] == "double *src_redshift, *src_lumdist_mpc"       # the last declaration, one-token type, no const
    names = [f[0] for f in _native.SummarySpec._fields_]
    assert names[-2:] == ["src_redshift", "src_lumdist_mpc"] and names[-3] == "lir_wavemax"
    assert all(f[1] is _native._dp for f in _native.SummarySpec._fields_[-2:])
    # a zero-initialised spec has them NULL, and they sit behind everything that was there
    s = _native.SummarySpec()
    assert _addr(s.src_redshift) is None and _addr(s.src_lumdist_mpc) is None
    assert _native.SummarySpec.src_redshift.offset == _native.SummarySpec.lir_wavemax.offset + 8
    assert C.sizeof(_native.SummarySpec) == _native.SummarySpec.src_lumdist_mpc.offset + C.sizeof(C.c_void_p)
