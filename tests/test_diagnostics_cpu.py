"""Chain diagnostics without a GPU: the references of tests/_diag_ref.py against the existing yardsticks, the window
condition on every chain the GPU tests use, and the argument validation of the Python layer."""
import numpy as np
import pytest

import _diag_ref as R

CASE_NAMES = sorted(R.CASES)


def _sources(name):
    ch = R.case_chain(name)
    return ch if ch.ndim == 4 else ch[None]


# ---------------------------------------------------------------- the reference against the yardsticks
@pytest.mark.parametrize("name", [n for n in CASE_NAMES if R.CASES[n][1].get("method", "mean") == "mean"])
def test_reference_mean_method_is_integrated_time(name):
    """The "mean" reference is ensemble.integrated_time of the ensemble-mean series (what get_autocorr_time computes),
    to the FFT's own rounding."""
    from mbb_emcee_amd.ensemble import integrated_time
    kw = R.CASES[name][1]
    burn, c = kw.get("burn", 0), kw.get("c", 5.0)
    for ch, ref in zip(_sources(name), R.case_ref(name)):
        for p in range(5):
            with np.errstate(invalid="ignore"):
                want = integrated_time(ch[:, burn:, p].mean(axis=0), c=c)
            if ref["status"][p] & (R.SHORT | R.CONSTANT | R.HAS_NAN):
                assert np.isnan(ref["tau"][p])
                if not ref["status"][p] & R.CONSTANT:          # (a constant series: its FFT leaves rounding noise)
                    assert np.isnan(want)
            else:
                np.testing.assert_allclose(ref["tau"][p], want, rtol=0, atol=100 * ref["tau_bound"][p])


def _walkers_fft(x, c):
    """emcee 3's autocorr.integrated_time, restated: every walker's normalised acf by FFT, averaged, windowed once."""
    nw, n = x.shape
    nfft = 1 << (2 * n - 1).bit_length()
    f = np.zeros(n)
    for w in range(nw):
        y = x[w] - x[w].mean()
        ft = np.fft.rfft(y, nfft)
        acf = np.fft.irfft(ft * np.conjugate(ft))[:n]
        f += acf / acf[0]
    f /= nw
    taus = 2.0 * np.cumsum(f) - 1.0
    win = np.arange(n) >= c * taus
    m = int(np.argmax(win)) if win.any() else n - 1
    return taus[m], m


@pytest.mark.parametrize("name", [n for n in CASE_NAMES if R.CASES[n][1].get("method") == "walkers"])
def test_reference_walkers_method_is_emcee3(name):
    kw = R.CASES[name][1]
    burn, c = kw.get("burn", 0), kw.get("c", 5.0)
    for ch, ref in zip(_sources(name), R.case_ref(name)):
        for p in range(5):
            if ref["status"][p] & (R.SHORT | R.CONSTANT | R.HAS_NAN):
                assert np.isnan(ref["tau"][p]) and ref["window"][p] == -1
                continue
            tau, m = _walkers_fft(ch[:, burn:, p], c)
            assert m == ref["window"][p]
            np.testing.assert_allclose(ref["tau"][p], tau, rtol=0, atol=100 * ref["tau_bound"][p])


@pytest.mark.parametrize("name", ["n257", "burn_n_odd", "nw250", "nsrc3", "ramp", "n7"])
def test_reference_rhat_is_gelman_rubin(name):
    burn = R.CASES[name][1].get("burn", 0)
    for ch, ref in zip(_sources(name), R.case_ref(name)):
        x = ch[:, burn:, :]
        n = x.shape[1]
        h = n // 2
        seqs = np.concatenate((x[:, :h], x[:, n - h:]), axis=0)              # [2 nw, h, 5]; n odd: the middle is dropped
        W = seqs.var(axis=1, ddof=1).mean(axis=0)
        B = h * seqs.mean(axis=1).var(axis=0, ddof=1)
        np.testing.assert_allclose(ref["rhat"], np.sqrt(((h - 1) / h * W + B / h) / W), rtol=1e-9)
        assert np.all(ref["rhat"] > 0.9)


def test_reference_status_and_seams():
    """The cases are what their names say."""
    ref = lambda name: R.case_ref(name)[0]
    assert np.all(ref("n7")["status"] == R.SHORT) and np.all(np.isnan(ref("n7")["tau"]))
    assert np.all(np.isfinite(ref("n7")["rhat"]))                              # (h = 3)
    assert np.all(np.isfinite(ref("n8")["tau"]))
    assert ref("seam_255")["window"][0] == 255 and ref("seam_256")["window"][0] == 256
    r = ref("ramp")
    assert np.all(r["status"] == R.UNRELIABLE) and np.all(r["window"] > 60) and np.all(r["window"] < 90)
    assert np.all(r["rhat"] > 1.5)
    for name in ("constant_column", "constant_column_walkers"):
        r = ref(name)
        assert r["status"][3] == R.CONSTANT and np.isnan(r["tau"][3]) and np.isnan(r["rhat"][3])
        assert np.all(np.isfinite(np.delete(r["tau"], 3)))
    r = ref("one_constant_walker")
    assert r["status"][2] == R.CONSTANT and np.isnan(r["tau"][2]) and np.isfinite(r["rhat"][2])
    assert np.isfinite(ref("one_constant_walker_mean")["tau"][2])
    for name in ("NaN_inside_the_window", "NaN_inside_the_window_walkers"):
        r = ref(name)
        assert r["status"][1] == R.HAS_NAN and np.isnan(r["tau"][1]) and np.isnan(r["rhat"][1])
    assert np.all(ref("NaN_outside_the_window")["status"] & R.HAS_NAN == 0)
    for name in ("n1000_nacf_beyond_M", "n1000_walkers_nacf_beyond_M", "longest"):
        r = ref(name)
        assert np.all(r["window"] < R.CASES[name][1]["nacf"] - 1)
    assert R.case_chain("burn_n_odd").shape[1] - 19 == 101
    srcs = R.case_ref("nsrc3")
    assert not np.allclose(srcs[0]["tau"], srcs[1]["tau"], rtol=0.05)


# ---------------------------------------------------------------- the window condition
@pytest.mark.parametrize("name", CASE_NAMES)
def test_window_decision_is_not_marginal(name):
    """The window is a comparison, m >= c tau(m), and would flip under rounding if it were marginal: on every chain and
    parameter the GPU tests use, min over m <= M of |m - c tau(m)| is at least 1e-3, far above the tau bound; and
    mean|x| / sigma stays below 1e4.  A condition on the inputs, not a tolerance."""
    for ref in R.case_ref(name):
        assert np.all(ref["margin"] >= 1e-3), ref["margin"]
        assert np.all(ref["tau_bound"] * R.CASES[name][1].get("c", 5.0) < 1e-3 * 1e-2)
        assert np.all(ref["rho_bound"] <= 16.0 * 40 * R.EPS * (1 + 1e4))


# ---------------------------------------------------------------- validation before the device
class _Like(object):
    """Stands where a likelihood would: touching the device is an error."""
    data_read = True

    def _sync_device(self):
        raise AssertionError("the device was touched")

    context = property(_sync_device)


def test_chain_diagnostics_validates_before_the_device():
    import mbb_emcee_amd
    from mbb_emcee_amd import diagnostics
    assert mbb_emcee_amd.chain_diagnostics is diagnostics.chain_diagnostics
    assert mbb_emcee_amd.ChainDiagnostics is diagnostics.ChainDiagnostics
    like, chain = _Like(), np.random.RandomState(0).rand(10, 20, 5)
    with pytest.raises(ValueError, match="chain must be"):
        diagnostics.chain_diagnostics(like, chain[..., :4])
    with pytest.raises(ValueError, match="chain must be"):
        diagnostics.chain_diagnostics(like, chain[0])
    with pytest.raises(ValueError, match="burn"):
        diagnostics.chain_diagnostics(like, chain, burn=20)
    with pytest.raises(ValueError, match="burn"):
        diagnostics.chain_diagnostics(like, chain, burn=-1)
    with pytest.raises(ValueError, match="method"):
        diagnostics.chain_diagnostics(like, chain, method="fft")
    with pytest.raises(ValueError, match="c must be positive"):
        diagnostics.chain_diagnostics(like, chain, c=0.0)
    with pytest.raises(ValueError, match="c must be positive"):
        diagnostics.chain_diagnostics(like, chain, c=float("nan"))
    with pytest.raises(ValueError, match="tol"):
        diagnostics.chain_diagnostics(like, chain, tol=-1.0)
    with pytest.raises(ValueError, match="nacf"):
        diagnostics.chain_diagnostics(like, chain, nacf=-1)
    with pytest.raises(ValueError, match="nacf"):
        diagnostics.chain_diagnostics(like, chain, burn=5, nacf=16)
    with pytest.raises(ValueError, match="more than 16384 kept steps"):
        diagnostics.chain_diagnostics(like, np.zeros((2, 16386, 5)), burn=1)
    with pytest.raises(AssertionError, match="the device was touched"):     # (valid arguments do get that far)
        diagnostics.chain_diagnostics(like, chain, burn=4, nacf=16, method="walkers")


def _bare_sampler():
    from mbb_emcee_amd import DeviceEnsembleSampler
    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s.k, s.dim, s.lnprobfn, s._h, s.summary = 10, 5, _Like(), None, None

    def handle():
        raise AssertionError("the device was touched")
    s._handle = handle
    return s


def test_run_mcmc_convergence_needs_a_resident_chain():
    """storechain=False without summary= keeps no chain on the device: convergence= says so before anything runs; so
    do bad keywords, and convergence() of a sampler that has no chain."""
    s = _bare_sampler()
    with pytest.raises(ValueError, match="needs summary= too"):
        s.run_mcmc(np.zeros((10, 5)), 16, storechain=False, convergence=True)
    with pytest.raises(ValueError, match="method"):
        s.run_mcmc(np.zeros((10, 5)), 16, convergence=dict(method="fft"))
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.run_mcmc(np.zeros((10, 5)), 16, convergence=dict(burn=16))
    with pytest.raises(TypeError):
        s.run_mcmc(np.zeros((10, 5)), 16, convergence=dict(thin=2))
    assert s.convergence_ is None
    with pytest.raises(ValueError, match="no chain of this sampler is resident"):
        s.convergence()
    s._resident = 16
    with pytest.raises(ValueError, match="burn leaves no step"):
        s.convergence(burn=16)


def test_sharded_run_is_not_diagnosed():
    from mbb_emcee_amd import DeviceEnsembleSampler

    class Ctx(object):
        xchg_barrier = None

        def info(self, name):
            return 2 if name == "nranks" else 0

    s = DeviceEnsembleSampler.__new__(DeviceEnsembleSampler)
    s._handle = lambda: (Ctx(), None)
    with pytest.raises(ValueError, match="sharded"):
        s.run_mcmc(np.zeros((10, 5)), 4, convergence=True)


def test_fitter_convergence_needs_the_device_sampler():
    from mbb_emcee_amd import mbb_fitter
    fit = mbb_fitter(nwalkers=10, sampler="native")
    with pytest.raises(ValueError, match="convergence= needs sampler"):
        fit.run(2, 2, np.zeros((10, 5)), convergence=True)
    assert fit.convergence is None


def test_cli_has_the_convergence_flag():
    from mbb_emcee_amd import run_mbb_emcee
    a = run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz"])
    assert a.convergence is False
    assert run_mbb_emcee.build_parser().parse_args(["phot.txt", "out.npz", "--convergence"]).convergence is True


def test_diagnostics_entries_are_declared_and_bound():
    import ctypes as C
    import os
    from mbb_emcee_amd import _native
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mbb_hip.h")).read()
    for name in ("mbb_chain_diagnostics", "mbb_sampler_diagnostics"):
        assert name in hdr and name in _native.SIGNATURES
    assert [f[0] for f in _native.DiagSpec._fields_] == ["burn", "method", "nacf", "c", "tol"]
    assert [f[0] for f in _native.DiagOut._fields_] == ["tau", "ess", "rhat", "window", "status", "acf"]
    assert C.sizeof(_native.DiagSpec) == 32 and C.sizeof(_native.DiagOut) == 48
    assert "#define MBB_DIAG_MAX_STEPS %d" % _native.DIAG_MAX_STEPS in hdr
    assert (_native.DIAG_SHORT, _native.DIAG_CONSTANT, _native.DIAG_HAS_NAN, _native.DIAG_UNRELIABLE) == (1, 2, 4, 8)


def test_diag_kernels_use_no_scratch():
    """Build hygiene: the compiler's resource remarks for the k_diag_* kernels (tools/kernel_resources.py; its table is
    profiles/r14/kernel_resources.txt) show no scratch and no spilled vector registers."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    table = open(os.path.join(root, "profiles", "r14", "kernel_resources.txt")).read()
    rows = [ln.split() for ln in table.splitlines() if re.search(r"k_diag_", ln)]
    names = {r[0] for r in rows}
    for k in ("k_diag_mean", "k_diag_acf", "k_diag_seq", "k_diag_rhat"):
        assert any(k in n for n in names), k
    for r in rows:
        vspill, scratch = int(r[-3]), int(r[-2])
        assert vspill == 0 and scratch == 0, r
