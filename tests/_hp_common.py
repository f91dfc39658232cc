"""What tests/test_device_math_cpu.py and tests/test_device_math_gpu.py share: the probe's loader, errors in ulp of
the true value, the seeded argument distributions of the dense sweeps and the parser of the vexp / vlog call sites."""
import importlib.util
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CSRC = os.path.join(ROOT, "mbb_emcee_amd", "csrc")

LD = np.longdouble
LD_OK = np.finfo(LD).nmant >= 63
LD_REASON = "numpy.longdouble has %d mantissa bits here: no denser reference than float64" % np.finfo(LD).nmant
TINY = 5e-324                      # 2^-1074

# the contract of mbb_math.hip.h, in ulp of the true value
ULP_BOUND = {"m_exp": 2.0, "m_expm1": 2.0, "m_exp_t": 2.0, "m_log": 2.0, "m_div": 1.5}


def _by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_mods = {}


def probe_module():
    """tests/_device_probe.py, the probe's loader"""
    import _device_probe
    return _device_probe


def generator_module():
    if "gen" not in _mods:
        _mods["gen"] = _by_path("mbb_make_golden_hp", os.path.join(GOLDEN, "make_golden_hp.py"))
    return _mods["gen"]


def ulp_of(v, sh=0):
    """spacing of the doubles at the true value v 2^sh (the subnormal spacing, scaled alike, at least)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.maximum(np.spacing(np.abs(np.asarray(v, dtype=np.float64))), np.ldexp(TINY, sh))


def ulp_err_dd(got, hi, lo, sh):
    """signed error of `got` in ulp of the true value (hi + lo) 2^-sh: exact in float64 (got 2^sh and hi are
    neighbours, their difference is a double)"""
    with np.errstate(invalid="ignore", over="ignore"):
        g = np.ldexp(np.asarray(got, dtype=np.float64), sh)
        return ((g - hi) - lo) / ulp_of(hi, sh)


def ulp_err_ld(got, ref):
    """signed error of `got` against a longdouble reference, in ulp (float64) of the reference"""
    with np.errstate(invalid="ignore", over="ignore"):
        return ((np.asarray(got).astype(LD) - ref) / ulp_of(ref.astype(np.float64)).astype(LD)).astype(np.float64)


def check_curated(probe, g_math, f, record=None):
    """-> (max |error| in ulp over the points held to the bound, points checked)"""
    x, hi, lo, sh, kind = (g_math[f + "/" + k] for k in ("x", "hi", "lo", "sh", "kind"))
    y = g_math["m_div/y"] if f == "m_div" else None
    got = probe.math(f, x, y)
    assert got.shape == x.shape
    exact = kind == 1
    bad = exact & ~((got == hi) & (np.signbit(got) == np.signbit(hi)))
    assert not bad.any(), "%s: outside the range the result must be exactly %r: x = %r gave %r" % (
        f, hi[bad][:4], x[bad][:4], got[bad][:4])
    err = np.abs(ulp_err_dd(got, hi, lo, sh.astype(np.int64)))
    err = np.where(np.isinf(hi) & (got == hi), 0.0, err)
    held = ~exact
    w = np.flatnonzero(held)[np.nanargmax(np.where(np.isnan(err[held]), np.inf, err[held]))]
    print("%s curated: %d points, max %.3f ulp at x = %r%s: got %r, true %r + %r (2^-%d)" % (
        f, x.size, err[w], x[w], "" if y is None else " / %r" % y[w], got[w], hi[w], lo[w], sh[w]))
    if record:
        record(f + " curated (ulp)", err[w], ULP_BOUND[f])
    assert np.all(err[held] <= ULP_BOUND[f]), (f, x[w], got[w], hi[w], err[w])
    assert not np.isnan(got).any(), (f, x[np.isnan(got)][:4])
    if f in ("m_exp", "m_exp_t", "m_expm1"):
        assert not (got < (-1.0 if f == "m_expm1" else 0.0)).any()
    return err[w], int(held.sum() + exact.sum())


def sweep_args(name, n, seed):
    """The seeded argument distributions of the dense sweeps -- those the accuracy tool of rounds 1-7 drew from
    (tools/test_math_host.cpp, retired), the lower end of exp and expm1 taken down to -745 -- and the longdouble
    reference.  -> (x, y or None, ref)"""
    rng = np.random.RandomState(seed)
    i = np.arange(n)
    if name in ("m_exp", "m_exp_t", "m_expm1"):
        x = -745.0 + (709.7 + 745.0) * rng.uniform(size=n)
        x = np.where(i % 3 == 0, -40.0 + 80.0 * rng.uniform(size=n), x)
        x = np.where(i % 3 == 1, (rng.uniform(size=n) - 0.5) * 2.0, x)
        if name == "m_expm1":          # and relative accuracy near 0, down to 2^-60
            xs = np.ldexp(rng.uniform(size=n) - 0.5, -(rng.uniform(size=n) * 60).astype(np.int64))
            x = np.where(i % 4 == 3, xs, x)
        xl = x.astype(LD)
        return x, None, (np.expm1(xl) if name == "m_expm1" else np.exp(xl))
    if name == "m_log":
        x = np.exp(-30.0 + 60.0 * rng.uniform(size=n))
        x = np.where(i % 2 == 1, 0.5 + rng.uniform(size=n), x)
        return x, None, np.log(x.astype(LD))
    assert name == "m_div"
    a = np.exp(-20.0 + 40.0 * rng.uniform(size=n)); b = np.exp(-30.0 + 110.0 * rng.uniform(size=n))
    return a, b, a.astype(LD) / b.astype(LD)


# ---- the vexp / vlog call sites of the product's sources
def _call_args(text, start):
    """the top-level arguments of the call whose '(' is at text[start]"""
    depth, args, cur = 0, [], []
    for ch in text[start:]:
        if ch in "([{":
            depth += 1
            if depth == 1:
                continue
        elif ch in ")]}":
            depth -= 1
            if depth == 0:
                args.append("".join(cur).strip())
                return args
        if ch == "," and depth == 1:
            args.append("".join(cur).strip()); cur = []
        else:
            cur.append(ch)
    raise ValueError("unbalanced call")


def source_row_instantiations():
    """{(islog, M1, K)} of every vexp<..>(out, args..) / vlog<..>(out, args..) CALL in csrc/*.h (the definitions and
    comments left out): K is the number of arguments after the output array"""
    found = set()
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".h", ".hip", ".inc")):
            continue
        text = open(os.path.join(CSRC, fn)).read()
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"\b(vexp|vlog)\s*<([^<>()]*)>\s*\(", text):
            targs = [t.strip() for t in m.group(2).split(",")]
            if any(t.startswith(("bool", "unsigned", "int", "typename")) for t in targs):
                continue                                           # a declaration's template head
            args = _call_args(text, m.end() - 1)
            k = len(args) - 1
            if m.group(1) == "vlog":
                found.add((True, 0, k))
            else:
                found.add((False, int(targs[1].rstrip("uU"), 16), k))
    return found


def probe_row_instantiations_in_source():
    """[(islog, M1, K)] of kRowInst in tests/_device_probe.hip, in order"""
    text = open(os.path.join(HERE, "_device_probe.hip")).read()
    body = re.search(r"kRowInst\[\]\s*=\s*\{(.*?)\};", text, flags=re.S).group(1)
    return [(bool(int(a)), int(b.rstrip("uU"), 16), int(c)) for a, b, c in
            re.findall(r"\{\s*(\d)\s*,\s*(0x[0-9A-Fa-f]+u|0u)\s*,\s*(\d+)\s*\}", body)]
