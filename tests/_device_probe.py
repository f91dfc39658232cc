"""ctypes loader of the test-only device probe (tests/_device_probe.hip).

    load()        tests/device_probe/libmbb_device_probe.so: gfx950, the product's DEVICE_FLAGS,
                  csrc/mbb_host_tables.cpp compiled in
    load_host()   tests/device_probe/libmbb_device_probe_host.so: the math part with MBB_MATH_HOST, g++, no HIP

The libraries live in a directory of their own, like the RCCL stand-in's: a shared library named after this module
and lying beside it would be taken for an extension module by `import _device_probe`.

Both are built on demand under a file lock (`python tests/_device_probe.py` builds both); `*.so` is ignored by
git, and __graft_entry__.build_test_standins() leaves them in the tree so that they travel to the GPU box.
The wrappers take and return float64 numpy arrays and raise on a non-zero code.
"""
import ctypes as C
import fcntl
import os
import shutil
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SRC = os.path.join(HERE, "_device_probe.hip")
CSRC = os.path.join(ROOT, "mbb_emcee_amd", "csrc")
SRC_TABLES = os.path.join(CSRC, "mbb_host_tables.cpp")
DEPS = [SRC, SRC_TABLES] + [os.path.join(CSRC, f) for f in
                            ("mbb_host_tables.h", "mbb_math.hip.h", "mbb_device.hip.h", "mbb_exp2_tab.inc",
                             "mbb_flow_index.h", "mbb_stretch.hip.h", "mbb_gammq.hip.h")]
LIBDIR = os.path.join(HERE, "device_probe")
SO = os.path.join(LIBDIR, "libmbb_device_probe.so")
SO_HOST = os.path.join(LIBDIR, "libmbb_device_probe_host.so")

OPS = {"m_exp": 0, "m_expm1": 1, "m_log": 2, "m_div": 3, "m_exp_t": 4, "m_gammq_half": 5}
ERRORS = {-1: "bad arguments", -2: "an input outside the probed function's domain", -3: "HIP error"}

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_up = C.POINTER(C.c_uint32)


def _stale(so):
    return not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in DEPS)


def _build(so, cmd):
    if not _stale(so):
        return so
    os.makedirs(os.path.dirname(so), exist_ok=True)
    with open(so + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if _stale(so):
            tmp = "%s.tmp.%d" % (so, os.getpid())
            subprocess.check_call(cmd + ["-o", tmp])
            os.replace(tmp, so)
    return so


def build_device():
    from mbb_emcee_amd import build as hipbuild
    return _build(SO, [hipbuild.hipcc(), "--offload-arch=" + hipbuild.ARCH, "-O3", "-std=c++17", "-fPIC", "-shared"] +
                  hipbuild.DEVICE_FLAGS + [SRC, SRC_TABLES])


def build_host():
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    if not cxx:
        raise RuntimeError("no host C++ compiler for the host build of the probe")
    return _build(SO_HOST, [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-DMBB_MATH_HOST",
                            "-x", "c++", SRC, SRC_TABLES])


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s: %s (%d)" % (what, ERRORS.get(rc, "?"), rc))


class Probe(object):
    def __init__(self, path):
        self.lib = lib = C.CDLL(path)
        lib.probe_math.argtypes = [C.c_int, _dp, _dp, C.c_long, _dp]
        lib.probe_poly.argtypes = [C.c_int, _dp, C.c_long, _dp]
        lib.mbbh_poly_tables.argtypes = [_dp, _dp]
        lib.mbbh_poly_counts.argtypes = [C.POINTER(C.c_int)] * 3
        self.is_host = bool(lib.probe_is_host())
        if not self.is_host:
            lib.probe_rows.argtypes = [C.c_int, _dp, C.c_long, C.c_int, _dp, _dp]
            lib.probe_rows_describe.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_int)]
            lib.probe_prologue.argtypes = [C.c_int, C.c_int, C.c_int, _dp, C.c_long, C.c_double, C.c_int, _dp, _ip, _ip]
            lib.probe_fnu.argtypes = [C.c_int, C.c_int, _dp, _dp, C.c_long, C.c_long, C.c_double, _dp, _dp, _ip]
            lib.probe_philox.argtypes = [_up, _up, C.c_long, _up]
            lib.probe_stretch_draw.argtypes = [_ip, _ip, C.POINTER(C.c_uint64), C.c_long, C.c_double, C.c_int, _dp, _ip, _dp]

    # ---- primitives
    def math(self, name, x, y=None, chunk=1 << 20):
        """m_exp / m_expm1 / m_log / m_div(x, y) / m_exp_t / m_gammq_half(nb = y, chisq = x) of every element"""
        x = _f64(x).ravel()
        y = _f64(y).ravel() if y is not None else None
        assert y is None or y.shape == x.shape
        out = np.empty_like(x)
        for i in range(0, x.size, chunk):
            xs = x[i:i + chunk]
            ys = y[i:i + chunk] if y is not None else None
            o = np.empty_like(xs)
            _check(self.lib.probe_math(OPS[name], _d(xs), _d(ys) if ys is not None else None, xs.size, _d(o)),
                   "probe_math(%s)" % name)
            out[i:i + chunk] = o
        return out

    def gammq(self, nb, chisq):
        """m_gammq_half(nb, chisq) of csrc/mbb_gammq.hip.h: Q(nb/2, chisq/2), nb (integers in [1, 256], or the probe
        refuses) broadcast against chisq (any double)"""
        y, x = np.broadcast_arrays(_f64(nb), _f64(chisq))
        return self.math("m_gammq_half", x, y).reshape(x.shape)

    def poly_tables(self):
        """the product's tables of b and C, rows of kPolyStride doubles (mbbh_poly_tables)"""
        nb, nc, k = C.c_int(), C.c_int(), C.c_int()
        self.lib.mbbh_poly_counts(C.byref(nb), C.byref(nc), C.byref(k))
        b = np.zeros((nb.value, k.value)); c = np.zeros((nc.value, k.value))
        self.lib.mbbh_poly_tables(_d(b), _d(c))
        return b, c

    def poly(self, which, X):
        """polyrow_eval on the table of b ("b", X = 8x in [0, 384]) or C ("c", X = 8y in [0, 296])"""
        X = _f64(X).ravel()
        out = np.empty_like(X)
        _check(self.lib.probe_poly({"b": 0, "c": 1}[which], _d(X), X.size, _d(out)), "probe_poly")
        return out

    # ---- device only
    def row_instantiations(self):
        """[(islog, M1, K)] of probe_rows, in its numbering"""
        out = []
        for i in range(self.lib.probe_rows_count()):
            a, m, k = C.c_int(), C.c_uint(), C.c_int()
            _check(self.lib.probe_rows_describe(i, C.byref(a), C.byref(m), C.byref(k)), "probe_rows_describe")
            out.append((bool(a.value), int(m.value), int(k.value)))
        return out

    def rows(self, inst, args, block):
        """args[n, K] -> (row form [n, 16, K]: what every lane of the element's row holds; lane form [n, K])"""
        args = _f64(args)
        n, k = args.shape
        row = np.empty((n, 16, k)); lane = np.empty((n, k))
        _check(self.lib.probe_rows(inst, _d(args), n, block, _d(row), _d(lane)), "probe_rows")
        return row, lane

    PRO_FIELDS = ("normfac", "xmerge", "kappa", "hcokt", "hokt9", "lhokt9", "lx0", "peak", "x0", "wavemerge")

    def prologue(self, pars, opthin, noalpha, row, wavenorm=500.0, block=256):
        """-> (out[n, 10] in PRO_FIELDS order, status[n], iters[n])"""
        p = _f64(pars).reshape(-1, 5)
        n = p.shape[0]
        w = self.lib.probe_prologue_words()
        assert w == len(self.PRO_FIELDS)
        out = np.empty((n, w)); st = np.empty(n, dtype=np.int32); it = np.empty(n, dtype=np.int32)
        _check(self.lib.probe_prologue(int(opthin), int(noalpha), int(row), _d(p), n, float(wavenorm), int(block),
                                       _d(out), _i(st), _i(it)), "probe_prologue")
        return out, st, it

    def fnu(self, pars, freq, opthin, noalpha, wavenorm=500.0):
        """pars[n, 5], freq[n, m] in GHz -> (f_nu by the table form, by the plain form, status[n])"""
        p = _f64(pars).reshape(-1, 5)
        f = _f64(freq)
        n, m = f.shape
        assert p.shape[0] == n
        ot = np.empty((n, m)); op = np.empty((n, m)); st = np.empty(n, dtype=np.int32)
        _check(self.lib.probe_fnu(int(opthin), int(noalpha), _d(p), _d(f), n, m, float(wavenorm), _d(ot), _d(op),
                                  _i(st)), "probe_fnu")
        return ot, op, st

    # ---- the sampler's draw (csrc/mbb_stretch.hip.h)
    def philox(self, ctr, key):
        """ctr[n, 4], key[n, 2] uint32 -> Philox4x32-10 output [n, 4] uint32"""
        ctr = np.ascontiguousarray(ctr, dtype=np.uint32).reshape(-1, 4)
        key = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1, 2)
        assert len(ctr) == len(key)
        out = np.empty_like(ctr)
        _check(self.lib.probe_philox(ctr.ctypes.data_as(_up), key.ctypes.data_as(_up), len(ctr), out.ctypes.data_as(_up)),
               "probe_philox")
        return out

    def stretch_draw(self, row, half, key, a, c_count):
        """stretch_draw(row[i], half[i], key[i]) with scale a and c_count partners -> (zz, pj, u3)"""
        row = np.ascontiguousarray(row, dtype=np.int32).ravel()
        half = np.ascontiguousarray(half, dtype=np.int32).ravel()
        key = np.ascontiguousarray(key, dtype=np.uint64).ravel()
        n = row.size
        assert half.size == n and key.size == n
        zz = np.empty(n); u3 = np.empty(n); pj = np.empty(n, dtype=np.int32)
        _check(self.lib.probe_stretch_draw(_i(row), _i(half), key.ctypes.data_as(C.POINTER(C.c_uint64)), n, float(a),
                                           int(c_count), _d(zz), _i(pj), _d(u3)), "probe_stretch_draw")
        return zz, pj, u3


_loaded = {}


def load():
    if "dev" not in _loaded:
        _loaded["dev"] = Probe(build_device())
    return _loaded["dev"]


def load_host():
    if "host" not in _loaded:
        _loaded["host"] = Probe(build_host())
    return _loaded["host"]


if __name__ == "__main__":
    print(build_device())
    print(build_host())
