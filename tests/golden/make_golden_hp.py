"""High-precision fixtures for tests/test_device_math_cpu.py and tests/test_device_math_gpu.py.

    python tests/golden/make_golden_hp.py [--check]

Needs mpmath (50 digits) and, for the oracle's recorded maxima, the repository's CPU oracle; the
tests read only the files it writes, tests/golden/hp_math.npz and tests/golden/hp_sed.npz.  It is
deterministic: a second run reproduces both files byte for byte (`--check` compares instead of
writing).  The definitions are the reference's formulas (modified_blackbody.py:228-337, :556-637,
fnu.pyx:9-108) with the constants of mbb_device.hip.h as the doubles they are.

hp_math.npz, per function f in m_exp, m_exp_t, m_expm1, m_log, m_div:
    f/x (f/y: m_div's denominator)   the arguments, exact doubles
    f/hi, f/lo                       the true value 2^sh as a double-double
    f/sh                             0, or 256 where the value lies below 2^-900 (so that lo is representable)
    f/kind                           0: held to the ulp bound; 1: hi is the exact result required (0, inf, -1);
                                     2 (m_div): b above the clamp at 8e307 -- the truth is that of a / 8e307
hp_sed.npz: see write_sed().
"""
import io
import os
import sys
import zipfile

import numpy as np
import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

mp.mp.dps = 50
M = mp.mpf
# mbb_device.hip.h:37-40, as doubles
H, K, C_UM, UM2GHZ = M(6.6260693e-34), M(1.3806505e-23), M(299792458e6), M(299792458e-3)
WAVENORM = 500.0
DBL_MIN, DBL_MAX = 2.2250738585072014e-308, 1.7976931348623157e308
VARIANTS = [("thin_noalpha", True, True), ("thin_walpha", True, False),
            ("thick_noalpha", False, True), ("thick_walpha", False, False)]
FLOOR = 1e-280            # f_nu below this fraction of fnorm is not held to a relative bound
NFREQ, NFNU_ROWS = 48, 64


# ------------------------------------------------------------------ helpers
def dd(v, sh=0):
    """double-double (hi, lo) of the mpmath value v 2^sh"""
    v = M(v) * M(2) ** sh
    if v > M(DBL_MAX) * (1 + M(2) ** -54):
        return np.inf, 0.0
    hi = float(v)
    lo = float(v - M(hi))
    return hi, lo


def near(v):
    return float(M(v))


def tri(x):
    """x and its two neighbours"""
    x = float(x)
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


def save_npz(path, arrays, check):
    """An uncompressed .npz with fixed time stamps and a fixed order of entries"""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    data = buf.getvalue()
    assert len(data) < 400 * 1024, (path, len(data))
    if check:
        same = os.path.exists(path) and open(path, "rb").read() == data
        print("%s: %s (%d bytes)" % (os.path.relpath(path, ROOT), "reproduced byte for byte" if same else "DIFFERS", len(data)))
        return same
    with open(path, "wb") as f:
        f.write(data)
    print("wrote %s (%d bytes, %d arrays)" % (os.path.relpath(path, ROOT), len(data), len(arrays)))
    return True


# --------------------------------------------------------------- hp_math.npz
LN2 = mp.log(2)


def exp_args(with_small):
    rng = np.random.RandomState(20261016)
    xs = []
    for e in (-745.2, -745.14, -745.13, -745.1, -745.0, -744.5, -744.0, -708.5, -708.4, -708.39, -708.3,
              709.0, 709.44, 709.5, 709.6, 709.7, 709.78, 709.782, 709.7827):
        xs += tri(e)
    xs += [-746.0, -750.0, -800.0, -1000.0, 709.79, 710.0, 710.2, 710.3, 710.4, 720.0, 800.0, 1000.0]
    for k in np.unique(np.concatenate([np.arange(-2150, 2048, 31), [-2150, -2149, -2045, -2044, -3, -2, -1, 1, 2, 3, 2046, 2047]])):
        xs += tri(near(int(k) * LN2 / 2))                          # seams of reduce_ln2
    for n in rng.randint(-381400, 363400, 240):
        xs += tri(near(int(n) * LN2 / 512))                        # seams of reduce_ln2_256
    xs += [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, DBL_MIN, -DBL_MIN, 1e-20, -1e-20, 2.0 ** -54, -2.0 ** -54,
           2.0 ** -53, -2.0 ** -53, 1.0, -1.0]
    xs += [s * v for v in (800.0, 1e9, 1e20, 1e89) for s in (1.0, -1.0)]     # the header's saturation cases
    if with_small:
        xs += [s * 2.0 ** -k for k in range(1, 61) for s in (1.0, -1.0)]
        xs += [-37.0, -37.4, -37.5, -38.0, -40.0, -50.0, -100.0, -500.0, -700.0]
    return np.array(xs, dtype=np.float64)


def exp_truth(x, minus1):
    n = x.size
    hi = np.zeros(n); lo = np.zeros(n); sh = np.zeros(n, dtype=np.int16); kind = np.zeros(n, dtype=np.int8)
    for i, xv in enumerate(x):
        if xv <= -746.0:
            hi[i], kind[i] = (-1.0 if minus1 else 0.0), 1
        elif xv >= 709.79:
            hi[i], kind[i] = np.inf, 1
        else:
            v = mp.expm1(M(float(xv))) if minus1 else mp.exp(M(float(xv)))
            if v != 0 and abs(v) < M(2) ** -900:
                sh[i] = 256
            hi[i], lo[i] = dd(v, int(sh[i]))
    return hi, lo, sh, kind


def log_args():
    m = 0.7071067811865476            # sqrt(1/2) to the nearest double; sqrt(2) is twice it, bit for bit
    xs = [DBL_MIN, np.nextafter(DBL_MIN, 1.0), DBL_MAX, np.nextafter(DBL_MAX, 1.0), 1.0]
    xs += [1.0 + k * 2.0 ** -52 for k in range(1, 41)] + [1.0 - k * 2.0 ** -53 for k in range(1, 41)]
    for e in range(-1021, 1025):      # both neighbours at every binade a normal double has
        xs += [np.ldexp(np.nextafter(m, 0.0), e), np.ldexp(np.nextafter(m, 1.0), e)]
        if e % 16 == 0:
            xs.append(np.ldexp(m, e))
    xs += [np.ldexp(1.0, e) for e in range(-1022, 1024)]
    return np.array(xs, dtype=np.float64)


def div_args():
    rng = np.random.RandomState(20261017)
    a, b, kind = [], [], []

    def add(x, y, k=0):
        a.append(float(x)); b.append(float(y)); kind.append(k)
    for _ in range(300):              # quotients near 1
        add(1.0 + rng.randint(-50, 51) * 2.0 ** -52, 1.0 + rng.randint(-50, 51) * 2.0 ** -52)
    for _ in range(200):
        e = int(rng.randint(-1000, 1000))
        add(np.ldexp(rng.uniform(1, 2), e), np.ldexp(rng.uniform(1, 2), e))
    for _ in range(500):              # the whole exponent range, both signs
        e2 = int(rng.randint(-1021, 1022))
        e1 = int(np.clip(e2 + rng.randint(-1015, 1016), -1021, 1022))
        if not -1015 <= e1 - e2 <= 1015:
            e1 = e2
        add(rng.choice([-1.0, 1.0]) * np.ldexp(rng.uniform(1, 2), e1), rng.choice([-1.0, 1.0]) * np.ldexp(rng.uniform(1, 2), e2))
    for _ in range(200):              # exactly representable quotients
        q = float(rng.randint(1 << 25, 1 << 26)); y = np.ldexp(float(rng.randint(1 << 25, 1 << 26)), int(rng.randint(-500, 500)))
        add(q * y, y)
    for _ in range(60):               # subnormal quotients
        e2 = int(rng.randint(0, 900))
        add(np.ldexp(rng.uniform(1, 2), e2 - int(rng.randint(1023, 1070))), np.ldexp(rng.uniform(1, 2), e2))
    top = 8.0e307
    for y in (top, np.nextafter(top, 0.0)):                       # at the clamp
        for e in range(2, 1000, 40):
            add(np.ldexp(rng.uniform(1, 2), e), y)
    for y in (np.inf, DBL_MAX, 1e308, np.nextafter(top, np.inf)):   # beyond it: taken as 8e307
        for x in (0.0, 1.0, -1.0, 1e-300, 3.7, -2.5e10, 1e100, 1e300, -1e300):
            add(x, y, 2)
    for x in (0.0, -0.0):
        add(x, 3.0); add(x, -7.0e200)
    return np.array(a), np.array(b), np.array(kind, dtype=np.int8)


def write_math(check):
    out = {}
    for name, small, minus1 in (("m_exp", False, False), ("m_exp_t", False, False), ("m_expm1", True, True)):
        x = exp_args(small)
        hi, lo, sh, kind = exp_truth(x, minus1)
        out.update({name + "/x": x, name + "/hi": hi, name + "/lo": lo, name + "/sh": sh, name + "/kind": kind})
    x = log_args()
    hl = np.array([dd(mp.log(M(float(v)))) for v in x])
    out.update({"m_log/x": x, "m_log/hi": hl[:, 0].copy(), "m_log/lo": hl[:, 1].copy(),
                "m_log/sh": np.zeros(x.size, dtype=np.int16), "m_log/kind": np.zeros(x.size, dtype=np.int8)})
    a, b, kind = div_args()
    hi = np.zeros(a.size); lo = np.zeros(a.size); sh = np.zeros(a.size, dtype=np.int16)
    for i in range(a.size):
        den = M(8.0e307) if kind[i] == 2 else M(float(b[i]))
        v = M(float(a[i])) / den
        if v != 0 and abs(v) < M(2) ** -900:
            sh[i] = 256
        hi[i], lo[i] = dd(v, int(sh[i]))
        if v == 0:
            hi[i] = np.copysign(0.0, a[i]) * np.copysign(1.0, b[i])
    out.update({"m_div/x": a, "m_div/y": b, "m_div/hi": hi, "m_div/lo": lo, "m_div/sh": sh, "m_div/kind": kind})
    return save_npz(os.path.join(HERE, "hp_math.npz"), out, check)


# ---------------------------------------------------------------- hp_sed.npz
def lambert_root(A):
    """root of x = A (1 - e^-x), A > 1"""
    return A + mp.lambertw(-A * mp.exp(-A))


def h_of(y):
    if y == 0:
        return M(1)
    if y > 5000:
        return M(0)                                   # y / expm1(y) < 1e-2000
    return y / mp.expm1(y)


def thick_root(alpha, beta, x0):
    """root of alpha_merge_eqn (modified_blackbody.py:122-151) on its analytic bracket"""
    def g(x):
        return x - (1 - mp.exp(-x)) * (3 + alpha + beta * h_of((x / x0) ** beta))
    lo, hi = 2 + alpha, 3 + alpha + beta + M("1e-6")
    x = mp.findroot(g, (lo, hi), solver="anderson", tol=M(10) ** -80, maxsteps=400, verify=False)
    assert abs(g(x)) < M(10) ** -40 and lo <= x <= hi, (alpha, beta, x0, x)
    return x


class Truth(object):
    def __init__(self, p, opthin, noalpha):
        T, beta, l0, alpha, fnorm = [M(float(v)) for v in p]
        self.opthin, self.noalpha, self.beta, self.alpha = opthin, noalpha, beta, alpha
        self.hokt9 = M(1e9) * H / (K * T)
        self.hcokt = self.hokt9 * UM2GHZ
        xn = self.hcokt / M(WAVENORM)
        self.x0 = None if opthin else self.hcokt / l0
        self.xmerge = self.kappa = None
        if opthin:
            bb = fnorm * mp.expm1(xn) / xn ** (3 + beta)
            if not noalpha:
                A = 3 + alpha + beta
                self.xmerge = lambert_root(A)
                self.kappa = self.xmerge ** A / mp.expm1(self.xmerge)
        else:
            bb = -fnorm * mp.expm1(xn) / (mp.expm1(-(xn / self.x0) ** beta) * xn ** 3)
            if not noalpha:
                self.xmerge = thick_root(alpha, beta, self.x0)
                self.kappa = -self.xmerge ** (3 + alpha) * mp.expm1(-(self.xmerge / self.x0) ** beta) / mp.expm1(self.xmerge)
        self.normfac = bb
        if not noalpha and xn > self.xmerge:
            self.normfac = fnorm * xn ** alpha / self.kappa
        # max_wave (:581-637): the stationary point of the blackbody side
        if opthin:
            if beta == 0:
                self.peak = C_UM / (M(2.82144) * K * T / H)
            else:
                self.peak = self.hcokt / lambert_root(3 + beta)
        else:
            self.peak = self.hcokt / thick_root(M(0), beta, self.x0)

    def fnu(self, nu):
        x = self.hokt9 * M(float(nu))
        if not self.noalpha and x > self.xmerge:
            return self.normfac * self.kappa * x ** (-self.alpha)
        if self.opthin:
            return self.normfac * x ** (3 + self.beta) / mp.expm1(x)
        return -self.normfac * mp.expm1(-(x / self.x0) ** self.beta) * x ** 3 / mp.expm1(x)


def param_rows():
    """about 1500 rows and what each was made for (`origin`): 0 wide, 1 box, 2 beta = 0, 3 beta = 1e-8,
    4 y at the root beside a switch of h_and_dh / the fp32 stage, 5 xnorm beside xmerge, 6 cold (T <= 6 K)"""
    rng = np.random.RandomState(20261018)
    n = 600
    wide = np.column_stack([np.exp(rng.uniform(np.log(3), np.log(200), n)), rng.uniform(0.0, 4.5, n),
                            np.exp(rng.uniform(np.log(5), np.log(3000), n)),
                            np.exp(rng.uniform(np.log(0.1), np.log(10), n)),
                            np.exp(rng.uniform(np.log(0.01), np.log(1000), n))])
    box = np.column_stack([rng.uniform(1, 80, n), rng.uniform(0.1, 21, n), rng.uniform(1, 4500, n),
                           rng.uniform(0.1, 21, n), rng.uniform(1e-3, 100, n)])
    b0 = wide[:40].copy(); b0[:, 1] = 0.0
    b8 = wide[40:80].copy(); b8[:, 1] = 1e-8
    rows, origin = [wide, box, b0, b8], [0] * n + [1] * n + [2] * 40 + [3] * 40
    hck = H * C_UM / K                                 # h c / k in um K
    # y = (xmerge / x0)^beta at the thick root beside 1e-4, 0.02, 80, 700: with y given the root is the thin
    # model's closed form with A = 3 + alpha + beta h(y); lambda0 follows from x0 = xmerge y^(-1/beta)
    edge = []
    for target in (1e-4, 0.02, 80.0, 700.0):
        for rel in (-1e-2, -1e-6, 1e-6, 1e-2):
            for beta in (1.5, 3.0, 8.0):
                for T, alpha in ((8.0, 0.7), (25.0, 2.0), (60.0, 4.5)):
                    y = M(target) * (1 + M(rel))
                    xm = lambert_root(3 + M(alpha) + M(beta) * h_of(y))
                    x0 = xm / y ** (1 / M(beta))
                    edge.append([T, beta, near(hck / M(T) / x0), alpha, 10.0])
    # xnorm within 1e-6 (relative) of xmerge: y at the root is then ((1 - d) lambda0 / wavenorm)^beta whatever T is, the
    # root again a closed form, and T follows from xnorm = xmerge / (1 - d)
    sw = []
    for d in (-1e-6, -1e-8, 1e-8, 1e-6):
        for beta in (0.5, 1.8, 3.5):
            for alpha in (0.5, 2.5, 6.0):
                for l0 in (60.0, 400.0, 1500.0):
                    y = ((1 - M(d)) * M(l0) / M(WAVENORM)) ** M(beta)
                    xm = lambert_root(3 + M(alpha) + M(beta) * h_of(y))
                    sw.append([near(hck / (M(WAVENORM) * xm / (1 - M(d)))), beta, l0, alpha, 3.0])
                # (and for the thin model, whose root does not know lambda0)
                xm = lambert_root(3 + M(alpha) + M(beta))
                sw.append([near(hck / (M(WAVENORM) * xm / (1 - M(d)))), beta, 200.0, alpha, 3.0])
    cold = box[:16].copy()
    cold[:, 0] = np.exp(np.linspace(0.0, np.log(6.0), 16))
    cold[:, 1] = np.minimum(cold[:, 1], 4.0)
    rows += [np.array(edge), np.array(sw), cold]
    origin += [4] * len(edge) + [5] * len(sw) + [6] * 16
    return np.vstack(rows), np.array(origin, dtype=np.int8)


def freq_for_row(p, tr):
    """48 frequencies (GHz) for a row: tr = {variant name: Truth}"""
    T, beta = float(p[0]), float(p[1])
    hokt9 = (1e9 * 6.6260693e-34 / 1.3806505e-23) / T           # as the kernels form it, in double
    c8 = 8.0 * hokt9

    def nu_of_x(x):
        return float(M(x) / tr["thin_noalpha"].hokt9)

    def on_edge(k):
        """a frequency whose X = (8 hokt9) nu is the integer k exactly, if a double does that"""
        nu = k / c8
        for _ in range(8):
            X = c8 * nu
            if X == k:
                break
            nu = np.nextafter(nu, np.inf if X < k else 0.0)
        return nu
    special = []
    for name in ("thin_walpha", "thick_walpha"):                  # either side of X = 8 xmerge
        nu = nu_of_x(tr[name].xmerge)
        special += [np.nextafter(nu, 0.0), np.nextafter(nu, np.inf)]
    nu = on_edge(384)                                             # either side of X = 384
    special += [nu, np.nextafter(nu, np.inf)]
    for k in (1, 8, 37, 200):                                     # table-row edges and one ulp below
        nu = on_edge(k)
        special += [nu, np.nextafter(nu, 0.0)]
    x0 = tr["thick_noalpha"].x0
    if beta > 0.05:                                               # Y = 8 y at the clamp 8 * 37, and in row 0 of C
        for y in (M(37) * (1 - M("1e-9")), M(37) * (1 + M("1e-9")), M("0.05"), M("1e-6")):
            special.append(nu_of_x(x0 * y ** (1 / M(beta))))
    if T <= 1.05:
        special.append(nu_of_x(M("709.6")))                       # where 2^k overflows in expm1 and e^x does not
    lo_nu, hi_nu = 299792.458 / 3000.0, 299792.458 / 20.0
    special = [v for v in special if np.isfinite(v) and 1.0 <= v <= 1e6]
    ngrid = NFREQ - len(special)
    grid = 299792.458 / np.exp(np.linspace(np.log(20.0), np.log(3000.0), ngrid))
    f = np.array(list(grid) + special)
    assert f.size == NFREQ and np.all(f > 0) and lo_nu > 0 and hi_nu > 0
    return f


def write_sed(check):
    """pars[n, 5], origin[n]; per variant v: v/normfac, and for the variants with alpha v/xmerge, v/kappa;
    thick/x0; thin/peak, thick/peak; fnu/rows[64], fnu/freq[64, 48], fnu/v[64, 48]; oracle_max/v =
    (max |d xmerge|, max rel kappa, max rel normfac) of the CPU oracle against these values"""
    from oracle import oracle as O
    O.build()
    pars, origin = param_rows()
    n = pars.shape[0]
    out = {"pars": pars, "origin": origin}
    truths = {}
    for name, opthin, noalpha in VARIANTS:
        tr = [Truth(p, opthin, noalpha) for p in pars]
        truths[name] = tr
        out[name + "/normfac"] = np.array([float(t.normfac) for t in tr])
        worst = [0.0, 0.0, 0.0]
        if not noalpha:
            out[name + "/xmerge"] = np.array([float(t.xmerge) for t in tr])
            out[name + "/kappa"] = np.array([float(t.kappa) for t in tr])
        for p, t in zip(pars, tr):
            s = O.OracleSED(*p, opthin=opthin, noalpha=noalpha).s       # (raises if the oracle cannot construct the row)
            if not noalpha:
                worst[0] = max(worst[0], float(abs(M(s.xmerge) - t.xmerge)))
                worst[1] = max(worst[1], float(abs(M(s.kappa) / t.kappa - 1)))
            worst[2] = max(worst[2], float(abs(M(s.normfac) / t.normfac - 1)))
        out["oracle_max/" + name] = np.array(worst)
        print(name, "oracle max |dxmerge| %.3g rel kappa %.3g rel normfac %.3g" % tuple(worst))
    out["thick/x0"] = np.array([float(t.x0) for t in truths["thick_noalpha"]])
    out["thin/peak"] = np.array([float(t.peak) for t in truths["thin_noalpha"]])
    out["thick/peak"] = np.array([float(t.peak) for t in truths["thick_noalpha"]])
    for a, b in (("thin_noalpha", "thin_walpha"), ("thick_noalpha", "thick_walpha")):
        assert all(x.peak == y.peak for x, y in zip(truths[a], truths[b]))
    for v in out.values():
        assert np.all(np.isfinite(v)), "a row without a finite truth"
    # the 64 rows with f_nu: the 16 cold ones and 48 spread over the others
    cold = np.flatnonzero(origin == 6)
    others = np.flatnonzero(origin != 6)
    pick = np.concatenate([cold, others[np.linspace(0, others.size - 1, NFNU_ROWS - cold.size).astype(int)]])
    assert pick.size == NFNU_ROWS and np.unique(pick).size == NFNU_ROWS and (pars[pick, 0] <= 6.0).sum() >= 16
    freq = np.zeros((NFNU_ROWS, NFREQ))
    for j, i in enumerate(pick):
        freq[j] = freq_for_row(pars[i], {name: truths[name][i] for name, _, _ in VARIANTS})
    out["fnu/rows"] = pick.astype(np.int32)
    out["fnu/freq"] = freq
    for name, _, _ in VARIANTS:
        f = np.array([[float(truths[name][i].fnu(nu)) for nu in freq[j]] for j, i in enumerate(pick)])
        assert np.all(np.isfinite(f)) and np.all(f >= 0)
        under = f < FLOOR * pars[pick, 4][:, None]
        print(name, "f_nu samples under the floor: %d of %d; X > 384: %d" %
              (under.sum(), f.size, (8 * 0.04799237 / pars[pick, 0][:, None] * freq > 384).sum()))
        assert under.sum() <= 0.02 * f.size, "more than 2 % of the samples fall under the floor"
        out["fnu/" + name] = f
    return save_npz(os.path.join(HERE, "hp_sed.npz"), out, check)


if __name__ == "__main__":
    chk = "--check" in sys.argv
    ok = write_math(chk)
    ok = write_sed(chk) and ok
    sys.exit(0 if ok else 1)
