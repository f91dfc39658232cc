"""The definition of a posterior draw restated in numpy and Python integers, for tests/test_draws_cpu.py and
tests/test_draws_gpu.py: its own Philox4x32-10, the multiply-shift (u * N) >> 64 in unbounded integers, the window
written as the list of kept steps, and the gather as plain indexing.  Nothing of it is shared with the library."""
import numpy as np

MASK32 = 0xFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
STREAM = 0x44524157                 # "DRAW"


def philox4x32(counter, key, rounds=10):
    """Philox4x32 (Salmon et al. 2011) of one counter (four 32-bit words) and key (two): four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & MASK32 for c in counter)
    k0, k1 = (int(k) & MASK32 for k in key)
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox_u64(n, src, seed):
    """u of draws 0 .. n - 1 of source src: words 0 and 1 of the counters (i, src, STREAM, 1), as Python integers.
    (numpy's unsigned 64-bit products of 32-bit words are exact; the same rounds as philox4x32, all draws at once.)"""
    u64 = np.uint64
    c = [np.arange(n, dtype=u64), np.full(n, src, dtype=u64), np.full(n, STREAM, dtype=u64), np.full(n, 1, dtype=u64)]
    k0, k1 = int(seed) & MASK32, (int(seed) >> 32) & MASK32
    m32, s32 = u64(MASK32), u64(32)
    for _ in range(10):
        p0, p1 = u64(PHILOX_M0) * c[0], u64(PHILOX_M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ u64(k0), p1 & m32, (p0 >> s32) ^ c[3] ^ u64(k1), p0 & m32]
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return [int(a) | (int(b) << 32) for a, b in zip(c[0], c[1])]


def picks(n, N, how="random", seed=0, src=0):
    """Which of a source's N window samples draws 0 .. n - 1 are: a list of Python integers."""
    n, N = int(n), int(N)
    if how == "even":
        return [(i * N) // n for i in range(n)]
    assert how == "random"
    return [(u * N) >> 64 for u in philox_u64(n, src, seed)]


def kept_steps(nsteps, burn, thin):
    """The steps of the window, as a (lazy) sequence."""
    return range(int(burn), int(nsteps), int(thin))


def indices(nsrc, nw, nsteps, burn, thin, n, how="random", seed=0):
    """(walker, step) of every draw, [nsrc, n, 2]: the window's samples are numbered walker by walker, each walker's
    kept steps in order."""
    steps = kept_steps(nsteps, burn, thin)
    nkept = len(steps)
    out = np.zeros((nsrc, n, 2), dtype=np.int64)
    for s in range(nsrc):
        for i, j in enumerate(picks(n, nw * nkept, how, seed, s)):
            w, k = divmod(j, nkept)
            out[s, i] = (w, steps[k])
    return out


def gather(chain, lnprob, index):
    """The cells of chain [nsrc, nw, nsteps, 5] (lnprob [nsrc, nw, nsteps] or None) at index [nsrc, n, 2]: rows
    [nsrc, n, 5] and lnprob [nsrc, n] (NaN without one)."""
    nsrc, n = index.shape[:2]
    src = np.arange(nsrc)[:, None]
    rows = chain[src, index[..., 0], index[..., 1]]
    lnp = lnprob[src, index[..., 0], index[..., 1]] if lnprob is not None else np.full((nsrc, n), np.nan)
    return np.ascontiguousarray(rows), np.ascontiguousarray(lnp)


def planted_chain(nsrc, nw, nsteps, scale=None):
    """A chain whose every cell says where it is: column k of cell (s, w, t) is scale_s * (1000 s + 100 k + w +
    t / 1024), lnprob -(s + w / 64 + t / 65536); all exact in doubles."""
    s, w, t = np.meshgrid(np.arange(nsrc), np.arange(nw), np.arange(nsteps), indexing="ij")
    sc = np.ones(nsrc) if scale is None else np.asarray(scale, dtype=np.float64)
    chain = np.empty((nsrc, nw, nsteps, 5))
    for k in range(5):
        chain[..., k] = sc[:, None, None] * (1000.0 * s + 100.0 * k + w + t / 1024.0)
    lnp = -(s + w / 64.0 + t / 65536.0)
    return chain, np.ascontiguousarray(lnp)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
