"""Plain numpy restatement of the marginals' definition (include/mbb_hip.h: "binned posterior marginals"), for the
marginals tests: tests/test_marginals_cpu.py holds it to numpy.histogram / numpy.histogram2d, and
tests/test_marginals_gpu.py holds the device to it exactly."""
import numpy as np

EMPTY, NONFINITE, ABSENT, ROW_SHIFT = 1, 2, 4, 8
NAMES = ("T", "beta", "lambda0", "alpha", "fnorm", "peaklambda", "lir", "dustmass")


def edges(lo, hi, nbins):
    """numpy.linspace(lo, hi, nbins + 1) by its stated formula: the product and the sum rounded separately."""
    lo, hi = np.float64(lo), np.float64(hi)
    step = (hi - lo) / np.float64(nbins)
    e = np.arange(nbins + 1, dtype=np.float64) * step
    e = e + lo
    e[nbins] = hi
    return e


def auto_range(x):
    """(lo, hi) over the finite samples, widened by 0.5 when they are equal; None without a finite sample."""
    x = np.asarray(x, dtype=np.float64)
    f = x[np.isfinite(x)]
    if f.size == 0:
        return None
    lo, hi = f.min(), f.max()
    if lo == hi:
        lo, hi = lo - 0.5, hi + 0.5
    return float(lo), float(hi)


def place(x, e):
    """Per sample: the bin i with e[i] <= x < e[i + 1] (the last bin also takes x == e[-1]), or -1 below the range,
    -2 above it, -3 not finite.  By comparisons with the edges alone."""
    x = np.asarray(x, dtype=np.float64)
    nb = len(e) - 1
    out = np.full(x.shape, -3, dtype=np.int64)
    fin = np.isfinite(x)
    with np.errstate(invalid="ignore"):
        below, above = fin & (x < e[0]), fin & (x > e[-1])
    inside = fin & ~below & ~above
    idx = np.searchsorted(e, x[inside], side="right") - 1           # the last i with e[i] <= x
    idx[x[inside] == e[-1]] = nb - 1
    out[below], out[above], out[inside] = -1, -2, idx
    return out


def hist1d(x, nbins, rng=None):
    """The definition for one column of one source: counts, edges, the four sample counts and the status bits."""
    x = np.asarray(x, dtype=np.float64).ravel()
    auto = auto_range(x)
    nonfinite = int((~np.isfinite(x)).sum())
    status = NONFINITE if nonfinite else 0
    if auto is None:                                                # no finite sample: whatever range was given
        return dict(counts=np.zeros(nbins, dtype=np.int64), edges=np.full(nbins + 1, np.nan), n_used=0, n_below=0,
                    n_above=0, n_nonfinite=nonfinite, status=status | EMPTY, place=np.full(x.shape, -3))
    lo, hi = rng if rng is not None else auto
    e = edges(lo, hi, nbins)
    p = place(x, e)
    counts = np.bincount(p[p >= 0], minlength=nbins).astype(np.int64)
    return dict(counts=counts, edges=e, n_used=int(counts.sum()), n_below=int((p == -1).sum()),
                n_above=int((p == -2).sum()), n_nonfinite=nonfinite, status=status, place=p)


def hist2d(x, y, nbins2, rx=None, ry=None):
    """H[i][j] over the two columns' own ranges: a sample counts when it is binned in both."""
    hx, hy = hist1d(x, nbins2, rx), hist1d(y, nbins2, ry)
    px, py = hx["place"], hy["place"]
    both = (px >= 0) & (py >= 0)
    H = np.bincount(px[both] * nbins2 + py[both], minlength=nbins2 * nbins2).astype(np.int64)
    return H.reshape(nbins2, nbins2), hx["edges"], hy["edges"]


def levels_direct(H, fractions):
    """The definition, quadratic in the bins: for each fraction f the largest count c of the table such that the bins
    with count >= c hold at least f of the binned samples; 0 for an empty table."""
    h = [int(v) for v in np.asarray(H).ravel()]
    total = sum(h)
    out = []
    for f in fractions:
        best = 0
        if total > 0:
            for c in h:
                if sum(v for v in h if v >= c) >= float(f) * total and c > best:
                    best = c
        out.append(best)
    return np.array(out, dtype=np.int64)


def column(chain4, s, slot, burn=0, thin=1, extra=None):
    """The samples of (source s, column slot) in [walker][kept step] order; extra: {slot: [nsrc, nw, nsteps]}."""
    a = chain4[s, :, burn::thin, slot] if slot < 5 else extra[slot][s, :, burn::thin]
    return np.ascontiguousarray(a).ravel()


def _same_edges(e, ref, rtol):
    if rtol:
        return np.allclose(e, ref, rtol=rtol, atol=0.0, equal_nan=True)
    return np.array_equal(e.view(np.int64), ref.view(np.int64))


def check(got, chain4, bins, bins2d=0, pairs=(), ranges=None, burn=0, thin=1, extra=None, multi=None, label="",
          derived_edge_rtol=0.0):
    """A ChainMarginals against the definition, EXACTLY: counts, n_* and status by array_equal, edges bit for bit.
    `extra` holds the derived columns' per-entry values where those are to be checked ({slot: array}); the slots not
    named in it must be ABSENT.  derived_edge_rtol: the edges of the derived columns (slots 5 to 7) are held to that
    relative bound instead of bit for bit (automatic ranges of values that are themselves known to 1e-13)."""
    ranges = ranges or {}
    extra = extra or {}
    nsrc = chain4.shape[0]
    multi = (nsrc > 1) if multi is None else multi
    pick = (lambda a, s: a[s]) if multi else (lambda a, s: a)
    for s in range(nsrc):
        st, used, below, above, nonf = (pick(a, s) for a in (got.status, got.n_used, got.n_below, got.n_above,
                                                             got.n_nonfinite))
        for slot in range(8):
            if slot >= 5 and slot not in extra:
                assert st[slot] == ABSENT and used[slot] == 0, (label, s, slot, st[slot])
                continue
            ref = hist1d(column(chain4, s, slot, burn, thin, extra), bins, ranges.get(slot))
            counts, e = got.hist1d(NAMES[slot])
            counts, e = pick(counts, s), pick(e, s)
            assert counts.dtype == np.int64
            assert _same_edges(e, ref["edges"], derived_edge_rtol if slot >= 5 else 0.0), (label, s, slot, "edges")
            assert np.array_equal(counts, ref["counts"]), (label, s, slot, "counts",
                                                           np.flatnonzero(counts != ref["counts"])[:8])
            assert (used[slot], below[slot], above[slot], nonf[slot]) == (ref["n_used"], ref["n_below"], ref["n_above"],
                                                                        ref["n_nonfinite"]), (label, s, slot)
            assert st[slot] & 7 == ref["status"], (label, s, slot, st[slot], ref["status"])
        for a, b in pairs:
            H, xe, ye = got.hist2d(NAMES[a], NAMES[b])
            H, xe, ye = pick(H, s), pick(xe, s), pick(ye, s)
            rH, rx, ry = hist2d(column(chain4, s, a, burn, thin, extra), column(chain4, s, b, burn, thin, extra), bins2d,
                                ranges.get(a), ranges.get(b))
            assert _same_edges(xe, rx, derived_edge_rtol if a >= 5 else 0.0), (label, s, a, b, "xedges")
            assert _same_edges(ye, ry, derived_edge_rtol if b >= 5 else 0.0), (label, s, a, b, "yedges")
            assert np.array_equal(H, rH), (label, s, a, b, "counts2")


def random_chain(nsrc, nw, nsteps, seed, scale=None):
    """A chain with 40 % rejected-move repeats about a centre per source; scale [nsrc] multiplies source s."""
    rng = np.random.RandomState(seed)
    centre = np.array([25.0, 1.8, 500.0, 3.0, 30.0])
    width = np.array([4.0, 0.3, 120.0, 0.5, 6.0])
    R = nsrc * nw
    chain = np.empty((R, nsteps, 5))
    chain[:, 0] = centre + width * rng.standard_normal((R, 5))
    for t in range(1, nsteps):
        move = rng.rand(R) < 0.6
        chain[:, t] = np.where(move[:, None], centre + width * rng.standard_normal((R, 5)), chain[:, t - 1])
    chain = chain.reshape(nsrc, nw, nsteps, 5)
    if scale is not None:
        chain = chain * np.asarray(scale, dtype=np.float64)[:, None, None, None]
    return chain


def edge_values(e):
    """Every edge with its two neighbours in the doubles: on, just under, just over."""
    return np.concatenate((e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)))
