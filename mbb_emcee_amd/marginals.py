"""Binned posterior marginals of a chain computed where the chain is (mbb_marginals.hip.h): per source and column
a histogram, per source and pair of columns a 2-D histogram -- the per-parameter PDFs, the T-beta contours and the
corner plot without the chain leaving the device.

The reference has no code for this: its users call ``numpy.histogram`` / ``corner`` on
``mbb_results.parameter_chain``.  numpy is the yardstick: the edges are ``numpy.linspace``'s bit for bit and the
counts are ``numpy.histogram``'s and ``numpy.histogram2d``'s exactly.
"""
import ctypes as C
import itertools

import numpy as np

from . import _analysis, _native
from . import results

__all__ = ["chain_marginals", "ChainMarginals"]

COLUMN_NAMES = ("T", "beta", "lambda0", "alpha", "fnorm", "peaklambda", "lir", "dustmass")
_range = range                # (``range`` is a keyword of the public calls, as it is of numpy.histogram)


def _slot(name):
    """Column slot of a name in ``results``' vocabulary (a parameter name or index, or a derived quantity)."""
    if isinstance(name, str) and name.lower() in results._DERIVED:
        return results._DERIVED[name.lower()]
    return results._paridx(name)


class _Request(_analysis.Window):
    """What one native marginals call is asked for (mbb_marginals_spec); everything is checked here, before the
    device is touched."""

    def __init__(self, bins=64, bins2d=0, pairs="params", range=None, burn=0, thin=1, derived=(), redshift=None,
                 lumdist_mpc=None, kappa=2.64, kappa_wave=125.0, lir_range=(8.0, 1000.0), peak_model="fit",
                 nsources=1):
        # burn, thin and the derived columns' settings are a summary request's (its percentiles are not used)
        self.summary = results._Request([50.0], burn, thin, None, derived, redshift, lumdist_mpc, kappa, kappa_wave,
                                        lir_range, peak_model, nsources=nsources)
        self.burn, self.thin, self.derived = self.summary.burn, self.summary.thin, self.summary.derived
        self.bins, self.bins2d = int(bins), int(bins2d)
        if not 1 <= self.bins <= _native.MARG_MAX_BINS:
            raise ValueError("bins must be between 1 and {:d}".format(_native.MARG_MAX_BINS))
        if not 0 <= self.bins2d <= _native.MARG_MAX_BINS2:
            raise ValueError("bins2d must be between 0 and {:d}".format(_native.MARG_MAX_BINS2))
        self.columns = list(_range(5)) + sorted(results._DERIVED[d] for d in set(self.derived))
        if isinstance(pairs, str):
            if pairs not in ("params", "all"):
                raise ValueError("pairs must be 'params', 'all' or a list of name pairs")
            cols = _range(5) if pairs == "params" else self.columns
            self.pairs = list(itertools.combinations(cols, 2)) if self.bins2d else []
        else:
            self.pairs = []
            for pr in pairs:
                if len(pr) != 2:
                    raise ValueError("a pair is two column names")
                a, b = _slot(pr[0]), _slot(pr[1])
                if a == b:
                    raise ValueError("a pair needs two different columns")
                for s in (a, b):
                    if s not in self.columns:
                        raise ValueError("{} was not asked for (derived=)".format(COLUMN_NAMES[s]))
                if (min(a, b), max(a, b)) not in self.pairs:
                    self.pairs.append((min(a, b), max(a, b)))
            if self.pairs and not self.bins2d:
                raise ValueError("pairs need bins2d > 0")
        if len(self.pairs) > _native.MARG_MAX_PAIRS:
            raise ValueError("at most {:d} pairs per call".format(_native.MARG_MAX_PAIRS))
        self.range = {}
        for key, (lo, hi) in (range or {}).items():
            slot = _slot(key)
            if slot not in self.columns:
                raise ValueError("{} was not asked for (derived=)".format(COLUMN_NAMES[slot]))
            lo, hi = float(lo), float(hi)
            if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and np.isfinite(hi - lo)):
                raise ValueError("the range of {} must be finite with lo < hi".format(COLUMN_NAMES[slot]))
            self.range[slot] = (lo, hi)

    def spec(self):
        s = _native.MarginalsSpec()
        s.nbins, s.nbins2, s.npairs = self.bins, self.bins2d, len(self.pairs)
        for i, (a, b) in enumerate(self.pairs):
            s.pairs[i][0], s.pairs[i][1] = a, b
        for slot, (lo, hi) in self.range.items():
            s.has_range[slot], s.lo[slot], s.hi[slot] = 1, lo, hi
        # (the summary spec lives as long as the spec that points at it)
        s._summary = self.summary.spec()
        s.summary = C.pointer(s._summary)
        return s


class _Raw(object):
    """The arrays of one native marginals call (mbb_marginals_out), nsrc leading."""

    def __init__(self, nsrc, nbins, nbins2, npairs):
        nc = _native.SUMMARY_COLS
        self.counts1 = np.zeros((nsrc, nc, nbins), dtype=np.uint32)
        self.edges1 = np.full((nsrc, nc, nbins + 1), np.nan)
        self.counts2 = np.zeros((nsrc, npairs, nbins2, nbins2), dtype=np.uint32)
        self.edges2 = np.full((nsrc, nc, nbins2 + 1), np.nan)     # (not written by a call without 2-d tables)
        self.n_used, self.n_below, self.n_above, self.n_nonfinite = (np.zeros((nsrc, nc), dtype=np.int64)
                                                                     for _ in _range(4))
        self.status = np.zeros((nsrc, nc), dtype=np.int32)

    def out(self):
        return _analysis.bind_out(_native.MarginalsOut, vars(self))


RAW_FIELDS = ("counts1", "edges1", "counts2", "edges2", "n_used", "n_below", "n_above", "n_nonfinite", "status")


def levels_of(H, fractions=(0.683, 0.954)):
    """Count thresholds of the highest-density regions of one table: for each fraction f the largest count c such
    that the bins with count >= c hold at least f of the binned samples (0 for an empty table)."""
    h = np.asarray(H, dtype=np.int64).ravel()
    total = int(h.sum())
    vals, mult = np.unique(h, return_counts=True)
    vals, mass = vals[::-1], np.cumsum((vals * mult)[::-1])            # mass of the bins with count >= vals[k]
    out = np.zeros(len(fractions), dtype=np.int64)
    for i, f in enumerate(fractions):
        f = float(f)
        if not 0.0 < f <= 1.0:
            raise ValueError("a fraction must be in (0, 1]")
        if total > 0:
            out[i] = vals[int(np.argmax(mass >= f * total))]
    return out


class ChainMarginals(_analysis.Result):
    """Binned marginals of a chain (a leading source axis for a multi-source chain).  Column names are
    ``results``' (a parameter name or index, "peaklambda", "lir", "dustmass").

    hist1d(name) : (counts, edges), ``numpy.histogram``'s;
    pdf1d(name) : (density, edges), ``numpy.histogram(..., density=True)``'s;
    hist2d(a, b) : (H, xedges, yedges), ``numpy.histogram2d``'s;
    mode(name) : the centre of the first bin of largest count;
    levels(a, b, fractions) : the count thresholds of the highest-density regions holding those fractions;
    n_used, n_below, n_above, n_nonfinite : samples binned, below / above the range, NaN or infinite, per column [8];
    status : bits EMPTY (no finite sample), NONFINITE, ABSENT (a derived column not asked for), and from ROW_SHIFT
        on the row status of failing SED rows, as a summary reports them."""

    EMPTY, NONFINITE, ABSENT, ROW_SHIFT = (_native.MARG_EMPTY, _native.MARG_NONFINITE, _native.MARG_ABSENT,
                                           _native.MARG_ROW_SHIFT)

    def __init__(self, request, raw, multi, nwalkers, nkept):
        self._req, self._raw, self._multi = request, raw, multi
        self.bins, self.bins2d = request.bins, request.bins2d
        self.pairs = [(COLUMN_NAMES[a], COLUMN_NAMES[b]) for a, b in request.pairs]
        self._set_window(request, nwalkers, nkept)

    def _column(self, name):
        slot = _slot(name)
        if slot not in self._req.columns:
            raise ValueError("{} was not asked for when the marginals were made (derived=)".format(COLUMN_NAMES[slot]))
        return slot

    def hist1d(self, name):
        slot = self._column(name)
        return (self._squeeze(self._raw.counts1[:, slot].astype(np.int64)), self._squeeze(self._raw.edges1[:, slot].copy()))

    def pdf1d(self, name):
        slot = self._column(name)
        n, e = self._raw.counts1[:, slot].astype(np.int64), self._raw.edges1[:, slot]
        with np.errstate(invalid="ignore", divide="ignore"):
            pdf = n / np.diff(e, axis=-1) / n.sum(axis=-1, keepdims=True)
        return self._squeeze(pdf), self._squeeze(e.copy())

    def hist2d(self, a, b):
        sa, sb = self._column(a), self._column(b)
        if sa == sb or (min(sa, sb), max(sa, sb)) not in self._req.pairs:
            raise ValueError("the pair ({}, {}) was not asked for when the marginals were made (pairs=, bins2d=)".format(
                COLUMN_NAMES[sa], COLUMN_NAMES[sb]))
        H = self._raw.counts2[:, self._req.pairs.index((min(sa, sb), max(sa, sb)))].astype(np.int64)
        if sa > sb:
            H = np.ascontiguousarray(np.swapaxes(H, -1, -2))
        return (self._squeeze(H), self._squeeze(self._raw.edges2[:, sa].copy()), self._squeeze(self._raw.edges2[:, sb].copy()))

    def mode(self, name):
        slot = self._column(name)
        n, e = self._raw.counts1[:, slot], self._raw.edges1[:, slot]
        i = np.argmax(n, axis=-1)                                          # (the first of tied maxima)
        rows = np.arange(n.shape[0])
        return self._squeeze(0.5 * (e[rows, i] + e[rows, i + 1]))

    def levels(self, a, b, fractions=(0.683, 0.954)):
        fractions = tuple(np.atleast_1d(fractions))
        H = self.hist2d(a, b)[0]
        H = H if self._multi else H[None]
        return self._squeeze(np.array([levels_of(h, fractions) for h in H]))

    n_used = property(lambda self: self._squeeze(self._raw.n_used).copy())
    n_below = property(lambda self: self._squeeze(self._raw.n_below).copy())
    n_above = property(lambda self: self._squeeze(self._raw.n_above).copy())
    n_nonfinite = property(lambda self: self._squeeze(self._raw.n_nonfinite).copy())
    status = property(lambda self: self._squeeze(self._raw.status).copy())

    def arrays(self, prefix="marginals_"):
        """The tables as plain arrays (for an .npz): counts1 [..., 8, bins], edges1 [..., 8, bins + 1], and with 2-D
        tables counts2 [..., npairs, bins2d, bins2d], edges2 [..., 8, bins2d + 1] and pairs [npairs, 2] (column slots)."""
        r = self._raw
        out = {prefix + "counts1": self._squeeze(r.counts1).copy(), prefix + "edges1": self._squeeze(r.edges1).copy(),
               prefix + "n_used": self.n_used, prefix + "n_below": self.n_below, prefix + "n_above": self.n_above,
               prefix + "n_nonfinite": self.n_nonfinite, prefix + "status": self.status,
               prefix + "columns": np.array(COLUMN_NAMES)}
        if self._req.pairs:
            out.update({prefix + "counts2": self._squeeze(r.counts2).copy(), prefix + "edges2": self._squeeze(r.edges2).copy(),
                        prefix + "pairs": np.array(self._req.pairs, dtype=np.int32).reshape(-1, 2)})
        return out

    def __str__(self):
        """One line per column: range, mode, outside counts; the first source of a multi-source result."""
        r = self._raw
        lines = []
        if self._multi:
            lines.append("Source 0 of {:d}".format(r.status.shape[0]))
        lines.append("Marginals over {:d} steps of {:d} walkers, {:d} bins{:s}".format(
            self.nsteps_used, self.nwalkers, self.bins,
            ", {:d} pairs of {:d} x {:d}".format(len(self.pairs), self.bins2d, self.bins2d) if self.pairs else ""))
        for slot in self._req.columns:
            st = int(r.status[0, slot])
            if st & self.EMPTY:
                lines.append("  {:10s} no finite sample".format(COLUMN_NAMES[slot]))
                continue
            e, n = r.edges1[0, slot], r.counts1[0, slot]
            i = int(np.argmax(n))
            lines.append("  {:10s} range: [{:.6g}, {:.6g}]  mode: {:.6g}  below: {:d}  above: {:d}  not finite: {:d}".format(
                COLUMN_NAMES[slot], e[0], e[-1], 0.5 * (e[i] + e[i + 1]), int(r.n_below[0, slot]),
                int(r.n_above[0, slot]), int(r.n_nonfinite[0, slot])))
        return "\n".join(lines)


def chain_marginals(like, chain, bins=64, bins2d=0, pairs="params", range=None, burn=0, thin=1, derived=(),
                    redshift=None, lumdist_mpc=None, kappa=2.64, kappa_wave=125.0, lir_range=(8.0, 1000.0),
                    peak_model="fit"):
    """Binned marginals of a stored chain [nw, nsteps, 5] (or [nsources, nw, nsteps, 5]) over the steps
    ``chain[:, burn::thin]``, computed on ``like``'s device; returns a ``ChainMarginals``.

    bins : bins of every 1-d histogram (1 to 4096);  bins2d : bins per axis of the 2-d tables (0: none; at most 100);
    pairs : "params" (all ten pairs of the five parameters), "all" (all pairs of the columns present), or a list of
        name pairs; either order of a pair is accepted;
    range : ``{name: (lo, hi)}``, one range for every source; a column without one gets, per source, the min and max of
        its finite samples (``numpy.histogram``'s default), widened by 0.5 on either side when they are equal;
    derived, redshift, lumdist_mpc, kappa, kappa_wave, lir_range, peak_model : ``results.chain_summary``'s."""
    c4, multi = _native.chain4(chain)
    nsrc, nw, nsteps = c4.shape[:3]
    if nsrc < 1 or nw < 1 or nsteps < 1:
        raise ValueError("the chain is empty")
    req = _Request(bins, bins2d, pairs, range, burn, thin, derived, redshift, lumdist_mpc, kappa, kappa_wave, lir_range,
                   peak_model, nsources=nsrc)
    nkept = req.check_steps(nsteps)
    ctx = _native.analysis_context(like)
    raw = _Raw(nsrc, req.bins, req.bins2d, len(req.pairs))
    spec, out = req.spec(), raw.out()
    _native.check_arg(ctx.lib.mbb_chain_marginals(ctx.h, _native._d(c4), nsrc, nw, nsteps, C.byref(spec), C.byref(out)), ctx)
    return ChainMarginals(req, raw, multi, nw, nkept)
