"""What the analyses of a chain have in common (summary, diagnostics, marginals, predictions, draws, goodness of fit,
evidence, WAIC / PSIS-LOO): the burn / thin window of a request, the percentiles of a central interval, the
likelihood's photometry, the coercion of the arrays handed in, and the plumbing of a result class.  An analysis adds
what is its own.
"""
import ctypes as C

import numpy as np


_POINTEE = {}        # a ctypes pointer type -> the dtype of what it points at


def bind_out(struct, arrays):
    """An output struct of ``_native`` (``SummaryOut``, ``DiagOut``, ...) whose pointer fields point at ``arrays``, a
    mapping from field names to the arrays the library is to fill (a field of several pointers: a sequence of as
    many arrays or ``None``s).  Each address is cast to the field's own declared pointer type: an array of another dtype is a
    ``TypeError``, one that is not C-contiguous a ``ValueError``.  A missing or ``None`` entry leaves its field null
    (an optional output); entries that name no field are ignored, so that a result object's ``vars()`` will do."""
    def pointer(ptype, a, name):
        if a is None:
            return ptype()
        want = _POINTEE.get(ptype)
        if want is None:
            want = _POINTEE[ptype] = np.dtype(ptype._type_)
        if not isinstance(a, np.ndarray) or a.dtype != want:
            raise TypeError("{}.{} takes an array of {}, not {}".format(
                struct.__name__, name, want, getattr(a, "dtype", type(a).__name__)))
        if not a.flags.c_contiguous:
            raise ValueError("{}.{} takes a C-contiguous array".format(struct.__name__, name))
        return a.ctypes.data_as(ptype)

    o = struct()
    for name, ctype in struct._fields_:
        a = arrays.get(name)
        if a is None:
            continue
        if issubclass(ctype, C.Array):
            if len(a) != ctype._length_:
                raise ValueError("{}.{} takes {:d} arrays, not {:d}".format(struct.__name__, name, ctype._length_, len(a)))
            for k, item in enumerate(a):
                getattr(o, name)[k] = pointer(ctype._type_, item, "{}[{:d}]".format(name, k))
        else:
            setattr(o, name, pointer(ctype, a, name))
    return o


def quantiles(percentile, percentiles):
    """(the central intervals asked for, the q values that serve them and ``percentiles``, each once)"""
    from . import results
    cens = [float(p) for p in np.atleast_1d(percentile)]
    qs = []
    for q in [q for p in cens for q in results._pval(p)] + [float(q) for q in percentiles]:
        if q not in qs:
            qs.append(q)
    return cens, qs


class Window(object):
    """The steps ``chain[:, burn::thin]`` of a request."""
    thin = 1

    def set_window(self, burn, thin):
        self.burn, self.thin = int(burn), int(thin)
        if self.burn < 0 or self.thin < 1:
            raise ValueError("burn must be >= 0 and thin >= 1")

    def check_steps(self, nsteps):
        """The number of kept steps per walker."""
        if int(nsteps) < 1 or self.burn >= int(nsteps):
            raise ValueError("burn leaves no step of the chain")
        return (int(nsteps) - self.burn + self.thin - 1) // self.thin


def check_sources(like_nsources, chain_nsources):
    if chain_nsources != like_nsources and like_nsources != 1:
        raise ValueError("the chain has {:d} sources, the likelihood {:d}: they must agree, or the likelihood hold "
                         "one source for all".format(chain_nsources, like_nsources))


def photometry(like, what):
    """(ndata, flux [nsources, ndata], sigma [nsources, ndata]) of the data ``like`` holds; ``what`` names the caller
    in the refusal."""
    if not like.data_read:
        raise Exception("Data not read: {} needs the likelihood's photometry".format(what))
    if like.nsources > 1:
        flux = np.array(like._flux_multi, dtype=np.float64)
        sigma = 1.0 / np.sqrt(np.asarray(like._ivar_multi, dtype=np.float64))
    else:
        flux = np.array(like._flux, dtype=np.float64)[None]
        sigma = np.array(like.data_flux_unc, dtype=np.float64)[None]
    return int(like._ndata), flux, sigma


def rows5(pars):
    """Parameter rows as the library takes them: contiguous [n, 5] doubles."""
    p = np.ascontiguousarray(np.atleast_2d(np.asarray(pars, dtype=np.float64)))
    if p.ndim != 2 or p.shape[1] != 5 or p.shape[0] < 1:
        raise ValueError("pars must be [n, 5]")
    return p


def lnprob_like(lnprob, c4, multi):
    """The lnprob of the chain ``c4`` [nsrc, nw, nsteps, 5] as the library takes it: contiguous [nsrc, nw, nsteps]."""
    lp = np.ascontiguousarray(lnprob, dtype=np.float64)
    if lp.shape != c4.shape[0 if multi else 1:3]:
        raise ValueError("lnprob must have the chain's shape without its last axis")
    return lp if multi else lp[None]


class Result(object):
    """The plumbing of a result class: the window it was made over, and the source axis."""

    def _set_window(self, request, nwalkers, nkept):
        self.burn, self.thin = request.burn, request.thin
        self.nwalkers, self.nsteps_used = int(nwalkers), int(nkept)

    def _squeeze(self, a):
        return a if self._multi else a[0]
