"""A model of the device sampler's calling contract (DeviceEnsembleSampler.run_mcmc / sample / reset: their
docstrings), a seeded generator of programs of calls, the runner that holds a sampler to the model after every call,
and a numpy stand-in sampler on which model and runner are themselves tested without a GPU.

The oracle is the trajectory.  A step's Philox key is its number in the sampler's life, so every interleaving of
run_mcmc and sample() that starts from one p0 and never sets a different state walks one trajectory: one
``run_mcmc(p0, T)`` of a fresh sampler with the same seed gives every position and log-probability (``ref_chain``,
``ref_lnp``), the same trajectory made one step per call gives every acceptance count (``acc_true[..., t]``: the accepted
moves of steps 0..t).  What a call may show is then a matter of three numbers -- how far the device is (``life``), how far
the attributes show (``shown``), where the counts were last zeroed (``base``) -- and the list of life steps in the stored
chain.  Everything is compared bit for bit.

Operations of a program (``Op``):
    R   run_mcmc(None, k, storechain=store)                      k = 0..20
    S   sample(..., iterations=k, chunk=chunk, storechain=store) consumed whole
    B   the same, left by ``break`` after j steps
    K   the same, the generator kept after j steps while ``nxt`` (an R, S, B or Z) runs; then it is resumed
        (RuntimeError) or closed / deleted (nothing may change)
    Z   reset(); run_mcmc(None, 1) raises; run_mcmc(pos, k, lnprob0=lnp) with the last returned state
The first operation of a program is given p0.  A later S, B or K passes None, or (``given``) the state the last call
returned with its log-probabilities as lnprob0: the same trajectory, since lnprob0 is taken as given.
"""
import collections
import gc

import numpy as np

CHUNK_KINDS = ("1", "3", "7", "k", "k+5")
KMAX = 20

Op = collections.namedtuple("Op", "kind k store chunk chunk_kind j fate given nxt onto used")
Op.__new__.__defaults__ = (None,) * 8


# ---------------------------------------------------------------------------------------------------- the programs
def _made(k, chunk, j):
    """Steps the device has made when step j (1-based) of sample(iterations=k, chunk=chunk) is out."""
    c = max(1, chunk)
    return min(k, -(-j // c) * c)


def program(seed, life=200):
    """The operations of program `seed`: drawn until `life` life steps are used (at most life + 2 KMAX - 1)."""
    rng = np.random.RandomState(7919 + int(seed))
    state = {"fresh": False, "stored": 0}       # is the last returned state the device's?  steps in the stored chain

    def draw(first, kinds, probs):
        kind = kinds[rng.choice(len(kinds), p=probs)]
        k = int(rng.randint(0, KMAX + 1))
        store = bool(rng.rand() < 0.75)
        if kind == "R":
            state["stored"] += k if store else 0
            state["fresh"] = True
            return Op("R", k, store, used=k)
        if kind == "Z":
            state["stored"] = k if store else 0
            state["fresh"] = True
            return Op("Z", k, store, used=k)
        ck = CHUNK_KINDS[rng.randint(len(CHUNK_KINDS))]
        if kind in "BK":
            k = max(k, 1)
        chunk = {"k": k, "k+5": k + 5}.get(ck) if ck in ("k", "k+5") else int(ck)
        given = bool(not first and state["fresh"] and rng.rand() < 0.4)
        onto = state["stored"] > 0
        if kind == "S":
            state["stored"] += k if store else 0
            state["fresh"] = state["fresh"] if k == 0 else True
            return Op("S", k, store, chunk, ck, given=given, onto=onto, used=k)
        j = int(rng.randint(1, k + 1))
        made = _made(k, chunk, j)
        state["stored"] += made if store else 0
        state["fresh"] = j == made
        if kind == "B":
            return Op("B", k, store, chunk, ck, j, given=given, onto=onto, used=made)
        fate = ("resume", "resume", "close", "del")[rng.randint(4)]
        nxt = draw(False, ("R", "S", "B", "Z"), (0.3, 0.3, 0.2, 0.2))
        return Op("K", k, store, chunk, ck, j, fate, given, nxt, onto, made + nxt.used)

    ops, n = [], 0
    while n < life:
        first = not ops
        op = draw(first, ("R", "S", "B", "K", "Z")[:4 if first else 5],
                  (0.25, 0.3, 0.2, 0.25) if first else (0.2, 0.28, 0.15, 0.22, 0.15))
        ops.append(op)
        n += op.used
    return ops


def flat_ops(ops):
    for op in ops:
        yield op
        if op.nxt is not None:
            yield op.nxt


def coverage(programs):
    """What a set of programs exercises: the counts that tests/test_sampler_contract_cpu.py holds to their minima."""
    c = collections.Counter()
    lives = []
    for ops in programs:
        lives.append(sum(op.used for op in ops))
        for op in flat_ops(ops):
            c[op.kind] += 1
            if op.kind == "K":
                c["K-resumed" if op.fate == "resume" else "K-closed"] += 1
            if not op.store:
                c["storechain=False"] += 1
            if op.kind in "SBK":
                c["chunk " + op.chunk_kind] += 1
                c["onto a stored chain"] += bool(op.onto)
                c["state and lnprob0 given"] += bool(op.given)
    c["life min"], c["life max"] = min(lives), max(lives)
    return dict(c)


# ------------------------------------------------------------------------------------------------------- the model
class Model(object):
    """What the contract lets a sampler show, over a reference trajectory: p0 [lead, 5], lnp0 [lead] (the state before
    step 0), ref_chain [lead, T, 5], ref_lnp [lead, T], acc_true [lead, T]."""

    def __init__(self, p0, lnp0, ref_chain, ref_lnp, acc_true):
        self.p0, self.lnp0 = np.asarray(p0, dtype=np.float64), np.asarray(lnp0, dtype=np.float64)
        self.ref_chain, self.ref_lnp, self.acc_true = ref_chain, ref_lnp, np.asarray(acc_true, dtype=np.float64)
        self.lead = self.p0.shape[:-1]
        self.T = ref_chain.shape[-2]
        assert ref_chain.shape == self.lead + (self.T, 5) and ref_lnp.shape == self.lead + (self.T,)
        assert self.acc_true.shape == self.lead + (self.T,) and self.lnp0.shape == self.lead
        self.life = self.shown = self.base = 0
        self.iterations = 0
        self.idx = []                              # the life steps of the stored chain, as the attributes show it
        self._s = None                             # the sample() that is out

    # ---- the trajectory
    def state_at(self, n):
        """(pos, lnprob) after n steps of the sampler's life"""
        if n == 0:
            return self.p0, self.lnp0
        return self.ref_chain[..., n - 1, :], self.ref_lnp[..., n - 1]

    def accepted(self, n):
        return self.acc_true[..., n - 1] if n > 0 else np.zeros(self.lead)

    # ---- the calls
    def run(self, k, store):
        assert self._s is None and self.shown == self.life and self.life + k <= self.T
        if store:
            self.idx = self.idx + list(range(self.life, self.life + k))
        self.life += k
        self.shown = self.life
        self.iterations += k

    def reset(self):
        assert self._s is None and self.shown == self.life
        self.idx, self.iterations, self.base = [], 0, self.life

    def begin(self, k, chunk, store):
        assert self._s is None and self.shown == self.life and self.life + k <= self.T
        self._s = dict(k=k, chunk=max(1, int(chunk)), store=store, L0=self.life, it0=self.iterations, idx0=self.idx, done=0)

    def _show(self, n):
        s = self._s
        self.shown = s["L0"] + n
        self.iterations = s["it0"] + n
        self.idx = s["idx0"] + list(range(s["L0"], s["L0"] + n)) if s["store"] else s["idx0"]

    def step(self):
        """the next step is handed out; returns the (pos, lnprob) it must be"""
        s = self._s
        s["done"] += 1
        assert s["done"] <= s["k"]
        self.life = s["L0"] + _made(s["k"], s["chunk"], s["done"])
        self._show(s["done"])
        return self.state_at(self.shown)

    def leave(self):
        """the generator ends, is left, closed or retired: the attributes go to the end of the chunk the device made"""
        self._show(self.life - self._s["L0"])
        self._s = None

    # ---- what must be seen
    def expected(self):
        i = np.asarray(self.idx, dtype=np.intp)
        nacc = self.accepted(self.shown) - self.accepted(self.base)
        return dict(chain=self.ref_chain[..., i, :], lnprobability=self.ref_lnp[..., i], iterations=self.iterations,
                    naccepted=nacc, acceptance_fraction=nacc / max(self.iterations, 1))

    def check(self, sampler, where=""):
        e = self.expected()
        n = len(self.idx)
        flat = (self.lead[0], self.lead[1] * n, 5) if len(self.lead) == 2 else (self.lead[0] * n, 5)
        _same(sampler.chain, e["chain"], "chain", where)
        _same(sampler.lnprobability, e["lnprobability"], "lnprobability", where)
        if tuple(sampler.flatchain.shape) != flat:
            raise AssertionError("%s: flatchain.shape %r, the contract says %r" % (where, sampler.flatchain.shape, flat))
        if sampler.iterations != e["iterations"]:
            raise AssertionError("%s: iterations %r, the contract says %r" % (where, sampler.iterations, e["iterations"]))
        _same(sampler.naccepted, e["naccepted"], "naccepted", where)
        _same(sampler.acceptance_fraction, e["acceptance_fraction"], "acceptance_fraction", where)


def _same(got, want, name, where):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError("%s: %s has shape %r, the contract says %r" % (where, name, got.shape, want.shape))
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %s differs from the reference trajectory in %d cells, first at %r: %r for %r"
                             % (where, name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------------ the runner
def run_program(sampler, model, ops, label=""):
    """Run the operations on the sampler and hold it to the model after every one, and at every step a sample() hands
    out.  Returns the number of checks made."""
    r = _Runner(sampler, model, label)
    for i, op in enumerate(ops):
        r.apply(op, first=(i == 0), where="%s op %d %s" % (label, i, _show_op(op)))
    return r.checks


def _show_op(op):
    return "%s(%s)" % (op.kind, ", ".join("%s=%r" % (f, getattr(op, f)) for f in ("k", "store", "chunk", "j", "fate", "given")
                                          if getattr(op, f) is not None))


class _Runner(object):
    def __init__(self, sampler, model, label):
        self.s, self.m, self.label = sampler, model, label
        self.last = None                           # (pos, lnprob, life steps they are the state after)
        self.checks = 0

    def check(self, where):
        self.m.check(self.s, where)
        self.checks += 1

    def took(self, pos, lnp, at, where):
        wp, wl = self.m.state_at(at)
        _same(pos, wp, "the returned positions", where)
        _same(lnp, wl, "the returned log-probabilities", where)
        self.last = (np.array(pos), np.array(lnp), at)

    def sample_args(self, op, first):
        if first:
            return self.m.p0, None
        if op.given:
            assert self.last is not None and self.last[2] == self.m.life, "a program gives a state that is not the device's"
            return self.last[0], self.last[1]
        return None, None

    def apply(self, op, first, where):
        s, m = self.s, self.m
        if op.kind == "R":
            pos, lnp, _ = s.run_mcmc(m.p0 if first else None, op.k, storechain=op.store)
            m.run(op.k, op.store)
            self.took(pos, lnp, m.life, where)
            self.check(where)
        elif op.kind == "Z":
            if self.last is None or self.last[2] != m.life:      # (left inside a chunk: the state is the device's, not the last handed out)
                pos, lnp, _ = s.run_mcmc(None, 0)
                m.run(0, True)
                self.took(pos, lnp, m.life, where + " [0 steps]")
                self.check(where + " [0 steps]")
            s.reset()
            m.reset()
            self.check(where + " [reset]")
            try:
                s.run_mcmc(None, 1)
            except ValueError:
                pass
            else:
                raise AssertionError("%s: run_mcmc(None, 1) after reset() must raise ValueError" % where)
            self.check(where + " [refused]")
            pos, lnp, _ = s.run_mcmc(self.last[0], op.k, lnprob0=self.last[1], storechain=op.store)
            m.run(op.k, op.store)
            self.took(pos, lnp, m.life, where)
            self.check(where)
        else:
            p0, l0 = self.sample_args(op, first)
            kw = dict(lnprob0=l0, iterations=op.k, storechain=op.store, chunk=op.chunk)
            if op.kind == "S":
                m.begin(op.k, op.chunk, op.store)
                for pos, lnp, _ in s.sample(p0, **kw):
                    self.stepped(pos, lnp, where)
                m.leave()
                self.check(where + " [whole]")
            elif op.kind == "B":
                m.begin(op.k, op.chunk, op.store)
                n = 0
                for pos, lnp, _ in s.sample(p0, **kw):
                    self.stepped(pos, lnp, where)
                    n += 1
                    if n == op.j:
                        break
                m.leave()
                self.check(where + " [left after %d]" % op.j)
            else:
                m.begin(op.k, op.chunk, op.store)
                g = s.sample(p0, **kw)
                for _ in range(op.j):
                    pos, lnp, _ = next(g)
                    self.stepped(pos, lnp, where)
                m.leave()                           # what the next call does first
                self.apply(op.nxt, False, where + " -> " + _show_op(op.nxt))
                if op.fate == "resume":
                    try:
                        next(g)
                    except RuntimeError:
                        pass
                    except StopIteration:
                        raise AssertionError("%s: a retired generator must raise RuntimeError when resumed; it ended" % where)
                    else:
                        raise AssertionError("%s: a retired generator must raise RuntimeError when resumed" % where)
                elif op.fate == "close":
                    g.close()
                del g
                gc.collect()
                self.check(where + " [kept generator: %s]" % op.fate)

    def stepped(self, pos, lnp, where):
        wp, wl = self.m.step()
        where = "%s step %d" % (where, self.m._s["done"])
        _same(pos, wp, "the yielded positions", where)
        _same(lnp, wl, "the yielded log-probabilities", where)
        self.last = (np.array(pos), np.array(lnp), self.m.shown)
        self.check(where)


# ---------------------------------------------------------------------------------------------------- the stand-in
def toy_trajectory(lead, T, seed):
    """(p0, lnp0, chain, lnp, acc_true) of a made-up sampler: a walker moves at a step with probability 0.4."""
    rng = np.random.RandomState(seed)
    lead = tuple(lead)
    p0 = rng.normal(size=lead + (5,))
    moved = rng.rand(*(lead + (T,))) < 0.4
    chain = np.empty(lead + (T, 5))
    cur = p0.copy()
    for t in range(T):
        cur = np.where(moved[..., t, None], cur + rng.normal(size=lead + (5,)), cur)
        chain[..., t, :] = cur
    lnp = -0.5 * (chain ** 2).sum(axis=-1)
    return p0, -0.5 * (p0 ** 2).sum(axis=-1), chain, lnp, np.cumsum(moved, axis=-1).astype(np.float64)


class StandIn(object):
    """The written contract as a sampler over a given trajectory, in numpy: what DeviceEnsembleSampler promises, with
    the device replaced by a counter.  ``retire=False`` is the sampler before the contract's fourth clause: a later call
    does not retire a suspended generator, whose end then overwrites what the call did."""

    def __init__(self, traj, retire=True):
        self.p0, self.lnp0, self.tc, self.tl, acc = traj
        self.moved = np.diff(np.concatenate((np.zeros(acc.shape[:-1] + (1,)), acc), axis=-1), axis=-1)
        self.lead = self.p0.shape[:-1]
        self.life, self.retire, self._open, self._state = 0, retire, None, False
        self.reset()

    def reset(self):
        self._retire()
        self.naccepted = np.zeros(self.lead)
        self.iterations = 0
        self._chain = np.empty(self.lead + (0, 5))
        self._lnprob = np.empty(self.lead + (0,))
        self._state = False

    chain = property(lambda self: self._chain)
    lnprobability = property(lambda self: self._lnprob)
    acceptance_fraction = property(lambda self: self.naccepted / max(self.iterations, 1))

    @property
    def flatchain(self):
        s = self._chain.shape
        return self._chain.reshape(s[:-3] + (s[-3] * s[-2], 5))

    def _at(self, n):
        return (self.p0, self.lnp0) if n == 0 else (self.tc[..., n - 1, :], self.tl[..., n - 1])

    def _advance(self, pos0, k, lnprob0):
        if pos0 is None:
            if not self._state:
                raise ValueError("Cannot have pos0=None if run_mcmc has never been called.")
        else:
            pos0 = np.asarray(pos0, dtype=np.float64)
            if pos0.shape != self.lead + (5,):
                raise ValueError("p0 must have shape {}".format(self.lead + (5,)))
            if lnprob0 is not None and np.shape(lnprob0) != self.lead:
                raise ValueError("lnprob0 must have shape {}".format(self.lead))
            # (the stand-in cannot leave its trajectory: a program that sets another state is a wrong program)
            assert np.array_equal(pos0, self._at(self.life)[0]), "a state that is not the trajectory's"
            assert lnprob0 is None or np.array_equal(lnprob0, self._at(self.life)[1])
            self._state = True
        lo, self.life = self.life, self.life + k
        return self.tc[..., lo:lo + k, :], self.tl[..., lo:lo + k], self.moved[..., lo:lo + k]

    def _retire(self):
        st, self._open = getattr(self, "_open", None), None
        if st is not None and st["live"] and self.retire:
            st["live"] = False
            st["leave"]()

    def run_mcmc(self, pos0, N, rstate0=None, lnprob0=None, storechain=True):
        self._retire()
        steps, lnps, moved = self._advance(pos0, int(N), lnprob0)
        self.iterations += int(N)
        self.naccepted = self.naccepted + moved.sum(axis=-1)
        if storechain:
            self._chain = np.concatenate((self._chain, steps), axis=-2)
            self._lnprob = np.concatenate((self._lnprob, lnps), axis=-1)
        pos, lnp = self._at(self.life)
        return pos.copy(), lnp.copy(), None

    def sample(self, p0, lnprob0=None, rstate0=None, iterations=1, storechain=True, chunk=64):
        self._retire()
        return self._sample(p0, lnprob0, int(iterations), storechain, max(1, int(chunk)))

    def _sample(self, p0, lnprob0, iterations, storechain, chunk):
        self._retire()
        c0, l0, it0, acc0 = self._chain, self._lnprob, self.iterations, self.naccepted
        got_c, got_l, acc = [c0], [l0], [acc0]        # the chunks the device has made; the counts after each of its steps
        st = {"live": True}

        def show(n):
            self.iterations, self.naccepted = it0 + n, acc[n]
            if storechain:
                self._chain = np.concatenate(got_c, axis=-2)[..., :c0.shape[-2] + n, :]
                self._lnprob = np.concatenate(got_l, axis=-1)[..., :l0.shape[-1] + n]
            else:
                self._chain, self._lnprob = c0, l0
        st["leave"] = lambda: show(len(acc) - 1)
        self._open = st
        done, pos0 = 0, p0
        try:
            while True:
                k = min(chunk, iterations - done)
                steps, lnps, moved = self._advance(pos0, k, lnprob0)
                pos0 = lnprob0 = None
                got_c.append(steps)
                got_l.append(lnps)
                for j in range(k):
                    acc.append(acc[-1] + moved[..., j])
                for j in range(k):
                    done += 1
                    show(done)
                    yield steps[..., j, :], lnps[..., j], None
                    if self.retire and not st["live"]:
                        raise RuntimeError("retired")
                if done >= iterations:
                    break
        finally:
            if st["live"] or not self.retire:
                st["live"] = False
                st["leave"]()
                if self._open is st:
                    self._open = None


# ------------------------------------------------------------------------------- the real Python layer without a GPU
class FakeDevice(object):
    """What DeviceEnsembleSampler needs of a likelihood and its native library, with the device replaced by a given
    trajectory: the sampler's own Python -- run_mcmc, sample, reset -- then runs on the CPU, call for call as on the GPU.
    ``rank`` / ``nranks``: a rank of a run sharded with the one-hop exchange, whose chain and counts hold its own rows only
    (zeros elsewhere), as mbb_sampler_run leaves them there."""

    def __init__(self, traj, rank=0, nranks=1):
        self.p0, self.lnp0, self.tc, self.tl, acc = traj
        self.moved = np.diff(np.concatenate((np.zeros(acc.shape[:-1] + (1,)), acc), axis=-1), axis=-1)
        self.lead = self.p0.shape[:-1]
        self.nsources = self.lead[0] if len(self.lead) == 2 else 1
        self.rows = int(np.prod(self.lead))
        self.life, self.nacc, self.calls = 0, np.zeros(self.lead), []
        self.h, self.lib, self.rank, self.nranks = 1, self, rank, nranks
        self.own = np.ones(self.lead[-1], dtype=bool)
        if nranks > 1:
            self.xchg_barrier = lambda: None
            half, per = self.lead[-1] // 2, self.lead[-1] // 2 // nranks
            self.own[:] = False
            self.own[rank * per:(rank + 1) * per] = self.own[half + rank * per:half + (rank + 1) * per] = True

    # ---- the likelihood's part
    def _sync_device(self):
        return self

    # ---- the context's part
    def info(self, name):
        return {"nranks": self.nranks, "rank": self.rank}.get(name, 0)

    def sync(self):
        pass

    # ---- the library's part
    def mbb_last_error(self):
        return b"fake"

    def mbb_sampler_create(self, *a):
        self.calls.append("create")
        return 0

    def mbb_sampler_destroy(self, *a):
        return 0

    def mbb_sampler_reset(self, *a):
        self.calls.append("reset")
        self.nacc = np.zeros(self.lead)
        return 0

    def _at(self, n):
        return (self.p0, self.lnp0) if n == 0 else (self.tc[..., n - 1, :], self.tl[..., n - 1])

    def mbb_sampler_set_state(self, ch, h, pos, lnp):
        self.calls.append("set_state")
        got = np.ctypeslib.as_array(pos, shape=(self.rows * 5,)).reshape(self.lead + (5,))
        assert np.array_equal(got, self._at(self.life)[0]), "a state that is not the trajectory's"
        if lnp:
            assert np.array_equal(np.ctypeslib.as_array(lnp, shape=(self.rows,)).reshape(self.lead), self._at(self.life)[1])
        return 0

    def mbb_sampler_run(self, ch, h, n, a, chain, lnp, pos, lnprob, nacc):
        self.calls.append("run")
        lo, self.life = self.life, self.life + n
        self.nacc = self.nacc + self.moved[..., lo:lo + n].sum(axis=-1)
        if chain and n:
            np.ctypeslib.as_array(chain, shape=(self.rows * n * 5,)).reshape(self.lead + (n, 5))[..., self.own, :, :] = \
                self.tc[..., self.own, lo:lo + n, :]
            np.ctypeslib.as_array(lnp, shape=(self.rows * n,)).reshape(self.lead + (n,))[..., self.own, :] = \
                self.tl[..., self.own, lo:lo + n]
        p, l = self._at(self.life)
        np.ctypeslib.as_array(pos, shape=(self.rows * 5,))[:] = p.reshape(-1)
        np.ctypeslib.as_array(lnprob, shape=(self.rows,))[:] = l.reshape(-1)
        np.ctypeslib.as_array(nacc, shape=(self.rows,)).reshape(self.lead)[..., self.own] = self.nacc[..., self.own]
        return 0
