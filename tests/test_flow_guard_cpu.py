"""The sharded lag guard of sampler forms 7 and 9 (mbb_flow_index.h: fm_shard, fm_shard_wgs, fm_done_word; flowm_words and
spec_words), through the hook mbbh_flowm_guard of mbb_host_tables.cpp.  No GPU.

The index arithmetic: for every grid the shards' counts add up to the grid, every workgroup arrives on a shard that exists,
every counter has a 128-byte line of its own inside the run's state and behind its decision words, and the state fits
the allocation.  Then the guard itself, as a model of who arrives where and who asks what: workgroups pass through the
half-steps in order, an arrival lands in its shard's running total (one per half-step mod the ring, as in the kernel) at
a random later time, and a workgroup enters half-step j only when every non-empty shard has reached its count for j - lag.
What the guard promises -- and what test_host_cpu.py::test_flowm_protocol_model shows to be enough for no slot to be reused
under a reader -- is that nobody enters j before everybody is through with j - lag.  With the last non-empty shard left
out of the predicate an adversary that stalls a workgroup of that shard breaks the promise.

Why this is a model of the guard alone and not tests/_flowm_model.py run with the sharded predicate: that model keeps its
completion counter in a dictionary local to run() and compares it to 2 n there (`done.get(j - LAG, 0) < 2 * n2`); neither
the store nor the predicate can be reached from outside without editing the file, which is another test's yardstick.  So
the two halves are held separately: _flowm_model (test_host_cpu.py::test_flowm_protocol_model) shows that "nobody enters j
before everybody is through with j - lag" keeps every slot from being reused under a reader, and the model here shows
that the sharded counters, asked shard by shard with the kernel's own arithmetic, keep exactly that promise."""
import ctypes as C
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "libmbb_hosttables.so"])
    lib = C.CDLL(os.path.join(ROOT, "oracle", "libmbb_hosttables.so"))
    lib.mbbh_flowm_guard.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_longlong)] * 4
    lib.mbbh_flowm_consts.argtypes = [C.POINTER(C.c_int)] * 5
    return lib


def _guard(lib, grid=2, wg=0, set_=0, slot=0, shard=0, nw=2):
    i = [C.c_int() for _ in range(3)]
    q = [C.c_longlong() for _ in range(4)]
    assert lib.mbbh_flowm_guard(grid, wg, set_, slot, shard, nw, *[C.byref(x) for x in i + q]) == 0
    keys = ("shards", "wg_shard", "shard_wgs", "word", "mseq_end", "words", "alloc_words")
    return dict(zip(keys, [x.value for x in i + q]))


def _consts(lib):
    v = [C.c_int() for _ in range(5)]
    lib.mbbh_flowm_consts(*[C.byref(x) for x in v])
    return [x.value for x in v]          # slots, lag, ring, C waves, LDS records


def test_shards_partition_every_grid(lib):
    S = _guard(lib)["shards"]
    assert S >= 1 and S & (S - 1) == 0
    for grid in range(2, 513):
        counts = [_guard(lib, grid=grid, shard=s)["shard_wgs"] for s in range(S)]
        assert sum(counts) == grid and min(counts) >= 0, (grid, counts)
        mine = [0] * S
        for wg in range(grid):
            s = _guard(lib, grid=grid, wg=wg)["wg_shard"]
            assert 0 <= s < S
            mine[s] += 1
        assert mine == counts, (grid, mine, counts)                 # (what a shard is asked for is what arrives on it)
        assert all(c == 0 for c in counts[grid:])                   # (an empty shard needs 0: it is never asked)
    # the ensembles of tests/test_flowm_guard_gpu.py: uneven shards (18 workgroups), one each (4), empty shards (2)
    assert S == 4
    assert [_guard(lib, grid=18, shard=s)["shard_wgs"] for s in range(S)] == [5, 5, 4, 4]
    assert [_guard(lib, grid=4, shard=s)["shard_wgs"] for s in range(S)] == [1, 1, 1, 1]
    assert [_guard(lib, grid=2, shard=s)["shard_wgs"] for s in range(S)] == [1, 1, 0, 0]


def test_every_counter_has_a_line_of_its_own_inside_the_state(lib):
    S = _guard(lib)["shards"]
    ring = _consts(lib)[2]
    for nw in list(range(2, 513)) + [4095, 4096]:                  # (a grid of nw workgroups: the state of nw rows)
        g = _guard(lib, nw=nw)
        first = _guard(lib, nw=nw)["word"]
        assert first % 32 == 0 and 0 <= first - g["mseq_end"] < 32    # (a 256-byte boundary, right behind the decision words)
        lines = set()
        for set_ in (0, 1):
            for slot in range(ring):
                for s in range(S):
                    w = _guard(lib, set_=set_, slot=slot, shard=s, nw=nw)["word"]
                    assert w % 16 == 0                                # 8-byte words: a 128-byte boundary
                    assert g["mseq_end"] <= w and w + 16 <= g["words"], (nw, set_, slot, s, w)
                    lines.add(w // 16)
        assert len(lines) == 2 * ring * S


def test_the_state_fits_its_allocation(lib):
    for nw in range(2, 4097):
        g = _guard(lib, nw=nw)
        assert g["mseq_end"] < g["words"] <= g["alloc_words"], nw


class Broken(Exception):
    pass


def _run_guard(lib, grid, nhalf, rng, skip_shard=None, stall=None):
    """Workgroups enter half-steps 0 .. nhalf - 1 in order; returns whether all of them got through.  stall = (workgroup, half-step,
    events): that workgroup does not enter that half-step before so many events.  skip_shard: left out of the predicate."""
    S = _guard(lib)["shards"]
    _, lag, ring, _, _ = _consts(lib)
    need = [_guard(lib, grid=grid, shard=s)["shard_wgs"] for s in range(S)]
    shard = [_guard(lib, grid=grid, wg=g)["wg_shard"] for g in range(grid)]
    total = [[0] * S for _ in range(ring)]           # running totals, per half-step mod the ring
    pending = []                                     # arrivals on their way: (ring slot, shard)
    at = [0] * grid                                  # the half-step a workgroup enters next (it is through with all before)
    events = 0

    def guard_open(j):
        if j < lag:
            return True
        rounds = (j - lag) // ring + 1
        return all(total[(j - lag) % ring][s] >= need[s] * rounds for s in range(S) if need[s] > 0 and s != skip_shard)

    def may_enter(g, seen):
        j = at[g]
        if j >= nhalf or (stall and stall[0] == g and stall[1] == j and events < stall[2]):
            return False
        if j not in seen:
            seen[j] = guard_open(j)
        return seen[j]

    while True:
        seen = {}
        ready = [g for g in range(grid) if may_enter(g, seen)]
        if not ready and not pending:
            if stall and events < stall[2]:
                events = stall[2]
                continue
            break
        events += 1
        if pending and (not ready or rng.random() < 0.5):
            slot, s = pending.pop(rng.randrange(len(pending)))
            total[slot][s] += 1
            continue
        g = rng.choice(ready)
        j = at[g]
        if j >= lag and min(at) <= j - lag:          # somebody is not through with j - lag: its slots are still being read
            raise Broken("workgroup %d enters half-step %d while workgroup %d is at %d" % (g, j, at.index(min(at)), min(at)))
        pending.append((j % ring, shard[g]))         # (through with j: the arrival, on its way)
        at[g] = j + 1
    return all(a == nhalf for a in at)


@pytest.mark.parametrize("grid", (2, 4, 18, 34, 68, 250))
def test_sharded_guard_holds_under_random_and_adversarial_schedules(lib, grid):
    nhalf = 40 if grid > 100 else 80                 # ten rounds of the ring (five for the largest grid: the model's time)
    for seed in range(3):
        assert _run_guard(lib, grid, nhalf, random.Random(seed))
    # adversary: one workgroup sleeps at half-step 5 while everything else runs as far as it may
    for g in (0, grid - 1):
        assert _run_guard(lib, grid, nhalf, random.Random(7), stall=(g, 5, 10 ** 6))


def test_a_shard_left_out_of_the_predicate_breaks_the_guard(lib):
    """Sensitivity: the reader ignores the last non-empty shard; a sleeper on that shard is run over."""
    S = _guard(lib)["shards"]
    for grid in (4, 18, 250):
        last = min(grid, S) - 1
        sleeper = next(g for g in range(grid) if _guard(lib, grid=grid, wg=g)["wg_shard"] == last)
        assert _run_guard(lib, grid, 40, random.Random(7), stall=(sleeper, 5, 10 ** 6))
        if S == 1:
            continue                                 # (one shard: nothing to leave out)
        with pytest.raises(Broken):
            _run_guard(lib, grid, 40, random.Random(7), skip_shard=last, stall=(sleeper, 5, 10 ** 6))
