// mbb_options.h -- a context's tunables (mbb_set_option): their fields, and the one table of their names, defaults and bounds.
//
// Plain C++, nothing of the HIP runtime: mbb_hip.hip holds one Options in its context and sets it through set_option();
// tests/options_main.cpp holds the table to its own rules and prints it, and tests/test_host_cpu.py holds the table of
// include/mbb_hip.h to what was printed.  A name, a default or a bound is written here and nowhere else in code.
#ifndef MBB_OPTIONS_H
#define MBB_OPTIONS_H
#include <limits.h>
#include <string.h>

namespace mbbopt {

constexpr long kAnyLow = LONG_MIN, kAnyHigh = LONG_MAX;   // no bound on that side

// X(field of Options, name, default, lowest, highest, what it is).  A value beyond a bound is set to the bound, never refused.
#define MBB_OPTIONS(X) \
    X(wpb, "walkers_per_group", 0, kAnyLow, kAnyHigh, "walkers per workgroup of a likelihood launch (0: the host's choice; at most 64)") \
    X(threads, "block_threads", 0, kAnyLow, kAnyHigh, "threads per workgroup of a likelihood launch (0: the host's choice)") \
    X(zero_copy, "zero_copy", 1, kAnyLow, kAnyHigh, "host path: kernel reads/writes pinned host memory (26 vs 34 us per call)") \
    X(seg_chunks, "seg_chunks", 4, kAnyLow, kAnyHigh, "chunks of 64 samples a band segment of the unit table has at most (next mbb_set_bands)") \
    X(debug, "debug", 0, kAnyLow, kAnyHigh, "a row's status carries the walker's pad bits too") \
    X(stage, "stage_tables", -1, kAnyLow, kAnyHigh, "-1 auto, 0 never, 1 whenever the tables fit in LDS") \
    X(spin, "spin_wait", 2, kAnyLow, kAnyHigh, "0 block on the stream; 1 poll hipStreamQuery (measured: no gain); " \
                                                "2 watch the result slots in pinned memory (zero-copy batches <= 8192 rows)") \
    X(spin_budget, "spin_budget", 20000000L, 0, kAnyHigh, "polls of the result slots before falling back to the stream") \
    X(pack_tails, "pack_tails", 1, kAnyLow, kAnyHigh, "band leftovers share chunks, one row of 16 lanes each (0: a chunk per leftover)") \
    X(bar_params, "bar_params", 1, kAnyLow, kAnyHigh, "host path: write the parameter rows into device memory through the BAR") \
    X(serve_overlap, "serve_overlap", 1, kAnyLow, kAnyHigh, "the served kernel starts a row's quadrature beside its constructor (0: one after the other)") \
    X(serve, "serve", 1, kAnyLow, kAnyHigh, "0: every boundary call is a launch; 2: a server even beside other contexts (tests)") \
    X(serve_after, "serve_after", 3, 1, kAnyHigh, "boundary calls in a row before a server is started") \
    X(serve_idle_us, "serve_idle_us", 1000, kAnyLow, kAnyHigh, "the server leaves after this long without a request (by the clock all CUs share)") \
    X(serve_budget_us, "serve_budget_us", 400, 1, kAnyHigh, "the host gives a served request this long before it falls back to a launch") \
    X(serve_lease_us, "serve_lease_us", 50000, 0, kAnyHigh, "a server is sent away after this long in one go (0: never): processes this library " \
                                                            "cannot see (other containers, other programs) get the CUs at least that often") \
    X(serve_grid, "serve_grid", 0, 0, 1 << 20, "workgroups of a resident server (0: as many as the calls have rows, in eights)") \
    X(serve_prefetch, "serve_prefetch", 32, 0, 256, "record lines asked for ahead of the host's scan once the first record has turned (0: none)") \
    X(prepass, "prepass", -1, kAnyLow, kAnyHigh, "big batches: the constructors by k_walker_pre, a lane per walker (launch_rows); -1 auto, 0 never, 1 always") \
    X(vranks, "virtual_ranks", 0, kAnyLow, kAnyHigh, "testing: run a sampler as this many shards on one GPU") \
    X(xchg_spin_max, "xchg_spin_max", 4000000, kAnyLow, kAnyHigh, "polls before a launch waiting for a peer of the exchange gives up " \
                                                                   "(back to the default when the exchange is closed)") \
    X(lookahead, "lookahead_sampler", 1, kAnyLow, kAnyHigh, "single-GPU sampler runs prepare the next half-step's proposals ahead of the decisions they depend on") \
    X(flow, "flow_sampler", 1, kAnyLow, kAnyHigh, "1: ... as ONE launch per run, the half-steps handing over row by row (forms 6, 7, 9)") \
    X(flowm, "merged_flow_sampler", 1, kAnyLow, kAnyHigh, "1: ... with the quadrature of both candidates running ahead too (k_flowm, form 7)") \
    X(flowr, "resident_sampler", 1, kAnyLow, kAnyHigh, "1: ensembles beyond one pair of walkers per CU run as ONE resident launch too, several walkers " \
        "per workgroup, the SED constructor a half-step ahead for both outcomes of each partner's pending move (k_flowa, form 9); " \
        "0: off; 2: every eligible ensemble takes it") \
    X(flowr_walkers, "resident_walkers", 0, kAnyLow, kAnyHigh, "walkers per workgroup and half of that form (0: the host's choice, ceil(half / CUs): " \
        "ensembles of 258-512 walkers on 256 CUs); 1, 2 force it (testing)") \
    X(flow_spin_log2, "flow_spin_log2", 0, kAnyLow, kAnyHigh, "one-launch run: log2 of the polls before a wait gives up (0: the kernel's 22)") \
    X(flow_min_steps, "flow_min_steps", 2, kAnyLow, kAnyHigh, "runs shorter than this take the launch train (a one-launch run costs ~14 us beside " \
        "its steps: 16.9 us for one step against 15.7)") \
    X(xflow, "sharded_flow_sampler", 1, kAnyLow, kAnyHigh, "... one launch per run also for a sharded ensemble with the one-hop exchange (SMODE 6)") \
    X(roof_wgs, "roof_wgs_per_cu", 0, kAnyLow, kAnyHigh, "measurement: geometry of mbb_roof_probe, workgroups per CU (0: 2)") \
    X(roof_threads, "roof_threads", 0, kAnyLow, kAnyHigh, "... and threads per workgroup (0: 512)") \
    X(pw_budget_mb, "pointwise_budget_mb", 16384, 0, kAnyHigh, "out-of-sample fit: its two columns per band of a group may take this much; at least one band a group")

struct Options {
#define MBB_OPTION_FIELD(field, name, def, low, high, what) long field = def;
    MBB_OPTIONS(MBB_OPTION_FIELD)
#undef MBB_OPTION_FIELD
};

struct OptionRow {
    const char *name;
    long Options::*field;
    long def, low, high;
    const char *what;
};
constexpr OptionRow kOptions[] = {
#define MBB_OPTION_ROW(field, name, def, low, high, what) {name, &Options::field, def, low, high, what},
    MBB_OPTIONS(MBB_OPTION_ROW)
#undef MBB_OPTION_ROW
};

// Sets the option of that name, brought within its bounds, and returns its row; nullptr, and `o` as it was, for a name
// the table does not have.
static inline const OptionRow *set_option(Options &o, const char *name, long value)
{
    for (const OptionRow &r : kOptions)
        if (!strcmp(name, r.name)) {
            o.*r.field = value < r.low ? r.low : (value > r.high ? r.high : value);
            return &r;
        }
    return nullptr;
}

}  // namespace mbbopt
#endif
