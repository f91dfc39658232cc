// mbb_flow_index.h -- index arithmetic of the one-launch sampler runs (k_lnlike SMODE 6, the sharded
// look-ahead run; k_flowm, form 7, and k_flowa, form 9, below), shared by the kernels and by the host-side
// models of their hand-over protocols (tests/test_host_cpu.py::test_flow_protocol_model and the two after it,
// through the hooks in mbb_host_tables.cpp).
//
// Half-steps are numbered j = 0, 1, 2, ... over a launch; half h = j & 1 of the ensemble moves in
// half-step j (h = 0: rows [0, n/2), h = 1: the rest).  Everything a row publishes is filed under
// the number m = 1, 2, ... of the move it belongs to, in slot m mod kFlowSlots; slot 0 also holds
// what the launch found (m = 0).
#pragma once
#include <stddef.h>
#if defined(__HIPCC__)
#define MBB_FLOW_HD __host__ __device__
#else
#define MBB_FLOW_HD
#endif

constexpr int kFlowSlots = 4;      // slots per row
constexpr int kFlowLag = 4;        // a mover of half-step j waits until every move of j - kFlowLag is complete

// moves half h has completed before half-step j
MBB_FLOW_HD constexpr int flow_cnt(int h, int j) { return (j - h + 1) > 0 ? (j - h + 1) >> 1 : 0; }
// what a row's word says once its m-th move is published: the half-step of that move plus one
MBB_FLOW_HD constexpr int flow_seq(int h, int m) { return m > 0 ? h + 2 * m - 1 : 0; }

// ---- sampler form 7 (k_flowm, mbb_flowm.hip.h): the same numbering of half-steps and moves
constexpr int kFmSlots = 4;    // slots per row (moves filed mod this)
constexpr int kFmMseq = kFmSlots;    // decision words per row as laid out, the stride of mseq (a 128-byte line per row, 16,
                                     // is no faster: profiles/r04/done_counters_alignment.txt)
constexpr int kFmLag = 4;      // a workgroup at half-step j waits until every workgroup is through with j - kFmLag
constexpr int kFmRing = 8;     // completion counters, by half-step mod this (a power of two >= 2 kFmLag)
// (8 slots and a lag of 8 were tried: 6.49 against 6.29 us per step -- the lag guard is not what a half-step waits for)
// The lag guard's completion counters are sharded: done[2][kFmRing][kFmShards], a 128-byte line per counter.  A
// workgroup arrives on the shard of its number mod kFmShards (under round-robin placement of workgroups on the eight
// XCDs that is two XCDs' workgroups per shard: a matter of speed only), and a reader asks every shard for the count of
// the workgroups that map to it: the conjunction of the shards' answers is the guard, no sum is formed.  Form 9
// (k_flowa) arrives on shard 0 alone and asks it for the full count.
// (How many: the hand-off measured alone is the idle chip's again from TWO counters on; in the kernel 2, 4, 8 and 16 all
// beat one by 0.5-1.5 % and differ from one another by no more than two builds of the same count do (0.5 %).  Four was
// ahead of two and eight in each of three runs, by that much and no more: a choice within the noise, at the price of two
// more 8-byte requests per accept-test pass than two shards -- profiles/r13/form7.txt.)
constexpr int kFmShards = 4;                 // a power of two (1, 2, 4, 8, 16 measured: profiles/r13/form7.txt)
constexpr int kFmDoneLine = 16;              // words from one counter to the next: 128 bytes
constexpr int kFmDoneWords = 2 * kFmRing * kFmShards * kFmDoneLine;      // both sets
static_assert((kFmShards & (kFmShards - 1)) == 0 && kFmShards >= 1 && kFmShards <= 32, "shards: a power of two, one reader lane each");
// the shard workgroup `wg` arrives on
MBB_FLOW_HD constexpr int fm_shard(int wg) { return wg & (kFmShards - 1); }
// workgroups of a grid that arrive on shard s (0 for an empty shard: it is never asked)
MBB_FLOW_HD constexpr int fm_shard_wgs(int grid, int s) { return grid > s ? (grid - s + kFmShards - 1) / kFmShards : 0; }
// the word of (set, ring slot, shard), counted from the first counter
MBB_FLOW_HD constexpr int fm_done_word(int set, int slot, int s) { return ((set * kFmRing + slot) * kFmShards + s) * kFmDoneLine; }
constexpr int kFmWords = 16;   // words per proposal / per row
// words of a run's state (FlowMView, mbb_kernels.hip.h): proposals, rows, decision words, then the completion counters
MBB_FLOW_HD constexpr size_t flowm_mseq_end(size_t nw) { return nw * ((size_t)kFmSlots * 2 * kFmWords + kFmSlots * kFmWords + kFmMseq); }
MBB_FLOW_HD constexpr size_t flowm_words(size_t nw)
{
    // (the completion counters begin on a 256-byte boundary: 250 atomic adds per half-step on a word that shared its
    // 128-byte line with the last rows' decision words, which their partners poll, cost every second launch of a
    // sampler 2 % -- profiles/r04/done_counters_alignment.txt.  Two sets of kFmRing x kFmShards counters, a 128-byte
    // line each: fm_done_word)
    return ((flowm_mseq_end(nw) + 31) & ~(size_t)31) + kFmDoneWords;
}
// ... and of the allocation it lives in, the one SMODE 6 lays out as FlowView (mbb_kernels.hip.h), with room behind that
// for the sharded counters (a small ensemble's FlowView is shorter than they are)
constexpr int kFlowRecN = 22, kFlowRec = 48;
MBB_FLOW_HD constexpr size_t spec_words(size_t nw)
{
    return nw * ((size_t)kFlowSlots * 2 * kFlowRec + kFlowSlots * 8 + 1 + kFlowSlots) + 8 * 16 + 16 * 8 + 32 + kFmDoneWords;
}
constexpr int kFmNC = 3;       // C waves of a workgroup: wave c takes the half-steps j = c mod kFmNC
constexpr int kFmNB = 4;       // hand-over records in a workgroup's LDS: half-step j uses buffer j mod kFmNB
