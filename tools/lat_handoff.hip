// One-way latency of a flag hand-off between two waves on different CUs: wave A stores k to its
// word (write-through, agent scope), wave B polls A's word until it reads k and stores k to its
// own word, A polls that ...  Time of N round trips / 2N.  Pairs on different XCDs (workgroups
// 2j, 2j+1) or on the same XCD (b, b+8); polling one load at a time (with or without s_sleep) or
// with several loads in flight; alone on the chip or with `noise` other pairs doing the same.
//   hipcc --offload-arch=gfx950 -O3 -o tools/lat_handoff tools/lat_handoff.hip && tools/lat_handoff
// `tools/lat_handoff load` (profiles/r13/lat_handoff_load.txt): 16 pairs on different XCDs, one workgroup per CU on the
// whole chip, and beside the hand-off, one at a time, what k_flowm puts beside its own: (i) every other CU adding to one
// counter, ~100 adds per us chip-wide, or to 2, 4, 8 counters on lines of their own, 4 KB apart, or inside one line;
// (ii) the producer's store behind a non-returning atomic and ahead of six 16-byte sc1 stores of the same wave; (iii) two
// more waves on the consumer's CU polling 37 lanes' 16-byte pairs, a line each; (iv) the consumer at s_setprio 1 beside
// two waves of dependent fp64 work on its SIMD.  One-way time per trip: median, p10, p90 over all trips of all pairs.
// Every poll is bounded; whatever runs beside the pairs ends on a word in LDS, an iteration count or the clock.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <vector>
#include <string>
#include <algorithm>

__device__ __forceinline__ unsigned long long ldw(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int POLL>   // 0: load, check, s_sleep 1;  1: load, check;  2: four loads in flight, ~a quarter round trip apart
__device__ __forceinline__ bool wait_for(const unsigned long long *w, unsigned long long k)
{
    if (POLL == 2) {
        unsigned long long v0 = ldw(w);
        __builtin_amdgcn_s_sleep(2);
        unsigned long long v1 = ldw(w);
        __builtin_amdgcn_s_sleep(2);
        unsigned long long v2 = ldw(w);
        __builtin_amdgcn_s_sleep(2);
        unsigned long long v3 = ldw(w);
        for (int i = 0; i < (1 << 20); ++i) {
            if (v0 >= k) return true;
            v0 = ldw(w);
            if (v1 >= k) return true;
            v1 = ldw(w);
            if (v2 >= k) return true;
            v2 = ldw(w);
            if (v3 >= k) return true;
            v3 = ldw(w);
        }
        return false;
    }
    for (int i = 0; i < (1 << 22); ++i) {
        if (ldw(w) >= k) return true;
        if (POLL == 0) __builtin_amdgcn_s_sleep(1);
    }
    return false;
}

template <int POLL>
__global__ void k_ping(unsigned long long *words, int n, int same_xcd, unsigned long long *ticks, int *err)
{
    const int b = blockIdx.x;
    int pair, side;
    if (same_xcd) { pair = (b / 16) * 8 + (b % 8); side = (b / 8) & 1; }
    else { pair = b >> 1; side = b & 1; }
    unsigned long long *mine = words + (size_t)(2 * pair + side) * 16, *other = words + (size_t)(2 * pair + (side ^ 1)) * 16;
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 1; i <= n; ++i) {
        if (side == 0) {
            __hip_atomic_store(mine, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!wait_for<POLL>(other, (unsigned long long)i)) { atomicMax(err, 1); break; }
        } else {
            if (!wait_for<POLL>(other, (unsigned long long)i)) { atomicMax(err, 1); break; }
            __hip_atomic_store(mine, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (side == 0) ticks[pair] = __builtin_amdgcn_s_memrealtime() - t0;      // 100 MHz
}


// ---- the hand-off with company (`load`)
struct LoadCfg {
    int pairs;          // blocks 0 .. 2 pairs - 1 play; the others add (if nctr > 0) or idle
    int n;              // round trips
    int nctr;           // (i) counters the other CUs add to (0: none) ...
    int ctr_stride;     //     ... this many words apart
    int add_ticks;      //     an adder's period, 100 MHz ticks
    int burst;          //     every adder at the same tick of the clock they share (k_flowm: once per half-step), not spread
    int run_ticks;      //     how long the adders go on
    int extra_stores;   // (ii) a non-returning atomic ahead of the store, six 16-byte stores behind it
    int pollers;        // (iii) waves 1, 2 of a playing workgroup poll 37 lines each
    int fp64;           // (iv) waves 4, 8 (wave 0's SIMD) run dependent fp64 work, wave 0 at s_setprio 1
};
constexpr int kLoadThreads = 768;            // 12 waves: 0, 4, 8 share a SIMD
constexpr int kCtrWords = 8 * 512 + 16;      // eight counters up to 4 KB apart
constexpr int kSideWords = 16 * 16;          // per workgroup: lines its extra stores and atomics go to
constexpr int kPollWords = 2 * 37 * 16;      // per workgroup: the lines its two polling waves ask for

__global__ void __launch_bounds__(kLoadThreads)
k_load(unsigned long long *words, unsigned long long *ctr, unsigned long long *side, unsigned long long *pollbuf,
       unsigned short *trip, double *sink, int *err, LoadCfg c)
{
    extern __shared__ int lds[];             // (sized so that a CU holds one workgroup)
    const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) lds[0] = 0;
    __syncthreads();
    if (b >= 2 * c.pairs) {                  // (i)
        if (threadIdx.x != 0 || c.nctr == 0) return;
        unsigned long long *w = ctr + (size_t)(b & (c.nctr - 1)) * c.ctr_stride;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        unsigned long long next = c.burst ? (t0 / c.add_ticks + 1) * c.add_ticks : t0 + (unsigned long long)(b % c.add_ticks);
        for (int i = 0; i < (1 << 22); ++i) {
            const unsigned long long t = __builtin_amdgcn_s_memrealtime();
            if (t - t0 > (unsigned long long)c.run_ticks) break;
            if (t >= next) {
                __hip_atomic_fetch_add(w, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                next += (unsigned long long)c.add_ticks;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        return;
    }
    const int pair = b >> 1, sd = b & 1;
    unsigned long long *mine = words + (size_t)(2 * pair + sd) * 16, *other = words + (size_t)(2 * pair + (sd ^ 1)) * 16;
    if (wave == 0) {
        if (lane != 0) return;
        if (c.fp64) __builtin_amdgcn_s_setprio(1);
        unsigned long long *sl = side + (size_t)b * kSideWords;
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        auto post = [&](unsigned long long i) {
            if (c.extra_stores) __hip_atomic_fetch_add(sl + 15 * 16, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(mine, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (c.extra_stores)
                for (int k = 0; k < 6; ++k) {
                    const u32x4 d = {(unsigned int)i, (unsigned int)k, 0u, 0u};
                    asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(sl + k * 2), "v"(d) : "memory");
                }
        };
        unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (int i = 1; i <= c.n; ++i) {
            if (sd == 0) {
                post((unsigned long long)i);
                if (!wait_for<0>(other, (unsigned long long)i)) { atomicMax(err, 1); break; }
                const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
                trip[(size_t)pair * c.n + (i - 1)] = (unsigned short)(t1 - t0 > 65535ull ? 65535ull : t1 - t0);
                t0 = t1;
            } else {
                if (!wait_for<0>(other, (unsigned long long)i)) { atomicMax(err, 1); break; }
                post((unsigned long long)i);
            }
        }
        __hip_atomic_store(lds, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    if (c.pollers && (wave == 1 || wave == 2)) {             // (iii)
        const unsigned long long *p = pollbuf + ((size_t)b * 2 + (wave - 1)) * 37 * 16 + (size_t)(lane < 37 ? lane : 0) * 16;
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        unsigned int seen = 0;
        for (int i = 0; i < (1 << 22); ++i) {
            if (__hip_atomic_load(lds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
            if (lane < 37) {
                u32x4 d;
                asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(d) : "v"(p) : "memory");
                seen += d.x;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        if (seen == 0xffffffffu) sink[0] = 1.0;             // (never: the lines stay zero)
        return;
    }
    if (c.fp64 && (wave == 4 || wave == 8)) {                // (iv)
        double x = 1.0 + lane * 1e-9;
        for (int i = 0; i < (1 << 22); ++i) {
            if (__hip_atomic_load(lds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
#pragma unroll
            for (int k = 0; k < 32; ++k) x = fma(x, 0.999999, 1e-7);
        }
        if (x == 12345.0) sink[1] = x;
        return;
    }
}

static int run_load()
{
    const int grid = 256, pairs = 16, n = 1500;
    unsigned long long *words, *ctr, *side, *pollbuf;
    unsigned short *trip;
    double *sink;
    int *err;
    hipMalloc(&words, pairs * 2 * 16 * 8);
    hipMalloc(&ctr, kCtrWords * 8);
    hipMalloc(&side, (size_t)grid * kSideWords * 8);
    hipMalloc(&pollbuf, (size_t)grid * kPollWords * 8);
    hipMalloc(&trip, (size_t)pairs * n * 2);
    hipMalloc(&sink, 16);
    hipMalloc(&err, 4);
    const int lds_bytes = 96 * 1024;
    if (hipFuncSetAttribute((const void *)k_load, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes) != hipSuccess) {
        printf("cannot ask for %d bytes of LDS\n", lds_bytes);
        return 1;
    }
    struct Case { const char *name; LoadCfg c; };
    const int A = grid - 2 * pairs;          // adders: one add per `A` ticks each is one per tick, 100 per us, chip-wide
    const int run = 1500000;                 // 15 ms
    auto cfg = [&](int nctr, int stride, int period, int xs, int po, int f, int burst = 0) {
        LoadCfg c = {pairs, n, nctr, stride, period, burst, run, xs, po, f};
        return c;
    };
    const int H = 246;                       // a half-step of the bench workload, in ticks
    const Case cases[] = {
        {"alone (the other CUs idle)                    ", cfg(0, 16, A, 0, 0, 0)},
        {"(i) 100 adds/us on 1 counter                  ", cfg(1, 16, A, 0, 0, 0)},
        {"(i) 100 adds/us on 2 counters, a line each    ", cfg(2, 16, A, 0, 0, 0)},
        {"(i) 100 adds/us on 4 counters, a line each    ", cfg(4, 16, A, 0, 0, 0)},
        {"(i) 100 adds/us on 8 counters, a line each    ", cfg(8, 16, A, 0, 0, 0)},
        {"(i) 100 adds/us on 8 counters, 4 KB apart     ", cfg(8, 512, A, 0, 0, 0)},
        {"(i) 100 adds/us on 8 counters inside one line ", cfg(8, 2, A, 0, 0, 0)},
        {"(i) 200 adds/us on 1 counter                  ", cfg(1, 16, A / 2, 0, 0, 0)},
        {"(i) 200 adds/us on 8 counters, a line each    ", cfg(8, 16, A / 2, 0, 0, 0)},
        {"(i) 224 adds at once per 2.46 us, 1 counter   ", cfg(1, 16, H, 0, 0, 0, 1)},
        {"(i) 224 adds at once per 2.46 us, 2 counters  ", cfg(2, 16, H, 0, 0, 0, 1)},
        {"(i) 224 adds at once per 2.46 us, 4 counters  ", cfg(4, 16, H, 0, 0, 0, 1)},
        {"(i) 224 adds at once per 2.46 us, 8 counters  ", cfg(8, 16, H, 0, 0, 0, 1)},
        {"(ii) atomic + store + six 16-byte sc1 stores  ", cfg(0, 16, A, 1, 0, 0)},
        {"(iii) two waves polling 37 lines each         ", cfg(0, 16, A, 0, 1, 0)},
        {"(iv) prio 1 beside two fp64 waves on the SIMD ", cfg(0, 16, A, 0, 0, 1)},
        {"(i) 1 counter + (ii) + (iii) + (iv)           ", cfg(1, 16, A, 1, 1, 1)},
        {"(i) 8 counters + (ii) + (iii) + (iv)          ", cfg(8, 16, A, 1, 1, 1)},
        {"alone, again                                  ", cfg(0, 16, A, 0, 0, 0)},
    };
    printf("16 pairs on different XCDs, %d workgroups (one per CU), %d round trips each; one-way = round trip / 2\n", grid, n);
    for (const Case &cs : cases) {
        hipMemset(words, 0, pairs * 2 * 16 * 8);
        hipMemset(ctr, 0, kCtrWords * 8);
        hipMemset(side, 0, (size_t)grid * kSideWords * 8);
        hipMemset(pollbuf, 0, (size_t)grid * kPollWords * 8);
        hipMemset(trip, 0, (size_t)pairs * n * 2);
        hipMemset(err, 0, 4);
        hipLaunchKernelGGL(k_load, dim3(grid), dim3(kLoadThreads), lds_bytes, 0, words, ctr, side, pollbuf, trip, sink, err, cs.c);
        if (hipDeviceSynchronize() != hipSuccess) { printf("the launch failed\n"); return 1; }
        std::vector<unsigned short> h((size_t)pairs * n);
        std::vector<unsigned long long> hc(kCtrWords);
        int e;
        hipMemcpy(h.data(), trip, h.size() * 2, hipMemcpyDeviceToHost);
        hipMemcpy(hc.data(), ctr, hc.size() * 8, hipMemcpyDeviceToHost);
        hipMemcpy(&e, err, 4, hipMemcpyDeviceToHost);
        std::vector<unsigned short> t;
        double total = 0.0, worst_med = 0.0;
        unsigned short longest = 0;
        for (int p = 0; p < pairs; ++p)
            for (int i = 100; i < n; ++i) { t.push_back(h[(size_t)p * n + i]); }      // (the first hundred: the start-up)
        for (int p = 0; p < pairs; ++p) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) s += h[(size_t)p * n + i];
            total = std::max(total, s);
            std::vector<unsigned short> tp(h.begin() + (size_t)p * n + 100, h.begin() + (size_t)(p + 1) * n);
            std::sort(tp.begin(), tp.end());
            worst_med = std::max(worst_med, tp[tp.size() / 2] * 10.0 / 2.0);
            longest = std::max(longest, tp.back());
        }
        std::sort(t.begin(), t.end());
        unsigned long long adds = 0;
        for (unsigned long long v : hc) adds += v;
        auto q = [&](double f) { return t[(size_t)(f * (t.size() - 1))] * 10.0 / 2.0; };
        printf("%s one-way %5.0f ns median, %5.0f p10, %5.0f p90; slowest pair %5.0f median, longest round trip %6.1f us%s, busy %4.1f ms; "
               "%7llu adds in %.0f ms%s\n", cs.name, q(0.5), q(0.1), q(0.9), worst_med, longest / 100.0, longest == 65535 ? "+" : " ",
               total / 1e5, adds, cs.c.nctr ? run / 1e5 : 0.0, e ? "  (TIMED OUT)" : "");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "load") return run_load();
    unsigned long long *words, *ticks;
    int *err;
    const int maxpairs = 128;
    hipMalloc(&words, maxpairs * 2 * 16 * 8);
    hipMalloc(&ticks, maxpairs * 8);
    hipMalloc(&err, 4);
    const int n = 2000;
    for (int same = 0; same < 2; ++same)
        for (int pairs : {1, 8, 64, 120})
            for (int poll = 0; poll < 3; ++poll) {
                if (same && pairs > 64) continue;
                hipMemset(words, 0, maxpairs * 2 * 16 * 8);
                hipMemset(err, 0, 4);
                const int grid = same ? ((pairs + 7) / 8) * 16 : 2 * pairs;
                if (poll == 0) hipLaunchKernelGGL(k_ping<0>, dim3(grid), dim3(64), 0, 0, words, n, same, ticks, err);
                if (poll == 1) hipLaunchKernelGGL(k_ping<1>, dim3(grid), dim3(64), 0, 0, words, n, same, ticks, err);
                if (poll == 2) hipLaunchKernelGGL(k_ping<2>, dim3(grid), dim3(64), 0, 0, words, n, same, ticks, err);
                hipDeviceSynchronize();
                std::vector<unsigned long long> h(maxpairs);
                int e;
                hipMemcpy(h.data(), ticks, pairs * 8, hipMemcpyDeviceToHost);
                hipMemcpy(&e, err, 4, hipMemcpyDeviceToHost);
                std::sort(h.begin(), h.begin() + pairs);
                printf("%s XCD, %3d pairs at once, %s: one-way hand-off %.0f ns median, %.0f ns slowest pair%s\n",
                       same ? "same     " : "different", pairs,
                       poll == 0 ? "load-check-sleep  " : (poll == 1 ? "load-check        " : "four loads in flight"),
                       h[pairs / 2] * 10.0 / (2.0 * n), h[pairs - 1] * 10.0 / (2.0 * n), e ? "  (TIMED OUT)" : "");
            }
    return 0;
}
