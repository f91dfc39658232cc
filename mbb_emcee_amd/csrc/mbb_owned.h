// mbb_owned.h -- the owners of the host library's device and pinned allocations.
//
// Every device or pinned block the library keeps is a member of one of these: it knows its capacity, it is remade
// through one grow(), and it frees itself with whatever it is a member of (a context, a sampler, a local).  Nothing here
// knows the HIP runtime: it is reached through the four functions declared first, which mbb_hip.hip defines with the
// HIP calls (0 or an MBB_ERR_* status, the message left for mbb_last_error) and tests/owned_main.cpp with malloc / free
// and counters.
#ifndef MBB_OWNED_H
#define MBB_OWNED_H
#include <stddef.h>

namespace mbbo {

enum DevKind { kDevPlain, kDevFine };          // hipMalloc; fine-grained: the host or a peer writes it while kernels run
enum PinKind { kPinDefault, kPinMapped };      // pinned; mapped and coherent: a kernel writes it while the host watches

int dev_alloc(void **p, size_t bytes, DevKind kind);
int dev_free(void *p);
int pin_alloc(void **p, void **alias, size_t bytes, PinKind kind);   // alias: the block as the device addresses it (kPinMapped)
int pin_free(void *p);

// Device memory.  Never shrinks; a failed allocation leaves it empty.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;                            // bytes
    DevKind kind = kDevPlain;
    DevBuf() = default;
    explicit DevBuf(DevKind k) : kind(k) {}
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() { if (p) (void)dev_free(p); p = nullptr; cap = 0; }
    // released first, then allocated: never two blocks of one owner at a time
    int remake(size_t bytes)
    {
        release();
        const int rc = dev_alloc(&p, bytes, kind);
        if (rc) p = nullptr; else cap = bytes;
        return rc;
    }
    // idle(): brings to rest whatever may still be using the old block (the context's stream); 0 or a status
    template <typename Idle> int grow(size_t bytes, Idle &&idle)
    {
        if (bytes <= cap) return 0;
        if (const int rc = idle()) return rc;
        return remake(bytes);
    }
};

// Pinned host memory, the same way.
struct PinBuf {
    void *p = nullptr, *alias = nullptr;
    size_t cap = 0;                            // bytes
    PinKind kind = kPinMapped;
    PinBuf() = default;
    explicit PinBuf(PinKind k) : kind(k) {}
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    ~PinBuf() { release(); }
    void release() { if (p) (void)pin_free(p); p = alias = nullptr; cap = 0; }
    int remake(size_t bytes)
    {
        release();
        const int rc = pin_alloc(&p, &alias, bytes, kind);
        if (rc) p = alias = nullptr; else cap = bytes;
        return rc;
    }
    template <typename Idle> int grow(size_t bytes, Idle &&idle)
    {
        if (bytes <= cap) return 0;
        if (const int rc = idle()) return rc;
        return remake(bytes);
    }
};

// ... as arrays of T (sizes stay in bytes)
template <typename T> struct Dev : DevBuf {
    using DevBuf::DevBuf;
    T *d() const { return static_cast<T *>(p); }
};
template <typename T> struct Pin : PinBuf {
    using PinBuf::PinBuf;
    T *h() const { return static_cast<T *>(p); }
    T *dv() const { return static_cast<T *>(alias); }
};

// The memory of a device-resident sampler (mbb_sampler_state, mbb_hip.hip)
struct SamplerMem {
    double *d_pos6 = nullptr;            // the state rows: pos6_own's, or the context's exchange buffer's
    Dev<double> pos6_own;                // ... empty when the rows live in the exchange buffer
    Dev<unsigned int> d_nacc;            // [shards][2][nsrc*per], launch-local order
    Dev<int> d_err;
    Dev<double> d_bak;                   // one-launch run: the rows and counts it started from (R x 6 doubles, R counts)
    Dev<double> d_spec;                  // one-launch run: its device state (FlowView or FlowMView, spec_words(rows))
    Dev<double> d_chain6;                // [shards][nsteps][2][nsrc*per][6]
    Dev<double> d_chain_out;             // the same chain in the caller's layout: [rows][nsteps][5] then [rows][nsteps]
    Pin<double> h_chain{kPinDefault};    // ... and its pinned landing place on the host (a D2H into the caller's pageable,
                                         // often untouched, arrays ran at ~1 GB/s: 18.8 us per step for 2000 stored steps)
};

}  // namespace mbbo
#endif
