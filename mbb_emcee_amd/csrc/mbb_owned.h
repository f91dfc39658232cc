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
#include <string.h>

#include <type_traits>
#include <vector>

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

// The result arrays of an analysis, one behind the other in one device block.  The analysis names each once --
// add(&p, n, dst): n values of T that the kernels reach through p and the caller gets in dst -- and the block's size,
// the device addresses and the way home all follow from that list.  An entry begins at a multiple of alignof(T), so a
// list in falling alignment has no padding.  dst may be null (the array stays on the device), n may be 0 (p is null then,
// nothing is copied), and add(&p, n, dst, first) sends home only the values from the first-th on: the ones before stay
// on the device.  The addresses are handed out by place(), which first grows the device block to the list's size.
class ResultBlock {
    struct Entry {
        void *slot;                              // the T * the kernels are given, written by set
        void (*set)(void *slot, char *p);
        size_t off, bytes, skip;                 // in the block; of which the first skip bytes do not go home
        void *dst;
    };
    std::vector<Entry> e_;
    std::vector<char> image_;
    size_t bytes_ = 0;
public:
    // ... returns where the entry begins in the block
    // (U: the caller's name for T's values where the two differ, int64_t for long long)
    template <typename T, typename U = T> size_t add(T **p, size_t n, U *dst = nullptr, size_t first = 0)
    {
        static_assert(sizeof(U) == sizeof(T) && std::is_integral<U>::value == std::is_integral<T>::value &&
                      std::is_signed<U>::value == std::is_signed<T>::value, "a destination holds what the kernels write");
        bytes_ = (bytes_ + alignof(T) - 1) / alignof(T) * alignof(T);
        e_.push_back(Entry{p, [](void *slot, char *at) { *static_cast<T **>(slot) = reinterpret_cast<T *>(at); }, bytes_,
                           n * sizeof(T), (first < n ? first : n) * sizeof(T), dst});
        bytes_ += n * sizeof(T);
        return e_.back().off;
    }
    size_t bytes() const { return bytes_; }
    template <typename Idle> int place(DevBuf &block, Idle &&idle)
    {
        if (const int rc = block.grow(bytes_, idle)) return rc;
        for (const Entry &e : e_) e.set(e.slot, e.bytes ? static_cast<char *>(block.p) + e.off : nullptr);
        return 0;
    }
    // Home as an image: the caller copies bytes() of the device block to image(), waits, and scatter() fills every dst.
    char *image() { image_.resize(bytes_); return image_.data(); }
    void scatter() const
    {
        (void)each([this](void *dst, size_t off, size_t bytes) { memcpy(dst, image_.data() + off, bytes); return 0; });
    }
    // Home entry by entry: copy(dst, block offset, bytes) for every entry with a dst and a value to send, in the list's
    // order; stops at the first status that is not 0 and returns it.
    template <typename Copy> int each(Copy &&copy) const
    {
        for (const Entry &e : e_)
            if (e.dst && e.bytes > e.skip)
                if (const int rc = copy(e.dst, e.off + e.skip, e.bytes - e.skip)) return rc;
        return 0;
    }
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
