// owned_main.cpp -- the owners of mbb_emcee_amd/csrc/mbb_owned.h over malloc / free, stand-alone.
//
// Built by tests/test_host_cpu.py with AddressSanitizer (leak detection on) and UBSan and run directly.  The four runtime
// functions the header declares are defined here with counters of live blocks and a switch that makes the n-th allocation
// from now fail; what mbb_hip.hip builds on -- grow, a failed allocation, destruction, a struct of owners, a sampler's
// state held by a unique_ptr, the result list of an analysis -- is checked against them.  Exit status 0: all held.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "../mbb_emcee_amd/csrc/mbb_owned.h"

static int g_live_dev = 0, g_live_pin = 0, g_allocs = 0, g_frees = 0, g_fail_in = 0, g_checks = 0;

static bool refused()
{
    return g_fail_in > 0 && --g_fail_in == 0;
}
int mbbo::dev_alloc(void **p, size_t bytes, DevKind)
{
    if (refused()) return -3;             // (left as it was: the owner is to empty itself)
    *p = malloc(bytes);
    ++g_live_dev; ++g_allocs;
    return 0;
}
int mbbo::dev_free(void *p)
{
    free(p);
    --g_live_dev; ++g_frees;
    return 0;
}
int mbbo::pin_alloc(void **p, void **alias, size_t bytes, PinKind kind)
{
    if (refused()) return -3;
    *p = malloc(bytes);
    if (kind == kPinMapped) *alias = *p;
    ++g_live_pin; ++g_allocs;
    return 0;
}
int mbbo::pin_free(void *p)
{
    free(p);
    --g_live_pin; ++g_frees;
    return 0;
}

#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

using namespace mbbo;

// grow(): nothing within capacity; beyond it idle, release, allocate, in that order; the capacity never shrinks
template <typename Buf> static void check_grow(int &live)
{
    int idles = 0, live_at_idle = -1, frees_at_idle = -1;
    auto idle = [&] { ++idles; live_at_idle = live; frees_at_idle = g_frees; return 0; };
    {
        Buf b;
        CHECK(b.p == nullptr && b.cap == 0);
        CHECK(b.grow(100, idle) == 0 && b.p && b.cap == 100 && live == 1 && idles == 1);
        static_cast<char *>(b.p)[99] = 1;
        const int allocs = g_allocs;
        void *const was = b.p;
        CHECK(b.grow(100, idle) == 0 && b.grow(7, idle) == 0 && b.grow(0, idle) == 0);
        CHECK(g_allocs == allocs && idles == 1 && b.p == was && b.cap == 100);      // within capacity: nothing happens
        const int frees = g_frees;
        CHECK(b.grow(1000, idle) == 0 && b.cap == 1000 && live == 1);
        CHECK(idles == 2 && live_at_idle == 1 && frees_at_idle == frees);           // idle() before the release
        CHECK(g_frees == frees + 1 && g_allocs == allocs + 1);                      // ... one release, one allocation
        static_cast<char *>(b.p)[999] = 1;
        CHECK(b.grow(500, idle) == 0 && b.cap == 1000 && g_allocs == allocs + 1);   // never shrinks
        // an idle() that fails leaves the block as it is
        CHECK(b.grow(2000, [] { return -7; }) == -7 && b.cap == 1000 && b.p && live == 1);
        // a failing allocation: the error comes back, the owner is empty, the next grow succeeds
        g_fail_in = 1;
        CHECK(b.grow(4000, idle) == -3 && b.p == nullptr && b.cap == 0 && live == 0);
        CHECK(b.grow(10, idle) == 0 && b.p && b.cap == 10 && live == 1);
        // release() twice is harmless
        const int frees2 = g_frees;
        b.release(); b.release();
        CHECK(g_frees == frees2 + 1 && live == 0 && b.p == nullptr && b.cap == 0);
        CHECK(b.remake(64) == 0 && live == 1);
    }
    CHECK(live == 0);                                                               // the destructor frees, once
}

static void check_pinned_alias()
{
    Pin<double> m;
    Pin<double> plain{kPinDefault};
    CHECK(m.remake(80) == 0 && plain.remake(80) == 0);
    CHECK(m.dv() == m.h() && m.h() != nullptr && plain.h() != nullptr && plain.dv() == nullptr);
    m.h()[9] = 1.0; plain.h()[9] = 1.0;
    m.release();
    CHECK(m.h() == nullptr && m.dv() == nullptr);
}

// A struct of owners whose allocations stop midway frees what it has got
struct Group {
    Dev<double> a, b;
    Pin<int> h;
    Dev<double> w{kDevFine};
    int make(size_t n)
    {
        int rc;
        if ((rc = a.remake(n * sizeof(double))) || (rc = b.remake(n * sizeof(double))) || (rc = h.remake(n * sizeof(int))) ||
            (rc = w.remake(n * sizeof(double))))
            return rc;
        return 0;
    }
};

static void check_group()
{
    for (int nth = 1; nth <= 5; ++nth) {
        {
            Group g;
            g_fail_in = nth;
            const int rc = g.make(16);
            CHECK(rc == (nth <= 4 ? -3 : 0));
            CHECK(g_live_dev + g_live_pin == (nth <= 4 ? nth - 1 : 4));
            if (nth == 3) CHECK(g.a.p && g.b.p && !g.h.p && !g.w.p && g.h.cap == 0);
        }
        CHECK(g_live_dev == 0 && g_live_pin == 0);
        g_fail_in = 0;
    }
}

// The way mbb_sampler_create makes a sampler: held by a unique_ptr until everything is there, the exchange's users counted
// only then
struct State : SamplerMem { int nw = 0; };

static int make_state(size_t rows, bool in_exchange, double *exchange_rows, int &users, State **out)
{
    std::unique_ptr<State> s(new State());
    int rc;
    if (in_exchange) s->d_pos6 = exchange_rows;
    else {
        if ((rc = s->pos6_own.remake(rows * 6 * sizeof(double)))) return rc;
        s->d_pos6 = s->pos6_own.d();
    }
    if ((rc = s->d_nacc.remake(rows * sizeof(unsigned int))) || (rc = s->d_err.remake(sizeof(int)))) return rc;
    if (!s->pos6_own.p) ++users;
    *out = s.release();
    return 0;
}

static void check_sampler_state()
{
    double rows[12] = {};
    for (int in_exchange = 0; in_exchange < 2; ++in_exchange) {
        int users = 0;
        State *s = nullptr;
        g_fail_in = 2;                    // the second allocation
        CHECK(make_state(2, in_exchange != 0, rows, users, &s) == -3);
        CHECK(s == nullptr && users == 0 && g_live_dev == 0 && g_live_pin == 0);
        g_fail_in = 0;
        CHECK(make_state(2, in_exchange != 0, rows, users, &s) == 0 && s && users == in_exchange);
        CHECK(g_live_dev == (in_exchange ? 2 : 3));
        // what a run adds: the chain store, exact sizes, regrown; the optional pinned landing place, refused once
        auto idle = [] { return 0; };
        CHECK(s->d_chain6.grow(480, idle) == 0 && s->d_chain_out.grow(480, idle) == 0);
        g_fail_in = 1;
        CHECK(s->h_chain.remake(480) == -3 && s->h_chain.p == nullptr);
        CHECK(s->d_chain6.grow(960, idle) == 0 && s->d_chain_out.grow(960, idle) == 0 && s->h_chain.remake(960) == 0);
        CHECK(g_live_dev == (in_exchange ? 4 : 5) && g_live_pin == 1);
        delete s;
        CHECK(g_live_dev == 0 && g_live_pin == 0);
    }
}

// A caller's array of n values with a guard of kGuard values on either side: ok() when the guards are untouched and the
// values are the n * sizeof(T) bytes at src (or untouched too, with a null src)
constexpr size_t kGuard = 4;
template <typename T> struct Guarded {
    std::vector<T> v;
    size_t n;
    explicit Guarded(size_t n_) : v(n_ + 2 * kGuard), n(n_) { memset(v.data(), 0xA5, v.size() * sizeof(T)); }
    T *dst() { return v.data() + kGuard; }
    bool ok(const void *src) const
    {
        const unsigned char *b = reinterpret_cast<const unsigned char *>(v.data());
        for (size_t i = 0; i < v.size() * sizeof(T); ++i) {
            const bool inside = i >= kGuard * sizeof(T) && i < (kGuard + n) * sizeof(T);
            const unsigned char want = inside && src ? static_cast<const unsigned char *>(src)[i - kGuard * sizeof(T)] : 0xA5;
            if (b[i] != want) return false;
        }
        return true;
    }
};

// The result list of an analysis (ResultBlock): sizes, offsets and padding; what place() hands out and when; both ways
// home over a malloc'd "device" block filled with a pattern
static void check_result_block()
{
    auto idle = [] { return 0; };
    {   // falling alignment: the plain sum, no padding
        ResultBlock rb;
        long long *p64; double *pd; int *pi;
        CHECK(rb.add(&p64, 3) == 0 && rb.add(&pd, 5) == 24 && rb.add(&pi, 7) == 64);
        CHECK(rb.bytes() == 3 * sizeof(long long) + 5 * sizeof(double) + 7 * sizeof(int) && rb.bytes() == 92);
    }
    {   // an int first: the double behind it is padded to 8, and the size says so
        ResultBlock rb;
        long long *p64; double *pd; int *pi;
        CHECK(rb.add(&pi, 7) == 0 && rb.add(&pd, 5) == 32 && rb.add(&p64, 3) == 72 && rb.bytes() == 96);
    }
    // the list of an analysis: a destined array, an empty one, device-only scratch, two arrays of one type side by side,
    // one array of which only the second half goes home, a 64-bit destination under the caller's name for it, 32-bit words
    long long *d_count; double *d_a, *d_empty, *d_scratch, *d_b, *d_pair; int *d_w; unsigned int *d_u;
    Guarded<int64_t> h_count(3);
    Guarded<double> h_a(4), h_empty(0), h_b(1), h_pair(5);
    Guarded<int> h_w(3);
    Guarded<unsigned int> h_u(2);
    ResultBlock rb;
    const size_t at_count = rb.add(&d_count, 3, h_count.dst());
    const size_t at_a = rb.add(&d_a, 4, h_a.dst());
    const size_t at_empty = rb.add(&d_empty, 0, h_empty.dst());
    const size_t at_scratch = rb.add(&d_scratch, 2);
    const size_t at_b = rb.add(&d_b, 1, h_b.dst());
    const size_t at_pair = rb.add(&d_pair, 10, h_pair.dst(), 5);
    const size_t at_pair2 = at_pair + 5 * sizeof(double);                          // (where what goes home begins)
    const size_t at_w = rb.add(&d_w, 3, h_w.dst());
    const size_t at_u = rb.add(&d_u, 2, h_u.dst());
    CHECK(at_count == 0 && at_a == 24 && at_empty == 56 && at_scratch == 56 && at_b == 72 && at_pair == 80 &&
          at_w == 160 && at_u == 172 && rb.bytes() == 180);
    CHECK(at_b == at_scratch + 2 * sizeof(double) && at_pair == at_b + sizeof(double));   // one type side by side: contiguous
    // place(): the block is grown first (idle() before a block in use is released), then the addresses are the new block's
    DevBuf block;
    CHECK(block.grow(16, idle) == 0);
    void *const small = block.p;
    int idles = 0;
    void *p_at_idle = nullptr;
    CHECK(rb.place(block, [&] { ++idles; p_at_idle = block.p; return 0; }) == 0);
    CHECK(idles == 1 && p_at_idle == small && block.cap == rb.bytes());
    char *const base = static_cast<char *>(block.p);
    CHECK((char *)d_count == base && (char *)d_a == base + at_a && (char *)d_scratch == base + at_scratch &&
          (char *)d_b == base + at_b && (char *)d_pair == base + at_pair && (char *)d_w == base + at_w && (char *)d_u == base + at_u);
    CHECK(d_empty == nullptr);                                                     // an empty array has no address
    CHECK(rb.place(block, [&] { ++idles; return 0; }) == 0 && idles == 1 && (char *)d_u == base + at_u);   // big enough: as it is
    {   // a block that cannot be grown: the status comes back and nothing is handed out
        ResultBlock big;
        double *q = nullptr;
        big.add(&q, 1000);
        DevBuf none;
        g_fail_in = 1;
        CHECK(big.place(none, idle) == -3 && q == nullptr && none.p == nullptr);
        CHECK(big.place(none, [] { return -7; }) == -7 && q == nullptr && none.p == nullptr);   // ... nor when idle() fails
        CHECK(big.place(none, idle) == 0 && q != nullptr && q == none.p);
    }
    for (size_t i = 0; i < rb.bytes(); ++i) base[i] = (char)(i * 7 + 1);
    // home entry by entry: exactly the destined arrays that hold something, in the list's order
    struct Visit { void *dst; size_t off, bytes; };
    std::vector<Visit> seen;
    CHECK(rb.each([&](void *dst, size_t off, size_t bytes) { seen.push_back(Visit{dst, off, bytes}); return 0; }) == 0);
    const Visit want[] = {{h_count.dst(), at_count, 24}, {h_a.dst(), at_a, 32}, {h_b.dst(), at_b, 8},
                          {h_pair.dst(), at_pair2, 40}, {h_w.dst(), at_w, 12}, {h_u.dst(), at_u, 8}};
    CHECK(seen.size() == 6);
    for (size_t i = 0; i < 6; ++i) CHECK(seen[i].dst == want[i].dst && seen[i].off == want[i].off && seen[i].bytes == want[i].bytes);
    // ... a copy that fails ends the walk with its status
    int calls = 0;
    CHECK(rb.each([&](void *, size_t, size_t) { return ++calls == 2 ? -5 : 0; }) == -5 && calls == 2);
    CHECK(h_count.ok(nullptr) && h_a.ok(nullptr) && h_b.ok(nullptr) && h_pair.ok(nullptr) && h_w.ok(nullptr) && h_u.ok(nullptr));
    // home as an image: every destination gets its own slice, nothing else is written
    {   // an entry whose first value to go home is beyond its last sends nothing
        ResultBlock none;
        double *q;
        Guarded<double> h(3);
        none.add(&q, 3, h.dst(), 3);
        none.add(&q, 2, h.dst(), 7);
        CHECK(none.bytes() == 40 && none.each([](void *, size_t, size_t) { return -1; }) == 0);
    }
    char *const image = rb.image();
    memcpy(image, base, rb.bytes());                                               // (the caller's one copy of the block)
    CHECK(rb.image() == image);
    rb.scatter();
    CHECK(h_count.ok(base + at_count) && h_a.ok(base + at_a) && h_empty.ok(nullptr) && h_b.ok(base + at_b) && h_pair.ok(base + at_pair2) &&
          h_w.ok(base + at_w) && h_u.ok(base + at_u));
}

int main()
{
    check_grow<DevBuf>(g_live_dev);
    check_grow<PinBuf>(g_live_pin);
    check_pinned_alias();
    check_group();
    check_sampler_state();
    check_result_block();
    CHECK(g_live_dev == 0 && g_live_pin == 0 && g_allocs == g_frees);
    printf("OWNED_OK %d checks\n", g_checks);
    return 0;
}
