// owned_main.cpp -- the owners of mbb_emcee_amd/csrc/mbb_owned.h over malloc / free, stand-alone.
//
// Built by tests/test_host_cpu.py with AddressSanitizer (leak detection on) and UBSan and run directly.  The four runtime
// functions the header declares are defined here with counters of live blocks and a switch that makes the n-th allocation
// from now fail; what mbb_hip.hip builds on -- grow, a failed allocation, destruction, a struct of owners, a sampler's
// state held by a unique_ptr -- is checked against them.  Exit status 0: all held.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

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

int main()
{
    check_grow<DevBuf>(g_live_dev);
    check_grow<PinBuf>(g_live_pin);
    check_pinned_alias();
    check_group();
    check_sampler_state();
    CHECK(g_live_dev == 0 && g_live_pin == 0 && g_allocs == g_frees);
    printf("OWNED_OK %d checks\n", g_checks);
    return 0;
}
