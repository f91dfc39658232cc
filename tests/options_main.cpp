// options_main.cpp -- the option table of mbb_emcee_amd/csrc/mbb_options.h held to its own rules, stand-alone.
//
// Built by tests/test_host_cpu.py with AddressSanitizer and UBSan and run directly.  For every row: a fresh Options holds
// the default; a value within the bounds lands in the row's field and in no other; a value beyond a bound lands on the
// bound; LONG_MIN and LONG_MAX are survived.  A name the table does not have -- unknown, empty, a proper prefix of a real
// one, a real one with more behind it -- is refused and leaves the Options as they were.  Exit status 0: all held.
// With an argument: the table instead, `name default lowest highest` a line (`-`: no bound), for the test that holds the
// table of include/mbb_hip.h to it.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../mbb_emcee_amd/csrc/mbb_options.h"

using namespace mbbopt;

static int g_checks = 0;
#define CHECK(cond)                                                            \
    do {                                                                       \
        ++g_checks;                                                            \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const OptionRow *find(const char *name)
{
    for (const OptionRow &r : kOptions)
        if (!strcmp(name, r.name)) return &r;
    return nullptr;
}

// every field but `but`'s (nullptr: every field) holds its default
static bool defaults_elsewhere(const Options &o, const OptionRow *but)
{
    for (const OptionRow &q : kOptions)
        if (&q != but && o.*q.field != q.def) return false;
    return true;
}

// sets the row's option on fresh Options and says where the value landed; nothing else may have moved
static long landed(const OptionRow &r, long value)
{
    Options o;
    CHECK(set_option(o, r.name, value) == &r);
    CHECK(defaults_elsewhere(o, &r));
    return o.*r.field;
}

static void refused(const std::string &name)
{
    Options o;
    CHECK(set_option(o, name.c_str(), 7) == nullptr);
    CHECK(defaults_elsewhere(o, nullptr));
}

int main(int argc, char **)
{
    if (argc > 1) {
        for (const OptionRow &r : kOptions) {
            printf("%s %ld ", r.name, r.def);
            if (r.low == kAnyLow) printf("- "); else printf("%ld ", r.low);
            if (r.high == kAnyHigh) printf("-\n"); else printf("%ld\n", r.high);
        }
        return 0;
    }
    // the table addresses every field of Options, each once, under a name of its own
    const size_t n = sizeof(kOptions) / sizeof(kOptions[0]);
    CHECK(sizeof(Options) == n * sizeof(long));
    for (const OptionRow &r : kOptions)
        for (const OptionRow &q : kOptions)
            if (&r != &q) { CHECK(r.field != q.field); CHECK(strcmp(r.name, q.name) != 0); }
    CHECK(defaults_elsewhere(Options(), nullptr));
    for (const OptionRow &r : kOptions) {
        CHECK(r.what && *r.what);
        CHECK(r.low <= r.def && r.def <= r.high);
        const long inside = r.def < r.high ? r.def + 1 : r.def - 1;      // within the bounds, and not the default
        CHECK(r.low <= inside && inside <= r.high);
        CHECK(landed(r, inside) == inside);
        CHECK(landed(r, r.low) == r.low);
        CHECK(landed(r, r.high) == r.high);
        if (r.low != kAnyLow) CHECK(landed(r, r.low - 1) == r.low);
        if (r.high != kAnyHigh) CHECK(landed(r, r.high + 1) == r.high);
        CHECK(landed(r, LONG_MIN) == r.low);
        CHECK(landed(r, LONG_MAX) == r.high);
        // a second value replaces the first
        Options o;
        CHECK(set_option(o, r.name, inside) == &r && set_option(o, r.name, r.def) == &r);
        CHECK(defaults_elsewhere(o, nullptr));
        // the name cut short, or with more behind it, is another name
        const std::string name = r.name;
        for (size_t len = 0; len < name.size(); ++len)
            if (!find(name.substr(0, len).c_str())) refused(name.substr(0, len));
        if (!find((name + "_").c_str())) refused(name + "_");
        refused(name + " ");
    }
    refused("");
    refused("no_such_option");
    refused("SERVE");
    printf("OPTIONS_OK %zu options, %d checks\n", n, g_checks);
    return 0;
}
