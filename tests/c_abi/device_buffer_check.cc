// The owners of gr_baz_amd/csrc/device_buffer.hip.h over a counting malloc / free policy: a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_device_buffer.py.  Includes only the header under test; exits 0 when every
// check holds (a failed check names its line and exits 1; a leak, double free or use after free is the sanitizer's to report).
#include "device_buffer.hip.h"

#include <cstdio>
#include <cstdlib>
#include <utility>

namespace {

struct Heap {
    using status = int;           // 0: ok
    static int allocs, frees, fail_in;   // fail_in: the allocation that fails, counting down (0: none)
    static int alloc(void** p, size_t bytes)
    {
        if (fail_in && --fail_in == 0) return 7;
        *p = std::malloc(bytes ? bytes : 1);
        if (!*p) return 7;
        ++allocs;
        return 0;
    }
    static void release(void* p)
    {
        std::free(p);
        ++frees;
    }
};
int Heap::allocs = 0, Heap::frees = 0, Heap::fail_in = 0;

template <typename T> using Dev = bazbuf::Buffer<T, bazbuf::Counted<Heap, &bazbuf::LiveCounts::device>>;
template <typename T> using Pin = bazbuf::Buffer<T, bazbuf::Counted<Heap, &bazbuf::LiveCounts::pinned>>;

int drains = 0, frees_at_drain = -1;
int drain()
{
    ++drains;
    frees_at_drain = Heap::frees;
    return 0;
}

int checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// the live counters equal allocations minus frees, at every step
#define CHECK_LIVE()                                                                      \
    do {                                                                                  \
        uint64_t live[2];                                                                 \
        bazbuf::g_live.report(live);                                                      \
        CHECK(live[0] + live[1] == (uint64_t)(Heap::allocs - Heap::frees));               \
    } while (0)

struct Set {   // the TableSet pattern: owners and plain members that swap as one unit
    Dev<double> a;
    Dev<float> b;
    Pin<int> c;
    int param = 0;
};

template <typename B>
void owner_checks()
{
    const int a0 = Heap::allocs, f0 = Heap::frees;
    {   // an empty owner releases nothing
        B e;
        CHECK(!e && e.cap() == 0);
        e.release();
    }
    CHECK(Heap::allocs == a0 && Heap::frees == f0);
    {   // allocate, then destruct: one allocation, one free
        B x;
        CHECK(x.allocate(10) == 0 && x && x.cap() == 10);
        x[9] = 1;              // (reads as a pointer)
        CHECK(*(x + 9) == 1);
        CHECK_LIVE();
    }
    CHECK(Heap::allocs == a0 + 1 && Heap::frees == f0 + 1);
    CHECK_LIVE();
    {   // move construction and move assignment leave the source empty and free the destination's old buffer exactly once
        B x, y;
        CHECK(x.allocate(4) == 0 && y.allocate(8) == 0);
        auto* const px = x.get();
        B z(std::move(x));
        CHECK(!x && x.cap() == 0 && z.get() == px && z.cap() == 4);
        CHECK(Heap::frees == f0 + 1);
        y = std::move(z);
        CHECK(Heap::frees == f0 + 2);           // y's 8 elements
        CHECK(!z && z.cap() == 0 && y.get() == px && y.cap() == 4);
        B& same = y;
        y = std::move(same);                    // self-move: harmless
        CHECK(y.get() == px && y.cap() == 4 && Heap::frees == f0 + 2);
        CHECK_LIVE();
    }
    CHECK(Heap::allocs == a0 + 3 && Heap::frees == f0 + 3);
    {   // regrow
        B x;
        drains = 0;
        CHECK(x.regrow(0, drain) == 0 && !x && drains == 0);                       // nothing asked of an empty owner
        CHECK(x.regrow(16, drain) == 0 && x.cap() == 16 && drains == 0);           // the first allocation waits for nothing
        auto* const p = x.get();
        const int a1 = Heap::allocs, f1 = Heap::frees;
        CHECK(x.regrow(16, drain) == 0 && x.regrow(3, drain) == 0);                // smaller or equal: nothing happens
        CHECK(x.get() == p && x.cap() == 16 && drains == 0 && Heap::allocs == a1 && Heap::frees == f1);
        CHECK(x.regrow(17, drain) == 0 && x.cap() == 17);                          // larger, on a full owner: one drain, in front of the free
        CHECK(drains == 1 && frees_at_drain == f1 && Heap::frees == f1 + 1 && Heap::allocs == a1 + 1);
        CHECK_LIVE();
        // a drain that fails keeps the buffer
        auto* const q = x.get();
        CHECK(x.regrow(40, [] { return 3; }) == 3 && x.get() == q && x.cap() == 17 && Heap::frees == f1 + 1);
        // the policy's allocation fails: empty, capacity 0, the old buffer freed once; a later regrow succeeds
        Heap::fail_in = 1;
        CHECK(x.regrow(64, drain) == 7);
        CHECK(!x && x.cap() == 0 && drains == 2 && Heap::frees == f1 + 2 && Heap::allocs == a1 + 1);
        CHECK_LIVE();
        CHECK(x.regrow(64, drain) == 0 && x.cap() == 64 && drains == 2);           // (empty again: no drain)
        CHECK_LIVE();
    }
    CHECK_LIVE();
}

}  // namespace

int main()
{
    owner_checks<Dev<int>>();
    owner_checks<Pin<unsigned char>>();
    {   // std::swap of two aggregates of owners neither allocates nor frees; both sides end up with the other's pointers
        Set s, t;
        CHECK(s.a.allocate(3) == 0 && s.b.allocate(5) == 0 && s.c.allocate(7) == 0 && t.a.allocate(11) == 0);
        s.param = 1; t.param = 2;
        double* const sa = s.a; float* const sb = s.b; int* const sc = s.c; double* const ta = t.a;
        const int a1 = Heap::allocs, f1 = Heap::frees;
        std::swap(s, t);
        CHECK(Heap::allocs == a1 && Heap::frees == f1);
        CHECK(t.a == sa && t.b == sb && t.c == sc && s.a == ta && !s.b && !s.c);
        CHECK(t.a.cap() == 3 && t.b.cap() == 5 && t.c.cap() == 7 && s.a.cap() == 11 && s.b.cap() == 0);
        CHECK(s.param == 2 && t.param == 1);
        uint64_t live[2];
        bazbuf::g_live.report(live);
        CHECK(live[0] == 3 && live[1] == 1);    // device and page-locked are counted apart
        CHECK_LIVE();
    }
    CHECK_LIVE();
    {   // buffers that grow together: one drain at the first that exists, repeated for none of the others
        Dev<int> x, y, z;
        CHECK(y.allocate(2) == 0 && z.allocate(2) == 0);
        drains = 0;
        bazbuf::Once once(drain);
        CHECK(x.retire(once) == 0 && drains == 0);
        CHECK(y.retire(once) == 0 && z.retire(once) == 0 && drains == 1 && !y && !z);
        int failing = 0;
        bazbuf::Once bad([&failing] { ++failing; return 5; });     // a failed drain is repeated to every buffer: none is freed
        CHECK(y.allocate(2) == 0 && z.allocate(2) == 0);
        CHECK(y.retire(bad) == 5 && z.retire(bad) == 5 && failing == 1 && y && z);
    }
    {   // an aggregate whose third allocation failed frees the first two on destruction
        const int a1 = Heap::allocs, f1 = Heap::frees;
        {
            Set s;
            Heap::fail_in = 3;
            CHECK(s.a.allocate(1) == 0 && s.b.allocate(1) == 0 && s.c.allocate(1) == 7);
            CHECK(s.a && s.b && !s.c && Heap::allocs == a1 + 2);
            CHECK_LIVE();
        }
        CHECK(Heap::frees == f1 + 2);
    }
    uint64_t live[2];
    bazbuf::g_live.report(live);
    CHECK(live[0] == 0 && live[1] == 0 && Heap::allocs == Heap::frees && Heap::allocs > 0);
    std::printf("device_buffer_check: %d checks hold, %d allocations, %d frees\n", checks, Heap::allocs, Heap::frees);
    return 0;
}
