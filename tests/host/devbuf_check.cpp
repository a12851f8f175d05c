// Host check of directdemod_amd/csrc/dd_devbuf.h without the HIP runtime: the four allocation calls are defined here over
// malloc / free.  They keep the set of live pointers, abort on a free of a pointer that is not live, and can fail the k-th
// allocation.  Built and run by tests/test_devbuf_host.py; the sanitizer build is in tools/README.md.
#include "../../directdemod_amd/csrc/dd_devbuf.h"
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <utility>

static std::set<void*> g_live;
static std::set<void*> g_pinned;        // the pinned ones among g_live
static long g_allocs = 0;               // allocations asked for so far
static long g_fail_at = -1;             // index of the allocation that fails (-1: none)
static unsigned g_last_flags = 0;

static hipError_t stub_alloc(void** p, size_t bytes, bool pinned) {
    *p = nullptr;
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    if (!*p) abort();
    g_live.insert(*p);
    if (pinned) g_pinned.insert(*p);
    return hipSuccess;
}
static hipError_t stub_free(void* p, bool pinned) {
    if (!p) return hipSuccess;
    if (!g_live.count(p) || (g_pinned.count(p) != 0) != pinned) {
        fprintf(stderr, "free of %p: not live, or freed by the wrong call\n", p);
        abort();
    }
    g_live.erase(p);
    g_pinned.erase(p);
    free(p);
    return hipSuccess;
}
extern "C" hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes, false); }
extern "C" hipError_t hipFree(void* p) { return stub_free(p, false); }
extern "C" hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int flags) { g_last_flags = flags; return stub_alloc(p, bytes, true); }
extern "C" hipError_t hipHostFree(void* p) { return stub_free(p, true); }

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

template <class Buf>
static void basic() {
    typedef double T;
    {
        Buf b;
        CHECK(!b.get() && b.count() == 0 && b.bytes() == 0 && g_live.empty());
        CHECK(b.alloc(10) == hipSuccess);
        CHECK(b.get() && b.count() == 10 && b.bytes() == 10 * sizeof(T) && g_live.size() == 1 && g_live.count(b.get()));
        T* raw = b;                                   // implicit conversion, pointer arithmetic, indexing
        CHECK(raw == b.get() && b + 3 == raw + 3);
        b[9] = 1.5;
        CHECK(raw[9] == 1.5);
        // alloc releases what it held
        CHECK(b.alloc(20) == hipSuccess);
        CHECK(g_live.size() == 1 && g_live.count(b.get()) && b.count() == 20);
        // grow to a smaller or equal count keeps the pointer; to a larger one it allocates anew
        T* before = b.get();
        CHECK(b.grow(5) == hipSuccess && b.get() == before && b.count() == 20);
        CHECK(b.grow(20) == hipSuccess && b.get() == before);
        CHECK(b.grow(21) == hipSuccess && b.count() == 21 && g_live.size() == 1 && g_live.count(b.get()));
        // reset frees and empties; twice is harmless
        b.reset();
        CHECK(!b.get() && b.count() == 0 && g_live.empty());
        b.reset();
        // grow of an empty owner allocates
        CHECK(b.grow(4) == hipSuccess && b.count() == 4 && g_live.size() == 1);
        // move construction and move assignment hand the pointer over, and assignment frees the target's own
        T* p = b.get();
        Buf c(std::move(b));
        CHECK(!b.get() && b.count() == 0 && c.get() == p && c.count() == 4 && g_live.size() == 1);
        Buf d;
        CHECK(d.alloc(7) == hipSuccess && g_live.size() == 2);
        d = std::move(c);
        CHECK(!c.get() && d.get() == p && d.count() == 4 && g_live.size() == 1 && g_live.count(p));
        Buf& self = d;
        d = std::move(self);                          // onto itself: nothing changes
        CHECK(d.get() == p && g_live.size() == 1);
        // release gives the pointer up without freeing
        T* r = d.release();
        CHECK(r == p && !d.get() && d.count() == 0 && g_live.size() == 1);
        Buf e;
        CHECK(e.alloc(3) == hipSuccess && g_live.size() == 2);
        CHECK(stub_free(r, g_pinned.count(r) != 0) == hipSuccess);
        CHECK(g_live.size() == 1);
    }                                                 // the destructors free what is left
    CHECK(g_live.empty());
    // a failed alloc or grow leaves the owner empty, and what it held before is gone
    {
        Buf b;
        CHECK(b.alloc(8) == hipSuccess);
        g_fail_at = g_allocs;
        CHECK(b.alloc(16) == hipErrorOutOfMemory);
        CHECK(!b.get() && b.count() == 0 && b.bytes() == 0 && g_live.empty());
        CHECK(b.alloc(8) == hipSuccess);
        g_fail_at = g_allocs;
        CHECK(b.grow(4) == hipSuccess && b.count() == 8);            // (no allocation: nothing to fail)
        CHECK(b.grow(16) == hipErrorOutOfMemory);
        CHECK(!b.get() && b.count() == 0 && g_live.empty());
        g_fail_at = -1;
        CHECK(b.grow(16) == hipSuccess && b.count() == 16 && g_live.size() == 1);
    }
    CHECK(g_live.empty());
}

// a handle as the library builds them: six owners allocated in sequence, the create abandoned at the first failure
struct Six {
    DDDevBuf<float> a, b;
    DDPinnedBuf<unsigned int> c;
    DDDevBuf<double> d[2];
    DDPinnedBuf<char> e;
    hipError_t create() {
        hipError_t r = a.alloc(100);
        if (r == hipSuccess) r = b.alloc(1);
        if (r == hipSuccess) r = c.alloc(2, hipHostMallocMapped);
        if (r == hipSuccess) r = d[0].alloc(33);
        if (r == hipSuccess) r = d[1].alloc(33);
        if (r == hipSuccess) r = e.alloc(4096);
        return r;
    }
};

int main() {
    basic<DDDevBuf<double>>();
    basic<DDPinnedBuf<double>>();
    {
        DDPinnedBuf<unsigned int> w;
        CHECK(w.alloc(2, hipHostMallocMapped) == hipSuccess && g_last_flags == hipHostMallocMapped && g_pinned.count(w.get()));
        CHECK(w.grow(3, hipHostMallocDefault) == hipSuccess && g_last_flags == hipHostMallocDefault);
    }
    CHECK(g_live.empty());
    for (int k = 0; k <= 6; ++k) {                    // k = 6: no failure
        {
            Six* s = new Six();
            g_fail_at = g_allocs + k;
            const hipError_t r = s->create();
            g_fail_at = -1;
            CHECK((r == hipSuccess) == (k == 6));
            CHECK(g_live.size() == (size_t)k);
            delete s;
        }
        CHECK(g_live.empty() && g_pinned.empty());
    }
    printf("devbuf_check: ok (%ld allocations)\n", g_allocs);
    return 0;
}
