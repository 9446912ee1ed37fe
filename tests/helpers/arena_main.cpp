// Stand-alone check of DeviceArena's ownership logic (overiva_amd/csrc/host_util.h) without a GPU: the allocators of
// host_util.hip are replaced by counting fakes on top of malloc / free, and no HIP runtime function is called.  Built and run by
// tests/test_host.py; exits 0 when every check holds, else prints the line of the first one that does not.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "host_util.h"

namespace {

enum Kind { kPlain, kFine, kPooled, kPinned };
struct Rec {
    Kind kind;
    size_t bytes;
    int frees = 0;
    int order = -1;      // position in the sequence of frees
};
std::map<void*, Rec> g_recs;      // every buffer ever handed out
int g_allocs = 0, g_frees = 0, g_bad = 0;
int g_fail_at = -1;               // the allocation (counted from 0) that reports out-of-memory; -1: none

hipError_t fake_alloc(Kind kind, void** out, size_t bytes) {
    if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
    // (one byte more: a freed block must not come back under the same address while its record is looked at)
    *out = std::malloc(bytes + 1);
    g_recs[*out] = Rec{kind, bytes};
    return hipSuccess;
}
// the memory itself is kept until the next reset(): every address of a check stays unique
void fake_free(Kind kind, void* p, size_t bytes) {
    auto it = g_recs.find(p);
    if (it == g_recs.end() || it->second.kind != kind || it->second.bytes != bytes || it->second.frees != 0) ++g_bad;
    if (it != g_recs.end()) {
        it->second.frees += 1;
        it->second.order = g_frees;
    }
    ++g_frees;
}
size_t live() {
    size_t n = 0;
    for (auto& r : g_recs) n += r.second.frees == 0;
    return n;
}
bool freed_once(void* p) { return g_recs.count(p) && g_recs[p].frees == 1; }
void reset() {
    for (auto& r : g_recs) std::free(r.first);
    g_recs.clear();
    g_allocs = g_frees = g_bad = 0;
    g_fail_at = -1;
}

}  // namespace

int oiva::fail_with(int code, const std::string&) { return code; }
hipError_t oiva::dev_malloc(void** out, size_t bytes) { return fake_alloc(kPlain, out, bytes); }
hipError_t oiva::fine_malloc(void** out, size_t bytes) { return fake_alloc(kFine, out, bytes); }
void oiva::dev_free(void* p, size_t bytes) { fake_free(g_recs.count(p) && g_recs[p].kind == kFine ? kFine : kPlain, p, bytes); }
hipError_t oiva::big_alloc(int, void** out, size_t bytes) { return fake_alloc(kPooled, out, bytes); }
void oiva::big_free(int, void* p, size_t bytes) { fake_free(kPooled, p, bytes); }
hipError_t oiva::pinned_malloc(void** out, size_t bytes) { return fake_alloc(kPinned, out, bytes); }
void oiva::pinned_free(void* p, size_t bytes) { fake_free(kPinned, p, bytes); }

using oiva::DeviceArena;
using oiva::Mem;

#define CHECK(cond)                                             \
    do {                                                        \
        if (!(cond)) {                                          \
            std::printf("line %d: %s\n", __LINE__, #cond);      \
            return 1;                                           \
        }                                                       \
    } while (0)

// every take is released exactly once, by its own kind's deallocator, with its own byte count, newest first
static int every_take_is_released_once() {
    reset();
    float *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
    void *pa, *pb, *pc, *pd;
    {
        DeviceArena mem(3);
        mem.take(&a, 100);
        mem.take(&b, 200, Mem::pooled);
        mem.take(&c, 8, Mem::pinned);
        mem.take(&d, 64, Mem::fine);
        CHECK(mem.ok() && a && b && c && d && live() == 4 && g_frees == 0);
        pa = a, pb = b, pc = c, pd = d;
    }
    CHECK(g_bad == 0 && g_frees == 4 && live() == 0);
    CHECK(!a && !b && !c && !d);
    CHECK(g_recs[pd].order == 0 && g_recs[pc].order == 1 && g_recs[pb].order == 2 && g_recs[pa].order == 3);
    CHECK(g_recs[pa].kind == kPlain && g_recs[pb].kind == kPooled && g_recs[pc].kind == kPinned && g_recs[pd].kind == kFine);
    return 0;
}

// after a failing take the later ones allocate nothing and err keeps the first error, until status() hands it over
static int first_error_wins() {
    reset();
    DeviceArena mem;
    int *a = nullptr, *b = nullptr, *c = nullptr, *d = nullptr;
    g_fail_at = 1;
    mem.take(&a, 16);
    mem.take(&b, 16);
    CHECK(!mem.ok() && a && !b);
    const int allocs = g_allocs;
    mem.take(&c, 16, Mem::pooled);
    CHECK(g_allocs == allocs && !c && !mem.ok() && live() == 1);
    CHECK(mem.status() == hipErrorOutOfMemory && mem.ok());
    CHECK(mem.take_one(&d, 16) == hipSuccess && d && live() == 2);
    g_fail_at = g_allocs;
    CHECK(mem.take_one(&c, 16) == hipErrorOutOfMemory && !c && mem.ok());
    mem.clear();
    CHECK(g_bad == 0 && live() == 0 && g_frees == 2);
    return 0;
}

// release_to(mark) frees exactly the later buffers, newest first, and nulls nothing it does not own
static int release_to_mark() {
    reset();
    DeviceArena mem;
    char *keep0 = nullptr, *keep1 = nullptr, *x = nullptr, *y = nullptr, *z = nullptr;
    mem.take(&keep0, 10);
    mem.take(&keep1, 20, Mem::pooled);
    const size_t mark = mem.mark();
    mem.take(&x, 30);
    mem.take(&y, 40, Mem::pooled);
    mem.take(&z, 50);
    void *px = x, *py = y, *pz = z;
    // the owner swapped y with a buffer the arena holds from before the mark (as a plan swaps What and res_what)
    std::swap(y, keep1);
    void* k0 = keep0;
    void* k1 = y;          // the buffer taken as keep1
    mem.release_to(mark);
    CHECK(g_bad == 0 && g_frees == 3 && live() == 2);
    CHECK(freed_once(px) && freed_once(py) && freed_once(pz));
    CHECK(g_recs[pz].order == 0 && g_recs[py].order == 1 && g_recs[px].order == 2);
    CHECK(x == nullptr && z == nullptr);
    CHECK(keep0 == k0 && y == k1);              // not the arena's to null: they hold buffers from before the mark
    CHECK(keep1 == py);                         // dangling by the owner's swap, and left alone: slot y holds another buffer
    CHECK(mem.mark() == mark);
    mem.clear();
    CHECK(g_bad == 0 && live() == 0 && g_frees == 5);
    return 0;
}

// release(&p) followed by clear() frees p once
static int release_then_clear() {
    reset();
    DeviceArena mem;
    double *p = nullptr, *q = nullptr, *none = nullptr;
    mem.take(&q, 80);
    mem.take(&p, 160, Mem::pooled);
    void* pp = p;
    mem.release(&p);
    CHECK(p == nullptr && freed_once(pp) && live() == 1 && g_bad == 0);
    mem.release(&p);                // null: nothing
    mem.release(&none);
    double other = 0., *foreign = &other;
    mem.release(&foreign);          // not this arena's: left alone
    CHECK(g_frees == 1 && foreign == &other);
    mem.take(&p, 320, Mem::pooled);          // regrown
    CHECK(p && live() == 2);
    mem.clear();
    CHECK(g_bad == 0 && live() == 0 && g_frees == 3 && g_recs[pp].frees == 1);
    mem.clear();
    CHECK(g_frees == 3);
    return 0;
}

// the shape of oiva_bsseval_create: `keep` buffers, then sets of five sized by the group, the group halved while the set
// does not fit; out-of-memory injected into the set of group 4
static int halve_until_it_fits() {
    reset();
    DeviceArena mem;
    const int n_keep = 13;
    std::vector<char*> fixed(n_keep, nullptr);
    char* set[5] = {};
    for (auto& f : fixed) mem.take(&f, 24, Mem::pooled);
    CHECK(mem.status() == hipSuccess);
    const size_t keep = mem.mark();
    int group = 4, tries = 0;
    hipError_t e;
    g_fail_at = g_allocs + 3;       // the fourth buffer of the first set, of group 4
    for (;;) {
        for (auto& s : set) mem.take(&s, (size_t)group * 100, Mem::pooled);
        e = mem.status();
        ++tries;
        if (e != hipErrorOutOfMemory || group == 1) break;
        CHECK(live() == (size_t)n_keep + 3);
        mem.release_to(keep);
        for (auto& s : set) CHECK(s == nullptr);
        CHECK(live() == (size_t)n_keep);
        group = (group + 1) / 2;
    }
    CHECK(tries == 2);
    CHECK(e == hipSuccess && group == 2 && mem.mark() == keep + 5 && live() == (size_t)n_keep + 5 && g_bad == 0);
    for (auto& f : fixed) CHECK(f && g_recs[f].frees == 0);
    for (auto& s : set) CHECK(s && g_recs[s].frees == 0 && g_recs[s].bytes == 200);
    mem.clear();
    CHECK(g_bad == 0 && live() == 0);
    return 0;
}

int main() {
    const int failed = every_take_is_released_once() || first_error_wins() || release_to_mark() || release_then_clear() || halve_until_it_fits();
    reset();
    if (!failed) std::printf("arena ok\n");
    return failed;
}
