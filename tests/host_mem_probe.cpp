// Stand-alone probe of csrc/host_mem.hpp against a counting fake backend (tests/test_host_mem.py compiles it with
// -fsanitize=address,undefined and runs it): exits non-zero with a message on the first violated condition.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_mem.hpp"

struct Call {
    char what;          // 'D' device alloc, 'P' pinned alloc, 'd' device free, 'p' pinned free, 'z' memset
    void* ptr;
    size_t bytes;
    unsigned flags;
    int stream;
};
static std::vector<Call> g_log;
static int g_allocs = 0;        // allocation calls so far, failed ones included
static int g_fail_at = -1;      // the allocation call (counted from 0) that fails; -1: none
static bool g_fail_memset = false;

struct Fake {
    using error_t = int;
    using stream_t = int;
    static constexpr int ok = 0;
    static int allocate(char what, void** p, size_t bytes, unsigned flags) {
        if (g_allocs++ == g_fail_at) { *p = nullptr; return 2; }
        *p = malloc(bytes);
        g_log.push_back({what, *p, bytes, flags, 0});
        return 0;
    }
    static int device_alloc(void** p, size_t bytes) { return allocate('D', p, bytes, 0); }
    static int pinned_alloc(void** p, size_t bytes, unsigned flags) { return allocate('P', p, bytes, flags); }
    static int device_free(void* p) { g_log.push_back({'d', p, 0, 0, 0}); free(p); return 0; }
    static int pinned_free(void* p) { g_log.push_back({'p', p, 0, 0, 0}); free(p); return 0; }
    static int memset_async(void* p, int v, size_t bytes, int stream) {
        if (g_fail_memset) return 3;
        g_log.push_back({'z', p, bytes, 0, stream});
        for (size_t i = 0; i < bytes; ++i) ((unsigned char*)p)[i] = (unsigned char)v;      // (ASan: the bytes are inside the block)
        return 0;
    }
};
using Owner = frl::MemOwner<Fake>;
using frl::MEM_DEVICE;
using frl::MEM_PINNED;

#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, __func__, #cond); \
            exit(1);                                                               \
        }                                                                          \
    } while (0)

static void reset() { g_log.clear(); g_allocs = 0; g_fail_at = -1; g_fail_memset = false; }
static size_t count(char what) { size_t n = 0; for (const Call& c : g_log) n += c.what == what; return n; }

// a. n mixed blocks: release_all frees each once, newest first, through the matching free; slots and live count are null
static void mixed_release() {
    reset();
    Owner m;
    float* f = nullptr; int* i = nullptr; unsigned* u = nullptr; double* d = nullptr; unsigned char* b = nullptr; long long* l = nullptr;
    CHECK(m.alloc(&f, 7, MEM_DEVICE) == 0);
    CHECK(m.alloc(&i, 3, MEM_PINNED) == 0);
    CHECK(m.alloc(&u, 5, MEM_DEVICE) == 0);
    CHECK(m.alloc(&d, 2, MEM_PINNED, 6u) == 0);
    CHECK(m.alloc(&b, 9, MEM_DEVICE) == 0);
    CHECK(m.alloc(&l, 1, MEM_PINNED) == 0);
    CHECK(f && i && u && d && b && l && m.live() == 6);
    const std::vector<Call> allocs = g_log;
    CHECK(allocs.size() == 6);
    CHECK(allocs[0].bytes == 28 && allocs[1].bytes == 12 && allocs[2].bytes == 20 && allocs[3].bytes == 16 && allocs[4].bytes == 9 && allocs[5].bytes == 8);
    f[6] = 1.f; i[2] = 1; u[4] = 1u; d[1] = 1.0; b[8] = 1; l[0] = 1;       // (ASan: every block holds its count)
    g_log.clear();
    m.release_all();
    CHECK(g_log.size() == 6);
    for (size_t k = 0; k < 6; ++k) {
        const Call& a = allocs[5 - k];
        CHECK(g_log[k].ptr == a.ptr);
        CHECK(g_log[k].what == (a.what == 'D' ? 'd' : 'p'));
    }
    CHECK(!f && !i && !u && !d && !b && !l && m.live() == 0);
    g_log.clear();
    m.release_all();                                                      // nothing is freed twice
    CHECK(g_log.empty());
}

// b. alloc on an owned slot frees the old block first; the live count stays
static void realloc_owned() {
    reset();
    Owner m;
    float* a = nullptr; int* b = nullptr;
    CHECK(m.alloc(&a, 4, MEM_DEVICE) == 0 && m.alloc(&b, 4, MEM_PINNED) == 0);
    void* old = a;
    g_log.clear();
    CHECK(m.alloc(&a, 8, MEM_DEVICE) == 0);
    CHECK(g_log.size() == 2 && g_log[0].what == 'd' && g_log[0].ptr == old && g_log[1].what == 'D' && g_log[1].bytes == 32);
    CHECK(a && m.live() == 2);
    g_log.clear();
    m.release_all();                       // a is now the newest block
    CHECK(g_log.size() == 2 && g_log[0].what == 'd' && g_log[1].what == 'p' && !a && !b);
    // release(slot) frees one block and nulls its slot; a slot that holds nothing is left alone
    CHECK(m.alloc(&a, 1, MEM_DEVICE) == 0 && m.alloc(&b, 1, MEM_PINNED) == 0);
    g_log.clear();
    m.release(&a);
    CHECK(!a && b && m.live() == 1 && g_log.size() == 1 && g_log[0].what == 'd');
    m.release(&a);
    CHECK(g_log.size() == 1 && m.live() == 1);
}

// c. grow: no backend call at or below the capacity; a larger request replaces the block; a failed one leaves slot null and cap 0
static void grow() {
    reset();
    Owner m;
    float* p = nullptr;
    size_t cap = 0;
    CHECK(m.grow(&p, cap, 10, MEM_DEVICE) == 0 && p && cap == 10 && m.live() == 1);
    float* first = p;
    g_log.clear();
    CHECK(m.grow(&p, cap, 10, MEM_DEVICE) == 0 && m.grow(&p, cap, 3, MEM_DEVICE) == 0);
    CHECK(p == first && cap == 10 && g_log.empty());
    CHECK(m.grow(&p, cap, 11, MEM_DEVICE) == 0);
    CHECK(g_log.size() == 2 && g_log[0].what == 'd' && g_log[0].ptr == first && g_log[1].what == 'D' && g_log[1].bytes == 44);
    CHECK(p && cap == 11 && m.live() == 1);
    p[10] = 1.f;
    g_fail_at = g_allocs;                  // the replacing allocation fails
    CHECK(m.grow(&p, cap, 70, MEM_DEVICE) == 2);
    CHECK(!p && cap == 0 && m.live() == 0);
    g_fail_at = -1;
    g_log.clear();
    CHECK(m.grow(&p, cap, 3, MEM_DEVICE) == 0);       // a smaller request after the failure allocates again
    CHECK(p && cap == 3 && m.live() == 1 && g_log.size() == 1 && g_log[0].what == 'D' && g_log[0].bytes == 12);
    p[2] = 1.f;
}

// d. a routine of n allocations that fails at its k-th, then release_all (or release_to the mark taken before it): nothing stays,
//    and a second run allocates exactly n blocks
struct Slots {
    float* a = nullptr; int* b = nullptr; double* c = nullptr; unsigned char* d = nullptr; float* e = nullptr; unsigned* f = nullptr;
    bool all_null() const { return !a && !b && !c && !d && !e && !f; }
};
static const int kRoutine = 6;
static int routine(Owner& m, Slots& s) {
    int rc;
    if ((rc = m.alloc(&s.a, 16, MEM_PINNED))) return rc;
    if ((rc = m.alloc_zero(&s.b, 5, 1))) return rc;
    if ((rc = m.alloc(&s.c, 4, MEM_DEVICE))) return rc;
    if ((rc = m.alloc(&s.d, 33, MEM_PINNED, 3u))) return rc;
    if ((rc = m.alloc_zero(&s.e, 8, 1))) return rc;
    if ((rc = m.alloc(&s.f, 2, MEM_DEVICE))) return rc;
    return 0;
}
static void failing_routine() {
    for (int k = 0; k < kRoutine; ++k) {
        reset();
        Owner m;
        Slots s;
        g_fail_at = k;
        CHECK(routine(m, s) == 2);
        CHECK((int)m.live() == k && (int)(count('D') + count('P')) == k);
        m.release_all();
        CHECK(m.live() == 0 && s.all_null() && (int)(count('d') + count('p')) == k);
        g_fail_at = -1;
        g_log.clear();
        CHECK(routine(m, s) == 0);
        CHECK((int)m.live() == kRoutine && (int)(count('D') + count('P')) == kRoutine && count('d') + count('p') == 0);
    }                                       // (the owner's destructor frees the second run's blocks: ASan's leak check)
    for (int k = 0; k < kRoutine; ++k) {    // the same with blocks from before the routine, which stay: release_to(mark)
        reset();
        Owner m;
        Slots s;
        long long* keep = nullptr;
        CHECK(m.alloc(&keep, 4, MEM_DEVICE) == 0);
        const size_t mark = m.live();
        g_fail_at = g_allocs + k;
        CHECK(routine(m, s) == 2);
        m.release_to(mark);
        CHECK(m.live() == 1 && keep && s.all_null());
        keep[3] = 1;
        g_fail_at = -1;
        g_log.clear();
        CHECK(routine(m, s) == 0);
        CHECK((int)m.live() == 1 + kRoutine && (int)(count('D') + count('P')) == kRoutine);
    }
}

// e. count == 0 records nothing (and frees what the slot held)
static void zero_count() {
    reset();
    Owner m;
    float* p = nullptr;
    size_t cap = 0;
    CHECK(m.alloc(&p, 0, MEM_DEVICE) == 0 && !p && m.live() == 0);
    CHECK(m.alloc(&p, 0, MEM_PINNED, 5u) == 0 && !p && m.live() == 0);
    CHECK(m.alloc_zero(&p, 0, 1) == 0 && !p && m.live() == 0);
    CHECK(m.grow(&p, cap, 0, MEM_DEVICE) == 0 && !p && cap == 0 && m.live() == 0);
    CHECK(g_log.empty());
    CHECK(m.alloc(&p, 2, MEM_DEVICE) == 0 && m.live() == 1);
    CHECK(m.alloc(&p, 0, MEM_DEVICE) == 0 && !p && m.live() == 0 && count('d') == 1);
}

// f. pinned flags reach the backend unchanged; alloc_zero memsets count * sizeof(T) bytes on the given stream
template <class T>
static void zeroed(size_t n, int stream) {
    reset();
    Owner m;
    T* p = nullptr;
    CHECK(m.alloc_zero(&p, n, stream) == 0 && p);
    CHECK(g_log.size() == 2 && g_log[0].what == 'D' && g_log[0].bytes == n * sizeof(T));
    CHECK(g_log[1].what == 'z' && g_log[1].ptr == (void*)p && g_log[1].bytes == n * sizeof(T) && g_log[1].stream == stream);
    for (size_t i = 0; i < n; ++i) CHECK(p[i] == T(0));
}
static void backend_arguments() {
    reset();
    Owner m;
    int* a = nullptr; float* b = nullptr;
    CHECK(m.alloc(&a, 16, MEM_PINNED, 0x6u) == 0 && m.alloc(&b, 1, MEM_PINNED) == 0);
    CHECK(g_log.size() == 2 && g_log[0].what == 'P' && g_log[0].flags == 0x6u && g_log[0].bytes == 64 && g_log[1].flags == 0u);
    zeroed<unsigned char>(13, 7);
    zeroed<int>(13, 8);
    zeroed<double>(13, 9);
    reset();                               // a memset that fails leaves nothing behind either: alloc_zero is one operation
    g_fail_memset = true;
    CHECK(m.alloc_zero(&b, 4, 1) == 3 && !b && count('D') == 1 && count('d') == 1);
}

// two slots of one kind may trade blocks (frl_rollout swaps obs and obs_next): still one free per block
static void swapped_slots() {
    reset();
    Owner m;
    float* a = nullptr; float* b = nullptr;
    CHECK(m.alloc(&a, 4, MEM_PINNED) == 0 && m.alloc(&b, 4, MEM_PINNED) == 0);
    float* t = a; a = b; b = t;
    m.release_all();
    CHECK(!a && !b && count('p') == 2 && g_log[2].ptr != g_log[3].ptr);
}

int main() {
    mixed_release();
    realloc_owned();
    grow();
    failing_routine();
    zero_count();
    backend_arguments();
    swapped_slots();
    {   // the destructor releases what is left
        reset();
        float* p = nullptr;
        { Owner m; CHECK(m.alloc(&p, 4, MEM_DEVICE) == 0); }
        CHECK(!p && count('d') == 1);
    }
    puts("host_mem ok");
    return 0;
}
