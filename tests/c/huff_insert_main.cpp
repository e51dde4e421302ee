// Stand-alone check of the level-wise initial inserts of csrc/lfm_huff_heap.h
// (heap_insert_levels, what huff_lengths_heap runs per lane before its merges)
// against the sequential UPHEAP of BZ2_hbMakeCodeLengths.  Built and run by
// tests/test_huff_tail_cpu.py.
//
// For every alphabet size 3 .. 258 and both entry widths, over the shape
// classes of huff_heap_main.cpp (all equal, 0/1, 0..3, random, powers of two
// with zeros, ramps up and down, Fibonacci weights in order and shuffled), the
// heap array after the inserts is compared entry by entry, sentinels included,
// with the one sequential inserts build.  It fails if it never met an insert
// that climbs to the root from the deepest level, a heap no insert of which
// climbs, or a heap every insert of which climbs to the root.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "lfm_huff_heap.h"

static constexpr int kMaxA = 258;
static uint64_t n_heaps = 0, n_deep_root = 0, n_no_climb = 0, n_all_root = 0;

[[noreturn]] static void die(const char* what, long a = 0, long b = 0)
{
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    std::exit(1);
}

// one heap in a checked array: the inserts touch positions 1 .. A only
template <typename Ent>
struct HostHeap {
    Ent e[kHeapEntries];
    uint32_t A = 0, reads = 0, writes = 0;
    void in(uint32_t i) const
    {
        if (i < 1u || i > A) die("position outside the leaves", (long)i, (long)A);
    }
    Ent ld(uint32_t i)
    {
        in(i);
        ++reads;
        return e[i];
    }
    void st(uint32_t i, Ent v)
    {
        in(i);
        ++writes;
        e[i] = v;
    }
    void fence() const {}
};

template <typename Ent>
static void fill(Ent* e, const uint32_t* f, int A)
{
    e[0] = 0;
    for (int i = 1; i < kHeapEntries; ++i) e[i] = heap_sent<Ent>();
    for (int i = 1; i <= A; ++i) e[i] = ((Ent)(f[i - 1] ? f[i - 1] : 1u) << 15) | (Ent)i;
}

template <typename Ent>
static void run_case(const uint32_t* f, int A)
{
    constexpr Ent kW = ~(Ent)1023;
    static Ent want[kHeapEntries];
    static HostHeap<Ent> h;
    fill(want, f, A);
    uint32_t to_root = 0, stayed = 0;
    for (int i = 1; i <= A; ++i) {  // huffman.c's UPHEAP, entries for nodes
        uint32_t z = (uint32_t)i;
        const Ent k = want[z];
        while (k < (want[z >> 1] & kW)) {
            want[z] = want[z >> 1];
            z >>= 1;
        }
        want[z] = k;
        to_root += z == 1u;
        stayed += z == (uint32_t)i;
        if (z == 1u && i >= 256) ++n_deep_root;
    }
    fill(h.e, f, A);
    h.A = (uint32_t)A;
    h.reads = h.writes = 0;
    heap_insert_levels<Ent>(h, (uint32_t)A);
    for (int i = 0; i < kHeapEntries; ++i)
        if (h.e[i] != want[i]) die("entry differs from the sequential inserts", A, i);
    // position z of level J: J + 1 reads and as many writes
    uint32_t expect = 0;
    for (int z = 2; z <= A; ++z) expect += (uint32_t)heap_levels((uint32_t)z) + 1u;
    if (h.reads != expect || h.writes != expect) die("reads or writes per insert", (long)h.reads, (long)expect);
    ++n_heaps;
    n_no_climb += stayed == (uint32_t)A;
    n_all_root += to_root == (uint32_t)A;
}

static uint64_t rng_state = 0x4C464D49ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// cap: the largest sum of weights the entry width holds; big: the largest weight drawn
template <typename Ent>
static void run_shapes(int A, uint64_t cap, uint32_t big)
{
    uint32_t f[kMaxA];
    const uint32_t each = (uint32_t)(cap / (uint64_t)A);
    auto go = [&]() { run_case<Ent>(f, A); };
    for (uint32_t v : {1u, 7u, each}) {  // all equal: no insert climbs
        for (int i = 0; i < A; ++i) f[i] = v;
        go();
    }
    for (int rep = 0; rep < 2; ++rep) {
        for (int i = 0; i < A; ++i) f[i] = rnd() & 1u;
        go();
        for (int i = 0; i < A; ++i) f[i] = rnd() & 3u;
        go();
        const uint32_t lim = each < big ? each : big;
        for (int i = 0; i < A; ++i) f[i] = rnd() % (lim + 1u);
        go();
    }
    {  // powers of two with zeros
        int top = 0;
        while ((2ull << top) * (uint64_t)A <= cap && (2u << top) <= big) ++top;
        for (int i = 0; i < A; ++i) f[i] = rnd() % 3u == 0 ? 0u : 1u << (rnd() % (uint32_t)(top + 1));
        go();
    }
    {  // ramps: rising (no insert climbs), then strictly falling (every insert climbs to the root)
        for (int i = 0; i < A; ++i) f[i] = (uint32_t)(i + 1);
        go();
        for (int i = 0; i < A / 2; ++i) std::swap(f[i], f[A - 1 - i]);
        go();
    }
    {  // Fibonacci weights as far as the width allows, ones after them; then shuffled
        uint64_t a = 1, b = 1, sum = 0;
        int i = 0;
        for (; i < A; ++i) {
            if (sum + a + (uint64_t)(A - i - 1) > cap || a > big) break;
            f[i] = (uint32_t)a;
            sum += a;
            const uint64_t c = a + b;
            a = b;
            b = c;
        }
        for (; i < A; ++i) f[i] = 1;
        go();
        for (int j = 0; j < A; ++j) std::swap(f[j], f[rnd() % (uint32_t)A]);
        go();
    }
}

int main()
{
    for (int A = 3; A <= kMaxA; ++A) {
        run_shapes<uint32_t>(A, (1u << 17) - 1u, 100000u);
        run_shapes<uint64_t>(A, 1ull << 30, 1u << 20);
    }
    std::printf("ok heaps %llu deeproot %llu noclimb %llu allroot %llu\n", (unsigned long long)n_heaps,
                (unsigned long long)n_deep_root, (unsigned long long)n_no_climb, (unsigned long long)n_all_root);
    if (!n_deep_root || !n_no_climb || !n_all_root) die("a premise of the test was never met");
    return 0;
}
