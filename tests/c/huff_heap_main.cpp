// Stand-alone check of csrc/lfm_huff_heap.h (the heap steps of the GPU
// encoder's Huffman code-length kernel) against a plain array restatement of
// BZ2_hbMakeCodeLengths.  Built and run by tests/test_huff_heap_path_cpu.py.
//
// One heap is driven the way a lane of the kernel drives it: entries
// (weight << 15 | node), the initial inserts, the pref bits built in one pass,
// then the merges in lockstep with a group whose largest heap holds hmax
// entries, the tree redone with halved weights while it is too long.  Code
// lengths and retry counts must equal the restatement's, and after every pop,
// sift and push each pref bit must equal the comparison of its node's children.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "lfm_huff_heap.h"

static constexpr int kMaxA = 258;

struct Counts {
    uint64_t heaps = 0, retries = 0, equal = 0, stop0 = 0, deepest = 0, rootpush = 0, sifts = 0, checks = 0;
};
static Counts g;

[[noreturn]] static void die(const char* what, long a = 0, long b = 0)
{
    std::printf("FAIL %s (%ld, %ld)\n", what, a, b);
    std::exit(1);
}

// ---- the restatement: arrays from 1, weights freq << 8 | depth -------------
static int ref_lengths(uint8_t* len, const uint32_t* freq, int alphaSize, int maxLen)
{
    int heap[kMaxA + 2], parent[2 * kMaxA];
    uint64_t weight[2 * kMaxA];
    int retries = 0;
    for (int i = 0; i < alphaSize; ++i) weight[i + 1] = (uint64_t)(freq[i] == 0 ? 1 : freq[i]) << 8;
    while (true) {
        int nNodes = alphaSize, nHeap = 0;
        heap[0] = 0;
        weight[0] = 0;
        parent[0] = -2;
        auto upheap = [&](int z) {
            const int tmp = heap[z];
            while (weight[tmp] < weight[heap[z >> 1]]) {
                heap[z] = heap[z >> 1];
                z >>= 1;
            }
            heap[z] = tmp;
        };
        auto downheap = [&](int z) {
            const int tmp = heap[z];
            while (true) {
                int yy = z << 1;
                if (yy > nHeap) break;
                if (yy < nHeap && weight[heap[yy + 1]] < weight[heap[yy]]) yy++;
                if (weight[tmp] < weight[heap[yy]]) break;
                heap[z] = heap[yy];
                z = yy;
            }
            heap[z] = tmp;
        };
        for (int i = 1; i <= alphaSize; ++i) {
            parent[i] = -1;
            heap[++nHeap] = i;
            upheap(nHeap);
        }
        while (nHeap > 1) {
            const int n1 = heap[1];
            heap[1] = heap[nHeap--];
            downheap(1);
            const int n2 = heap[1];
            heap[1] = heap[nHeap--];
            downheap(1);
            ++nNodes;
            parent[n1] = parent[n2] = nNodes;
            const uint64_t d1 = weight[n1] & 0xff, d2 = weight[n2] & 0xff;
            weight[nNodes] = ((weight[n1] & ~(uint64_t)0xff) + (weight[n2] & ~(uint64_t)0xff)) | (1 + (d1 > d2 ? d1 : d2));
            parent[nNodes] = -1;
            heap[++nHeap] = nNodes;
            upheap(nHeap);
        }
        bool tooLong = false;
        for (int i = 1; i <= alphaSize; ++i) {
            int j = 0, k = i;
            while (parent[k] >= 0) {
                k = parent[k];
                ++j;
            }
            len[i - 1] = (uint8_t)j;
            if (j > maxLen) tooLong = true;
        }
        if (!tooLong) return retries;
        ++retries;
        for (int i = 1; i <= alphaSize; ++i) weight[i] = (uint64_t)(1 + (weight[i] >> 8) / 2) << 8;
    }
}

// ---- the accessor: one heap in a checked array -----------------------------
template <typename Ent>
struct HostHeap {
    Ent e[kHeapEntries];
    uint16_t parent[2 * kMaxA + 4];
    uint32_t lockstep = 1;
    static void in(uint32_t i)
    {
        if (i >= (uint32_t)kHeapEntries) die("entry index out of range", (long)i);
    }
    Ent ld(uint32_t i) const
    {
        in(i);
        return e[i];
    }
    void st(uint32_t i, Ent v)
    {
        in(i);
        if (i >= kHeapSentPair && v != heap_sent<Ent>()) die("an entry written to the sentinel pair", (long)i);
        e[i] = v;
    }
    void ld_pair(uint32_t i, Ent& a, Ent& b) const
    {
        if (i & 1u) die("odd pair", (long)i);
        in(i + 1u);
        a = e[i];
        b = e[i + 1u];
    }
    void fence() const {}
    void set_parent(uint32_t node, uint32_t p)
    {
        if (node >= 2 * kMaxA + 4) die("parent index out of range", (long)node);
        parent[node] = (uint16_t)p;
    }
    // a neighbour in the group is often still climbing: the heap then repeats its last step
    bool any(bool b)
    {
        lockstep = lockstep * 1103515245u + 12345u;
        return b || (lockstep >> 16 & 3u) != 0;
    }
    void note_sift(uint32_t went, uint32_t L)
    {
        ++g.sifts;
        if (L >= 1 && went == 0) ++g.stop0;
        if (L >= 2 && went == L) ++g.deepest;
    }
    void note_push(uint32_t from, uint32_t to)
    {
        if (from >= 4 && to == 1) ++g.rootpush;
    }
    // the invariants: pref bits, sentinels past the heap, the heap order
    void check(const HeapPref& m, uint32_t nHeap) const
    {
        ++g.checks;
        for (uint32_t p = 1; p < 160; ++p) {
            const uint32_t want = 2 * p + 1 < (uint32_t)kHeapEntries && heap_wless(e[2 * p + 1], e[2 * p]) ? 1u : 0u;
            const uint32_t got = heap_pref_at(m, 31 - __builtin_clz(p), p);
            if (want != got) die("pref bit differs from its children's comparison", (long)p, (long)nHeap);
        }
        if (m.w[4] >> 31) die("bit 31 of the last pref word set");
        if (g.checks % 5) return;  // the scans of the whole array: every fifth time
        // (the last merge sifts its second key into an empty heap: position 1, overwritten by the push)
        for (uint32_t i = (nHeap ? nHeap : 1u) + 1; i < (uint32_t)kHeapEntries; ++i)
            if (e[i] != heap_sent<Ent>()) die("an entry past the heap", (long)i, (long)nHeap);
        for (uint32_t i = 2; i <= nHeap; ++i)
            if (heap_wless(e[i], e[i >> 1])) die("heap order", (long)i, (long)nHeap);
    }
};

template <typename Ent>
static int lane_lengths(uint8_t* len, const uint32_t* freq, int A, uint32_t hmax)
{
    constexpr Ent kW = ~(Ent)1023;
    constexpr int kMaxRetries = sizeof(Ent) == 4 ? 17 : 32;
    static HostHeap<Ent> h;
    int retries = 0;
    uint32_t nNodes = (uint32_t)A;
    while (true) {
        h.e[0] = 0;
        for (int i = 1; i < kHeapEntries; ++i) h.e[i] = heap_sent<Ent>();
        for (int i = 1; i <= A; ++i) {
            uint32_t w = freq[i - 1] ? freq[i - 1] : 1u;
            for (int r = 0; r < retries; ++r) w = 1u + w / 2u;
            if (sizeof(Ent) == 4 && w >= (1u << 17)) die("weight too wide for narrow entries");
            h.e[i] = ((Ent)w << 15) | (Ent)i;
        }
        for (int i = 1; i <= A; ++i) {  // the initial inserts
            uint32_t z = (uint32_t)i;
            const Ent k = h.e[z];
            while (k < (h.e[z >> 1] & kW)) {
                h.e[z] = h.e[z >> 1];
                z >>= 1;
            }
            h.e[z] = k;
        }
        HeapPref m;
        heap_pref_build<Ent>(h, m, (uint32_t)A);
        h.check(m, (uint32_t)A);
        nNodes = (uint32_t)A;
        uint32_t tooLong = 0;
        heap_merge_all<Ent>(h, m, (uint32_t)A, hmax, nNodes, tooLong);
        if (nNodes != 2u * (uint32_t)A - 1u) die("node count", (long)nNodes, A);
        if (!tooLong || retries >= kMaxRetries) break;
        ++retries;
    }
    uint16_t depth[2 * kMaxA + 4];
    depth[nNodes] = 0;
    for (uint32_t k = nNodes - 1; k >= 1; --k) {
        const uint32_t p = h.parent[k];
        if (p <= k || p > nNodes) die("parent order", (long)k, (long)p);
        depth[k] = (uint16_t)(depth[p] + 1);
    }
    for (int i = 1; i <= A; ++i) len[i - 1] = (uint8_t)depth[i];
    return retries;
}

static uint64_t rng_state = 0x4C464D48ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

template <typename Ent>
static void run_case(const uint32_t* freq, int A, uint32_t hmax)
{
    uint8_t want[kMaxA], got[kMaxA];
    const int rw = ref_lengths(want, freq, A, 17);
    const int rg = lane_lengths<Ent>(got, freq, A, hmax);
    if (rw != rg) die("retry count", rw, rg);
    if (std::memcmp(want, got, (size_t)A)) die("code lengths", A, (long)hmax);
    ++g.heaps;
    g.retries += (uint64_t)rw;
    bool eq = true;
    for (int i = 1; i < A; ++i) eq = eq && (freq[i] ? freq[i] : 1u) == (freq[0] ? freq[0] : 1u);
    if (eq) ++g.equal;
}

// the shape classes; cap: the largest sum of weights the entry width holds
template <typename Ent>
static void run_shapes(int A, uint64_t cap, uint32_t big)
{
    uint32_t f[kMaxA];
    const uint32_t each = (uint32_t)(cap / (uint64_t)A);  // a weight that A symbols may all have
    auto go = [&]() {
        uint64_t sum = 0;
        for (int i = 0; i < A; ++i) sum += f[i] ? f[i] : 1u;
        if (sum > cap) die("test vector exceeds the entry width", A);
        run_case<Ent>(f, A, (uint32_t)A);
        run_case<Ent>(f, A, (uint32_t)kMaxA);                 // beside the largest heap
        run_case<Ent>(f, A, (uint32_t)A + rnd() % (uint32_t)(kMaxA - A + 1));
    };
    for (uint32_t v : {1u, 7u, each}) {  // all equal
        for (int i = 0; i < A; ++i) f[i] = v;
        go();
    }
    for (int rep = 0; rep < 2; ++rep) {
        for (int i = 0; i < A; ++i) f[i] = rnd() & 1u;  // 0 / 1
        go();
        for (int i = 0; i < A; ++i) f[i] = rnd() & 3u;  // 0 .. 3
        go();
        const uint32_t lim = each < big ? each : big;  // random below 100 000 (wide: 2^20)
        for (int i = 0; i < A; ++i) f[i] = rnd() % (lim + 1u);
        go();
    }
    {  // powers of two with zeros
        int top = 0;
        while ((2ull << top) * (uint64_t)A <= cap && (2u << top) <= big) ++top;
        for (int i = 0; i < A; ++i) f[i] = rnd() % 3u == 0 ? 0u : 1u << (rnd() % (uint32_t)(top + 1));
        go();
    }
    {  // ramps
        const uint32_t step = each / (uint32_t)A ? each / (uint32_t)A : 1u;
        for (int i = 0; i < A; ++i) f[i] = each >= (uint32_t)A ? (uint32_t)(i + 1) * step : (uint32_t)(i + 1) * each / (uint32_t)A;
        go();
        for (int i = 0; i < A / 2; ++i) std::swap(f[i], f[A - 1 - i]);
        go();
    }
    {  // Fibonacci weights as far as the width allows, ones after them: trees too long, hence retries
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
    std::printf("ok heaps %llu retries %llu equal %llu stop0 %llu deepest %llu rootpush %llu sifts %llu checks %llu\n",
                (unsigned long long)g.heaps, (unsigned long long)g.retries, (unsigned long long)g.equal,
                (unsigned long long)g.stop0, (unsigned long long)g.deepest, (unsigned long long)g.rootpush,
                (unsigned long long)g.sifts, (unsigned long long)g.checks);
    if (!g.retries || !g.equal || !g.stop0 || !g.deepest || !g.rootpush) die("a premise of the test was never met");
    return 0;
}
