// The heap steps of the Huffman code-length kernel (huff_lengths_heap) and, on
// the host, of its stand-alone test (tests/c/huff_heap_main.cpp).  No HIP, no
// allocation: plain integer code over an entry accessor.
//
// A heap entry is one word of type Ent: the weight (freq << 5 | height) above
// bit 10, the node in bits 0 .. 9.  Position 0 holds 0 (it ends every climb),
// positions 1 .. nHeap the heap, every position after it heap_sent(), which is
// never less than an entry: no heap step needs a bound.
//
// The downheap path without the walk.  Per heap, one bit per internal node p:
// pref[p] = 1 iff the right child's weight is strictly less than the left
// child's (huffman.c's `yy++` test: ties go left).  With the bits in registers
// the path a sift takes from the root is pure arithmetic, p0 = 1,
// p(j + 1) = 2 p(j) + pref[p(j)], whatever the key: a sift of L levels reads the
// L children pairs of its path in one round trip, decides with selects where
// the key stops, rewrites the L + 1 positions without a branch (a position
// below the stop gets its old entry back) and recomputes the L bits from the
// entries it holds.  A pop clears the bit of the popped position's parent, a
// push recomputes the bit of every position its climb changed.
//
// The accessor A supplies the entries:
//   Ent  ld(e)                entry e
//   void st(e, v)
//   void ld_pair(e, a, b)     entries e (even) and e + 1
//   void fence()              every read above goes out before anything below
//   void set_parent(node, p)
//   bool any(bool)            true in some heap of the group walked in lockstep
//   void note_sift(went, L), note_push(from, to), check(m, nHeap)   (test hooks)
#pragma once
#include <cstdint>

#ifndef LFM_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFM_HD __host__ __device__
#else
#define LFM_HD
#endif
#endif

// entries 0 .. 259, then four sentinels that nothing but a sentinel is written
// to: a children pair past the array reads kHeapSentPair
constexpr int kHeapEntries = 264;
constexpr uint32_t kHeapSentPair = 260;
constexpr int kHeapMaxLevels = 8;  // floor(log2(258))
constexpr int kPrefWords = 5;      // nodes 1 .. 31, 32 .. 63, 64 .. 95, 96 .. 127, 128 .. 129

struct HeapPref {
    uint32_t w[kPrefWords];
};

// a < b on weights (bits 10 and up) <=> (a with its node bits set) < b; a
// sentinel (all ones) is never less
template <typename Ent>
LFM_HD inline bool heap_wless(Ent a, Ent b)
{
    return (a | (Ent)1023) < b;
}

template <typename Ent>
LFM_HD inline Ent heap_sent()
{
    return ~(Ent)0;
}

// pref[p] for a node p of level j (2^j <= p < 2^(j + 1)): the word is known
// from the level, but for level 6 (two words).  Level 7 has two nodes with
// children (128, 129); every other one reads bit 31 of its word, never set.
LFM_HD inline uint32_t heap_pref_at(const HeapPref& m, int j, uint32_t p)
{
    if (j <= 4) return (m.w[0] >> (p & 31u)) & 1u;
    if (j == 5) return (m.w[1] >> (p & 31u)) & 1u;
    if (j == 6) return ((p & 32u ? m.w[3] : m.w[2]) >> (p & 31u)) & 1u;
    const uint32_t b = p - 128u < 31u ? p - 128u : 31u;
    return (m.w[4] >> b) & 1u;
}

LFM_HD inline uint32_t heap_put_bit(uint32_t w, uint32_t b, uint32_t bit)
{
    return (w & ~(1u << b)) | (bit << b);
}

// flips pref[p] of a node p of level j where flip is 1: d collects the flips
// of a sift (its nodes are distinct), one exclusive-or per word ends it
LFM_HD inline void heap_pref_flip(HeapPref& d, int j, uint32_t p, uint32_t flip)
{
    if (j <= 4) {
        d.w[0] |= flip << (p & 31u);
    } else if (j == 5) {
        d.w[1] |= flip << (p & 31u);
    } else if (j == 6) {
        const uint32_t x = flip << (p & 31u);
        d.w[2] |= p & 32u ? 0u : x;
        d.w[3] |= p & 32u ? x : 0u;
    } else {
        // past node 158 both children are sentinels: no flip, and bit 31 stays 0
        const uint32_t b = p - 128u < 31u ? p - 128u : 31u;
        d.w[4] |= flip << b;
    }
}

// the same for a node known only at run time (p < 160)
LFM_HD inline void heap_pref_set_any(HeapPref& m, uint32_t p, uint32_t bit)
{
    const uint32_t b = p & 31u, wi = p >> 5;
#pragma unroll
    for (uint32_t i = 0; i < (uint32_t)kPrefWords; ++i) m.w[i] = wi == i ? heap_put_bit(m.w[i], b, bit) : m.w[i];
}

// The initial inserts.  Positions 1 .. A hold the leaves in insertion order
// (an insert's climb only touches positions above it in the tree, all below
// it in the array) and are inserted in that order, level by level: position z
// of level J (2^J <= z < 2^(J + 1)) has J ancestors, z >> 1 .. z >> J = 1,
// read with it in one round trip and rewritten without a branch -- the
// parent's entry where the key climbs past it, the key where it stops, the
// old entry above (weights only grow downwards, so the key passes a prefix of
// the levels; the root ends the climb, position 0 is not read).
template <int J, typename Ent, typename Acc>
LFM_HD inline void heap_insert_at(Acc& acc, uint32_t z)
{
    Ent v[J + 1];
#pragma unroll
    for (int j = 0; j <= J; ++j) v[j] = acc.ld(z >> j);  // v[0]: the key, the leaf at z
    acc.fence();
    const Ent k = v[0], kk = k | (Ent)1023;
    bool below = true;  // the key climbed past the level below
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const bool lt = kk < v[j + 1];
        acc.st(z >> j, lt ? v[j + 1] : (below ? k : v[j]));
        below = lt;
    }
    acc.st(1u, below ? k : v[J]);
}

template <int J, typename Ent, typename Acc>
LFM_HD inline void heap_insert_level(Acc& acc, uint32_t A)
{
    const uint32_t last = A < (2u << J) - 1u ? A : (2u << J) - 1u;
    for (uint32_t z = 1u << J; z <= last; ++z) heap_insert_at<J, Ent>(acc, z);
}

// all inserts of a heap of A <= 511 leaves (the leaf at position 1 is the heap of one)
template <typename Ent, typename Acc>
LFM_HD inline void heap_insert_levels(Acc& acc, uint32_t A)
{
    heap_insert_level<1, Ent>(acc, A);
    heap_insert_level<2, Ent>(acc, A);
    heap_insert_level<3, Ent>(acc, A);
    heap_insert_level<4, Ent>(acc, A);
    heap_insert_level<5, Ent>(acc, A);
    heap_insert_level<6, Ent>(acc, A);
    heap_insert_level<7, Ent>(acc, A);
    heap_insert_level<8, Ent>(acc, A);
}

// the bits of nodes 1 .. A / 2 from the entries, after the initial inserts
// (every other node's children are sentinels), eight pairs per round trip
template <typename Ent, typename Acc>
LFM_HD inline void heap_pref_build(Acc& acc, HeapPref& m, uint32_t A)
{
    const uint32_t last = A >> 1;
#pragma unroll
    for (uint32_t wi = 0; wi < (uint32_t)kPrefWords; ++wi) {
        uint32_t word = 0;
        for (uint32_t b0 = 0; b0 < 32u && 32u * wi + b0 <= last; b0 += 8u) {
            Ent l[8], r[8];
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) {
                const uint32_t p = 32u * wi + b0 + q;
                acc.ld_pair(2u * (p <= last ? p : last), l[q], r[q]);
            }
            acc.fence();
#pragma unroll
            for (uint32_t q = 0; q < 8u; ++q) {
                const uint32_t p = 32u * wi + b0 + q;
                word |= (p >= 1u && p <= last && heap_wless(r[q], l[q]) ? 1u : 0u) << (b0 + q);
            }
        }
        m.w[wi] = word;
    }
}

// Downheap from the root with key k over L levels (the heap holds fewer than
// 2^(L + 1) entries); returns the new root.
template <int L, typename Ent, typename Acc>
LFM_HD inline Ent heap_sift_path(Acc& acc, HeapPref& m, Ent k)
{
    if constexpr (L == 0) {
        acc.st(1u, k);
        acc.note_sift(0u, 0u);
        return k;
    } else {
        // p[j]: the path; cb[j]: the children pair of p[j] (clamped past the
        // array: level 7 only); p[j + 1] = cb[j] + r[j]
        uint32_t p[L + 1], cb[L], r[L];
        p[0] = 1u;
#pragma unroll
        for (int j = 0; j < L; ++j) {
            r[j] = heap_pref_at(m, j, p[j]);
            cb[j] = 2u * p[j];
            if (j == 7) cb[j] = cb[j] < kHeapSentPair ? cb[j] : kHeapSentPair;
            p[j + 1] = cb[j] | r[j];
        }
        Ent a[L], b[L];
#pragma unroll
        for (int j = 0; j < L; ++j) acc.ld_pair(cb[j], a[j], b[j]);
        acc.fence();
        const Ent kk = k | (Ent)1023;
        Ent c[L], sib[L], nv[L + 1];
        bool go[L];
        bool g = true;
        uint32_t went = 0;
#pragma unroll
        for (int j = 0; j < L; ++j) {
            c[j] = r[j] ? b[j] : a[j];
            sib[j] = r[j] ? a[j] : b[j];
            g = g && !(kk < c[j]);  // a sentinel child stops the walk
            go[j] = g;
            went += g ? 1u : 0u;
        }
        nv[0] = go[0] ? c[0] : k;
#pragma unroll
        for (int j = 1; j < L; ++j) nv[j] = go[j] ? c[j] : (go[j - 1] ? k : c[j - 1]);
        nv[L] = go[L - 1] ? k : c[L - 1];
#pragma unroll
        for (int j = 0; j <= L; ++j) acc.st(p[j], nv[j]);
        HeapPref d = {{0u, 0u, 0u, 0u, 0u}};  // r[j] is the bit pref[p[j]] holds
#pragma unroll
        for (int j = 0; j < L; ++j) {
            const Ent right = r[j] ? nv[j + 1] : sib[j], left = r[j] ? sib[j] : nv[j + 1];
            heap_pref_flip(d, j, p[j], r[j] ^ (heap_wless(right, left) ? 1u : 0u));
        }
#pragma unroll
        for (int i = 0; i < kPrefWords; ++i) m.w[i] ^= d.w[i];
        acc.note_sift(went, (uint32_t)L);
        return nv[0];
    }
}

// takes the heap's last entry out; returns it
template <typename Ent, typename Acc>
LFM_HD inline Ent heap_pop_last(Acc& acc, HeapPref& m, uint32_t& nHeap)
{
    const Ent last = acc.ld(nHeap);
    acc.st(nHeap, heap_sent<Ent>());
    heap_pref_set_any(m, nHeap >> 1, 0u);
    --nHeap;
    return last;
}

// Upheap of key k from position z; returns the final position.  Every
// position the climb changed (the final one included) has its parent's bit
// recomputed from its new entry and its sibling.  A merged node climbs 0.15
// levels on average, but the heaps walk in lockstep and some heap of the group
// nearly always climbs one: the first kPushAhead levels' ancestors and
// siblings are read in one round trip (a step writes only the position below
// the ones later steps read), the rare steps after them read their own.
constexpr int kPushAhead = 3;

template <typename Ent, typename Acc>
LFM_HD inline uint32_t heap_push(Acc& acc, HeapPref& m, uint32_t z, Ent k)
{
    constexpr Ent kW = ~(Ent)1023;
    const uint32_t from = z;
    Ent upa[kPushAhead], sba[kPushAhead];
#pragma unroll
    for (int t = 0; t < kPushAhead; ++t) {
        upa[t] = acc.ld(z >> (t + 1));
        sba[t] = acc.ld((z >> t) ^ 1u);
    }
    acc.fence();
    bool go = true;
    Ent up = upa[0], sib = sba[0];
    // one step with the parent and the sibling of z; a heap that stopped repeats its last step
    auto step = [&]() {
        go = go && k < (up & kW);  // the 0 at position 0 stops it
        const Ent v = go ? up : k;
        acc.st(z, v);
        if (z >= 2u) {
            const Ent right = z & 1u ? v : sib, left = z & 1u ? sib : v;
            heap_pref_set_any(m, z >> 1, heap_wless(right, left) ? 1u : 0u);
        }
        z = go ? z >> 1 : z;
        return acc.any(go);
    };
    bool more = step();
#pragma unroll
    for (int t = 1; t < kPushAhead; ++t) {
        if (!more) break;
        up = go ? upa[t] : up;
        sib = go ? sba[t] : sib;
        more = step();
    }
    for (int t = kPushAhead; more && t < kHeapMaxLevels + 1; ++t) {  // z < 512 reaches position 0 in nine steps
        up = acc.ld(z >> 1);
        sib = acc.ld(z ^ 1u);
        more = step();
    }
    acc.note_push(from, z);
    return z;
}

// One merge of BZ2_hbMakeCodeLengths: the two smallest nodes leave the heap
// (top is the root, kept in a register), their parent enters it.  L covers the
// heap after the first pop: 2^(L + 1) > nHeap - 1.
template <int L, typename Ent, typename Acc>
LFM_HD inline void heap_merge_step(Acc& acc, HeapPref& m, uint32_t& nHeap, uint32_t& nNodes, Ent& top, uint32_t& tooLong)
{
    const Ent k1 = top;
    const Ent l1 = heap_pop_last<Ent>(acc, m, nHeap);
    acc.check(m, nHeap);
    const Ent k2 = heap_sift_path<L, Ent>(acc, m, l1);
    acc.check(m, nHeap);
    const Ent l2 = heap_pop_last<Ent>(acc, m, nHeap);
    acc.check(m, nHeap);
    const Ent r2 = heap_sift_path<L, Ent>(acc, m, l2);
    acc.check(m, nHeap);
    ++nNodes;
    acc.set_parent((uint32_t)k1 & 1023u, nNodes);
    acc.set_parent((uint32_t)k2 & 1023u, nNodes);
    const uint32_t h1 = (uint32_t)(k1 >> 10) & 31u, h2 = (uint32_t)(k2 >> 10) & 31u;
    const uint32_t hm = h1 > h2 ? h1 : h2;
    const uint32_t h = hm + 1u < 30u ? hm + 1u : 30u;
    tooLong |= h > 17u ? 1u : 0u;
    const Ent kn = ((((k1 >> 15) + (k2 >> 15)) << 5 | (Ent)h) << 10) | (Ent)nNodes;
    ++nHeap;
    top = heap_push<Ent>(acc, m, nHeap, kn) == 1u ? kn : r2;
    acc.check(m, nHeap);
}

// levels of a heap of n >= 1 entries: floor(log2(n))
LFM_HD inline int heap_levels(uint32_t n)
{
    return 31 - __builtin_clz(n);
}

// the merge step of a heap group whose largest heap holds hmax > 1 entries
template <typename Ent, typename Acc>
LFM_HD inline void heap_merge_step_at(Acc& acc, HeapPref& m, uint32_t hmax, uint32_t& nHeap, uint32_t& nNodes, Ent& top,
                                      uint32_t& tooLong)
{
    switch (heap_levels(hmax - 1u)) {
    case 0: heap_merge_step<0, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    case 1: heap_merge_step<1, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    case 2: heap_merge_step<2, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    case 3: heap_merge_step<3, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    case 4: heap_merge_step<4, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    case 5: heap_merge_step<5, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    case 6: heap_merge_step<6, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    case 7: heap_merge_step<7, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    default: heap_merge_step<8, Ent>(acc, m, nHeap, nNodes, top, tooLong); break;
    }
}

// All merges of one heap of A entries, walked as a member of a group whose
// largest heap holds hmax >= A entries.
template <typename Ent, typename Acc>
LFM_HD inline void heap_merge_all(Acc& acc, HeapPref& m, uint32_t A, uint32_t hmax, uint32_t& nNodes, uint32_t& tooLong)
{
    uint32_t nHeap = A;
    Ent top = acc.ld(1u);
    for (uint32_t it = 0; it + 1u < hmax; ++it)
        if (nHeap > 1u) heap_merge_step_at<Ent>(acc, m, hmax - it, nHeap, nNodes, top, tooLong);
}
