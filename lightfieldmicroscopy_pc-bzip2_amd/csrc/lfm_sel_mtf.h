// The selector move-to-front of huff_final as a prefix problem and, on the
// host, of its stand-alone test (tests/c/sel_mtf_main.cpp).  No HIP, no
// allocation: plain integer code over a byte accessor.
//
// compress.c moves each selector to the front of a list of the nGroups <= 6
// tables and sends its old position.  A list is one word of 4-bit entries,
// entry i in nibble i, 0x543210 at the start; a nibble of 15 is an empty slot,
// and the empty slots come last.
//
// A run of selectors acts on any list as "its distinct symbols by last
// occurrence, most recent first, then the list without them".  That prefix is
// the run's summary: the list the run leaves when it starts from six empty
// slots (a symbol that is not found takes the first empty slot's place).  The
// count of a summary is the number of its nibbles that are not 15.
//
// Summaries compose associatively: the later run's symbols first, then the
// earlier run's without them, which is the later summary's symbols moved to
// the front of the earlier one, least recent first.  A full list is a summary
// of six, so the same compose puts a summary on top of a starting list.
//
// The scan: lane l of a wave owns selectors [l * C, (l + 1) * C) of a pass of
// 64 * C.  It summarises them, an inclusive scan composes the summaries on top
// of the carry (lane 0 takes the previous pass's last list, 0x543210 in the
// first pass), lane l starts from lane l - 1's result and replays its chunk
// for the positions.  selmtf_scan_host walks the same steps over arrays.
#pragma once
#include <cstdint>

#ifndef LFM_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFM_HD __host__ __device__
#else
#define LFM_HD
#endif
#endif

constexpr uint32_t kSelMtfStart = 0x543210u;  // entry i in nibble i
constexpr uint32_t kSelMtfEmpty = 0xFFFFFFu;  // six empty slots: the summary of no selector
constexpr uint32_t kSelMtfLanes = 64;

// bit 4 i + 3 for a zero nibble i of x's low six (x < 2^24).  Only the lowest
// set bit is exact (a borrow can mark nibbles above the first zero one), and
// only that one is used.  The callers add bit 23, which ends a search that
// finds nothing: never the case for a selector below nGroups.
LFM_HD inline uint32_t selmtf_zero_nibbles(uint32_t x)
{
    return (x - 0x111111u) & ~x & 0x888888u;
}

// moves the entry at position j to the front with value ll
LFM_HD inline uint32_t selmtf_front(uint32_t list, uint32_t j, uint32_t ll)
{
    const uint32_t m = (1u << (4u * (j + 1u))) - 1u;
    return (list & ~m) | (((list << 4) | ll) & m);
}

// One step on a full list (every table below nGroups is in it): the position
// of ll, which goes to the front.
LFM_HD inline uint32_t selmtf_step(uint32_t& list, uint32_t ll)
{
    const uint32_t z = selmtf_zero_nibbles(list ^ (ll * 0x111111u)) | 0x800000u;
    const uint32_t j = (uint32_t)__builtin_ctz(z) >> 2;
    list = selmtf_front(list, j, ll);
    return j;
}

// One step on a list with empty slots: ll goes to the front from where it is,
// or from the first empty slot.  One of the two exists: a list of six entries
// holds every symbol.
LFM_HD inline void selmtf_step_any(uint32_t& list, uint32_t ll)
{
    const uint32_t z = selmtf_zero_nibbles(list ^ (ll * 0x111111u)) | selmtf_zero_nibbles(~list & 0xFFFFFFu) | 0x800000u;
    list = selmtf_front(list, (uint32_t)__builtin_ctz(z) >> 2, ll);
}

LFM_HD inline uint32_t selmtf_count(uint32_t summary)
{
    uint32_t n = 0;
#pragma unroll
    for (uint32_t i = 0; i < 6u; ++i) n += ((summary >> (4u * i)) & 15u) != 15u ? 1u : 0u;
    return n;
}

// summary of selectors get(0) .. get(n - 1), walked as a chunk of C >= n
template <typename Get>
LFM_HD inline uint32_t selmtf_summary(Get get, uint32_t n, uint32_t C)
{
    uint32_t list = kSelMtfEmpty;
#pragma unroll
    for (uint32_t g = 0; g < C; ++g) {
        uint32_t next = list;
        selmtf_step_any(next, get(g) & 7u);
        list = g < n ? next : list;
    }
    return list;
}

// the summary (or list) of `earlier` followed by the run that `later` sums up
LFM_HD inline uint32_t selmtf_compose(uint32_t earlier, uint32_t later)
{
    uint32_t list = earlier;
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        const uint32_t ll = (later >> (4 * i)) & 15u;
        uint32_t next = list;
        selmtf_step_any(next, ll);
        list = ll != 15u ? next : list;
    }
    return list;
}

// positions of selectors get(0) .. get(n - 1) from the full list `list`, to
// put(g, position); put(g, 0) for the rest of the chunk of C.  Returns the
// list after them.
template <typename Get, typename Put>
LFM_HD inline uint32_t selmtf_replay(uint32_t list, Get get, Put put, uint32_t n, uint32_t C)
{
#pragma unroll
    for (uint32_t g = 0; g < C; ++g) {
        uint32_t next = list;
        const uint32_t j = selmtf_step(next, get(g) & 7u);
        list = g < n ? next : list;
        put(g, g < n ? j : 0u);
    }
    return list;
}

// selectors of a lane's chunk in a pass that starts at selector i0 of nSel
LFM_HD inline uint32_t selmtf_chunk_count(uint32_t nSel, uint32_t i0, uint32_t lane, uint32_t C)
{
    const uint32_t b = i0 + lane * C;
    return b >= nSel ? 0u : (nSel - b < C ? nSel - b : C);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The scan as huff_final runs it, lane by lane over arrays (host only): the
// positions of sel[0 .. nSel) to out, chunks of C selectors per lane, in a
// wave of `lanes` (a power of two; the kernel's is kSelMtfLanes).
// `passes_with_carry`, `chunks_of_six`, `chunks_of_one` count what it met
// (chunks_of_one: a chunk of two or more selectors, all equal).
struct SelMtfMet {
    uint64_t passes_with_carry = 0, chunks_of_six = 0, chunks_of_one = 0;
};

inline void selmtf_scan_host(const uint8_t* sel, uint8_t* out, uint32_t nSel, uint32_t C, SelMtfMet* met = nullptr,
                             uint32_t lanes = kSelMtfLanes)
{
    uint32_t carry = kSelMtfStart;
    for (uint32_t i0 = 0; i0 < nSel; i0 += lanes * C) {
        uint32_t incl[kSelMtfLanes], n[kSelMtfLanes];
        for (uint32_t l = 0; l < lanes; ++l) {
            n[l] = selmtf_chunk_count(nSel, i0, l, C);
            const uint8_t* p = sel + i0 + l * C;
            const uint32_t nl = n[l];
            const uint32_t sum = selmtf_summary([&](uint32_t g) { return g < nl ? (uint32_t)p[g] : 7u; }, nl, C);
            if (met) {
                met->chunks_of_six += selmtf_count(sum) == 6u;
                met->chunks_of_one += nl >= 2u && selmtf_count(sum) == 1u;
            }
            incl[l] = l == 0 ? selmtf_compose(carry, sum) : sum;
        }
        if (met && i0) ++met->passes_with_carry;
        for (uint32_t d = 1; d < lanes; d <<= 1) {  // what the wave does with shuffles
            uint32_t prev[kSelMtfLanes];
            for (uint32_t l = 0; l < lanes; ++l) prev[l] = l >= d ? incl[l - d] : 0u;
            for (uint32_t l = d; l < lanes; ++l) incl[l] = selmtf_compose(prev[l], incl[l]);
        }
        for (uint32_t l = 0; l < lanes; ++l) {
            const uint8_t* p = sel + i0 + l * C;
            uint8_t* o = out + i0 + l * C;
            const uint32_t nl = n[l];
            selmtf_replay(l ? incl[l - 1] : carry, [&](uint32_t g) { return g < nl ? (uint32_t)p[g] : 7u; },
                          [&](uint32_t g, uint32_t j) { if (g < nl) o[g] = (uint8_t)j; }, nl, C);
        }
        carry = incl[lanes - 1];
    }
}
#endif
