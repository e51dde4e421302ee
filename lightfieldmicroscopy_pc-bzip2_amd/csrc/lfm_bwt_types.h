// Word-level classifier of the two-stage BWT's rotation types, for the bucket
// pass (bwt_bucket) and, on the host, for its stand-alone test
// (tests/c/bwt_types_main.cpp).  No HIP, no allocation: plain integer code.
//
// Rotation i of a text T is of type B when it sorts before rotation i + 1:
// T[i] < T[i + 1], or equal bytes and i + 1 of type B; else of type A.  The
// bucket pass decides a type from at most 8 comparisons (9 bytes); a rotation
// that starts 9 equal bytes is "undecided" and sends its stream through the
// sort whole.
//
// A lane holds a group of 8 consecutive positions k .. k + 7 and the 8 bytes
// after them, as two big-endian words: P = T[k .. k + 7] with T[k] in the top
// byte, Q = T[k + 8 .. k + 15] likewise.  Every mask below carries one flag
// per position, at bit 7 of that position's byte of P (position k + j: bit
// 63 - 8 j).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LFM_HD __host__ __device__
#else
#define LFM_HD
#endif

constexpr uint64_t kByteFlags = 0x8080808080808080ull, kByteLow7 = 0x7F7F7F7F7F7F7F7Full;

// flag where byte of x < byte of y (unsigned).  (x | 0x80) - (y & 0x7f) never
// borrows from the next byte; its bit 7 says low7(x) >= low7(y).
LFM_HD inline uint64_t bytes_lt(uint64_t x, uint64_t y)
{
    const uint64_t t = (x | kByteFlags) - (y & kByteLow7);
    return ((~x & y) | (~(x ^ y) & ~t)) & kByteFlags;
}

// flag where byte of x == byte of y
LFM_HD inline uint64_t bytes_eq(uint64_t x, uint64_t y)
{
    const uint64_t z = x ^ y;
    return ~(((z & kByteLow7) + kByteLow7) | z) & kByteFlags;
}

// flags of the group's first `valid` positions (1 .. 8)
LFM_HD inline uint64_t group_valid(uint32_t valid)
{
    return valid < 8u ? kByteFlags & ~(~0ull >> (8u * valid)) : kByteFlags;
}

struct BwtTypes {
    uint64_t lt;         // T[k + j] <  T[k + j + 1]
    uint64_t eq;         // T[k + j] == T[k + j + 1]
    uint64_t b;          // rotation k + j is of type B (meaningless where undecided)
    uint32_t undecided;  // one of the first `valid` positions starts 9 equal bytes
};

// The types of positions k .. k + 7.  B[j] = lt[j] | (eq[j] & B[j + 1]) is the
// carry recurrence of an addition that runs from position k + 7 down to k: in
// a big-endian word that is from P's low byte up to its top byte.  With the
// low 7 bits of every byte set in one addend, a carry into a byte reaches its
// bit 7, where lt generates and eq propagates: the carry into bit 7 is
// B[j + 1], and it is read back as sum ^ addends.  The carry into the word is
// the type of position k + 8 as far as the lookahead decides it: T[k + 8 ..
// k + 14] against T[k + 9 .. k + 15] as strings, one comparison of 56-bit
// big-endian integers.  What lies past k + 15 can reach a position of the
// group only through 8 equal bytes, which `undecided` reports.
LFM_HD inline BwtTypes bwt_types8(uint64_t P, uint64_t Q, uint32_t valid)
{
    BwtTypes r;
    const uint64_t y = (P << 8) | (Q >> 56);
    r.lt = bytes_lt(P, y);
    r.eq = bytes_eq(P, y);
    const uint64_t q0 = Q >> 8, q1 = Q & 0x00FFFFFFFFFFFFFFull;
    const uint64_t s = (r.lt | r.eq | kByteLow7) + r.lt + (q0 < q1 ? 1u : 0u);
    r.b = r.lt | (r.eq & ~s);
    // a: equal flags in a row ending at position k + 7; e: in a row from k + 8
    // (7 at the most).  Position k + j starts 9 equal bytes iff 8 - a <= j <= e.
    const uint64_t ne = ~r.eq & kByteFlags, z = q0 ^ q1;
    const uint32_t a = ne ? (uint32_t)__builtin_ctzll(ne) >> 3 : 8u;
    const uint32_t e = z ? ((uint32_t)__builtin_clzll(z) >> 3) - 1u : 7u;
    const uint32_t last = valid - 1u < e ? valid - 1u : e;
    r.undecided = 8u - a <= last ? 1u : 0u;
    return r;
}

// The byte loop the words replace: 1 = B, 0 = A, 2 = undecided after 8 equal
// bytes; w[0 .. 8] are the rotation's first 9 bytes.  Kept as the reference
// of the classifier's test.
LFM_HD inline uint32_t bwt_type_bytes(const uint8_t* w)
{
    for (uint32_t d = 0; d < 8; ++d)
        if (w[d] != w[d + 1]) return w[d] < w[d + 1] ? 1u : 0u;
    return 2u;
}
