// Stand-alone check of the bucket pass's word-level rotation classifier
// (csrc/lfm_bwt_types.h) against the byte loop it replaces, on the host.
// Built and run by tests/test_bwt_bucket_lanes_cpu.py; never loaded into
// Python.  Prints "ok <groups> <undecided>" and exits 0, or the first
// mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lfm_bwt_types.h"

static uint64_t g_groups = 0, g_undecided = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;

static uint32_t rnd(uint32_t m)
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)((g_rng >> 20) % m);
}

static uint64_t be8(const std::vector<uint8_t>& T, size_t i)
{
    uint64_t w = 0;
    for (size_t d = 0; d < 8; ++d) w = (w << 8) | T[(i + d) % T.size()];
    return w;
}

// every group of 8 positions that starts at `phase` mod 8, types cyclic over
// the wrap n - 1 -> 0; the last group of a pass is cut at n (valid < 8)
static bool check_text(const std::vector<uint8_t>& T, const char* what)
{
    const size_t n = T.size();
    for (size_t phase = 0; phase < 8 && phase < n; ++phase) {
        for (size_t k = phase; k < n; k += 8) {
            const uint32_t valid = (uint32_t)(n - k < 8 ? n - k : 8);
            const BwtTypes r = bwt_types8(be8(T, k), be8(T, k + 8), valid);
            ++g_groups;
            uint32_t und = 0;
            uint32_t want[8];
            for (uint32_t j = 0; j < valid; ++j) {
                uint8_t w[9];
                for (uint32_t d = 0; d < 9; ++d) w[d] = T[(k + j + d) % n];
                want[j] = bwt_type_bytes(w);
                und |= want[j] == 2u;
            }
            g_undecided += und;
            bool bad = r.undecided != und;
            for (uint32_t j = 0; j < valid && !bad; ++j) {
                const uint32_t x = T[(k + j) % n], y = T[(k + j + 1) % n];
                const uint32_t sh = 63u - 8u * j;
                bad |= ((r.lt >> sh) & 1u) != (x < y ? 1u : 0u);
                bad |= ((r.eq >> sh) & 1u) != (x == y ? 1u : 0u);
                if (want[j] != 2u) bad |= ((r.b >> sh) & 1u) != want[j];
            }
            if ((r.lt | r.eq | r.b) & ~kByteFlags) bad = true;
            if (bad) {
                std::printf("mismatch: %s n %zu group at %zu valid %u undecided %u (want %u)\n", what, n, k, valid,
                            r.undecided, und);
                return false;
            }
        }
    }
    return true;
}

int main()
{
    // the byte-wise comparisons, every pair of bytes in every byte lane
    for (uint32_t x = 0; x < 256; ++x)
        for (uint32_t y = 0; y < 256; ++y) {
            const uint64_t X = 0x0101010101010101ull * x, Y = 0x0101010101010101ull * y;
            if (bytes_lt(X, Y) != (x < y ? kByteFlags : 0) || bytes_eq(X, Y) != (x == y ? kByteFlags : 0)) {
                std::printf("mismatch: bytes %u %u\n", x, y);
                return 1;
            }
            // a lane's result does not depend on its neighbours
            const uint64_t M = 0x00FF00FF00FF00FFull;
            if (bytes_lt(X & M, Y & ~M) != (y ? kByteFlags & ~M : 0) ||
                bytes_eq(X & M, Y & M) != ((kByteFlags & ~M) | (x == y ? kByteFlags & M : 0))) {
                std::printf("mismatch: mixed lanes %u %u\n", x, y);
                return 1;
            }
        }
    for (uint32_t v = 1; v <= 8; ++v)
        if (__builtin_popcountll(group_valid(v)) != (int)v || (group_valid(v) >> (63 - 8 * (v - 1)) & 1) != 1) return 1;

    std::vector<uint8_t> T;
    // random texts, alphabets of 2, 3, 4, 16 and 256 symbols, lengths 1 .. 300
    const uint32_t alphabets[5] = {2, 3, 4, 16, 256};
    for (uint32_t it = 0; it < 4000; ++it) {
        const uint32_t a = alphabets[it % 5], n = 1 + rnd(300);
        T.resize(n);
        for (auto& c : T) c = (uint8_t)(rnd(a) * (it & 1 && a < 256 ? 255 / (a - 1) : 1));
        if (!check_text(T, "random")) return 1;
    }
    // 16-bit little-endian symbols, small values (the encoder's usual text)
    for (uint32_t it = 0; it < 200; ++it) {
        const uint32_t n = 2 + rnd(400);
        T.resize(n);
        for (uint32_t i = 0; i < n; ++i) T[i] = i & 1 ? (uint8_t)(rnd(16) == 0) : (uint8_t)rnd(40);
        if (!check_text(T, "symbols")) return 1;
    }
    // equal runs of 2 .. 12 bytes ending at every offset of a group, ascending
    // and descending after the run, in the text and across the wrap
    for (uint32_t run = 2; run <= 12; ++run)
        for (uint32_t end = 0; end < 8; ++end)
            for (uint32_t after = 0; after < 2; ++after)
                for (uint32_t wrap = 0; wrap < 2; ++wrap) {
                    const uint32_t n = 64;
                    T.resize(n);
                    for (uint32_t i = 0; i < n; ++i) T[i] = (uint8_t)(1 + (i * 37 + (i >> 2)) % 200);
                    // the run's last byte at position `last`
                    const uint32_t last = wrap ? end : 32 + end;
                    const uint8_t c = 100;
                    for (uint32_t d = 0; d < run; ++d) T[(last + n - d) % n] = c;
                    T[(last + 1) % n] = after ? c + 1 : c - 1;
                    T[(last + n - run) % n] = after ? c - 3 : c + 3;
                    if (!check_text(T, "run")) return 1;
                }
    // constant texts and texts of one long run (every position undecided)
    for (uint32_t n = 1; n <= 40; ++n) {
        T.assign(n, 0xFB);
        if (!check_text(T, "constant")) return 1;
        T[n / 2] = 3;
        if (!check_text(T, "one other byte")) return 1;
    }
    std::printf("ok %llu %llu\n", (unsigned long long)g_groups, (unsigned long long)g_undecided);
    return g_undecided ? 0 : 1;
}
