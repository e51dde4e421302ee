// Stand-alone check of csrc/lfm_sel_mtf.h (the selector move-to-front of
// huff_final as a scan of run summaries) against the serial move-to-front of
// compress.c.  Built and run by tests/test_huff_tail_cpu.py.
//
//   * every selector sequence of length 0 .. 7 over six symbols, in chunks of
//     1, 2 and 3 over a wave of eight lanes (every 64th over the 64 lanes the
//     kernel has), and its summary against a direct restatement (distinct
//     symbols by last occurrence, most recent first);
//   * random sequences up to 18 002 selectors over 2 .. 6 tables;
//   * every chunk length 1 .. 64 at stream lengths one below, at and one above
//     each multiple of the wave pass (64 chunks);
//   * associativity of the compose on random triples of summaries.
// It fails if it never met a chunk that holds all six symbols, a chunk of one
// repeated symbol, or a carry across a pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lfm_sel_mtf.h"

static SelMtfMet met;
static uint64_t n_seq = 0, n_triples = 0;

[[noreturn]] static void die(const char* what, long a = 0, long b = 0, long c = 0)
{
    std::printf("FAIL %s (%ld, %ld, %ld)\n", what, a, b, c);
    std::exit(1);
}

// compress.c: pos[] = 0 .. nGroups - 1; each selector moves to the front
static void ref_mtf(const uint8_t* sel, uint8_t* out, uint32_t n, int nGroups)
{
    uint8_t pos[6];
    for (int i = 0; i < nGroups; ++i) pos[i] = (uint8_t)i;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t ll_i = sel[i];
        int j = 0;
        uint8_t tmp = pos[j];
        while (ll_i != tmp) {
            j++;
            const uint8_t tmp2 = tmp;
            tmp = pos[j];
            pos[j] = tmp2;
        }
        pos[0] = tmp;
        out[i] = (uint8_t)j;
    }
}

// the summary, restated: distinct symbols by last occurrence, most recent first
static uint32_t ref_summary(const uint8_t* sel, uint32_t n)
{
    uint32_t list = kSelMtfEmpty, k = 0;
    bool seen[6] = {false, false, false, false, false, false};
    for (uint32_t i = n; i-- > 0;) {
        if (seen[sel[i]]) continue;
        seen[sel[i]] = true;
        list = (list & ~(15u << (4 * k))) | ((uint32_t)sel[i] << (4 * k));
        ++k;
    }
    return list;
}

static uint32_t summary_of(const uint8_t* sel, uint32_t n, uint32_t C)
{
    return selmtf_summary([&](uint32_t g) { return g < n ? (uint32_t)sel[g] : 7u; }, n, C);
}

static void check_stream(const uint8_t* sel, uint32_t n, int nGroups, uint32_t C, uint32_t lanes = kSelMtfLanes)
{
    static std::vector<uint8_t> want, got;
    want.assign(n + 1, 0xEE);
    got.assign(n + 1, 0xEE);
    ref_mtf(sel, want.data(), n, nGroups);
    selmtf_scan_host(sel, got.data(), n, C, &met, lanes);
    if (got[n] != 0xEE) die("the scan wrote past the stream", (long)n, (long)C);
    if (std::memcmp(want.data(), got.data(), n)) {
        uint32_t i = 0;
        while (want[i] == got[i]) ++i;
        die("position differs from the serial move-to-front", (long)n, (long)C, (long)i);
    }
    ++n_seq;
}

static uint64_t rng_state = 0x4C464D53ull;
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// selectors as the encoder makes them: runs of one table, sometimes long
static void draw(std::vector<uint8_t>& s, uint32_t n, int nGroups, uint32_t stay)
{
    s.resize(n + 1);
    uint8_t cur = (uint8_t)(rnd() % (uint32_t)nGroups);
    for (uint32_t i = 0; i < n; ++i) {
        if (rnd() % (stay + 1u) == 0) cur = (uint8_t)(rnd() % (uint32_t)nGroups);
        s[i] = cur;
    }
}

int main()
{
    // every sequence of length 0 .. 7 over six symbols
    for (uint32_t n = 0; n <= 7; ++n) {
        uint32_t total = 1;
        for (uint32_t i = 0; i < n; ++i) total *= 6;
        for (uint32_t code = 0; code < total; ++code) {
            uint8_t s[8];
            uint32_t c = code;
            for (uint32_t i = 0; i < n; ++i) {
                s[i] = (uint8_t)(c % 6);
                c /= 6;
            }
            const uint32_t want = ref_summary(s, n);
            for (uint32_t C = n ? n : 1; C <= 8; ++C)
                if (summary_of(s, n, C) != want) die("summary differs from its restatement", (long)n, (long)code, (long)C);
            if (selmtf_count(want) > n) die("summary count", (long)n, (long)code);
            // a summary on top of a list: the list the serial walk leaves
            uint32_t list = kSelMtfStart;
            for (uint32_t i = 0; i < n; ++i) selmtf_step(list, s[i]);
            if (selmtf_compose(kSelMtfStart, want) != list) die("summary applied to the start list", (long)n, (long)code);
            for (uint32_t C = 1; C <= 3; ++C) check_stream(s, n, 6, C, 8);  // a wave of eight lanes holds them
            if (code % 64u == 0) check_stream(s, n, 6, 1 + code / 64u % 8u);
        }
    }
    std::vector<uint8_t> s;
    // every chunk length at the seams of the wave pass
    for (uint32_t C = 1; C <= 64; ++C) {
        const uint32_t pass = kSelMtfLanes * C;
        for (uint32_t mult = 1; mult <= 3; ++mult)
            for (int d = -1; d <= 1; ++d) {
                const uint32_t n = mult * pass + (uint32_t)d;
                const int nGroups = 2 + (int)(rnd() % 5u);
                draw(s, n, nGroups, (C + mult) % 3u == 0 ? 40u : (C + mult) % 3u);
                check_stream(s.data(), n, nGroups, C);
            }
        // and at the lane chunk's own seams
        for (uint32_t n : {C - 1u, C, C + 1u, 2u * C, 63u * C + 1u}) {
            draw(s, n, 6, 1);
            check_stream(s.data(), n, 6, C);
        }
    }
    // random streams up to 18 002 selectors (900 000 symbols + EOB at 50 per selector)
    for (int rep = 0; rep < 400; ++rep) {
        const int nGroups = 2 + rep % 5;
        const uint32_t n = rep < 10 ? 18002u - (uint32_t)rep : 1u + rnd() % 18002u;
        const uint32_t Cs[4] = {16u, 32u, 1u + rnd() % 64u, 64u};
        draw(s, n, nGroups, rep % 4 == 0 ? 0u : rnd() % 60u);
        check_stream(s.data(), n, nGroups, Cs[rep % 4]);
    }
    // one table only, and two alternating
    for (uint32_t C : {1u, 31u, 32u, 33u}) {
        s.assign(5000, 3);
        check_stream(s.data(), 4999, 6, C);
        for (uint32_t i = 0; i < 5000; ++i) s[i] = (uint8_t)(i & 1u ? 4 : 1);
        check_stream(s.data(), 4999, 5, C);
    }
    // the compose is associative: summaries of random runs, short ones mostly
    for (int rep = 0; rep < 200000; ++rep) {
        uint32_t sum[3];
        uint8_t all[3 * 12];
        uint32_t total = 0;
        for (int k = 0; k < 3; ++k) {
            const uint32_t n = rnd() % (rep % 5 == 0 ? 12u : 4u);
            for (uint32_t i = 0; i < n; ++i) all[total + i] = (uint8_t)(rnd() % 6u);
            sum[k] = ref_summary(all + total, n);
            total += n;
        }
        const uint32_t left = selmtf_compose(selmtf_compose(sum[0], sum[1]), sum[2]);
        const uint32_t right = selmtf_compose(sum[0], selmtf_compose(sum[1], sum[2]));
        if (left != right) die("compose is not associative", (long)sum[0], (long)sum[1], (long)sum[2]);
        if (left != ref_summary(all, total)) die("compose differs from the summary of the joined runs", (long)rep);
        ++n_triples;
    }
    std::printf("ok sequences %llu triples %llu six %llu one %llu carry %llu\n", (unsigned long long)n_seq,
                (unsigned long long)n_triples, (unsigned long long)met.chunks_of_six, (unsigned long long)met.chunks_of_one,
                (unsigned long long)met.passes_with_carry);
    if (!met.chunks_of_six || !met.chunks_of_one || !met.passes_with_carry) die("a premise of the test was never met");
    return 0;
}
