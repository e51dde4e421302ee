// lfm_bzip2.hip -- block-parallel bzip2 (libbzip2 1.0.6 byte-exact) on gfx950.
//
// The .lfm writer compresses every 5-D block as its own bzip2 stream at
// level min(9, ceil(blockBytes / 1e5)) with workFactor 30
// (klb_imageIO.cpp:108, :217).  For a default 96x96x8 uint16 block that is
// one bzip2 block per stream, and a config-3 stack has 3 872 of them: the
// unit of parallelism here is the stream.  Every stage reproduces the
// published bzip2-1.0.6 algorithm (vendored at src/external/bzip2-1.0.6 of the
// reference; restated, not copied):
//
//   rle1    gather_blocks, rle1_crc: bzlib.c ADD_CHAR_TO_BLOCK / add_pair_to_block:
//           runs of 4..255 equal bytes -> 4 bytes + (len-4); block CRC
//           (MSB-first CRC-32, poly 0x04c11db7) over the raw bytes; inUse map.
//           One workgroup per stream: per-thread chunks, a scan carries the
//           run state across chunks, CRCs of chunks are combined with GF(2)
//           shift matrices.
//   BWT     blocksort.c sorts the cyclic rotations of the RLE1 block (the
//           order is unique for a non-periodic block, so any correct sort
//           gives libbzip2's bytes).  Two stages: the rotations of one type
//           are sorted (bwt_bucket, chunk sorts by the 8-byte prefix, text
//           rounds over what still ties; prefix doubling over every rotation
//           only for long repeats), the others placed by one induction scan
//           (the sorts' own placement or bwt_place_sorted, then bwt_induce).  A periodic block (equal
//           rotations) is handed back to the host library.
//   mtf     compress.c generateMTFValues: move-to-front per 4096-symbol
//           segment (mtf_last, mtf_prefix, mtf_win), then RUNA/RUNB zero runs
//           and the symbol frequencies (rle2).
//   huffman compress.c sendMTFValues + huffman.c: table count by nMTF,
//           initial partition, 4 refinement passes (selector per 50
//           symbols: first minimum cost; BZ2_hbMakeCodeLengths with
//           maxLen 17 and its weight-halving retry), selector MTF, codes.
//   emit    the bit stream: "BZh" + level, block magic, CRC, origPtr,
//           mapping table, selectors, delta-coded lengths, the symbols,
//           end magic and combined CRC; MSB-first bits.  Symbol codes are
//           written by all threads at prefix-summed bit offsets; the streams
//           are then compacted into the payload.
//
// A stream whose RLE1 text reaches nblockMAX = 100000 * level - 19 is several
// bzip2 blocks in libbzip2 (every block above ~900 kB; smaller ones whose data
// grows under RLE1).  lfm_hip_bzip2_blocks_multi gives a stream max_parts
// slots of the batch, one per bzip2 block ("part"): rle1_crc<.., MULTI> writes
// the text uncut, finds the cuts as libbzip2 does and the parts' CRCs,
// place_parts copies every part's text into its slot, BWT / MTF / Huffman run
// per slot as they do per stream, emit_stream<MULTI> writes a slot by role
// (stream header in the first only, no trailer) and join_parts concatenates
// the parts at bit offsets and adds the end magic and the combined CRC.  With
// max_parts == 1 it is lfm_hip_bzip2_blocks: one slot per stream, a stream
// that would need a second block flagged for the host library.  Periodic
// streams (any periodic part) are flagged too: the output stays
// byte-identical in every case.
#include <hip/hip_runtime.h>
#include <rocprim/block/block_exchange.hpp>
#include <rocprim/block/block_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>
#include "lfm_bwt_types.h"  // bwt_types8, bytes_eq, group_valid
#include "lfm_bz_caps.h"  // rle_cap, out_cap, sel_cap, kGSize, align_up, max_parts
#include "lfm_hip.h"
#include "lfm_huff_heap.h"  // the heap steps of huff_lengths_heap
#include "lfm_sel_mtf.h"    // the selector move-to-front of huff_final

#ifndef LFM_BWT_FORCE_FULL
#define LFM_BWT_FORCE_FULL 0  // timing variants: every rotation sorted, no induction
#endif

namespace lfm {
namespace bz {

constexpr int kRleThreads = 512;
constexpr int kMaxGroups = 6;
constexpr int kMaxAlpha = 258;
constexpr int kIters = 4;
constexpr uint32_t kRunA = 0, kRunB = 1;

// flags
constexpr uint32_t kFlagHost = 1;  // compress this stream with the host library

struct Geometry {
    uint32_t dims[5];   // x y z c t
    uint32_t bs[5];     // block size (clamped)
    uint32_t nb[5];     // blocks per dim
    uint32_t bpp;
};

struct Batch {
    // inputs
    const uint8_t* img;      // symbols / pixels, image layout (device)
    Geometry g;
    uint32_t first_block;    // global id of stream 0 of this batch
    uint32_t nstreams;
    uint32_t raw_cap;        // bytes reserved per stream for the raw block
    uint32_t cap;            // elements reserved per stream for the RLE1 block
    uint32_t level;          // blockSize100k
    uint32_t nblock_max;     // 100000 * level - 19
    uint32_t out_cap;        // bytes reserved per stream for the compressed stream
    // work buffers (per stream s at s * cap, etc.)
    uint8_t* raw;
    uint32_t* raw_len;
    uint8_t* T;              // RLE1 blocks
    uint32_t* n;             // RLE1 length
    uint32_t* crc;           // finalised block CRC
    uint32_t* inuse;         // 8 words per stream
    uint32_t* flags;
    uint32_t* done;          // BWT finished
    uint64_t* keys_a;
    uint64_t* keys_b;
    uint32_t* vals_a;        // rotation start indices (input of a sort)
    uint32_t* sa;            // sorted rotation starts (output of a sort)
    uint32_t* rank;
    uint32_t* vals_b;        // sorted values of the compacted rounds
    uint32_t* cl0;           // slots of unresolved rotations (compacted)
    uint32_t* cl1;
    uint8_t* uflag;          // per slot / per compacted entry: still tied
    uint32_t* seg_begin;
    uint32_t* seg_end;
    uint16_t* mtfv;          // cap + 8 per stream (16-byte aligned rows)
    uint32_t* nmtf;
    uint32_t* mtf_freq;      // kMaxAlpha per stream
    uint32_t* orig_ptr;
    uint8_t* sel;            // selectors, sel_cap per stream
    uint8_t* sel_mtf;
    uint32_t sel_cap;
    uint32_t* nsel;
    uint32_t* ngroups;
    uint8_t* len;            // kMaxGroups * kMaxAlpha per stream
    uint32_t* code;          // kMaxGroups * kMaxAlpha per stream
    uint32_t* rfreq;         // kMaxGroups * kMaxAlpha per stream
    uint32_t* words;         // out_cap / 4 per stream, MSB-first bit words
    uint32_t* out_bytes;
    uint32_t* wide;          // (stream, table) tasks whose heap weights exceed 17 bits
    uint32_t* wide_cnt;
    // two-stage BWT (bwt_bucket, bwt_induce)
    uint32_t* nsub;          // rotations sorted per stream (the A or B rotations, or all of them)
    uint32_t* bwt_mode;      // per stream: kModeSortA / kModeSortB / kModeFull
    uint32_t* abcnt;         // per stream: A rotations per first byte [256], then B rotations [256]
    uint32_t* itab;          // per stream: tq, cs, cl, s0 [256] each (bwt_bucket, for the placement and bwt_induce)
    uint2* ent;              // bwt_induce's entries per compact scan index (the keys_a area: only the segmented sort and the tie rounds use it)
    uint32_t it_full;        // sort every rotation (no induction): the fallback for ties that need doubling
    // streams of several bzip2 blocks (lfm_hip_bzip2_blocks_multi): a stream
    // owns `parts` consecutive slots, one per bzip2 block ("part") libbzip2
    // would cut; every per-stream buffer above is then per slot (nstreams
    // slots) except raw / raw_len, which stay per stream.  parts == 1: a
    // stream is its slot and none of the fields below is used.
    uint32_t parts;
    uint32_t full_cap;       // bytes reserved per stream for the uncut RLE1 text
    uint8_t* Tfull;          // uncut RLE1 texts (rle1_crc), copied into the slots by place_parts
    uint32_t* part_toff;     // per slot: the part's offset in its stream's RLE1 text (its length: n)
    uint32_t* part_roff;     // per slot: the part's offset and length in the raw block
    uint32_t* part_rlen;
    uint32_t* out_bits;      // per slot: bits emit_stream wrote (stream header / block, no trailer)
    uint32_t* nparts;        // per stream: parts in use
    uint32_t* sflags;        // per stream: kFlagHost
    uint32_t* sbytes;        // per stream: bytes of the joined stream
    uint32_t* jwords;        // per stream: the joined stream, jcap bytes, MSB-first bit words
    uint32_t jcap;
    uint32_t pay_cap;        // bytes the payload reserves per stream: a longer joined stream goes to the host
};

// ------------------------------------------------------------- gather --
// Block id -> origin/size, x fastest (klb_imageIO.cpp:133-140); the block's
// bytes are gathered x fastest, then y, z, c, t (blockCompressor).
__device__ __forceinline__ void block_box(const Geometry& g, uint32_t id, uint32_t org[5], uint32_t sz[5])
{
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        const uint32_t q = id % g.nb[d];
        id /= g.nb[d];
        org[d] = q * g.bs[d];
        sz[d] = min(g.bs[d], g.dims[d] - org[d]);
    }
}

__global__ __launch_bounds__(256) void gather_blocks(Batch B)
{
    const uint32_t s = blockIdx.y;
    uint32_t org[5], sz[5];
    block_box(B.g, B.first_block + s, org, sz);
    const uint32_t rowb = sz[0] * B.g.bpp;
    const uint32_t nrows = sz[1] * sz[2] * sz[3] * sz[4];
    uint8_t* dst = B.raw + (size_t)s * B.raw_cap;
    for (uint32_t r = blockIdx.x; r < nrows; r += gridDim.x) {
        uint32_t q = r;
        const uint32_t y = q % sz[1]; q /= sz[1];
        const uint32_t z = q % sz[2]; q /= sz[2];
        const uint32_t c = q % sz[3]; q /= sz[3];
        const uint32_t t = q;
        const size_t src = ((((size_t)(org[4] + t) * B.g.dims[3] + (org[3] + c)) * B.g.dims[2] + (org[2] + z)) *
                                B.g.dims[1] + (org[1] + y)) * B.g.dims[0] + org[0];
        const uint8_t* sp = B.img + src * B.g.bpp;
        uint8_t* dp = dst + (size_t)r * rowb;
        for (uint32_t i = threadIdx.x; i < rowb; i += blockDim.x) dp[i] = sp[i];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) B.raw_len[s] = rowb * nrows;
}

// ----------------------------------------------------------- RLE1 + CRC --
// One workgroup per stream walks the raw block in tiles of kRleTile bytes,
// kRleChunk bytes per thread (two 16-byte loads, straight from the image when
// the block rows are 16-byte granular, else from the gathered raw block):
//   * run summary of the chunk (first / last byte, leading / trailing run),
//     scanned across the tile (wave shuffles, then the waves) on top of the
//     run carried in from the previous tiles: the bzip2 run state at the
//     chunk start (a run restarts every 255 bytes from its first byte);
//   * the chunk's RLE1 bytes (bzlib.c ADD_CHAR_TO_BLOCK / flush_RL) counted,
//     placed by a scan of the counts into an LDS copy of the tile's output and
//     stored with coalesced writes;
//   * the chunk CRC (slicing by 4, tables in LDS) from a zero register (the
//     stream's first chunk from 0xffffffff), combined over the tile by a tree
//     of GF(2) "shift by 32 << k zero bytes" matrices and folded into the
//     stream CRC; the tail of the last tile is zero padding, removed at the
//     end by the inverse shift (the CRC is linear: crc(D . 0^p) = Z^p crc(D));
//   * inUse: bytes present (register masks, OR-reduced once) and run-length
//     bytes (LDS atomics, rare).
// Run summary of a byte range, combined left to right by the scan.
struct RunSum {
    uint32_t len;    // bytes in the range (0 = identity)
    uint32_t first, last;
    uint32_t lead;   // length of the leading run
    uint32_t trail;  // length of the trailing run
};

// (selects, no early returns: the scans keep RunSums in registers)
__device__ __forceinline__ RunSum run_combine(const RunSum& a, const RunSum& b)
{
    const bool ae = a.len == 0, be = b.len == 0;
    const bool join = a.last == b.first && !ae && !be;
    RunSum r;
    r.len = a.len + b.len;
    r.first = ae ? b.first : a.first;
    r.last = be ? a.last : b.last;
    r.lead = ae ? b.lead : ((join && a.lead == a.len) ? a.len + b.lead : a.lead);
    r.trail = be ? a.trail : ((join && b.trail == b.len) ? b.len + a.trail : b.trail);
    return r;
}

__device__ __forceinline__ RunSum run_shfl_up(const RunSum& a, int d)
{
    RunSum r;
    r.len = __shfl_up(a.len, d);
    r.first = __shfl_up(a.first, d);
    r.last = __shfl_up(a.last, d);
    r.lead = __shfl_up(a.lead, d);
    r.trail = __shfl_up(a.trail, d);
    return r;
}

constexpr uint32_t kRleChunk = 32;
constexpr uint32_t kRleTile = kRleThreads * kRleChunk;  // 16 KiB
constexpr int kCrcLevels = 10;                          // shift by kRleChunk << k bytes, k = 0..9 (9: one tile)
constexpr int kCrcUnshift = 14;                         // inverse shift by 2^k bytes (padding < kRleTile)
static_assert(kRleTile == (kRleChunk << (kCrcLevels - 1)) && kRleTile == (1u << kCrcUnshift), "CRC tables");

__constant__ uint32_t c_crc4[4][256];  // 4 zero feeds of a register holding byte v at byte k
__constant__ uint32_t c_crc_unshift[kCrcUnshift][32];

// 32x32 GF(2) matrix as 32 columns (column k = image of bit k); m is a
// wave-uniform constant, so its columns are scalar loads
__device__ __forceinline__ uint32_t gf2_apply(const uint32_t* m, uint32_t v)
{
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) r ^= ((v >> k) & 1u) ? m[k] : 0u;
    return r;
}

// CRC shift by 32 << l zero bytes as byte tables: Z(v) = T[l][0][v & 255] ^
// T[l][1][(v >> 8) & 255] ^ T[l][2][(v >> 16) & 255] ^ T[l][3][v >> 24]
// (four LDS reads instead of a 32-column GF(2) product per lane)
__constant__ uint32_t c_crc_shb[kCrcLevels][4][256];

__device__ __forceinline__ uint32_t crc_shift_b(const uint32_t (*t)[256], uint32_t v)
{
    return t[0][v & 255u] ^ t[1][(v >> 8) & 255u] ^ t[2][(v >> 16) & 255u] ^ t[3][v >> 24];
}

// The bytes of a chunk as a bitmask: bit i set when byte i equals byte i - 1
// (bit 0 clear), i < nv, four bytes per word by a zero-byte test of
// w ^ (w << 8 | previous byte)
__device__ __forceinline__ uint32_t chunk_eq_mask(const uint32_t (&w)[kRleChunk / 4], uint32_t nv)
{
    uint32_t E = 0;
#pragma unroll
    for (uint32_t q = 0; q < kRleChunk / 4; ++q) {
        const uint32_t x = w[q], pb = q ? w[q - 1] >> 24 : x & 255u;
        const uint32_t y = x ^ ((x << 8) | pb);
        const uint32_t eq = ~((((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y)) & 0x80808080u;  // bit 7: byte equal
        const uint32_t e4 = ((eq >> 7) & 1u) | ((eq >> 14) & 2u) | ((eq >> 21) & 4u) | ((eq >> 28) & 8u);
        E |= e4 << (4 * q);
    }
    return E & ~1u & (nv >= 32 ? ~0u : (1u << nv) - 1u);
}

__device__ __forceinline__ uint32_t chunk_byte(const uint32_t (&w)[kRleChunk / 4], uint32_t i)
{
    uint32_t x = w[0];
#pragma unroll
    for (uint32_t q = 1; q < kRleChunk / 4; ++q) x = (i >> 2) == q ? w[q] : x;
    return (x >> (8 * (i & 3u))) & 255u;
}

// CRC register arithmetic for the part CRCs: the register is a polynomial
// over GF(2) mod 0x104c11db7 (bit k = x^k) and a zero byte fed is a
// multiplication by x^8, so Z^m(v) = v * x^(8 m).
__device__ inline uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t r = 0;
#pragma unroll 1
    for (int i = 31; i >= 0; --i) {
        r = (r << 1) ^ ((r >> 31) ? 0x04c11db7u : 0u);
        r ^= ((b >> i) & 1u) ? a : 0u;
    }
    return r;
}

__device__ inline uint32_t crc_xpow8(uint32_t m)  // x^(8 m)
{
    uint32_t r = 1u, b = 2u;
#pragma unroll 1
    for (uint64_t e = 8ull * m; e; e >>= 1) {
        if (e & 1u) r = crc_mul(r, b);
        b = crc_mul(b, b);
    }
    return r;
}

// MULTI (Batch::parts > 1): the text goes to Tfull uncut and the kernel finds
// the stream's parts as libbzip2 cuts them (bzlib.c copy_input_until_stop,
// handle_compress).  RLE1 works in pieces (a run of equal bytes, cut every 255)
// flushed into the block when the next input byte arrives, and nblock >=
// nblockMAX is tested before each input byte: a block ends in front of the
// first piece whose text position has reached nblockMAX past the block's start
// -- unless that piece is the stream's last byte, which libbzip2 has already
// read when it looks (it joins the block).  The run state survives a cut, so
// the parts' texts are consecutive ranges of the uncut text.  A tile holds
// less text than a block, so at most one cut falls in it.  The CRC register
// P(r) at a cut r comes from the chunk CRCs in front of it; a part [a, b)
// then has CRC ~(P(b) ^ Z^(b-a)(P(a) ^ ~0)) (the register is affine in its
// start value).
template <bool FROM_IMG, bool MULTI>
__global__ __launch_bounds__(kRleThreads) __attribute__((amdgpu_waves_per_eu(4))) void rle1_crc(Batch B)
{
    constexpr uint32_t NW = kRleThreads / 64;
    __shared__ uint32_t crc4[4][256];
    __shared__ uint32_t crcsh[kCrcLevels][4][256];
    // the tile's RLE1 bytes at tout[po ..), po = the stream offset mod 16:
    // tout[0 .. po) holds the previous tile's last partial 16-byte unit
    __shared__ __attribute__((aligned(16))) uint8_t tout[16 + kRleTile + kRleTile / 4 + 64];
    __shared__ uint8_t junk[kRleThreads];  // where a thread's skipped byte writes land
    __shared__ RunSum wrs[NW];
    __shared__ uint32_t wcnt[NW], wcrc[NW];
    __shared__ RunSum s_carry;
    __shared__ uint32_t s_wr, s_crc;
    __shared__ uint32_t s_ps, s_np, s_cut_r, s_cut_tp, s_red[NW];  // MULTI: the open part's text start and index, a tile's cut
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t org[5], sz[5];
    block_box(B.g, B.first_block + s, org, sz);
    const uint32_t rowb = sz[0] * B.g.bpp;
    const uint32_t L = rowb * sz[1] * sz[2] * sz[3] * sz[4];
    const uint8_t* raw = B.raw + (size_t)s * B.raw_cap;
    // divisions by the block's row bytes and extents: float reciprocal and
    // one correction step (exact for x < 2^23, integer division above): a
    // 32-bit integer division is ~40 instructions, four per load
    struct FDiv {
        uint32_t d;
        float inv;
        __device__ __forceinline__ uint32_t div(uint32_t x) const
        {
            if (x >= (1u << 23)) return x / d;  // (huge blocks only)
            uint32_t q = (uint32_t)((float)x * inv);
            const int32_t r = (int32_t)(x - q * d);
            q += r >= (int32_t)d ? 1u : 0u;
            q -= r < 0 ? 1u : 0u;
            return q;
        }
    };
    const FDiv frow{rowb, 1.0f / (float)rowb}, fy{sz[1], 1.0f / (float)sz[1]}, fz{sz[2], 1.0f / (float)sz[2]},
        fc{sz[3], 1.0f / (float)sz[3]};
    auto load16 = [&](uint32_t g) -> uint4 {
        if (FROM_IMG) {  // rows are whole 16-byte pieces at 16-byte aligned addresses
            const uint32_t row = frow.div(g), col = g - row * rowb;
            uint32_t q = row, qn;
            qn = fy.div(q); const uint32_t y = q - qn * sz[1]; q = qn;
            qn = fz.div(q); const uint32_t z = q - qn * sz[2]; q = qn;
            qn = fc.div(q); const uint32_t c = q - qn * sz[3]; q = qn;
            const size_t src = ((((size_t)(org[4] + q) * B.g.dims[3] + (org[3] + c)) * B.g.dims[2] + (org[2] + z)) *
                                    B.g.dims[1] + (org[1] + y)) * B.g.dims[0] + org[0];
            return *(const uint4*)(B.img + src * B.g.bpp + col);
        } else {
            return *(const uint4*)(raw + g);
        }
    };
    for (uint32_t i = t; i < 1024; i += kRleThreads) crc4[i >> 8][i & 255] = c_crc4[i >> 8][i & 255];
    for (uint32_t i = t; i < kCrcLevels * 1024; i += kRleThreads)
        crcsh[i >> 10][(i >> 8) & 3][i & 255] = c_crc_shb[i >> 10][(i >> 8) & 3][i & 255];
    if (t == 0) {
        s_carry = RunSum{0, 0, 0, 0, 0};
        s_wr = 0;
        s_crc = 0;
        s_ps = 0;
        s_np = 0;
        s_cut_r = ~0u;
    }
    uint8_t* Tout = MULTI ? B.Tfull + (size_t)s * B.full_cap : B.T + (size_t)s * B.cap;
    const uint32_t wlim = (MULTI ? B.full_cap : B.cap) - 8;  // RLE1 bytes past this are not stored (the stream goes to the host)
    // this thread's 32 bytes of a tile; the next tile's are loaded while this
    // one is processed
    // (unconditional loads at clamped offsets: a load under a branch makes the
    // compiler wait for every outstanding load at the next use)
    const uint32_t glim = FROM_IMG ? L - 16 : B.raw_cap - 16;  // L >= 16: rows are whole 16-byte pieces
    auto load_chunk = [&](uint32_t g, uint32_t nv, uint4& a, uint4& b) {
        const uint4 va = load16(min(g, glim)), vb = load16(min(g + 16, glim));
        const uint4 z = make_uint4(0, 0, 0, 0);
        a = nv ? va : z;
        b = nv > 16 ? vb : z;
    };
    uint4 na, nb;
    {
        const uint32_t g = t * kRleChunk;
        load_chunk(g, g < L ? min(kRleChunk, L - g) : 0u, na, nb);
    }
    __syncthreads();
    for (uint32_t tb = 0; tb < L; tb += kRleTile) {
        const uint32_t g = tb + t * kRleChunk;
        const uint32_t nv = g < L ? min(kRleChunk, L - g) : 0u;
        uint32_t w[8];
        w[0] = na.x; w[1] = na.y; w[2] = na.z; w[3] = na.w;
        w[4] = nb.x; w[5] = nb.y; w[6] = nb.z; w[7] = nb.w;
        {
            const uint32_t g2 = g + kRleTile;
            load_chunk(g2, g2 < L ? min(kRleChunk, L - g2) : 0u, na, nb);
        }
        if (nv < kRleChunk) {  // zero padding past L
#pragma unroll
            for (uint32_t q = 0; q < 8; ++q) {
                if (nv <= 4 * q) w[q] = 0;
                else if (nv < 4 * q + 4) w[q] &= (1u << (8 * (nv - 4 * q))) - 1u;
            }
        }
        // chunk CRC
        uint32_t cc = g == 0 ? 0xffffffffu : 0u;
#pragma unroll
        for (uint32_t q = 0; q < 8; ++q) {
            const uint32_t x = cc ^ __builtin_bswap32(w[q]);
            cc = crc4[3][x >> 24] ^ crc4[2][(x >> 16) & 255u] ^ crc4[1][(x >> 8) & 255u] ^ crc4[0][x & 255u];
        }
        const uint32_t cc0 = cc;  // (MULTI: the register at a cut)
        // chunk run summary from the equal-neighbour mask
        const uint32_t Ein = chunk_eq_mask(w, nv);
        const uint32_t b0 = w[0] & 255u;
        const uint32_t blast = nv == kRleChunk ? w[7] >> 24 : chunk_byte(w, nv ? nv - 1 : 0u);
        RunSum rs{nv, b0, blast, 0, 0};
        if (nv) {
            rs.lead = 1u + (uint32_t)__builtin_ctz(~(Ein >> 1));
            rs.trail = 1u + (uint32_t)__clz(~(Ein << (32u - nv)));
        }
        // scan of the run summaries: wave, then waves, on top of the carry
        RunSum inc = rs;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const RunSum o = run_shfl_up(inc, d);
            if ((int)lane >= d) inc = run_combine(o, inc);
        }
        RunSum exc = run_shfl_up(inc, 1);
        if (lane == 0) exc = RunSum{0, 0, 0, 0, 0};
        if (lane == 63) wrs[wave] = inc;
        __syncthreads();
        RunSum pre = s_carry;
#pragma unroll
        for (uint32_t w2 = 0; w2 < NW - 1; ++w2) {
            const RunSum o = wrs[w2];
            if (w2 < wave) pre = run_combine(pre, o);
        }
        pre = run_combine(pre, exc);
        // the bzip2 run state at the chunk start: byte ch0 (256: none) in a
        // run piece of rl0 bytes (a piece restarts every 255 bytes)
        const uint32_t ch0 = pre.len ? pre.last : 256u, rl0 = pre.len ? (pre.trail - 1) % 255 + 1 : 0u;
        const bool has_end = nv && g + nv == L;
        const uint32_t valid = nv >= 32 ? ~0u : (1u << nv) - 1u;
        const uint32_t E = Ein | (nv && b0 == ch0 ? 1u : 0u);
        // a piece reaching 255 bytes splits only when the carried piece is that long
        const bool slow = rl0 >= 224 && (E & 1u);
        // byte i is copied when it is among the first four of its piece, and a
        // piece of >= 4 bytes ends with its count byte (written before the
        // next piece's first byte, or at the stream end): with Y = E << 3 | the
        // carried piece's bytes, r_i >= k <=> bits i .. i + k - 2 of Y set
        const uint64_t Y = ((uint64_t)E << 3) | (rl0 >= 4 ? 1u : 0u) | (rl0 >= 3 ? 2u : 0u) | (rl0 >= 2 ? 4u : 0u);
        const uint64_t Q = Y & (Y >> 1) & (Y >> 2);  // bit i: the piece through byte i - 1 has >= 4 bytes
        const uint32_t S = ~E & valid;               // bytes starting a piece
        const uint32_t omask = ~(uint32_t)(Q & (Y >> 3)) & valid;
        const uint32_t cmask = S & (uint32_t)Q;
        const bool endc = has_end && ((Q >> nv) & 1u);
        // the same bytes by the sequential state machine (a piece reaches
        // 255 bytes inside the chunk): emit(byte, is a count byte) in order
        auto walk = [&](auto&& emit) {
            uint32_t ch = ch0, r = rl0;
            for (uint32_t i = 0; i < nv; ++i) {
                const uint32_t c = chunk_byte(w, i);
                const bool same = c == ch && r < 255;
                if (!same && r >= 4) emit(r - 4, true);
                r = same ? r + 1 : 1u;
                ch = c;
                if (r <= 4) emit(c, false);
            }
            if (has_end && r >= 4) emit(r - 4, true);  // flush_RL of the final run
        };
        uint32_t cnt = 0;
        if (!slow) {
            cnt = (uint32_t)__popc(omask) + (uint32_t)__popc(cmask) + (endc ? 1u : 0u);
        } else {
            walk([&](uint32_t, bool) { ++cnt; });
        }
        uint32_t cinc = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(cinc, d);
            if ((int)lane >= d) cinc += o;
        }
        if (lane == 63) wcnt[wave] = cinc;
        // tile CRC: tree over the wave's chunks (byte tables of the shifts)
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const uint32_t o = __shfl_xor(cc, 1 << k);
            const bool right = (lane >> k) & 1u;
            cc = crc_shift_b(crcsh[k], right ? o : cc) ^ (right ? cc : o);
        }
        if (lane == 0) wcrc[wave] = cc;
        __syncthreads();
        const uint32_t wr0 = s_wr, po = wr0 & 15u;
        uint32_t base = po + cinc - cnt, total = 0;
        for (uint32_t w2 = 0; w2 < NW; ++w2) {
            if (w2 < wave) base += wcnt[w2];
            total += wcnt[w2];
        }
        // MULTI: the first piece start of the chunk at or past the open part's limit
        uint32_t hit_tp = 0;
        if (MULTI) {
            const uint32_t thr = s_ps + B.nblock_max;
            const uint32_t tpos = (wr0 & ~15u) + base;  // text position of the chunk's first output byte
            uint32_t hit = ~0u;
            if (nv && tpos + cnt > thr) {
                if (!slow) {
                    uint32_t sm = S;
                    while (sm) {
                        const uint32_t i = (uint32_t)__builtin_ctz(sm);
                        sm &= sm - 1u;
                        const uint32_t lt = (1u << i) - 1u;
                        const uint32_t p = tpos + (uint32_t)__popc(omask & lt) + (uint32_t)__popc(cmask & (lt | (1u << i)));
                        if (p >= thr) {
                            hit = i;
                            hit_tp = p;
                            break;
                        }
                    }
                } else {
                    uint32_t ch = ch0, r = rl0, q = tpos;
                    for (uint32_t i = 0; i < nv; ++i) {
                        const uint32_t c = chunk_byte(w, i);
                        const bool same = c == ch && r < 255;
                        if (!same) {
                            q += r >= 4 ? 1u : 0u;
                            if (q >= thr && hit == ~0u) {
                                hit = i;
                                hit_tp = q;
                            }
                        }
                        r = same ? r + 1 : 1u;
                        ch = c;
                        q += r <= 4 ? 1u : 0u;
                    }
                }
            }
            if (hit != ~0u) atomicMin(&s_cut_r, g + hit);
        }
        if (!slow) {
            // copies in order, the count bytes after (each a few per chunk at most)
            uint32_t pos = base;
#pragma unroll
            for (uint32_t i = 0; i < kRleChunk; ++i) {
                pos += (cmask >> i) & 1u;
                const bool of = (omask >> i) & 1u;
                uint8_t* dst = of ? &tout[pos] : &junk[t];
                *dst = (uint8_t)(w[i >> 2] >> (8 * (i & 3u)));
                pos += of ? 1u : 0u;
            }
            uint32_t cm = cmask;
            while (cm) {
                const uint32_t i = (uint32_t)__builtin_ctz(cm);
                cm &= cm - 1u;
                const uint32_t lt = (1u << i) - 1u, m = S & lt;
                const uint32_t len = m ? i - (31u - (uint32_t)__clz(m)) : rl0 + i;
                tout[base + (uint32_t)__popc(omask & lt) + (uint32_t)__popc(cmask & lt)] = (uint8_t)(len - 4u);
            }
            if (endc) {
                const uint32_t m = S & valid;
                const uint32_t len = m ? nv - (31u - (uint32_t)__clz(m)) : rl0 + nv;
                tout[base + cnt - 1u] = (uint8_t)(len - 4u);
            }
        } else {
            walk([&](uint32_t v, bool) { tout[base++] = (uint8_t)v; });
        }
        RunSum ncarry{0, 0, 0, 0, 0};
        if (t == 0) {
            ncarry = s_carry;
#pragma unroll
            for (uint32_t w2 = 0; w2 < NW; ++w2) ncarry = run_combine(ncarry, wrs[w2]);
        }
        // the tile's CRC: wave CRCs shifted by the waves after them (lane
        // w < 8 of wave 0: (7 - w) * 2048 bytes, levels 6..8), xor-reduced,
        // on top of the stream CRC shifted by the tile (level 9)
        uint32_t ncrc = 0;
        if (wave == 0) {
            static_assert(NW == 8 && kRleChunk * 64 == (32u << 6), "wave CRC levels");
            uint32_t x = lane < NW ? wcrc[lane] : 0u;
            const uint32_t sh = NW - 1 - min(lane, NW - 1);
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const uint32_t y = crc_shift_b(crcsh[6 + l], x);
                x = (sh >> l) & 1u ? y : x;
            }
            x ^= __shfl_xor(x, 1);
            x ^= __shfl_xor(x, 2);
            x ^= __shfl_xor(x, 4);
            ncrc = crc_shift_b(crcsh[9], s_crc) ^ x;
        }
        __syncthreads();
        if (MULTI) {
            const uint32_t cr = s_cut_r;
            if (cr != ~0u && cr != L - 1) {  // (every thread sees the same cr)
                // P(cr): the stream register shifted over the tile's bytes in
                // front of the cut, the whole chunks there shifted likewise,
                // and the cut chunk's bytes before the cut
                uint32_t x = 0;
                if (nv && g + kRleChunk <= cr) {
                    x = crc_mul(cc0, crc_xpow8(cr - g - kRleChunk));
                } else if (nv && g <= cr) {
                    x = g == 0 ? 0xffffffffu : 0u;
                    for (uint32_t i = 0; i < cr - g; ++i) x = (x << 8) ^ crc4[0][(x >> 24) ^ chunk_byte(w, i)];
                    s_cut_tp = hit_tp;
                }
                if (t == 0) x ^= crc_mul(s_crc, crc_xpow8(cr - tb));
#pragma unroll
                for (int d = 32; d; d >>= 1) x ^= __shfl_xor(x, d);
                if (lane == 0) s_red[wave] = x;
                __syncthreads();
                if (t == 0) {
                    uint32_t P = 0;
                    for (uint32_t w2 = 0; w2 < NW; ++w2) P ^= s_red[w2];
                    const uint32_t k = s_np + 1, slot = s * B.parts + k;
                    if (k < B.parts) {  // (more parts than slots: the stream goes to the host)
                        B.part_toff[slot] = s_cut_tp;
                        B.part_roff[slot] = cr;
                        B.crc[slot] = P;
                    }
                    s_np = k;
                    s_ps = s_cut_tp;
                }
            }
        }
        // whole 16-byte units out (16-byte stores; a unit starting before
        // wlim ends inside the 256-aligned cap), the last partial unit kept
        {
            const uint32_t end = po + total, full = end >> 4, ub = wr0 & ~15u;
            for (uint32_t u = t; u < full; u += kRleThreads)
                if (ub + 16u * u < wlim) *(uint4*)(Tout + ub + 16u * u) = *(const uint4*)(tout + 16u * u);
            const uint8_t keep = t < 16u ? tout[16u * full + t] : (uint8_t)0;
            __syncthreads();
            if (t < 16u) tout[t] = keep;
        }
        if (t == 0) {
            s_carry = ncarry;
            s_crc = ncrc;
            s_wr = wr0 + total;
            if (MULTI) s_cut_r = ~0u;
        }
    }
    __syncthreads();
    {  // the stream's last partial unit (bytes past the end are not read)
        const uint32_t wr = s_wr;
        if ((wr & 15u) && t == 0 && (wr & ~15u) < wlim) *(uint4*)(Tout + (wr & ~15u)) = *(const uint4*)tout;
    }
    if (t == 0) {
        const uint32_t total = s_wr;
        uint32_t crc = s_crc;
        const uint32_t pad = (L + kRleTile - 1) / kRleTile * kRleTile - L;
        for (int j = 0; j < kCrcUnshift; ++j)
            if ((pad >> j) & 1u) crc = gf2_apply(c_crc_unshift[j], crc);
        if (!MULTI) {
            const bool host = total >= B.nblock_max || total > wlim;
            B.crc[s] = L ? ~crc : 0u;
            B.n[s] = total;
            B.flags[s] = host ? kFlagHost : 0u;
            B.done[s] = host ? 1u : 0u;
            B.seg_begin[s] = s * B.cap;
            B.seg_end[s] = s * B.cap + (host ? 0u : total);
        } else {
            // the parts into their slots: offsets, lengths and CRCs (B.crc of
            // the slots past the first holds P at their cut until here); the
            // slots not in use are skipped like host streams
            const uint32_t np = s_np + 1, s0 = s * B.parts;
            bool host = np > B.parts || total > wlim;
            for (uint32_t k = 0; k < np && !host; ++k) {
                const uint32_t a = k ? B.part_toff[s0 + k] : 0u, b = k + 1 < np ? B.part_toff[s0 + k + 1] : total;
                host = b - a > B.cap - 8;
            }
            for (uint32_t k = 0; k < B.parts; ++k) {
                const uint32_t slot = s0 + k;
                const bool used = !host && k < np;
                uint32_t n = 0;
                if (used) {
                    const bool last = k + 1 == np;
                    const uint32_t ta = k ? B.part_toff[slot] : 0u, tb2 = last ? total : B.part_toff[slot + 1];
                    const uint32_t ra = k ? B.part_roff[slot] : 0u, rb = last ? L : B.part_roff[slot + 1];
                    const uint32_t Pa = k ? B.crc[slot] : 0xffffffffu, Pb = last ? crc : B.crc[slot + 1];
                    n = tb2 - ta;
                    B.part_toff[slot] = ta;
                    B.part_roff[slot] = ra;
                    B.part_rlen[slot] = rb - ra;
                    B.crc[slot] = ~(Pb ^ crc_mul(Pa ^ 0xffffffffu, crc_xpow8(rb - ra)));
                }
                B.n[slot] = n;
                B.flags[slot] = used ? 0u : kFlagHost;
                B.done[slot] = used ? 0u : 1u;
                B.seg_begin[slot] = slot * B.cap;
                B.seg_end[slot] = slot * B.cap + n;
            }
            B.nparts[s] = host ? 0u : np;
            B.sflags[s] = host ? kFlagHost : 0u;
        }
    }
    // the byte map of the RLE1 text comes from bwt_bucket's histogram
    for (uint32_t i = t; i < 8 * (MULTI ? B.parts : 1u); i += kRleThreads) B.inuse[s * (MULTI ? B.parts : 1u) * 8 + i] = 0u;
}

// MULTI: every part's text from the stream's uncut text into its slot
// (dword stores; the source starts at any byte)
__global__ __launch_bounds__(256) void place_parts(Batch B)
{
    const uint32_t slot = blockIdx.y;
    if (B.flags[slot] & kFlagHost) return;
    const uint32_t n = B.n[slot];
    const uint8_t* src = B.Tfull + (size_t)(slot / B.parts) * B.full_cap + B.part_toff[slot];
    uint32_t* dst = (uint32_t*)(B.T + (size_t)slot * B.cap);
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; 4 * i < n; i += gridDim.x * 256) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; ++b) v |= 4 * i + b < n ? (uint32_t)src[4 * i + b] << (8 * b) : 0u;
        dst[i] = v;
    }
}

// ------------------------------------------------------------------ BWT --
// Sort values carry the rotation start i (bits 0-23, n < 2^20) and the byte
// preceding it (bits 24-31): after sorting, that byte IS the BWT output
// column, so the MTF stage reads it in sorted order without a gather.
constexpr uint32_t kIdxMask = 0x00FFFFFFu;
constexpr uint32_t kKeyBytes = 8;  // first-round key: the 8-byte prefix (0.02 % of rotations tie on symbols)

// First round: every rotation by its 8-byte prefix, in two steps.
//  bwt_bucket      one workgroup per stream: a counting sort of the rotations
//                  by their leading kBucketBits bits (byte 0, top bits of byte 1), the
//                  histogram in LDS; only the values are scattered (the sorters rebuild the 8-byte big-endian keys from the text).
//                  The stream's slot range is cut at bucket ends into chunks
//                  of < 2 kChunk rotations (a cut after the bucket that holds
//                  each multiple of kChunk; a bucket larger than kChunk is a
//                  chunk of its own).
//  bwt_chunk_sort  one workgroup per sort job (a chunk, or one of the two parts
//                  of a multi-bucket chunk: ChunkLists): its rotations sorted by the
//                  whole key in LDS (buckets are ordered by the key's top bits,
//                  so sorting a run of whole buckets sorts each bucket), and
//                  the still-tied flags (equal keys never cross a bucket).
// On light-field symbols a 147k-rotation stream has ~1 000 buckets of at most
// ~2 000 rotations: each rotation is read and written once per step; the
// previous device-wide 60-bit radix sort made 8 HBM passes.  Chunks above the
// large sorter's capacity (one bucket of > kBigCap equal-prefix rotations) go
// to a rocPRIM segmented sort.
constexpr uint32_t kBucketBits = 14;               // 64 KiB histogram, two workgroups per CU (15 bits / one workgroup
                                                   // per CU measured 3 % slower end to end, 13 bits 18 % slower: more
                                                   // buckets overflow the small sorter)
constexpr int kBucketThreads = 1024;               // each walks 8 positions of a tile (kBktG, kBktTile below)
constexpr uint32_t kChunk = 1024;  // (512 equal, 2 048 slower end to end in round 5)
constexpr int kCsThreads = 512, kCsItems = 4;      // jobs up to 2 048 (single buckets above kChunk); 512 x 4 measured
                                                   // 10 % faster than 256 x 8
constexpr int kBigThreads = 512, kBigItems = 8;    // single buckets up to 4 096
constexpr uint32_t kSmallCap = kCsThreads * kCsItems, kBigCap = kBigThreads * kBigItems;
constexpr uint32_t kMaxCuts = 1024;                // cut entries a stream may need, exclusive: one per kChunk sorted
                                                   // rotations plus two per bucket above kChunk, so up to about
                                                   // 3 * nsub / kChunk.  That stays below kMaxCuts up to ~350 000 sorted
                                                   // rotations whatever the text (the 96 x 96 x 8 uint16 block sorts
                                                   // < 185 000); a longer stream that does need kMaxCuts entries or
                                                   // more is flagged for the host library (bwt_bucket)

// chunk classes by size: [3] <= kTinyCap, [0] <= kSmallCap, [1] <= kBigCap,
// [2] larger (rocPRIM segmented sort).  The classes are counted; what the
// sorters run over are the sort jobs below.
constexpr uint32_t kTinyCap = 1024;  // half-size sorter: the ~40 % of chunks at most
                                     // this long would pad a kSmallCap sort to twice their size
constexpr uint32_t kMiniCap = 512;   // quarter-size sorter (sort jobs only)

// Sort jobs: slot ranges [b, e) of whole buckets, one workgroup each, listed
// by the smallest sorter that holds them.  A chunk is one job, except that a
// chunk of several buckets and more than kMiniCap rotations which cuts_of
// closed after its last bucket is two: the slots before that bucket, and the
// bucket.  Such a chunk's earlier buckets lie between two multiples of kChunk
// and its last bucket is at most kChunk, so both parts fit the half-size
// sorter, where the whole chunk (1.2 kChunk on average on light-field symbols)
// padded a kSmallCap sort; the sorters cost their capacity, not their content.
// A job never cuts a bucket, so equal keys stay inside one workgroup.
// (The chunks that end at nsub or in front of a bucket above kChunk hold no
// multiple of kChunk: at most kChunk rotations, one job.)
// Lists: [0] <= kSmallCap (single buckets only), [1] <= kBigCap and [2] larger
// (the chunks of classes 1 and 2, one job each: their counters are the class
// counters), [3] <= kTinyCap, [4] <= kMiniCap.
constexpr int kJobLists = 5;
struct ChunkLists {
    uint32_t* b[kJobLists];
    uint32_t* e[kJobLists];
    uint32_t* cnt;  // the workspace's counters (Scratch)
};
// counter words (Scratch::cnt) of the job lists, and of the two classes that have no list of their own
__device__ __host__ constexpr uint32_t job_cnt_word(uint32_t list)
{
    return list == 0 ? 6u : list == 1 ? 1u : list == 2 ? 2u : list == 3 ? 4u : 3u;
}
__device__ __forceinline__ uint32_t job_list(uint32_t m)
{
    return m <= kMiniCap ? 4u : (m <= kTinyCap ? 3u : (m <= kSmallCap ? 0u : (m <= kBigCap ? 1u : 2u)));
}
// A cut entry (a slot below 2^20) that closes a chunk after a bucket of at
// most kChunk carries that bucket's size - 1 above the slot, and a flag.
constexpr uint32_t kCutSlotBits = 20, kCutSlotMask = (1u << kCutSlotBits) - 1u, kCutHasLast = 1u << 30;

// A tile of the text for the bucket pass: T[i0 - 1 .. i0 + m + 8) cyclically
// in tile[kTOff - 1 .. kTOff + m + 8), m = min(n - i0, kBktTile) (T[i0 + k]
// at tile[kTOff + k]: 8-byte aligned stores and group reads).  A lane walks a
// group of kBktG = 8 consecutive positions from registers: bucket_fetch loads
// this thread's part (8 bytes; one edge byte for threads 0..8) a tile ahead,
// bucket_put stores it into LDS, bucket_group reads the lane's group, the 8
// bytes after it and the byte before it back.  One LDS buffer: the tile is
// double-buffered through the lanes' registers instead (two 8 KiB buffers
// beside the 64 KiB histogram would leave one workgroup per CU), so a tile
// costs two barriers, the second straight after the group reads -- as many per
// byte as one barrier per 4 096-byte tile.
constexpr uint32_t kBktG = 8;
constexpr uint32_t kBktTile = kBucketThreads * kBktG;
constexpr uint32_t kTOff = 8;
struct BktPart {
    uint2 w;
    uint32_t e;
};
struct BktGroup {
    uint64_t P, Q;  // T[i0 + 8 t ..] big endian (lfm_bwt_types.h)
    uint32_t prev;  // T[i0 + 8 t - 1]
};

__device__ __forceinline__ BktPart bucket_fetch(const uint8_t* __restrict__ T, uint32_t n, uint32_t i0)
{
    // loads at clamped offsets for every thread (no load under a branch: the
    // compiler would wait for all outstanding loads at the next use)
    const uint32_t t = threadIdx.x;
    const uint32_t i0c = min(i0, n ? n - 1 : 0u);
    const uint32_t m = n > i0c ? min(n - i0c, kBktTile) : 0u;
    // 8 bytes (may read up to 7 bytes past n: inside the stream's cap, which
    // is a multiple of 256 and leaves 8 bytes after n)
    const uint2 w = *(const uint2*)(T + min(i0c + kBktG * t, n ? (n - 1) & ~7u : 0u));
    uint32_t j = n ? (t < 8 ? (i0c + m + t) % n : (i0c ? i0c - 1 : n - 1)) : 0u;
    const uint32_t e = T[j];
    const bool in = i0 < n && kBktG * t < m;
    BktPart p;
    p.w.x = in ? w.x : 0u;
    p.w.y = in ? w.y : 0u;
    p.e = (i0 < n && t <= 8) ? e : 0u;
    return p;
}

__device__ __forceinline__ uint32_t bucket_put(const BktPart& p, uint32_t n, uint32_t i0, uint8_t* tile)
{
    const uint32_t t = threadIdx.x;
    const uint32_t m = min(n - i0, kBktTile);
    if (kBktG * t + kBktG <= m) {
        *(uint2*)(tile + kTOff + kBktG * t) = p.w;
    } else if (kBktG * t < m) {  // the last partial group: its valid bytes only (the edge bytes follow)
        const uint64_t w = (uint64_t)p.w.x | ((uint64_t)p.w.y << 32);
        for (uint32_t b = 0; b < m - kBktG * t; ++b) tile[kTOff + kBktG * t + b] = (uint8_t)(w >> (8 * b));
    }
    if (t < 8) tile[kTOff + m + t] = (uint8_t)p.e;
    else if (t == 8) tile[kTOff - 1] = (uint8_t)p.e;
    return m;  // the caller's barrier publishes the tile
}

// this lane's group (the bytes past T[i0 + m + 8) are whatever the buffer
// held: no valid position's type or key reads them)
__device__ __forceinline__ BktGroup bucket_group(const uint8_t* tile)
{
    const uint8_t* p = tile + kTOff + kBktG * threadIdx.x;
    BktGroup g;
    g.P = __builtin_bswap64(*(const uint64_t*)p);
    g.Q = __builtin_bswap64(*(const uint64_t*)(p + 8));
    g.prev = p[-1];
    return g;
}

// position j of a group: its bucket (the top BITS bits of T[j], T[j + 1]),
// its first byte and the byte before it
template <uint32_t BITS>
__device__ __forceinline__ uint32_t group_key(const BktGroup& g, uint32_t j)
{
    const uint32_t ab = j < 7u ? (uint32_t)(g.P >> (48u - 8u * j)) & 0xFFFFu
                               : (((uint32_t)g.P & 0xFFu) << 8) | (uint32_t)(g.Q >> 56);
    return ab >> (16 - BITS);
}
__device__ __forceinline__ uint32_t group_byte(const BktGroup& g, uint32_t j)
{
    return (uint32_t)(g.P >> (56u - 8u * j)) & 0xFFu;
}
__device__ __forceinline__ uint32_t group_prev(const BktGroup& g, uint32_t j)
{
    return j ? group_byte(g, j - 1u) : g.prev;
}
__device__ __forceinline__ bool group_has(uint64_t flags, uint32_t j)
{
    return (flags >> (63u - 8u * j)) & 1u;
}

// LDS slot of bucket `key` (BITS bits: the first byte, then the top BITS - 8
// bits of the second).  A dword's bank is its index mod 32, i.e. the key's
// low bits -- the top bits of the SECOND byte, which on 16-bit little-endian
// symbols is the high byte (mostly 0) for every other rotation: half the
// lanes of an atomic landed on one bank with different addresses.  XOR-ing
// the low 5 bits with the first byte spreads them (a bijection; every access
// to the histogram goes through it).
template <uint32_t BITS>
__device__ __forceinline__ uint32_t bkt_slot(uint32_t key)
{
    return key ^ ((key >> (BITS - 8)) & 31u);
}

// Two-stage BWT (Itoh & Tanaka).  Rotation i is of type B when it sorts
// before rotation i + 1 (T[i] < T[i + 1], or equal bytes and i + 1 of type B)
// and of type A otherwise; the types of a non-periodic block are well defined
// cyclically.  Only the rotations of ONE type (about half) go through the sort
// below (bucket pass, chunk sorts, ties); bwt_induce places the others by one
// scan of the sorted order.  Inside the bucket of first byte c the A rotations
// come first; the A rotations of a bucket are ordered as their successors are
// (i + 1 precedes i in the final order) and the B rotations likewise (i + 1
// follows i).  So with the B rotations sorted a left-to-right scan places the
// A ones (kModeSortB), with the A rotations sorted a right-to-left scan places
// the B ones (kModeSortA).  The pass sorts the A rotations unless the B ones
// are clearly fewer: on 16-bit little-endian symbols the A rotations start at
// the low bytes, whose first byte spreads them over the buckets, while the B
// ones start at the (mostly zero) high bytes.  bwt_types8 (lfm_bwt_types.h)
// decides the types of a lane's 8 positions from their bytes and the 8 after
// them (the tile holds 8 bytes past its end), by byte-wise comparisons on
// words; a type still undecided after 8 equal bytes (only runs of 0xFB
// survive RLE1 that long) sends the stream through the sort whole, kModeFull.
constexpr uint32_t kModeSortA = 0, kModeSortB = 1, kModeFull = 2;

// The rotations of a lane's group that go through the sort in `mode`, as
// flags (lfm_bwt_types.h); m: the tile's length.  A group past m has none.
struct BktSorted {
    uint64_t valid, sorted;
    BwtTypes ty;  // (not in kModeFull)
};
__device__ __forceinline__ BktSorted group_sorted(const BktGroup& g, uint32_t m, uint32_t mode)
{
    const uint32_t k = kBktG * threadIdx.x;
    BktSorted r;
    r.valid = k < m ? group_valid(min(m - k, kBktG)) : 0ull;
    r.ty = BwtTypes{0, 0, 0, 0};
    if (mode == kModeFull) {
        r.sorted = r.valid;
    } else {
        r.ty = bwt_types8(g.P, g.Q, k < m ? min(m - k, kBktG) : 1u);
        r.sorted = (mode == kModeSortB ? r.ty.b : ~r.ty.b) & r.valid;
        if (k >= m) r.ty.undecided = 0;
    }
    return r;
}

template <uint32_t BITS>
__global__ __launch_bounds__(kBucketThreads) __attribute__((amdgpu_waves_per_eu(8))) void bwt_bucket(Batch B, ChunkLists L)
{
    constexpr uint32_t kBuckets = 1u << BITS;
    __shared__ uint32_t hist[kBuckets];  // 64 KiB at 14 bits
    __shared__ __attribute__((aligned(16))) uint8_t tile[kTOff + kBktTile + 8];  // (a last group's 16 bytes end here)
    __shared__ uint32_t cuts[kMaxCuts];
    __shared__ uint32_t wsum[kBucketThreads / 64], wcut[kBucketThreads / 64];
    __shared__ uint32_t ccount[2];  // chunks of class 0 and of class 3 (classes 1 and 2 are job lists 1 and 2)
    __shared__ uint32_t jcount[kJobLists], jbase[kJobLists];
    __shared__ uint32_t sinuse[8];                  // bytes present in the RLE1 text (the stream's inUse map)
    __shared__ uint32_t cnt_u[256], cnt_s[256];     // unsorted / sorted rotations per first byte
    __shared__ uint32_t cnt_l[256];                 // unsorted rotations that induce ("live"), per first byte
    __shared__ uint32_t undecided, n_unsorted;
    __shared__ uint32_t tsum[12];
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t n = B.n[s];
    const uint8_t* T = B.T + (size_t)s * B.cap;
    const uint32_t o = s * B.cap;
    if (t < 2) ccount[t] = 0;
    if (t < (uint32_t)kJobLists) jcount[t] = 0;
    if (t < 8) sinuse[t] = 0;
    // histogram of the BITS-bit bucket over the rotations to sort; the pass
    // restarts (at most twice) for the B rotations when they are clearly fewer
    // and for every rotation when a type is undecided
    uint32_t mode = B.it_full ? kModeFull : kModeSortA;
    for (;;) {
        for (uint32_t b = t; b < kBuckets; b += kBucketThreads) hist[b] = 0;
        if (t < 256) cnt_u[t] = cnt_s[t] = cnt_l[t] = 0;
        if (t == 0) undecided = n_unsorted = 0;
        __syncthreads();
        // unsorted rotations starting with byte 0 (the high bytes of small
        // 16-bit symbols: about half of all rotations) are counted in a
        // register, by popcounts of the group's masks -- their LDS atomics
        // all hit one word and serialise
        uint32_t u_zero = 0, l_zero = 0;
        mode = __builtin_amdgcn_readfirstlane(mode);  // (the same in every lane: kept on the scalar side)
        BktPart nx = bucket_fetch(T, n, 0);
        for (uint32_t i0 = 0; i0 < n; i0 += kBktTile) {
            const BktPart cur = nx;
            nx = bucket_fetch(T, n, i0 + kBktTile);
            const uint32_t m = bucket_put(cur, n, i0, tile);
            __syncthreads();
            const BktGroup g = bucket_group(tile);
            __syncthreads();
            const BktSorted r = group_sorted(g, m, mode);
            if (r.ty.undecided) undecided = 1u;
            // an unsorted rotation k induces k - 1 ("live") when k - 1 is
            // unsorted too: by bwt_induce's own byte rule, T[k-1] against T[k]
            // in the direction of the mode's scan.  For the group's later
            // positions that is the comparison of the position before.
            const uint64_t unsorted = r.valid & ~r.sorted;
            const uint32_t first = (uint32_t)(g.P >> 56);
            const uint64_t step = mode == kModeSortA ? r.ty.lt | r.ty.eq : ~r.ty.lt & kByteFlags;
            const uint64_t live = (step >> 8) | ((mode == kModeSortA ? g.prev <= first : g.prev >= first) ? 1ull << 63 : 0ull);
            const uint64_t uz = unsorted & bytes_eq(g.P, 0);
            u_zero += __popcll(uz);
            l_zero += __popcll(uz & live);
            // one atomic per counted position, its word chosen without a
            // branch: the bucket of a sorted rotation, else the first byte
            const uint64_t rest = unsorted & ~uz, counted = r.sorted | rest;
#pragma unroll
            for (uint32_t j = 0; j < kBktG; ++j) {
                uint32_t* word = group_has(r.sorted, j) ? &hist[bkt_slot<BITS>(group_key<BITS>(g, j))] : &cnt_u[group_byte(g, j)];
                if (group_has(counted, j)) atomicAdd(word, 1u);
            }
            if (rest & live) {  // (few on 16-bit symbols: their unsorted rotations start with the zero high bytes)
#pragma unroll
                for (uint32_t j = 0; j < kBktG; ++j)
                    if (group_has(rest & live, j)) atomicAdd(&cnt_l[group_byte(g, j)], 1u);
            }
        }
        if (u_zero) atomicAdd(&cnt_u[0], u_zero);
        if (l_zero) atomicAdd(&cnt_l[0], l_zero);
        __syncthreads();
        if (mode == kModeFull) break;
        if (undecided) {
            mode = kModeFull;
        } else {
            if (t < 256 && cnt_u[t]) atomicAdd(&n_unsorted, cnt_u[t]);
            __syncthreads();
            // the other type clearly fewer (by 1/8): sort it instead
            if (mode != kModeSortA || (uint64_t)n_unsorted * 8 >= (uint64_t)(n - n_unsorted) * 7) break;
            mode = kModeSortB;
        }
        __syncthreads();
    }
    // exclusive scan of the buckets; chunk cuts at bucket ends
    constexpr uint32_t per = kBuckets / kBucketThreads;
    static_assert(per <= (1u << (BITS - 8)), "a thread's buckets share their first byte");
    uint32_t sum = 0;
    for (uint32_t q = 0; q < per; ++q) sum += hist[bkt_slot<BITS>(t * per + q)];
    if (sum) atomicAdd(&cnt_s[(t * per) >> (BITS - 8)], sum);
    uint32_t isum = sum;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t a = __shfl_up(isum, d);
        if ((int)lane >= d) isum += a;
    }
    if (lane == 63) wsum[wave] = isum;
    __syncthreads();
    uint32_t psum = 0, nsub = 0;
    for (uint32_t w = 0; w < kBucketThreads / 64; ++w) {
        if (w < wave) psum += wsum[w];
        nsub += wsum[w];
    }
    const uint32_t my0 = psum + isum - sum;
    // every byte of the text starts a rotation: byte c is present iff it
    // starts a sorted or an unsorted rotation
    if (t < 256 && (cnt_u[t] | cnt_s[t])) atomicOr(&sinuse[t >> 5], 1u << (t & 31));
    // the chunk sorts flag positions < nsub; tie_compact's 16-byte loads also
    // see up to 15 bytes past nsub, which must read as "not tied"
    if (t < 16 && nsub + t < B.cap) B.uflag[o + nsub + t] = 0;
    // cut positions of this thread's buckets (ascending): after a bucket that
    // holds a multiple of kChunk, and around a bucket larger than kChunk
    auto cuts_of = [&](auto&& emit) {
        uint32_t off = my0;
        for (uint32_t q = 0; q < per; ++q) {
            const uint32_t c = hist[bkt_slot<BITS>(t * per + q)];
            if (c) {
                const uint32_t e = off + c;
                if (c > kChunk) {
                    if (off) emit(off);
                    emit(e);
                } else if ((e - 1) / kChunk >= (off + kChunk - 1) / kChunk && e - 1 >= kChunk) {
                    emit(e | ((c - 1u) << kCutSlotBits) | kCutHasLast);
                }
            }
            off += c;
        }
    };
    uint32_t ncut = 0;
    cuts_of([&](uint32_t) { ++ncut; });
    uint32_t icut = ncut;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t a = __shfl_up(icut, d);
        if ((int)lane >= d) icut += a;
    }
    if (lane == 63) wcut[wave] = icut;
    __syncthreads();
    uint32_t pcut = 0, tcut = 0;
    for (uint32_t w = 0; w < kBucketThreads / 64; ++w) {
        if (w < wave) pcut += wcut[w];
        tcut += wcut[w];
    }
    // more cut entries than cuts[] (and the kBucketThreads lanes that turn
    // them into chunks) hold: the chunks past the last kept entry would be
    // one chunk of many buckets, which the segmented sort of the low key bits
    // must never see.  The host library takes the stream; it gets no chunks,
    // so nothing after this pass touches it (tcut is the same in every lane).
    if (tcut >= kMaxCuts) {
        if (t == 0) B.flags[s] |= kFlagHost;
        return;
    }
    {
        uint32_t at = pcut + icut - ncut;
        cuts_of([&](uint32_t p) {
            if (at < kMaxCuts) cuts[at] = p;
            ++at;
        });
    }
    if (t < 8) B.inuse[s * 8 + t] = sinuse[t];  // (written after the scan's barrier)
    {  // A / B rotations per first byte for bwt_induce, and the tables of
       // bwt_place_sorted and bwt_induce (see "induction" below): the final
       // position of bucket c's first sorted rotation (tq), the first sa slot
       // of its sorted rotations (s0), and, by scan bucket u, the compact
       // scan index of its first live slot (cs) and its live count (cl)
        uint32_t na = 0, nb = 0, ns = 0, nl = 0, x = 0, y = 0, z = 0;
        if (t < 256) {
            na = mode == kModeSortA ? cnt_s[t] : cnt_u[t];
            nb = mode == kModeSortA ? cnt_u[t] : cnt_s[t];
            ns = mode == kModeSortA ? na : nb;  // (kModeFull: all in the B counts)
            nl = mode == kModeFull ? 0u : cnt_l[t];
            B.abcnt[(size_t)s * 512 + t] = na;
            B.abcnt[(size_t)s * 512 + 256 + t] = nb;
            x = na + nb;
            y = ns;
            z = nl + ns;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t a = __shfl_up(x, d), b = __shfl_up(y, d), c = __shfl_up(z, d);
                if ((int)lane >= d) {
                    x += a;
                    y += b;
                    z += c;
                }
            }
            if (lane == 63) {
                tsum[wave] = x;
                tsum[4 + wave] = y;
                tsum[8 + wave] = z;
            }
        }
        __syncthreads();
        if (t < 256) {
            for (uint32_t w = 0; w < wave; ++w) {
                x += tsum[w];
                y += tsum[4 + w];
                z += tsum[8 + w];
            }
            const uint32_t nc = tsum[8] + tsum[9] + tsum[10] + tsum[11];  // the compact scan's length
            const uint32_t qs = x - na - nb;
            const bool rev = mode == kModeSortA;  // the scan runs right to left: scan bucket u = 255 - c
            const uint32_t u = rev ? 255u - t : t;
            uint32_t* it = B.itab + (size_t)s * 1024;
            it[t] = mode == kModeSortB ? qs + na : qs;
            it[256 + u] = rev ? nc - z : z - (nl + ns);
            it[512 + u] = nl;
            it[768 + t] = y - ns;
        }
    }
    if (t == 0) {
        B.nsub[s] = nsub;
        B.bwt_mode[s] = mode;
    }
    // bucket starts for the scatter
    {
        uint32_t off = my0;
        for (uint32_t q = 0; q < per; ++q) {
            const uint32_t c = hist[bkt_slot<BITS>(t * per + q)];
            hist[bkt_slot<BITS>(t * per + q)] = off;
            off += c;
        }
    }
    __syncthreads();
    // chunks = runs between consecutive cuts (the last ends at nsub), counted
    // by class; each gives one sort job or two (see ChunkLists)
    const uint32_t nch = min(tcut, kMaxCuts - 1) + 1;
    // this lane's chunk [cb, ce): jobs [cb, mid) and, where mid < ce, [mid, ce)
    uint32_t cb = 0, mid = 0, ce = 0, l0 = 0, l1 = 0, s0 = 0, s1 = 0;
    if (t < nch) {
        cb = t ? cuts[t - 1] & kCutSlotMask : 0u;
        const uint32_t cut = t + 1 < nch ? cuts[t] : nsub;
        ce = cut & kCutSlotMask;
        const uint32_t m = ce > cb ? ce - cb : 0u;
        const uint32_t last = (cut & kCutHasLast) ? ((cut >> kCutSlotBits) & (kChunk - 1u)) + 1u : m;
        mid = last < m && m > kMiniCap ? ce - last : ce;
        if (m) {
            if (m <= kSmallCap) atomicAdd(&ccount[m <= kTinyCap ? 1 : 0], 1u);
            l0 = job_list(mid - cb);
            s0 = atomicAdd(&jcount[l0], 1u);
            if (mid < ce) {
                l1 = job_list(ce - mid);
                s1 = atomicAdd(&jcount[l1], 1u);
            }
        } else {
            cb = mid = ce;
        }
    }
    __syncthreads();
    if (t < (uint32_t)kJobLists) jbase[t] = jcount[t] ? atomicAdd(&L.cnt[job_cnt_word(t)], jcount[t]) : 0u;
    else if (t == 64 && ccount[0]) atomicAdd(&L.cnt[0], ccount[0]);
    else if (t == 65 && ccount[1]) atomicAdd(&L.cnt[5], ccount[1]);
    __syncthreads();
    if (mid > cb) {
        L.b[l0][jbase[l0] + s0] = o + cb;
        L.e[l0][jbase[l0] + s0] = o + mid;
    }
    if (ce > mid) {
        L.b[l1][jbase[l1] + s1] = o + mid;
        L.e[l1][jbase[l1] + s1] = o + ce;
    }
    // scatter of the values only (start | preceding byte << 24): the sorters
    // rebuild the 8-byte keys from the text (rot_key8_fast), which the L2s
    // hold, instead of 8-byte scattered key writes and their re-read
    BktPart nx = bucket_fetch(T, n, 0);
    for (uint32_t i0 = 0; i0 < n; i0 += kBktTile) {
        const BktPart cur = nx;
        nx = bucket_fetch(T, n, i0 + kBktTile);
        const uint32_t m = bucket_put(cur, n, i0, tile);
        __syncthreads();
        const BktGroup g = bucket_group(tile);
        __syncthreads();
        const uint64_t sorted = group_sorted(g, m, mode).sorted;
#pragma unroll
        for (uint32_t j = 0; j < kBktG; ++j) {
            if (group_has(sorted, j)) {
                const uint32_t pos = atomicAdd(&hist[bkt_slot<BITS>(group_key<BITS>(g, j))], 1u);
                B.vals_a[o + pos] = (i0 + kBktG * t + j) | (group_prev(g, j) << 24);
            }
        }
    }
}


// the first-round key of rotation i of a stream's text T (length n): its
// 8-byte prefix, big endian.  Away from the wrap, three aligned dwords (the
// stream's cap leaves >= 8 bytes after n) funnel-shifted; else byte by byte.
__device__ __forceinline__ uint64_t rot_key8_fast(const uint8_t* __restrict__ T, uint32_t n, uint32_t i)
{
    if (i + 8 <= n) {
        const uint32_t* w = (const uint32_t*)(T + (i & ~3u));
        const uint32_t d0 = w[0], d1 = w[1], d2 = w[2];
        const uint32_t sh = (i & 3u) * 8u;
        const uint64_t x = (uint64_t)d0 | ((uint64_t)d1 << 32);
        const uint64_t le = sh ? (x >> sh) | ((uint64_t)d2 << (64u - sh)) : x;
        return __builtin_bswap64(le);
    }
    uint64_t k = 0;
    uint32_t j = i;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        k = (k << 8) | T[j];
        j = j + 1 == n ? 0u : j + 1;
    }
    return k;
}

// text_prev4: T[i-2] | T[i-3] << 8 | T[i-4] << 16 | T[i-5] << 24 (cyclic)
__device__ __forceinline__ uint32_t text_prev4(const uint8_t* __restrict__ T, uint32_t n, uint32_t i)
{
    // two aligned dwords around T[i-5 .. i-2] (i - 1 < n: inside the text),
    // loaded at a clamped address; the first five rotations wrap
    const uint32_t a = i >= 5 ? i - 5 : 0u;
    const uint32_t* w = (const uint32_t*)(T + (a & ~3u));
    const uint64_t x = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    uint32_t r = __builtin_bswap32((uint32_t)(x >> ((a & 3u) * 8u)));
    if (i < 5) {
        r = 0;
        for (uint32_t k = 2; k <= 5; ++k) r |= (uint32_t)T[(i + 5 * n - k) % n] << (8 * (k - 2));
    }
    return r;
}

// keys_a for the chunks the rocPRIM segmented sort takes (one workgroup per chunk)
__global__ __launch_bounds__(256) void bwt_chunk_keys(Batch B, const uint32_t* __restrict__ cbp,
                                                      const uint32_t* __restrict__ cep)
{
    const uint32_t cb = cbp[blockIdx.x], ce = cep[blockIdx.x];
    const uint32_t s = cb / B.cap, n = B.n[s];
    const uint8_t* T = B.T + (size_t)s * B.cap;
    for (uint32_t j = cb + threadIdx.x; j < ce; j += 256) B.keys_a[j] = rot_key8_fast(T, n, B.vals_a[j] & kIdxMask);
}

// Runs of rotations whose 8-byte prefixes are equal, resolved right after the
// chunk sorts when short: at most kTieRunMax rotations, ordered by insertion
// on their cyclic text from byte kKeyBytes on, kTieCmpBytes at most per
// comparison (bzip2 orders the rotations of the block lexicographically).  A
// longer run, or one with a comparison still equal after kTieCmpBytes, is left
// to the device-wide tie rounds, whose result does not depend on the order
// the run is left in.
constexpr uint32_t kTieRunMax = 32;
constexpr uint32_t kTieCmpBytes = 64;

// -1 / 1: rotation i sorts before / after rotation j, given equal first
// kKeyBytes bytes; 0: still equal after kTieCmpBytes more
__device__ __forceinline__ int tie_cmp(const uint8_t* __restrict__ T, uint32_t n, uint32_t i, uint32_t j)
{
    uint32_t a = (i + kKeyBytes) % n, b = (j + kKeyBytes) % n;
    for (uint32_t d = 0; d < kTieCmpBytes; d += 8) {
        const uint64_t ka = rot_key8_fast(T, n, a), kb = rot_key8_fast(T, n, b);
        if (ka != kb) return ka < kb ? -1 : 1;
        a = (a + 8) % n;
        b = (b + 8) % n;
    }
    return 0;
}

// One thread per run of the tied list (the still-tied slots after the chunk
// sorts, in slot order; a run is consecutive slots of one prefix): the run's
// values in sa sorted in place.  The slots keep their flags, so tie rounds
// that still run (some run here too long or undecided: counted in *unres)
// re-sort the resolved runs to the same order; with *unres == 0 the host
// skips them.  A separate launch keeps the chunk sort's registers (inlined
// there, this code took it from 37 to 88 VGPRs and 8 to 5 waves per SIMD).
__global__ __launch_bounds__(256) void tie_runs_direct(Batch B, const uint32_t* __restrict__ cl,
                                                  const uint32_t* __restrict__ cnt_p, uint32_t* __restrict__ unres)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        const uint32_t slot = cl[c];
        const uint32_t s = slot / B.cap, n = B.n[s];
        const uint8_t* T = B.T + (size_t)s * B.cap;
        const uint64_t K = rot_key8_fast(T, n, B.sa[slot] & kIdxMask);
        if (c > 0 && cl[c - 1] == slot - 1 && rot_key8_fast(T, n, B.sa[slot - 1] & kIdxMask) == K) continue;
        uint32_t g = 1;
        while (c + g < cnt && g <= kTieRunMax && cl[c + g] == slot + g &&
               rot_key8_fast(T, n, B.sa[slot + g] & kIdxMask) == K)
            ++g;
        if (g > kTieRunMax) {
            atomicAdd(unres, 1u);
            continue;
        }
        uint32_t* sv = B.sa + slot;
        bool ok = true;
        for (uint32_t x = 1; x < g && ok; ++x) {
            const uint32_t vx = sv[x];
            uint32_t y = x;
            while (y > 0) {
                const int cmp = tie_cmp(T, n, sv[y - 1] & kIdxMask, vx & kIdxMask);
                if (cmp == 0) {  // undecided: the rounds re-sort the run (same elements, any order)
                    ok = false;
                    break;
                }
                if (cmp < 0) break;
                sv[y] = sv[y - 1];
                --y;
            }
            sv[y] = vx;
        }
        if (!ok) atomicAdd(unres, 1u);
    }
}

__device__ __forceinline__ void make_u2s(const Batch& B, uint32_t s, uint8_t* u2s, uint32_t lane, uint32_t* nin_out)
{
    uint32_t inu[8], nin = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        inu[q] = B.inuse[s * 8 + q];
        nin += __popc(inu[q]);
    }
    for (uint32_t c = lane; c < 256; c += 64) {
        uint32_t below = 0;
        for (uint32_t q = 0; q < (c >> 5); ++q) below += __popc(inu[q]);
        below += __popc(inu[c >> 5] & ((1u << (c & 31)) - 1u));
        u2s[c] = (uint8_t)below;
    }
    *nin_out = nin;
}

// ------------------------------------------------------------ placement --
// One sorted rotation placed: the one statement of what "induction" below
// says about a sorted slot (the final order, `ent`, itab).  Three callers: the
// chunk sorts' epilogue (PLACE), which holds the rotation when it is sorted;
// bwt_place_tied, over the slots tie_runs_direct re-ordered; bwt_place_sorted,
// over every slot of the batch, for the calls that leave the common path.
constexpr uint32_t kIndPend = 0xFFFFFFFFu;  // never an entry: nprev <= 3
constexpr uint32_t kIndIdx = 0xFFFFFu;      // n < nblock_max < 2^20
constexpr uint32_t kIndPlaced = 1u << 23;

// A stream's placement tables in LDS: tq, s0 (itab), cb[c] the compact index
// of bucket c's first sorted rotation (kModeSortA: the ranks count down from
// it), and the byte -> symbol map.
struct PlaceTabs {
    uint32_t tq_[256], s0_[256], cb_[256];
    uint8_t u2s_[256];
    __device__ __forceinline__ uint32_t tq(uint32_t c) const { return tq_[c]; }
    __device__ __forceinline__ uint32_t s0(uint32_t c) const { return s0_[c]; }
    __device__ __forceinline__ uint32_t cb(uint32_t c) const { return cb_[c]; }
    __device__ __forceinline__ uint32_t sym(uint32_t b) const { return u2s_[b]; }
};

// compact index of bucket c's first sorted rotation (an empty sorted part: never used)
__device__ __forceinline__ uint32_t place_cb(const uint32_t* __restrict__ it, const uint32_t* __restrict__ ab, bool rev,
                                            uint32_t c)
{
    const uint32_t u = rev ? 255u - c : c;
    return it[256 + u] + it[512 + u] + (rev ? ab[c] - 1u : 0u);
}

// by all TH threads of a workgroup, 256 entries whatever TH (the first wave
// also builds the symbol map); the caller's barrier publishes the tables
template <int TH>
__device__ __forceinline__ void place_tabs_load(const Batch& B, uint32_t s, uint32_t mode, PlaceTabs& P, uint32_t t)
{
    if (t < 64) {
        uint32_t nin;
        make_u2s(B, s, P.u2s_, t, &nin);
    }
    const uint32_t* it = B.itab + (size_t)s * 1024;
    for (uint32_t c = t; c < 256; c += TH) {
        P.tq_[c] = it[c];
        P.s0_[c] = it[768 + c];
        P.cb_[c] = place_cb(it, B.abcnt + (size_t)s * 512, mode == kModeSortA, c);
    }
}

// the same tables read where they lie, for the few slots of bwt_place_tied
struct PlaceTabsGlobal {
    const uint32_t* it;
    const uint32_t* ab;
    const uint32_t* inuse;
    bool rev;
    __device__ __forceinline__ uint32_t tq(uint32_t c) const { return it[c]; }
    __device__ __forceinline__ uint32_t s0(uint32_t c) const { return it[768 + c]; }
    __device__ __forceinline__ uint32_t cb(uint32_t c) const { return place_cb(it, ab, rev, c); }
    __device__ __forceinline__ uint32_t sym(uint32_t b) const
    {
        uint32_t below = __popc(inuse[b >> 5] & ((1u << (b & 31)) - 1u));
        for (uint32_t q = 0; q < (b >> 5); ++q) below += __popc(inuse[q]);
        return below;
    }
};

// T[i-4 .. i] of rotation i: two aligned dwords at a clamped address (the
// first four rotations wrap and read byte by byte), so that a caller can
// issue the loads of all its rotations before it uses any.
__device__ __forceinline__ const uint32_t* place_text_at(const uint8_t* __restrict__ T, uint32_t i)
{
    return (const uint32_t*)(T + ((i >= 4 ? i - 4 : 0u) & ~3u));
}
// x = T[i-4] | T[i-3] << 8 | T[i-2] << 16 | T[i-1] << 24, c = T[i]
__device__ __forceinline__ void place_text(const uint8_t* __restrict__ T, uint32_t n, uint32_t i, uint32_t w0, uint32_t w1,
                                           uint32_t& x, uint32_t& c)
{
    if (i >= 4) {
        const uint32_t sh = ((i - 4) & 3u) * 8u;
        const uint64_t d = (uint64_t)w0 | ((uint64_t)w1 << 32);
        x = (uint32_t)(d >> sh);
        c = (uint32_t)(d >> (sh + 32)) & 0xFFu;
    } else {
        x = 0;
        for (uint32_t r = 1; r <= 4; ++r) x |= (uint32_t)T[(i + 4 * n - r) % n] << (32 - 8 * r);
        c = T[i];
    }
}

// Sorted slot j of a stream (value v = i | T[i-1] << 24, x and c as above):
// its final position is known, so the symbol goes to LL there, origPtr is
// that position for rotation 0, and (unless the stream is sorted whole) the
// entry goes to its compact index, counted from cb[c] in the scan's direction.
template <class Tabs>
__device__ __forceinline__ void place_slot(const Tabs& P, uint32_t mode, uint32_t j, uint32_t v, uint32_t x, uint32_t c,
                                           uint8_t* __restrict__ LL, uint2* __restrict__ E, uint32_t* __restrict__ orig_ptr)
{
    const uint32_t r = j - P.s0(c), qq = P.tq(c) + r;
    LL[qq] = (uint8_t)P.sym(v >> 24);
    if ((v & kIdxMask) == 0) *orig_ptr = qq;
    if (mode != kModeFull)
        E[mode == kModeSortA ? P.cb(c) - r : P.cb(c) + r] =
            make_uint2(v | (3u << 20), ((x >> 16) & 0xFFu) | (((x >> 8) & 0xFFu) << 8) | ((x & 0xFFu) << 16) | (c << 24));
}

// Thread t's items of chunk [cb, cb + m), striped (item q is slot q * TH + t:
// coalesced): the values and their 8-byte keys rebuilt from the text; items
// past m get key ~0, value 0.  Every load is unconditional (clamped
// indices) and all of one kind are issued before any is used: one memory
// round trip for the values and one for the text of all IPT items (under
// per-item branches the compiler waited for each item's loads in turn: 2 IPT
// round trips).  BLOCKED: item q is slot t * IPT + q instead, the arrangement
// the block sort takes (IPT consecutive values per lane: the same lines, and
// no exchange through LDS afterwards).
template <int TH, int IPT, bool BLOCKED>
__device__ __forceinline__ void chunk_load(const Batch& B, uint32_t cb, uint32_t m, uint32_t t, uint64_t (&k)[IPT],
                                           uint32_t (&v)[IPT])
{
    const uint32_t s = cb / B.cap, n = B.n[s];
    const uint8_t* T = B.T + (size_t)s * B.cap;
    auto slot = [&](int q) { return BLOCKED ? t * IPT + q : q * TH + t; };
#pragma unroll
    for (int q = 0; q < IPT; ++q) v[q] = B.vals_a[cb + min(slot(q), m ? m - 1u : 0u)];
    uint32_t d[IPT][3];
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const uint32_t i = v[q] & kIdxMask;
        const uint32_t* w = (const uint32_t*)(T + ((i + 8u <= n ? i : 0u) & ~3u));
        d[q][0] = w[0];
        d[q][1] = w[1];
        d[q][2] = w[2];
    }
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const uint32_t j = slot(q), i = v[q] & kIdxMask;
        if (j >= m) {
            k[q] = ~0ull;
            v[q] = 0u;
        } else if (i + 8u <= n) {  // rot_key8_fast's fast path on the loaded dwords
            const uint32_t sh = (i & 3u) * 8u;
            const uint64_t x = (uint64_t)d[q][0] | ((uint64_t)d[q][1] << 32);
            k[q] = __builtin_bswap64(sh ? (x >> sh) | ((uint64_t)d[q][2] << (64u - sh)) : x);
        } else {
            k[q] = rot_key8_fast(T, n, i);
        }
    }
}

// The chunk's keys / values are loaded striped (element q * TH + t: coalesced),
// sorted (rocPRIM block merge sort: thread t ends with sorted positions
// t * IPT .. t * IPT + IPT - 1), the still-tied flags come from the
// neighbours in registers (each thread's edge keys through LDS), and (without
// PLACE) sa / uflag go back striped through LDS.  The sorted keys are not stored: the few
// consumers (tie groups) recompute them from the text (rot_key8).
//
// PLACE: the workgroup also places its rotations (place_slot) from the blocked
// arrangement, where it holds each one's value, its sorted slot and T[i] (the
// key's top byte); the stream's tables are loaded into LDS ahead of the sort
// (a chunk never spans streams).  T[i-4 .. i-2] are read again after the sort
// and not carried through it: a second value word would make rocPRIM's merge
// passes move 8-byte values.  Tied slots are placed in the provisional order;
// bwt_place_tied places them again once tie_runs_direct has ordered them.
// A placing sort loads blocked (chunk_load: no exchange) and writes sa only at
// its tied slots, which it appends to the tied list `tl` itself (length *tcnt,
// at most tcap entries): nothing after it on that path reads sa or uflag
// anywhere else.  A workgroup's entries are in slot order and contiguous (one
// atomic add per workgroup), which is what tie_runs_direct needs to see a run:
// a run never leaves its bucket, and a sort job (the [cb, ce) of a workgroup
// here) holds whole buckets.  When a run is left to
// the text rounds, which do read every slot, first_round sorts again without
// PLACE.
template <int TH, int IPT, bool PLACE>
__global__ __launch_bounds__(TH) void bwt_chunk_sort(Batch B, const uint32_t* __restrict__ cbp,
                                                     const uint32_t* __restrict__ cep, uint32_t nch, uint32_t per,
                                                     uint32_t* __restrict__ tl, uint32_t* __restrict__ tcnt, uint32_t tcap)
{
    // per > 0: XCD-aware order (workgroup b runs on XCD b % 8; chunks
    // x * per .. x * per + per - 1, consecutive and mostly of one stream, all
    // go to XCD x, so a stream's text is pulled into one L2)
    const uint32_t c = per ? (blockIdx.x & 7u) * per + (blockIdx.x >> 3) : blockIdx.x;
    if (c >= nch) return;
    static_assert(IPT == 2 || IPT == 4 || IPT == 8, "flags are packed 2, 4 or 8 per thread");
    using Sort = rocprim::block_sort<uint64_t, TH, IPT, uint32_t, rocprim::block_sort_algorithm::merge_sort>;
    using ExK = rocprim::block_exchange<uint64_t, TH, IPT>;
    using ExV = rocprim::block_exchange<uint32_t, TH, IPT>;
    constexpr uint32_t NI = TH * IPT;
    struct Xch {
        uint64_t first[TH], last[TH];
        uint32_t sv[NI];
        uint8_t fl[NI];
        // PLACE: whether a wave holds a tied slot, the tied counts per wave, the workgroup's place in the tied list
        alignas(16) uint32_t wany[TH / 64];
        uint32_t wsum[TH / 64], base;
    };
    __shared__ union alignas(16) {
        typename Sort::storage_type s;
        typename ExK::storage_type ek;
        typename ExV::storage_type ev;
        Xch x;
    } sm;
    __shared__ std::conditional_t<PLACE, PlaceTabs, char> P;
    const uint32_t cb = cbp[c], ce = cep[c], m = ce - cb, t = threadIdx.x;
    const uint32_t s = cb / B.cap, mode = PLACE ? B.bwt_mode[s] : 0u;
    // (the tables are published by the barrier after the sort, below: their
    // first use is place_slot in the epilogue, and with the blocked load no
    // barrier stands ahead of the sort's own)
    if constexpr (PLACE) place_tabs_load<TH>(B, s, mode, P, t);
    uint64_t k[IPT];
    uint32_t v[IPT];
    chunk_load<TH, IPT, PLACE>(B, cb, m, t, k, v);
    if constexpr (!PLACE) {
        // the sort's valid-item count refers to the blocked arrangement
        ExK().striped_to_blocked(k, k, sm.ek);
        __syncthreads();
        ExV().striped_to_blocked(v, v, sm.ev);
        __syncthreads();
    }
    Sort().sort(k, v, sm.s, m);
    __syncthreads();
    sm.x.first[t] = k[0];
    sm.x.last[t] = k[IPT - 1];
    __syncthreads();
    const uint64_t kprev = t ? sm.x.last[t - 1] : 0ull, knext = t + 1 < (uint32_t)TH ? sm.x.first[t + 1] : 0ull;
    uint32_t nt = 0;
    uint64_t fpack = 0;
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
        const uint32_t pos = t * IPT + q;
        const uint64_t lo = q ? k[q - 1] : kprev, hi = q + 1 < IPT ? k[q + 1] : knext;
        const bool f = pos < m && ((pos > 0 && lo == k[q]) || (pos + 1 < m && hi == k[q]));
        nt += f ? 1u : 0u;
        fpack |= (uint64_t)(f ? 1u : 0u) << (8 * q);
    }
    if constexpr (PLACE) {
        const uint8_t* T = B.T + (size_t)s * B.cap;
        uint32_t w0[IPT], w1[IPT];
#pragma unroll
        for (int q = 0; q < IPT; ++q) {  // (items past m hold value 0: the loads stay inside the text)
            const uint32_t* w = place_text_at(T, v[q] & kIdxMask);
            w0[q] = w[0];
            w1[q] = w[1];
        }
        // The tied slots, while the text loads are under way.  The branch is
        // uniform: a word per wave in LDS and one barrier.  Thread t's entries
        // follow those of the threads below it.
        const uint32_t lane = t & 63u, wave = t >> 6;
        const uint32_t wave_tied = __any(nt) ? 1u : 0u;
        if (lane == 0) sm.x.wany[wave] = wave_tied;
        __syncthreads();
        uint32_t any_tied = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)TH / 64; ++w) any_tied |= sm.x.wany[w];
        if (any_tied) {
            uint32_t inc = nt;
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t a = __shfl_up(inc, d);
                if ((int)lane >= d) inc += a;
            }
            if (lane == 63) sm.x.wsum[wave] = inc;
            __syncthreads();
            uint32_t at = inc - nt, tot = 0;
            for (uint32_t w = 0; w < (uint32_t)TH / 64; ++w) {
                if (w < wave) at += sm.x.wsum[w];
                tot += sm.x.wsum[w];
            }
            if (t == 0) sm.x.base = atomicAdd(tcnt, tot);
            __syncthreads();
            at += sm.x.base;
#pragma unroll
            for (int q = 0; q < IPT; ++q) {
                if ((fpack >> (8 * q)) & 1u) {
                    B.sa[cb + t * IPT + q] = v[q];
                    if (at < tcap) tl[at] = cb + t * IPT + q;
                    ++at;
                }
            }
        }
        const size_t o = (size_t)s * B.cap;
        const uint32_t n = B.n[s], j0 = cb - (uint32_t)o + t * IPT;
        uint8_t* LL = (uint8_t*)B.mtfv + o;
        uint2* E = B.ent + o;
#pragma unroll
        for (int q = 0; q < IPT; ++q) {
            if (t * IPT + q < m) {
                uint32_t x, ci;
                place_text(T, n, v[q] & kIdxMask, w0[q], w1[q], x, ci);
                place_slot(P, mode, j0 + q, v[q], x, (uint32_t)(k[q] >> 56), LL, E, B.orig_ptr + s);
            }
        }
        return;
    }
    if constexpr (IPT == 2) {
        *(uint2*)&sm.x.sv[t * IPT] = make_uint2(v[0], v[1]);
        *(uint16_t*)&sm.x.fl[t * IPT] = (uint16_t)fpack;
    } else {
#pragma unroll
        for (int q = 0; q < IPT; q += 4) *(uint4*)&sm.x.sv[t * IPT + q] = make_uint4(v[q], v[q + 1], v[q + 2], v[q + 3]);
        if constexpr (IPT == 8) *(uint64_t*)&sm.x.fl[t * IPT] = fpack;
        else *(uint32_t*)&sm.x.fl[t * IPT] = (uint32_t)fpack;
    }
    __syncthreads();
    for (uint32_t j = t; j < m; j += TH) {
        B.sa[cb + j] = sm.x.sv[j];
        B.uflag[cb + j] = sm.x.fl[j];
    }
    if (__any(nt)) {
        for (int d = 32; d > 0; d >>= 1) nt += __shfl_xor(nt, d);
        if ((threadIdx.x & 63) == 0 && nt) atomicAdd(&B.done[cb / B.cap], nt);
    }
}

// the first-round key of rotation i of stream s: its 8-byte prefix, big endian
__device__ __forceinline__ uint64_t rot_key8(const Batch& B, uint32_t s, uint32_t i)
{
    const uint32_t n = B.n[s];
    const uint8_t* T = B.T + (size_t)s * B.cap;
    uint64_t k = 0;
    uint32_t j = i;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        k = (k << 8) | T[j];
        j = j + 1 == n ? 0u : j + 1;
    }
    return k;
}

// still-tied flag of sorted position j of a chunk [cb, ce) (keys_b)
__device__ __forceinline__ uint8_t tied_flag(const uint64_t* __restrict__ K, uint32_t cb, uint32_t ce, uint32_t j,
                                             uint64_t k)
{
    return ((j > cb && K[j - 1] == k) || (j + 1 < ce && K[j + 1] == k)) ? 1 : 0;
}

// flags of the chunks sorted by rocPRIM (one workgroup per chunk)
__global__ __launch_bounds__(256) void bwt_chunk_flags(Batch B, const uint32_t* __restrict__ cbp,
                                                       const uint32_t* __restrict__ cep)
{
    const uint32_t cb = cbp[blockIdx.x], ce = cep[blockIdx.x];
    uint32_t nt = 0;
    for (uint32_t j = cb + threadIdx.x; j < ce; j += blockDim.x) {
        const uint8_t f = tied_flag(B.keys_b, cb, ce, j, B.keys_b[j]);
        B.uflag[j] = f;
        nt += f;
    }
    for (int d = 32; d > 0; d >>= 1) nt += __shfl_xor(nt, d);
    if ((threadIdx.x & 63) == 0 && nt) atomicAdd(&B.done[cb / B.cap], nt);
}

// The tied list (slots whose 8-byte prefix is shared), in slot order: per
// stream offsets of the tie counts (one workgroup), then each stream with
// ties compacts its flags (B.done = ties per stream -> exclusive offsets).
__global__ __launch_bounds__(1024) void tie_offsets(Batch B, uint32_t* __restrict__ total)
{
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, ns = B.nstreams;
    const uint32_t per = (ns + 1023) / 1024;
    const uint32_t s0 = min(ns, t * per), s1 = min(ns, s0 + per);
    uint32_t sum = 0;
    for (uint32_t s = s0; s < s1; ++s) sum += B.done[s];
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t acc = part[t] - sum;
    for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t c = B.done[s];
        B.done[s] = c ? acc : ~0u;
        acc += c;
    }
    if (t == 1023) *total = part[1023];
}

__global__ __launch_bounds__(256) void tie_compact(Batch B, uint32_t* __restrict__ cl)
{
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t carry;
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t base = B.done[s];
    if (base == ~0u) return;
    const uint32_t n = B.nsub[s], o = s * B.cap;
    if (t == 0) carry = base;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < n; j0 += 256 * 16) {
        const uint32_t j = j0 + 16 * t;
        uint4 w = make_uint4(0, 0, 0, 0);
        if (j < n) w = *(const uint4*)(B.uflag + o + j);  // uflag is zero past n (cap is a multiple of 256)
        const uint32_t c = __popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w);  // flags are 0 / 1 bytes
        uint32_t inc = c;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t a = __shfl_up(inc, d);
            if ((int)lane >= d) inc += a;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t at = carry + inc - c;
        for (uint32_t w2 = 0; w2 < wave; ++w2) at += wsum[w2];
        if (c) {
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
            for (int q = 0; q < 16; ++q)
                if ((words[q >> 2] >> (8 * (q & 3))) & 1u) cl[at++] = o + j + q;
        }
        __syncthreads();
        if (t == 255) carry = at;
        __syncthreads();
    }
}

// After the first sort (6-byte prefixes, sa): rank[sa[j]] = first
// sorted position of j's group, uflag[slot] = 1 where j's group has more than
// one rotation.  Tiles of 1024 consecutive positions keep every load
// coalesced; the group start is a running max carried across tiles.
__global__ __launch_bounds__(1024) void bwt_rank0(Batch B)
{
    __shared__ uint32_t wmax[16];
    __shared__ uint32_t carry;
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t n = B.n[s];
    const size_t o = (size_t)s * B.cap;
    const uint32_t* SA = B.sa + o;
    auto K = [&](uint32_t j) { return rot_key8(B, s, SA[j] & kIdxMask); };  // keys from the text (fallback path)
    if (t == 0) carry = 0;
    __syncthreads();
    for (uint32_t j0 = 0; j0 < n; j0 += 1024) {
        const uint32_t j = j0 + t;
        bool head = false, next_head = true;
        if (j < n) {
            // Flag contract: the chunk sort flags every slot whose 8-byte key
            // equals a neighbour's; tie_runs_direct re-orders such runs from
            // the text but leaves their flags set, so the rounds below re-sort
            // them to the same order.  A slot joins its predecessor's group
            // when it is flagged and its key equals the predecessor's.  Equal
            // keys never straddle a chunk (chunks end at bucket ends), so an
            // equal key implies the flag; the flag test only saves the key
            // comparison for unflagged slots.  Both flags are read before the
            // barrier ahead of the rewrite.
            const bool fj = B.uflag[o + j] != 0;
            const bool fn = j + 1 < n && B.uflag[o + j + 1] != 0;
            const uint64_t k = K(j);
            head = j == 0 || !fj || k != K(j - 1);
            next_head = j + 1 >= n || !fn || K(j + 1) != k;
        }
        uint32_t v = head ? j : 0u;
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t u = __shfl_up(v, off);
            if ((int)lane >= off) v = max(v, u);
        }
        if (lane == 63) wmax[wave] = v;
        __syncthreads();
        uint32_t pre = carry;
        for (uint32_t w = 0; w < wave; ++w) pre = max(pre, wmax[w]);
        const uint32_t g = max(pre, v);
        if (j < n) {
            B.rank[o + (SA[j] & kIdxMask)] = g;
            B.uflag[o + j] = (head && next_head) ? 0 : 1;
        }
        __syncthreads();
        if (t == 1023) carry = g;
        __syncthreads();
    }
}

// Tie resolution by more text.  After the first sort only the rotations in
// a group of equal 6-byte prefixes are still unordered (2.4 % on light-field
// symbols, 0.01 % after 11 bytes): they are re-sorted inside their groups by
// the next 5 bytes of text, kTextRounds times, without the inverse suffix
// array (a random 4-byte scatter per rotation) that prefix doubling needs.
// Only ties that survive those rounds (long repeats) fall back to doubling.
constexpr int kTextRounds = 3;
constexpr uint32_t kTextBytes = 5;

__global__ __launch_bounds__(256) void text_gather_keys(Batch B, const uint32_t* __restrict__ cl,
                                                        const uint32_t* __restrict__ cnt_p, uint64_t* __restrict__ gk)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        const uint32_t slot = cl[c];
        gk[c] = rot_key8(B, slot / B.cap, B.sa[slot] & kIdxMask);
    }
}

// group starts of the tied list (equal keys, same stream)
__global__ __launch_bounds__(256) void text_bounds(Batch B, const uint32_t* __restrict__ cl,
                                                   const uint32_t* __restrict__ cnt_p, const uint64_t* __restrict__ gk,
                                                   uint32_t* __restrict__ bnd)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x)
        bnd[c] = (c == 0 || gk[c] != gk[c - 1] || cl[c] / B.cap != cl[c - 1] / B.cap) ? 1u : 0u;
}

// key = (group index, next kTextBytes of the rotation at offset `off`)
__global__ __launch_bounds__(256) void text_keys(Batch B, const uint32_t* __restrict__ cl,
                                                 const uint32_t* __restrict__ cnt_p, const uint32_t* __restrict__ gidx,
                                                 uint32_t off, uint32_t tb)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        const uint32_t slot = cl[c];
        const uint32_t s = slot / B.cap;
        const uint32_t n = B.n[s];
        const uint8_t* T = B.T + (size_t)s * B.cap;
        const uint32_t v = B.sa[slot];
        uint32_t j = (v & kIdxMask) + (off % n);
        if (j >= n) j -= n;
        uint64_t k = 0;
#pragma unroll
        for (uint32_t q = 0; q < kTextBytes; ++q) {
            if (q < tb) {
                k = (k << 8) | T[j];
                j = j + 1 == n ? 0 : j + 1;
            }
        }
        B.keys_a[c] = ((uint64_t)(gidx[c] - 1) << (8 * tb)) | k;
        B.vals_a[c] = v;
    }
}

// refined order back into sa; still-tied flags of the list
__global__ __launch_bounds__(256) void text_write(Batch B, const uint32_t* __restrict__ cl,
                                                  const uint32_t* __restrict__ cnt_p)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        B.sa[cl[c]] = B.vals_b[c];
        const uint64_t k = B.keys_b[c];
        B.uflag[c] = ((c > 0 && B.keys_b[c - 1] == k) || (c + 1 < cnt && B.keys_b[c + 1] == k)) ? 1 : 0;
    }
}

// fallback to doubling: rank[i] = sorted slot of rotation i for every rotation
// (the tied ones are fixed up to their group start by text_rank_tied)
__global__ __launch_bounds__(256) void bwt_rank_all(Batch B, size_t N)
{
    for (size_t slot = blockIdx.x * (size_t)blockDim.x + threadIdx.x; slot < N;
         slot += (size_t)gridDim.x * blockDim.x) {
        const uint32_t s = (uint32_t)(slot / B.cap);
        const uint32_t j = (uint32_t)(slot - (size_t)s * B.cap);
        const uint32_t n = (B.flags[s] & kFlagHost) ? 0u : B.n[s];
        if (j < n) B.rank[(size_t)s * B.cap + (B.sa[slot] & kIdxMask)] = j;
    }
}

__global__ __launch_bounds__(256) void text_head_slots(const uint32_t* __restrict__ cl, const uint32_t* __restrict__ cnt_p,
                                                       const uint32_t* __restrict__ bnd, uint32_t* __restrict__ hv)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x)
        hv[c] = bnd[c] ? cl[c] : 0u;
}

__global__ __launch_bounds__(256) void text_rank_tied(Batch B, const uint32_t* __restrict__ cl,
                                                      const uint32_t* __restrict__ cnt_p, const uint32_t* __restrict__ hvs)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        const uint32_t head = hvs[c];
        const size_t o = (size_t)(head / B.cap) * B.cap;
        B.rank[o + (B.sa[cl[c]] & kIdxMask)] = (uint32_t)(head - o);
    }
}

// keys of a compacted doubling round: (stream slot of the group start,
// rank[i + h]) -- groups never mix, and inside a group the order is by the
// rank of the rotation h further on
__global__ __launch_bounds__(256) void bwt_comp_keys(Batch B, const uint32_t* __restrict__ cl,
                                                     const uint32_t* __restrict__ cnt_p, uint32_t h)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        const uint32_t slot = cl[c];
        const uint32_t s = slot / B.cap;
        const size_t o = (size_t)s * B.cap;
        const uint32_t n = B.n[s];
        const uint32_t v = B.sa[slot];
        const uint32_t i = v & kIdxMask;
        uint32_t i2 = i + (h % n);
        if (i2 >= n) i2 -= n;
        B.keys_a[c] = ((uint64_t)(o + B.rank[o + i]) << 20) | B.rank[o + i2];
        B.vals_a[c] = v;
    }
}

// write the refined order back into sa and mark the new group heads
__global__ __launch_bounds__(256) void bwt_comp_heads(Batch B, const uint32_t* __restrict__ cl,
                                                      const uint32_t* __restrict__ cnt_p, uint32_t* __restrict__ hv)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        B.sa[cl[c]] = B.vals_b[c];
        const bool head = c == 0 || B.keys_b[c] != B.keys_b[c - 1];
        hv[c] = head ? cl[c] : 0u;
    }
}

// new ranks (slot of the new group head) and the still-tied flags
__global__ __launch_bounds__(256) void bwt_comp_rank(Batch B, const uint32_t* __restrict__ cnt_p,
                                                     const uint32_t* __restrict__ hvs)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        const uint32_t head_slot = hvs[c];
        const uint32_t s = head_slot / B.cap;
        const size_t o = (size_t)s * B.cap;
        B.rank[o + (B.vals_b[c] & kIdxMask)] = (uint32_t)(head_slot - o);
        const bool head = c == 0 || B.keys_b[c] != B.keys_b[c - 1];
        const bool next_head = c + 1 >= cnt || B.keys_b[c + 1] != B.keys_b[c];
        B.uflag[c] = (head && next_head) ? 0 : 1;
    }
}

// rotations still tied after h covers the whole block: equal rotations of a
// periodic block -> the host library produces that stream
__global__ __launch_bounds__(256) void bwt_flag_periodic(Batch B, const uint32_t* __restrict__ cl,
                                                         const uint32_t* __restrict__ cnt_p)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x)
        atomicOr(&B.flags[cl[c] / B.cap], kFlagHost);
}

// ------------------------------------------------------------ induction --
// Placement (above) + bwt_induce: the final order from the sorted rotations.
// In the final order (position q) bucket c (first byte c) holds its A
// rotations, then its B rotations.  One type is sorted (sa); the other is
// placed by one scan: kModeSortB scans left to right placing the A rotations,
// kModeSortA scans right to left placing the B rotations.  In "scan order" v
// (q, or n - 1 - q) with bytes mirrored the same way (x' = x, or 255 - x),
// bucket u = c' starts with its placed part, and the rotation i met in bucket u
// induces i - 1 when b' = T[i-1]' > u, or b' == u and i was placed itself;
// i - 1 takes the next free slot of bucket b''s placed part (head[b']).
//
// The output is ll[]: at every final position the symbol of the byte before
// its rotation, and origPtr, the position of rotation 0.  Whoever places a
// rotation holds that byte and writes the symbol there: place_slot for the
// sorted rotations, bwt_induce for each rotation it induces.
//
// A placed rotation p induces in its turn only when p - 1 is placed too, by
// the rule above when T[p-1]' >= T[p]': it is "live".  The others are dead:
// nothing reads them again (on 16-bit little-endian symbols the placed
// rotations start at the high bytes and 98 % of them are dead), so the scan
// does not visit them.  It runs over a compact index: for each bucket u in
// scan order cl[u] slots for its live rotations, from cs[u], then its sorted
// rotations in scan order; bwt_bucket counts cl[] with the same byte rule.
// Beside head[b'] the scan keeps chead[b'], the next free live slot.
//
// Entries (`ent`, by compact index): lo = i | nprev << 20 | placed << 23 |
// T[i-1] << 24 (the sort value's layout, bits 20-23 free since n < 2^20),
// hi = T[i-2] | T[i-3] << 8 | T[i-4] << 16 | T[i] << 24: nprev of the three
// bytes before T[i-1] are valid (3 for a sorted rotation, one fewer per
// induction: a longer chain of placed rotations reads the text), and T[i] is
// the rotation's bucket.  place_slot writes the sorted entries; the live slots
// start as kIndPend (bwt_pend_live, or bwt_place_sorted where it runs) and
// bwt_induce fills them as it goes.
//
// itab (bwt_bucket), 256 words each: tq[c] the final position of bucket c's
// first sorted rotation, cs[u], cl[u], and s0[c] the sa slot of bucket c's
// first sorted rotation.
constexpr uint32_t kPlaceChunk = 2048;  // (1 024, 4 096, 8 192 equal or slower end to end)  // sorted slots / positions per bwt_place_sorted workgroup

// One workgroup per kPlaceChunk sorted slots and compact scan indices of a
// stream, the chunks of a stream consecutive on one XCD (workgroup w runs on
// XCD w % 8): the text reads are random inside the stream, so a stream's text
// should stay in one L2 while its chunks run.
__global__ __launch_bounds__(256) void bwt_place_sorted(Batch B, uint32_t chunks)
{
    __shared__ PlaceTabs P;
    __shared__ uint32_t cs[256], cl[256];
    const uint32_t t = threadIdx.x, k = blockIdx.x >> 3;
    const uint32_t s = (blockIdx.x & 7u) + 8u * (k / chunks), base = (k % chunks) * kPlaceChunk;
    if (s >= B.nstreams || (B.flags[s] & kFlagHost)) return;
    const uint32_t n = B.n[s], ns = B.nsub[s], mode = B.bwt_mode[s];
    if (base >= n) return;
    place_tabs_load<256>(B, s, mode, P, t);
    cs[t] = B.itab[(size_t)s * 1024 + 256 + t];
    cl[t] = B.itab[(size_t)s * 1024 + 512 + t];
    __syncthreads();
    const size_t o = (size_t)s * B.cap;
    const uint8_t* T = B.T + o;
    uint8_t* LL = (uint8_t*)B.mtfv + o;  // the BWT output symbols (mtf_last<true> and mtf_win read them)
    uint2* E = B.ent + o;
    // the sorted slots [base, base + kPlaceChunk): sa, then T[i-4 .. i], all
    // loads issued before any is used
    constexpr int K = kPlaceChunk / 256;
    uint32_t v[K], w0[K], w1[K];
#pragma unroll
    for (int q = 0; q < K; ++q) v[q] = B.sa[o + min(base + q * 256 + t, ns ? ns - 1 : 0u)];
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const uint32_t* w = place_text_at(T, v[q] & kIdxMask);
        w0[q] = w[0];
        w1[q] = w[1];
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
        const uint32_t j = base + q * 256 + t;
        if (j >= ns) break;
        uint32_t x, c;
        place_text(T, n, v[q] & kIdxMask, w0[q], w1[q], x, c);
        place_slot(P, mode, j, v[q], x, c, LL, E, B.orig_ptr + s);
    }
    if (mode == kModeFull) return;
    // the live slots among the compact indices [base, base + kPlaceChunk): of
    // the buckets overlapping the range, from the last one starting at or
    // before base (every live range lies below the compact length)
    const uint32_t end = base + kPlaceChunk;
    uint32_t lo = 0, hi = 255;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (cs[mid] <= base) lo = mid;
        else hi = mid - 1;
    }
    for (uint32_t u = lo; u < 256 && cs[u] < end; ++u)
        for (uint32_t q = max(cs[u], base) + t; q < min(cs[u] + cl[u], end); q += 256) E[q] = make_uint2(kIndPend, 0u);
}

// The fused path's two small kernels.  bwt_pend_live: kIndPend into a
// stream's live slots (one workgroup per stream, a wave per scan bucket);
// they and the sorted slots are disjoint compact indices, so its order against
// the sorts does not matter.  bwt_place_tied: the slots of the tied list placed
// again from sa, after tie_runs_direct: a run keeps its slots and positions,
// only which rotation sits in each changes, so overwriting is enough.
__global__ __launch_bounds__(256) void bwt_pend_live(Batch B)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x & 63;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t n = B.n[s];
    if (n == 0 || B.bwt_mode[s] == kModeFull) return;
    __shared__ uint32_t c0[256], c1[256];
    const uint32_t* it = B.itab + (size_t)s * 1024;
    uint2* E = B.ent + (size_t)s * B.cap;
    c0[threadIdx.x] = it[256 + threadIdx.x];
    c1[threadIdx.x] = min(it[256 + threadIdx.x] + it[512 + threadIdx.x], n);  // (every live range lies below the compact length <= n)
    __syncthreads();
    for (uint32_t u = threadIdx.x >> 6; u < 256; u += 4)
        for (uint32_t q = c0[u] + lane; q < c1[u]; q += 64) E[q] = make_uint2(kIndPend, 0u);
}

__global__ __launch_bounds__(256) void bwt_place_tied(Batch B, const uint32_t* __restrict__ cl,
                                                      const uint32_t* __restrict__ cnt_p)
{
    const uint32_t cnt = *cnt_p;
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cnt; c += gridDim.x * blockDim.x) {
        const uint32_t slot = cl[c];
        const uint32_t s = slot / B.cap, n = B.n[s], mode = B.bwt_mode[s];
        const size_t o = (size_t)s * B.cap;
        const uint8_t* T = B.T + o;
        const uint32_t v = B.sa[slot], i = v & kIdxMask;
        const uint32_t* w = place_text_at(T, i);
        uint32_t x, ch;
        place_text(T, n, i, w[0], w[1], x, ch);
        const PlaceTabsGlobal P{B.itab + (size_t)s * 1024, B.abcnt + (size_t)s * 512, B.inuse + s * 8, mode == kModeSortA};
        place_slot(P, mode, slot - (uint32_t)o, v, x, ch, (uint8_t*)B.mtfv + o, B.ent + o, B.orig_ptr + s);
    }
}

// bwt_induce: one wave per stream scans the compact index, in blocks of
// kIndSlices slices of 64 indices through an LDS ring of two blocks: live
// entries placed into the current or the next block go to the ring, those
// further ahead to `ent`; while a block is scanned the next block's entries
// are loaded (LDS-DMA, 16 bytes per lane) and written into the ring after the
// scan (kIndPend = not placed yet).  Every induced rotation's symbol goes to
// ll[] at its final position (head[b'] + rank: the lanes of one b' store
// consecutive bytes); only a live one also gets an entry, at chead[b'] + its
// rank among the live ones.  The inducing lanes of a slice are ranked per b'
// with one ballot per distinct b' (the predecessors of a run of sorted
// rotations take few distinct bytes), so the slots follow the scan order; an
// entry still pending when its slice is scanned is placed by an earlier lane
// of the same slice: the step then runs in rounds up to its first pending
// lane.  The counts are checked as the scan goes (no slot past its bucket's
// part, no live slot left pending) and at its end (every head at the end of
// its part): a stream that fails goes to the host library.
constexpr uint32_t kIndSlices = 8;
constexpr uint32_t kIndBlock = 64 * kIndSlices;
constexpr int kIndStepSlices = 4;  // slices scanned together (2 and 8 measured slower in the pipeline)
constexpr uint32_t kIndRing = 2 * kIndBlock;

// LDS-DMA of 16 bytes per lane into LDS at `lds` + 16 * lane, from L2 (sc1:
// the entries were written by this wave earlier, and a line may sit in the
// L1 from the previous block's load).  Inline asm: the compiler does not
// track the DMA, so nothing of it ties up VGPRs while the wave works
// (bwt_induce waits with vm_drain before it reads the staged entries).
__device__ __forceinline__ void glds16(const void* g, const void* lds)
{
    const uint32_t m0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(size_t)(const __attribute__((address_space(3))) void*)lds);
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off sc1" ::"s"(m0), "v"(g) : "memory", "m0");
}

__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__global__ __launch_bounds__(64) void bwt_induce(Batch B)
{
    __shared__ uint32_t head[256], hlim[256];    // next free scan position of bucket u's placed part, and its end
    __shared__ uint32_t chead[256], clim[256];   // next free compact index of bucket u's live slots, and their end
    __shared__ uint2 ring[kIndRing];
    __shared__ __attribute__((aligned(16))) uint2 stg[kIndBlock];  // the next block's entries
    __shared__ uint8_t u2s[256];
    const uint32_t s = blockIdx.x, lane = threadIdx.x;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t n = B.n[s];
    const uint32_t mode = B.bwt_mode[s];
    if (n == 0 || mode == kModeFull) return;  // kModeFull: the placement wrote the final order
    const bool rev = mode == kModeSortA;      // right to left, mirrored bytes
    const uint32_t mir = rev ? 255u : 0u;
    const size_t o = (size_t)s * B.cap;
    uint8_t* LL = (uint8_t*)B.mtfv + o;  // the BWT output symbols (mtf_last<true> and mtf_win read them)
    uint2* E = B.ent + o;
    const uint8_t* T = B.T + o;
    uint32_t nin;
    make_u2s(B, s, u2s, lane, &nin);
    const bool u2s_id = nin == 256;  // every byte in use: the map is the identity
    const uint32_t* it = B.itab + (size_t)s * 1024;
    // the compact scan's length: the end of the last bucket's sorted part
    const uint32_t nc = min(n, it[256 + 255] + it[512 + 255] + B.abcnt[(size_t)s * 512 + (rev ? 0u : 256u) + (255u ^ mir)]);
    {  // head[u] = scan-order start of bucket u (its placed part comes first)
        uint32_t nt[4], np[4], l = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t u = 4 * lane + q, c = u ^ mir;
            const uint32_t na = B.abcnt[(size_t)s * 512 + c], nb = B.abcnt[(size_t)s * 512 + 256 + c];
            nt[q] = na + nb;
            np[q] = rev ? nb : na;
            l += nt[q];
            const uint32_t c0 = it[256 + u], c1 = c0 + it[512 + u];
            chead[u] = c0;
            clim[u] = min(c1, nc);
        }
        uint32_t x = l;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d);
            if ((int)lane >= d) x += y;
        }
        x -= l;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            head[4 * lane + q] = x;
            hlim[4 * lane + q] = x + np[q];
            x += nt[q];
        }
    }
    for (uint32_t i = lane; i < kIndRing; i += 64) ring[i].x = kIndPend;
    __syncthreads();
    // `ent` is in scan order; ll[] is in final order: position n - 1 - v for
    // scan position v of a right-to-left scan
    const uint32_t qa = rev ? n - 1 : 0u;
    auto qof = [&](uint32_t v) { return rev ? qa - v : v; };
    const uint32_t qmax = B.cap - 2;
    auto issue = [&](uint32_t vb) {  // the block at vb into stg (clamped: every lane loads)
#pragma unroll
        for (uint32_t j = 0; j < kIndBlock / 128; ++j) glds16(E + min(vb + 128 * j + 2 * lane, qmax), &stg[128 * j]);
    };
    auto stage = [&](uint32_t vb) {  // into the ring: entries known when loaded
        vm_drain();
        uint2 x[kIndSlices];
#pragma unroll
        for (uint32_t k = 0; k < kIndSlices; ++k) x[k] = stg[64 * k + lane];
        asm volatile("" ::: "memory");  // every read issued before the first write
#pragma unroll
        for (uint32_t k = 0; k < kIndSlices; ++k) {
            const uint32_t v = vb + 64 * k + lane;
            if (v < nc && x[k].x != kIndPend) ring[v % kIndRing] = x[k];
        }
    };
    issue(0);
    stage(0);
    bool bad = false;  // inconsistent counts or a pending entry no earlier lane places (never)
    uint32_t org = ~0u;
    for (uint32_t v0 = 0; v0 < nc && !bad; v0 += kIndBlock) {
        // the next block's ring slots held the previous block: not placed yet
#pragma unroll
        for (uint32_t k = 0; k < kIndSlices; ++k) ring[(v0 + kIndBlock + 64 * k + lane) % kIndRing].x = kIndPend;
        const bool more = v0 + kIndBlock < nc;
        if (more) issue(v0 + kIndBlock);
        // steps of kIndStepSlices slices: item k of lane l is compact index
        // vs + 64 k + l, and the scan order is (k, l)
        for (uint32_t vs = v0; vs < min(nc, v0 + kIndBlock) && !bad; vs += 64 * kIndStepSlices) {
            constexpr int KS = kIndStepSlices;
            uint2 e[KS];
            uint64_t todo[KS];
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                const uint32_t v = vs + 64 * k + lane;
                todo[k] = __ballot(v < nc);
                e[k] = ring[v % kIndRing];
            }
            // rounds up to the first pending entry: one round unless an entry
            // of the step is placed by an earlier one of the same step
            for (;;) {
                uint64_t act[KS], pend[KS], anyp = 0;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    pend[k] = __ballot(e[k].x == kIndPend) & todo[k];
                    anyp |= pend[k];
                }
                if (!anyp) {
#pragma unroll
                    for (int k = 0; k < KS; ++k) act[k] = todo[k];
                } else {
                    bool seen = false;
                    uint64_t any = 0;
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        const uint64_t pk = pend[k];
                        act[k] = seen ? 0ull : (pk ? todo[k] & ((pk & (0ull - pk)) - 1ull) : todo[k]);
                        seen = seen || pk;
                        any |= act[k];
                    }
                    if (!any) {
                        bad = true;
                        break;
                    }
                }
                uint32_t b[KS];
                bool ind[KS];
                uint64_t rem[KS], left = 0;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    const bool me = (act[k] >> lane) & 1u;
                    const uint32_t lo = e[k].x, hi = e[k].y;
                    b[k] = (lo >> 24) ^ mir;
                    const uint32_t u = (hi >> 24) ^ mir;
                    ind[k] = me && (b[k] > u || (b[k] == u && (lo & kIndPlaced)));
                    rem[k] = __ballot(ind[k]);
                    left |= rem[k];
                }
                if (left) {
                    // the induced rotation p = i - 1: its entry (T[p-1] =
                    // T[i-2] ... and T[p] = T[i-1]), and whether it is live
                    bool np0 = false;
                    uint32_t plo[KS], phi[KS];
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        const uint32_t lo = e[k].x, hi = e[k].y;
                        const uint32_t idx = lo & kIndIdx, np = (lo >> 20) & 7u;
                        const uint32_t p = idx ? idx - 1 : n - 1;
                        plo[k] = p | ((np - 1) << 20) | kIndPlaced | ((hi & 0xFFu) << 24);
                        phi[k] = ((hi >> 8) & 0xFFFFu) | (lo & 0xFF000000u);
                        np0 = np0 || (ind[k] && np == 0);
                    }
                    if (__any(np0)) {
#pragma unroll
                        for (int k = 0; k < KS; ++k) {
                            const uint32_t lo = e[k].x;
                            if (!ind[k] || ((lo >> 20) & 7u)) continue;
                            // a chain of placed rotations longer than the carried bytes
                            const uint32_t idx = lo & kIndIdx, p = idx ? idx - 1 : n - 1;
                            const uint32_t x = text_prev4(T, n, p + 1);  // T[p-1] .. T[p-4]
                            plo[k] = p | (3u << 20) | kIndPlaced | ((x & 0xFFu) << 24);
                            phi[k] = ((x >> 8) & 0xFFFFFFu) | (lo & 0xFF000000u);
                        }
                    }
                    bool live[KS];
                    uint64_t lmask[KS];
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        live[k] = ind[k] && ((plo[k] >> 24) ^ mir) >= b[k];
                        lmask[k] = __ballot(live[k]);
                    }
                    // ranks among the inducing entries with the same b, in
                    // scan order, and among the live ones of them: a round of
                    // ballots per distinct b
                    uint32_t rank[KS], tot_of[KS], lrank[KS], ltot_of[KS];
                    bool inm[KS];
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        rank[k] = 0;
                        tot_of[k] = 0;
                        lrank[k] = 0;
                        ltot_of[k] = 0;
                    }
                    while (left) {
                        uint32_t bl = 0;
                        bool got = false;
#pragma unroll
                        for (int k = 0; k < KS; ++k)
                            if (!got && rem[k]) {
                                bl = (uint32_t)__builtin_amdgcn_readlane((int)b[k], __builtin_ctzll(rem[k]));
                                got = true;
                            }
                        uint32_t sb = 0, sl = 0;
                        left = 0;
#pragma unroll
                        for (int k = 0; k < KS; ++k) {
                            const uint64_t m = __ballot(b[k] == bl) & rem[k], ml = m & lmask[k];
                            inm[k] = (m >> lane) & 1u;
                            const uint32_t r =
                                sb + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                            const uint32_t rl =
                                sl + __builtin_amdgcn_mbcnt_hi((uint32_t)(ml >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ml, 0u));
                            rank[k] = inm[k] ? r : rank[k];
                            lrank[k] = inm[k] ? rl : lrank[k];
                            sb += (uint32_t)__popcll(m);
                            sl += (uint32_t)__popcll(ml);
                            rem[k] &= ~m;
                            left |= rem[k];
                        }
#pragma unroll
                        for (int k = 0; k < KS; ++k) {
                            tot_of[k] = inm[k] ? sb : tot_of[k];
                            ltot_of[k] = inm[k] ? sl : ltot_of[k];
                        }
                    }
                    // final scan position, and compact index if live (the
                    // first lane of each b has lrank 0 and moves both counters)
                    uint32_t dest[KS], cdest[KS], dlim[KS], cdlim[KS];
#pragma unroll
                    for (int k = 0; k < KS; ++k) {  // all reads first
                        dest[k] = head[b[k]] + rank[k];
                        cdest[k] = chead[b[k]] + lrank[k];
                        dlim[k] = hlim[b[k]];
                        cdlim[k] = clim[b[k]];
                    }
#pragma unroll
                    for (int k = 0; k < KS; ++k)
                        if (ind[k] && rank[k] == 0) {
                            head[b[k]] = dest[k] + tot_of[k];
                            chead[b[k]] = cdest[k] + ltot_of[k];
                        }
                    bool over = false;
#pragma unroll
                    for (int k = 0; k < KS; ++k)
                        over = over || (ind[k] && dest[k] >= dlim[k]) || (live[k] && cdest[k] >= cdlim[k]);
                    if (__any(over)) {  // past the bucket's part: the counts do not fit the scan
                        bad = true;
                        break;
                    }
#pragma unroll
                    for (int k = 0; k < KS; ++k) {
                        if (ind[k]) {  // the symbol at the final position; origPtr at rotation 0
                            const uint32_t q = qof(dest[k]), y = plo[k] >> 24;
                            LL[q] = u2s_id ? (uint8_t)y : u2s[y];
                            if ((plo[k] & kIndIdx) == 0) org = q;
                        }
                        const bool near = cdest[k] < v0 + kIndRing;
                        if (live[k] && near) ring[cdest[k] % kIndRing] = make_uint2(plo[k], phi[k]);
                        if (live[k] && !near) E[cdest[k]] = make_uint2(plo[k], phi[k]);
                    }
                }
                if (!anyp) break;
                uint64_t rest = 0;
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    todo[k] &= ~act[k];
                    rest |= todo[k];
                }
                if (!rest) break;
#pragma unroll
                for (int k = 0; k < KS; ++k) e[k] = ring[(vs + 64 * k + lane) % kIndRing];
            }
        }
        if (more && !bad) stage(v0 + kIndBlock);
    }
    // every placed rotation induced once, every live slot filled
    __syncthreads();
    bool short_of = false;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        short_of = short_of || head[4 * lane + q] != hlim[4 * lane + q] || chead[4 * lane + q] != clim[4 * lane + q];
    bad = bad || __any(short_of);
    if (bad && lane == 0) B.flags[s] |= kFlagHost;  // the host library redoes the stream
    if (org != ~0u) B.orig_ptr[s] = org;
}

// ------------------------------------------------------------------ MTF --
// compress.c generateMTFValues in three parallel steps.  The move-to-front
// list in front of position j is a function of the last occurrences before
// j: symbols ordered by their last occurrence (most recent first), then the
// never-seen symbols in their initial order.  So every 4096-symbol segment of
// a stream can run its own MTF once those last occurrences are known:
//   mtf_last    per segment: the sorted symbols ll[j] (inUse-mapped bytes
//               before each sorted rotation) and each symbol's last position
//   mtf_prefix  per stream: exclusive running max over the segments
//   mtf_win     per segment, one wave: initial list from the ranks of those
//               positions (a bitonic sort in registers), then the MTF of the
//               segment's run heads in windows of 64 (below)
//   rle2        per stream: zero runs -> RUNA/RUNB digits, v -> v + 1, EOB,
//               symbol frequencies (the run state is carried across thread
//               chunks by a scan, as in rle1_crc)
constexpr uint32_t kSeg = 4096;


// FROM_LL: bwt_place_sorted / bwt_induce already wrote the symbols ll[] (and
// origPtr); else (a batch sorted whole) they come from sa here
template <bool FROM_LL>
__global__ __launch_bounds__(256) void mtf_last(Batch B, uint32_t nseg_max, int32_t* __restrict__ seg_last)
{
    __shared__ uint8_t u2s[4][256];
    __shared__ int32_t last[4][256];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t s = blockIdx.y, k = blockIdx.x * 4 + wave;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t n = B.n[s];
    const uint32_t j0 = k * kSeg;
    if (j0 >= n) return;
    const size_t o = (size_t)s * B.cap;
    uint32_t nin;
    make_u2s(B, s, u2s[wave], lane, &nin);
    for (uint32_t c = lane; c < 256; c += 64) last[wave][c] = -1;
    __builtin_amdgcn_wave_barrier();
    uint8_t* llbuf = (uint8_t*)B.mtfv + o;  // the mtfv area is free until rle2
    const uint32_t j1 = min(n, j0 + kSeg);
    // four consecutive positions per lane (16-byte loads of sa, 4-byte stores
    // of the symbols), loaded an iteration ahead at a clamped, aligned index
    // (sa holds cap >= n + 8 entries per stream)
    const uint32_t jlast = (j1 - 1) & ~3u;
    uint4 vn;
    uint32_t wn = 0;
    if constexpr (FROM_LL) wn = *(const uint32_t*)(llbuf + min(j0 + 4 * lane, jlast));
    else vn = *(const uint4*)(B.sa + o + min(j0 + 4 * lane, jlast));
    for (uint32_t jb = j0; jb < j1; jb += 256) {
        const uint32_t j = jb + 4 * lane;
        uint32_t ll[4];
        if constexpr (FROM_LL) {
            const uint32_t w4 = wn;
            wn = *(const uint32_t*)(llbuf + min(j + 256, jlast));
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) ll[q] = (w4 >> (8 * q)) & 0xFFu;
        } else {
            const uint4 v4 = vn;
            vn = *(const uint4*)(B.sa + o + min(j + 256, jlast));
            const uint32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                ll[q] = u2s[wave][v[q] >> 24];
                if (j + q < j1 && (v[q] & kIdxMask) == 0) B.orig_ptr[s] = j + q;  // BZ2_blockSort: origPtr = sorted position of rotation 0
            }
            if (j + 3 < j1) {
                *(uint32_t*)(llbuf + j) = ll[0] | (ll[1] << 8) | (ll[2] << 16) | (ll[3] << 24);
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q)
                    if (j + q < j1) llbuf[j + q] = (uint8_t)ll[q];
            }
        }
        // only the last position of each run of equal symbols can be the
        // symbol's last: the BWT output is runs, and 64 lanes on one LDS word
        // serialise
        const uint32_t nxt0 = (uint32_t)__builtin_amdgcn_mov_dpp((int)ll[0], 0x130, 0xF, 0xF, false);  // wave_shl:1
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t pos = j + q;
            const uint32_t nx = q < 3 ? ll[q + 1] : nxt0;
            const bool end = pos + 1 >= j1 || (q == 3 && lane == 63) || nx != ll[q];
            if (pos < j1 && end) atomicMax(&last[wave][ll[q]], (int32_t)pos);
        }
    }
    __builtin_amdgcn_wave_barrier();
    int32_t* dst = seg_last + ((size_t)s * nseg_max + k) * 256;
    for (uint32_t c = lane; c < 256; c += 64) dst[c] = last[wave][c];
}

__global__ __launch_bounds__(256) void mtf_prefix(Batch B, uint32_t nseg_max, int32_t* __restrict__ seg_last)
{
    const uint32_t s = blockIdx.x, c = threadIdx.x;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t nseg = (B.n[s] + kSeg - 1) / kSeg;
    int32_t lb = -1;
    for (uint32_t k = 0; k < nseg; ++k) {
        int32_t* p = seg_last + ((size_t)s * nseg_max + k) * 256 + c;
        const int32_t v = *p;
        *p = lb;
        lb = max(lb, v);
    }
}

// Window-parallel MTF (the default): one wave per 4096-symbol segment, with
// the list state (P = place of each symbol, L = symbol at each place) in LDS.
// A position whose symbol equals the one before it has value 0 and leaves the
// list alone, so only the run heads are walked (the segment's first position
// and every position whose symbol differs from its predecessor's; about 55 %
// of the column of 16-bit pixels, whose low bytes follow a high byte that
// seldom changes).  The column is read in loads of 64 positions.  Of a load
// with fewer than kMtfDense heads the others store their 0 at once and the
// heads go into a ring in LDS (symbol and segment offset, slots by ballot and
// mbcnt); whenever the ring holds 64 heads the 64 oldest make a window, one
// lane per head, and what is left at the segment's end makes a last, partial
// window.  A load with kMtfDense heads or more is a window as it stands, its
// few repeats included, after the ring has been emptied into a window of its
// own: compacting such a load costs more than its repeats save, and a column
// without runs never touches the ring (the dense half of every stream of
// pixels does not either).  Walking every load's heads through the ring, as
// first built, measured 1.78 ms per launch against the parent's 1.77 on
// config-3 symbols and 2.61 against 2.25 on random bytes.  A value goes to
// its lane's own position, so no store leaves [js, je).  For lane l of a
// window whose symbol c occurred earlier in the window at lane p:
//     m = number of distinct symbols at positions (p, l),
// otherwise (first occurrence in the window)
//     m = P(c) + number of distinct earlier window symbols d with P(d) > P(c),
// P taken at the window start.  Distinct counts come from the match masks
// (ds_or_b64 per symbol): position i is the last occurrence before l of its
// symbol unless some k < l has i as its previous occurrence, so with
// U_l = OR_{k<l} bit(prev_k) the distinct symbols of (p, l) are the bits of
// lanemask_lt(l) & ~U_l above p.  After the window the list becomes the window
// symbols by last occurrence (most recent first) followed by the old list
// without them.
__device__ __forceinline__ void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint64_t ballot64(bool p) { return __ballot(p); }

// exclusive prefix OR of a 64-bit value over the wave's lanes with DPP row
// shifts and row broadcasts (VALU only: the ds_bpermute shuffles it replaces
// were a chain of 14 LDS round trips per 64-position window)
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t dpp_get(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWS, 0xF, false);
}
__device__ __forceinline__ uint32_t wave_or_scan_excl32(uint32_t x)
{
    x |= dpp_get<0x111, 0xF>(x);  // row_shr:1
    x |= dpp_get<0x112, 0xF>(x);  // row_shr:2
    x |= dpp_get<0x114, 0xF>(x);  // row_shr:4
    x |= dpp_get<0x118, 0xF>(x);  // row_shr:8
    x |= dpp_get<0x142, 0xA>(x);  // row_bcast:15 into rows 1 and 3
    x |= dpp_get<0x143, 0xC>(x);  // row_bcast:31 into rows 2 and 3
    return dpp_get<0x138, 0xF>(x);  // wave_shr:1: exclusive
}
__device__ __forceinline__ uint64_t wave_or_scan_excl(uint64_t x)
{
    return ((uint64_t)wave_or_scan_excl32((uint32_t)(x >> 32)) << 32) | wave_or_scan_excl32((uint32_t)x);
}

constexpr uint32_t kMtfDense = 48;  // heads from which a load is a window as it stands
constexpr uint32_t kMtfRing = 128;  // at most 63 heads pending plus kMtfDense - 1 of a load

// Bitonic sort of 256 words over a wave, ascending: element i = 4 lane + q.
// x of lane ^ M (M a power of two): DPP where one row holds both lanes,
// ds_swizzle inside 32 lanes, ds_bpermute across the halves.  Every lane active.
template <uint32_t M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t x)
{
    if constexpr (M == 1) return dpp_get<0xB1, 0xF>(x);        // quad_perm:[1,0,3,2]
    else if constexpr (M == 2) return dpp_get<0x4E, 0xF>(x);   // quad_perm:[2,3,0,1]
    else if constexpr (M == 8) return dpp_get<0x128, 0xF>(x);  // row_ror:8
    else if constexpr (M == 4 || M == 16) return (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, (int)((M << 10) | 0x1Fu));  // xor M
    else return (uint32_t)__shfl_xor((int)x, (int)M);
}
__device__ __forceinline__ void cmpx(uint32_t& a, uint32_t& b)
{
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}
template <uint32_t M>
__device__ __forceinline__ void bitonic_lanes(uint32_t (&x)[4], uint32_t lane)
{
    const bool low = (lane & M) == 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t y = lane_xor<M>(x[q]);
        x[q] = low ? min(x[q], y) : max(x[q], y);
    }
}
// merges the sorted runs of K / 2 elements into runs of K, alternately up and
// down (all up for K = 256): a run that goes down sorts its complements up
template <uint32_t K>
__device__ __forceinline__ void bitonic_merge(uint32_t (&x)[4], uint32_t lane)
{
    const uint32_t f = (K < 256 && (4 * lane & K)) ? ~0u : 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] ^= f;
    if constexpr (K >= 256) bitonic_lanes<32>(x, lane);
    if constexpr (K >= 128) bitonic_lanes<16>(x, lane);
    if constexpr (K >= 64) bitonic_lanes<8>(x, lane);
    if constexpr (K >= 32) bitonic_lanes<4>(x, lane);
    if constexpr (K >= 16) bitonic_lanes<2>(x, lane);
    if constexpr (K >= 8) bitonic_lanes<1>(x, lane);
    cmpx(x[0], x[2]);
    cmpx(x[1], x[3]);
    cmpx(x[0], x[1]);
    cmpx(x[2], x[3]);
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] ^= f;
}
__device__ __forceinline__ void bitonic_sort256(uint32_t (&x)[4], uint32_t lane)
{
    cmpx(x[0], x[1]);
    cmpx(x[3], x[2]);
    bitonic_merge<4>(x, lane);
    bitonic_merge<8>(x, lane);
    bitonic_merge<16>(x, lane);
    bitonic_merge<32>(x, lane);
    bitonic_merge<64>(x, lane);
    bitonic_merge<128>(x, lane);
    bitonic_merge<256>(x, lane);
}

__global__ __launch_bounds__(256) void mtf_win(Batch B, uint32_t nseg_max, const int32_t* __restrict__ seg_last)
{
    __shared__ uint64_t mt[4][256];
    __shared__ uint8_t Pt[4][256], Lt[4][256], inw[4][256];
    __shared__ uint32_t ring[4][kMtfRing];  // pending heads: symbol | segment offset << 8
    const uint32_t lane = threadIdx.x & 63;
    // (in a scalar register: the segment's bounds and the loop below branch on it)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t s = blockIdx.y, k = blockIdx.x * 4 + wave;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t n = B.n[s];
    const uint32_t js = k * kSeg;
    if (js >= n) return;
    const size_t o = (size_t)s * B.cap;
    uint32_t nin = 0;
    for (int q = 0; q < 8; ++q) nin += __popc(B.inuse[s * 8 + q]);
    // list at js: seen symbols by last position (descending), then the unseen
    // ones by symbol index (ascending) -- key(unseen c) = -1 - c.  The keys
    // are distinct, so the place of a symbol is its rank in the sorted order
    // of (key descending): one word per symbol, the complemented key above
    // the symbol (key + 256 < 2^23: a block holds under 2^20 positions), the
    // words of the symbols not in use last, sorted in registers
    const int32_t* lb = seg_last + ((size_t)s * nseg_max + k) * 256;
    const int4 lv = *(const int4*)(lb + 4 * lane);
    const int32_t lq[4] = {lv.x, lv.y, lv.z, lv.w};
    uint32_t x[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t c = 4 * lane + q;
        const int32_t key = lq[q] < 0 ? -1 - (int32_t)c : lq[q];
        x[q] = c < nin ? ((0x7FFFFFu - (uint32_t)(key + 256)) << 8) | c : ~0u;
    }
    for (uint32_t c = lane; c < 256; c += 64) inw[wave][c] = 0;
    bitonic_sort256(x, lane);
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) {
        const uint32_t p = 4 * lane + q, c = x[q] & 0xFFu;
        if (p < nin) {
            Lt[wave][p] = (uint8_t)c;
            Pt[wave][c] = (uint8_t)p;
        }
    }
    wsync();
    const uint8_t* llbuf = (const uint8_t*)B.mtfv + o;
    uint8_t* mraw = B.uflag + o;
    const uint32_t je = min(n, js + kSeg);
    const uint64_t lt = (1ull << lane) - 1ull, gt = ~lt & ~(1ull << lane);
    // one window: lane l holds the head with symbol c at segment offset off
    auto window = [&](const uint32_t c, const uint32_t off, const bool valid) {
        // match mask of c in this window
        if (valid) mt[wave][c] = 0;
        wsync();
        if (valid) atomicOr((unsigned long long*)&mt[wave][c], 1ull << lane);
        wsync();
        const uint64_t M = valid ? mt[wave][c] : 0ull;
        const uint64_t before = M & lt;
        const bool has_prev = before != 0ull;
        const uint32_t p_in = has_prev ? 63u - (uint32_t)__clzll(before) : 0u;
        const uint32_t P0 = Pt[wave][c];
        // U = OR over lanes k < lane of bit(prev_k)  (exclusive prefix OR)
        const uint64_t U = wave_or_scan_excl(has_prev ? (1ull << p_in) : 0ull);
        uint32_t m;
        if (has_prev) {
            m = (uint32_t)__popcll((lt & ~U) >> (p_in + 1));
        } else {
            m = P0;
        }
        // first occurrences: earlier first-occurrence symbols placed behind c.
        // Their ranks at the window start are distinct, so the count is the
        // number of bits above P0 in the exclusive prefix OR of the earlier
        // first-occurrence lanes' one-hot ranks (8 words, DPP scans); a
        // serial loop over them (~27 per window, a readlane each) was
        // scalar-unit bound
        // only the words from the lowest to the highest first-occurrence
        // rank carry bits that count (usually one or two of the eight)
        const bool isF = valid && !has_prev;
        const uint32_t wm = (uint32_t)__builtin_amdgcn_readlane(
            (int)(wave_or_scan_excl32(isF ? 1u << (P0 >> 5) : 0u) | (isF ? 1u << (P0 >> 5) : 0u)), 63);
        const uint32_t wlo = wm ? (uint32_t)__builtin_ctz(wm) : 8u, whi = wm ? 31u - (uint32_t)__clz(wm) : 0u;
        {
            const uint32_t pw = P0 >> 5, pb = P0 & 31u;
            uint32_t cnt = 0;
            for (uint32_t wd = wlo; wd <= whi; ++wd) {
                const uint32_t oh = (isF && pw == wd) ? (1u << pb) : 0u;
                const uint32_t pre = wave_or_scan_excl32(oh);
                const uint32_t above = wd > pw ? ~0u : (wd == pw ? (pb == 31 ? 0u : ~0u << (pb + 1)) : 0u);
                cnt += (uint32_t)__popc(pre & above);
            }
            if (isF) m += cnt;
        }
        if (valid) mraw[js + off] = (uint8_t)m;  // off is a valid lane's own position: js + off < je
        // list update: window symbols by last occurrence, then the rest.  The
        // window symbols' old places (their first occurrences' P0) are below
        // 32 * (whi + 1), and every entry past them keeps its place (nw
        // removed before it, nw inserted in front), so only the blocks of 64
        // places up to there move (place p = 64 q + lane)
        const bool is_last = valid && (M & gt) == 0ull;
        const uint64_t Lw = ballot64(is_last);
        const uint32_t nw = (uint32_t)__popcll(Lw);
        const uint32_t nblk = whi / 2u + 1u;  // wave-uniform
        if (isF) inw[wave][P0] = 1;  // flags by old place: the update reads them in order
        wsync();
        uint32_t sym[4], fl[4];
        uint64_t fb[4];
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (q < nblk) {
                const uint32_t p = 64u * q + lane;
                sym[q] = Lt[wave][p];
                fl[q] = p < nin ? inw[wave][p] : 1u;
                fb[q] = ballot64(fl[q] != 0);
            }
        }
        wsync();
        uint32_t fl_blocks = 0;  // flagged places in the blocks before q
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            if (q < nblk) {
                const uint32_t p = 64u * q + lane;
                if (!fl[q]) {
                    const uint32_t np = nw + p - (fl_blocks + (uint32_t)__popcll(fb[q] & lt));
                    Lt[wave][np] = (uint8_t)sym[q];
                    Pt[wave][sym[q]] = (uint8_t)np;
                }
                fl_blocks += (uint32_t)__popcll(fb[q]);
            }
        }
        if (is_last) {
            const uint32_t np = (uint32_t)__popcll(Lw & gt);
            Lt[wave][np] = (uint8_t)c;
            Pt[wave][c] = (uint8_t)np;
        }
        if (isF) inw[wave][P0] = 0;
        wsync();
    };
    // The symbols of four loads (256 positions) are fetched four loads ahead,
    // unconditionally (clamped indices: a load under a branch made the
    // compiler wait for every outstanding load at the next use): a sparse
    // load is too short to hide a fetch issued one load earlier.  Byte q of
    // lane l is position jg + 64 q + l.
    uint32_t nq[4];
    auto fetch = [&](const uint32_t jg) {
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) nq[q] = llbuf[min(jg + 64u * q + lane, je - 1)];
    };
    fetch(js);
    uint32_t cur = 0;         // the symbols of the four loads in hand, a byte each
    uint32_t plast = 0;       // the previous load's last symbol
    uint32_t wr = 0, rd = 0;  // ring entries written and taken (wave-uniform): wr - rd < 128
    uint32_t j0 = js;         // the next load (wave-uniform)
    uint32_t c = 0;           // the load in hand: this lane's symbol
    bool valid = false, held = false;  // held: a dense load waits until the ring is empty
    for (;;) {
        if (!held && j0 < je) {
            const uint32_t q = ((j0 - js) >> 6) & 3u;
            if (q == 0) {
                cur = nq[0] | (nq[1] << 8) | (nq[2] << 16) | (nq[3] << 24);
                fetch(j0 + 256);
            }
            const uint32_t j = j0 + lane;
            valid = j < je;
            c = valid ? (cur >> (8u * q)) & 0xFFu : 0u;
            const uint32_t pd = dpp_get<0x138, 0xF>(c);  // wave_shr:1, every lane active
            const uint32_t pv = lane ? pd : plast;
            plast = (uint32_t)__builtin_amdgcn_readlane((int)c, 63);
            const bool head = valid && (j == js || c != pv);
            const uint64_t H = ballot64(head);
            const uint32_t nh = (uint32_t)__popcll(H);
            if (nh >= kMtfDense) {
                held = true;
            } else {
                if (valid && !head) mraw[j] = 0;
                if (head) ring[wave][(wr + (uint32_t)__popcll(H & lt)) % kMtfRing] = c | ((j - js) << 8);
                wr += nh;
                j0 += 64;
            }
        }
        const uint32_t cnt = wr - rd;
        const bool direct = held && cnt == 0;
        if (!direct && !held && cnt < 64 && !(j0 >= je && cnt)) {
            if (j0 >= je) break;
            continue;
        }
        uint32_t wc, woff;
        bool wvalid;
        if (direct) {  // the load as it stands, its repeats included (they come out as 0)
            wc = c;
            woff = j0 + lane - js;
            wvalid = valid;
            held = false;
            j0 += 64;
        } else {  // the 64 oldest heads; all of them before a dense load and at the segment's end
            const uint32_t take = min(cnt, 64u);
            wsync();
            const uint32_t e = ring[wave][(rd + lane) % kMtfRing];  // lanes >= take: a stale entry, unused
            wvalid = lane < take;
            wc = wvalid ? e & 0xFFu : 0u;
            woff = e >> 8;
            rd += take;
        }
        window(wc, woff, wvalid);
    }
}

// zero-run digits of a run of z >= 1 zeros (compress.c: z-1, then RUNA/RUNB
// by bit, (z-2)/2 ... : bijective base 2, whose length is floor(log2(z + 1)))
__device__ __forceinline__ uint32_t run_digits(uint32_t z) { return 31u - (uint32_t)__clz(z + 1u); }

// A (stream, table) heap is "narrow" when every node weight of
// BZ2_hbMakeCodeLengths fits 17 bits: the table's frequencies sum to at most
// nMTF, and each zero frequency counts 1.  Narrow heaps (nearly every default
// 96x96x8 uint16 block: nMTF ~ 95-100k) take u32 entries in huff_lengths_heap,
// the others u64 entries (rle2 lists those streams).
constexpr uint32_t kNarrowWeight = 1u << 17;
__device__ __forceinline__ bool heap_narrow(const Batch& B, uint32_t s, int alphaSize)
{
    return B.nmtf[s] + (uint32_t)alphaSize < kNarrowWeight;
}

constexpr int kRle2Threads = 256;  // (512 and 1 024 measured slower)
constexpr uint32_t kRle2Per = 64;                        // m values per thread and tile
constexpr uint32_t kRle2Tile = kRle2Threads * kRle2Per;  // 16384

// One workgroup per stream walks it in tiles of 16384 MTF values, 64 per
// thread.  A thread's zero values are a 64-bit mask; the zero run pending at
// each thread's first value comes from a scan (trailing zeros, all zero) over
// the tile on top of the run carried from the previous tiles.  Every nonzero
// value v ends the zero run before it: the run's RUNA / RUNB digits, then
// v + 1, go into an LDS copy of the tile's output (placed by a scan of the
// counts; the digits of a run of z zeros are the bits of z + 1 below its top
// bit, lowest first) and out with coalesced stores.  Frequencies: RUNA / RUNB
// and the four hottest symbols in registers, the others by LDS atomics.
__device__ __forceinline__ uint64_t zero_byte_mask64(const uint32_t (&q)[kRle2Per / 4])
{
    uint64_t Z = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRle2Per / 4; ++k) {
        const uint32_t y = q[k];
        const uint32_t z = ~((((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y)) & 0x80808080u;  // bit 7: byte zero
        const uint32_t z4 = ((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u);
        Z |= (uint64_t)z4 << (4 * k);
    }
    return Z;
}

// tile_out index swizzle: a thread writes its outputs at its own offset, and
// the offsets of the 64 lanes lie one thread's output count apart -- often a
// multiple of 32 words, i.e. one LDS bank.  XOR-ing the word index's low 5
// bits with its 32-word row number spreads them over the banks; rows stay
// whole, so the coalesced read-out (consecutive indices) is a permutation
// inside each row, conflict-free as well.
__device__ __forceinline__ uint32_t rle2_swz(uint32_t p) { return p ^ (((p >> 6) & 31u) << 1); }

__global__ __launch_bounds__(kRle2Threads) __attribute__((amdgpu_waves_per_eu(4))) void rle2(Batch B)
{
    constexpr uint32_t NW = kRle2Threads / 64;
    __shared__ uint32_t wz[NW], wa[NW], wc[NW];  // per-wave scan totals
    // freq[kMaxAlpha + t] and tile_out[kRle2Tile + 64 + t]: thread t's junk slots
    __shared__ uint32_t freq[kMaxAlpha + kRle2Threads];
    __shared__ uint16_t tile_out[kRle2Tile + 64 + kRle2Threads];
    __shared__ uint32_t s_carry, s_wr;
    const uint32_t s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t n = B.n[s];
    const size_t o = (size_t)s * B.cap;
    const uint8_t* m = B.uflag + o;
    uint16_t* out = B.mtfv + (size_t)s * (B.cap + 8);
    uint32_t nin = 0;
    for (int q = 0; q < 8; ++q) nin += __popc(B.inuse[s * 8 + q]);
    const uint32_t EOB = nin + 1;
    for (uint32_t v = t; v < kMaxAlpha; v += kRle2Threads) freq[v] = 0;
    if (t == 0) {
        s_carry = 0;
        s_wr = 0;
    }
    uint32_t nrunA = 0, nrunB = 0;
    uint64_t hot = 0;  // symbols 2 .. 5 (values 1 .. 4): 16-bit counters
    // zero-run scan element: (trailing zeros, all zeros); a then b
    auto zcomb = [](uint32_t atz, uint32_t aaz, uint32_t btz, uint32_t baz, uint32_t& rtz, uint32_t& raz) {
        rtz = baz ? atz + btz : btz;
        raz = aaz & baz;
    };
    // this thread's 64 values of a tile, in registers, loaded a tile ahead
    uint4 nq[kRle2Per / 16];
    auto load_vals = [&](uint32_t tb2) {
        const uint32_t a0 = min(n, tb2 + t * kRle2Per), l2 = min(n, a0 + kRle2Per) - a0;
#pragma unroll
        for (uint32_t i = 0; i < kRle2Per / 16; ++i)
            nq[i] = 16 * i < l2 ? *(const uint4*)(m + a0 + 16 * i) : make_uint4(0, 0, 0, 0);
    };
    load_vals(0);
    __syncthreads();
    for (uint32_t tb = 0; tb < n; tb += kRle2Tile) {
        const uint32_t c0 = min(n, tb + t * kRle2Per), c1 = min(n, c0 + kRle2Per), len = c1 - c0;
        const bool last_tile = tb + kRle2Tile >= n;
        uint32_t q[kRle2Per / 4];
#pragma unroll
        for (uint32_t i = 0; i < kRle2Per / 16; ++i) {
            q[4 * i] = nq[i].x; q[4 * i + 1] = nq[i].y; q[4 * i + 2] = nq[i].z; q[4 * i + 3] = nq[i].w;
        }
        load_vals(tb + kRle2Tile);
        const uint64_t valid = len >= 64 ? ~0ull : (1ull << len) - 1ull;
        const uint64_t Z = zero_byte_mask64(q) & valid, NZ = ~Z & valid;
        // chunk summary: trailing zeros, all-zero (empty chunks pass the carry through)
        const uint32_t az = NZ == 0ull ? 1u : 0u;
        const uint32_t tz = az ? len : (uint32_t)__clzll(NZ << (64u - len));
        // inclusive scan over the wave, then the waves before
        uint32_t itz = tz, iaz = az;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t otz = (uint32_t)__shfl_up((int)itz, d), oaz = (uint32_t)__shfl_up((int)iaz, d);
            if ((int)lane >= d) zcomb(otz, oaz, itz, iaz, itz, iaz);
        }
        if (lane == 63) {
            wz[wave] = itz;
            wa[wave] = iaz;
        }
        const uint32_t tile_carry = s_carry;
        __syncthreads();
        uint32_t ptz = tile_carry, paz = 1;  // everything before the wave, the tile carry first
        for (uint32_t w2 = 0; w2 < wave; ++w2) zcomb(ptz, paz, wz[w2], wa[w2], ptz, paz);
        uint32_t etz = (uint32_t)__shfl_up((int)itz, 1), eaz = (uint32_t)__shfl_up((int)iaz, 1);
        if (lane == 0) { etz = 0; eaz = 1; }
        uint32_t carry, cz;  // zeros pending at the chunk start
        zcomb(ptz, paz, etz, eaz, carry, cz);
        uint32_t tile_end_zeros = tile_carry, tez = 1;
        for (uint32_t w2 = 0; w2 < NW; ++w2) zcomb(tile_end_zeros, tez, wz[w2], wa[w2], tile_end_zeros, tez);
        const bool has_last = last_tile && len && c1 == n;
        // zero runs ending here: at a nonzero value after a zero (or after
        // the carried zeros), and the stream's final run
        const uint64_t R = NZ & ((Z << 1) | (carry ? 1ull : 0ull));
        const uint32_t zend = az ? carry + len : tz;  // zeros at the chunk end (the stream's final run when has_last)
        auto run_len = [&](uint32_t i) {  // zeros before the nonzero value i
            const uint64_t below = NZ & ((1ull << i) - 1ull);
            return below ? i - 1u - (63u - (uint32_t)__clzll(below)) : carry + i;
        };
        uint32_t ndig = 0;
        for (uint64_t r = R; r; r &= r - 1ull) ndig += run_digits(run_len((uint32_t)__builtin_ctzll(r)));
        const uint32_t dend = has_last && zend ? run_digits(zend) : 0u;
        const uint32_t w = (uint32_t)__popcll(NZ) + ndig + dend + (has_last ? 1u : 0u);
        // output offsets: scan of the counts
        uint32_t ic = w;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t oc = (uint32_t)__shfl_up((int)ic, d);
            if ((int)lane >= d) ic += oc;
        }
        if (lane == 63) wc[wave] = ic;
        __syncthreads();
        uint32_t wr = ic - w, tile_total = 0;
        for (uint32_t w2 = 0; w2 < NW; ++w2) {
            if (w2 < wave) wr += wc[w2];
            tile_total += wc[w2];
        }
        // the digits of a run of z zeros at p .. p + d - 1
        auto digits = [&](uint32_t p, uint32_t z) {
            const uint32_t d = run_digits(z), x = z + 1u;
            const uint32_t nb = (uint32_t)__popc(x & ((1u << d) - 1u));
            nrunB += nb;
            nrunA += d - nb;
            for (uint32_t k = 0; k < d; ++k) tile_out[rle2_swz(p + k)] = (uint16_t)((x >> k) & 1u);
        };
        // symbols v + 1: one write per value (zeros into a junk slot), the
        // position advanced past the digits of the run each one ends
        {
            uint32_t pos = wr, z = carry;
#pragma unroll
            for (uint32_t i = 0; i < kRle2Per; ++i) {
                const uint32_t v = (q[i >> 2] >> (8 * (i & 3))) & 0xFFu;
                const bool nz = (NZ >> i) & 1u;
                pos += nz && z ? run_digits(z) : 0u;
                tile_out[rle2_swz(nz ? pos : kRle2Tile + 64 + t)] = (uint16_t)(v + 1u);
                atomicAdd(&freq[nz && v > 4u ? v + 1u : kMaxAlpha + t], 1u);
                hot += nz && v <= 4u ? 1ull << (16u * (v - 1u)) : 0ull;
                pos += nz ? 1u : 0u;
                z = nz ? 0u : z + 1u;
            }
        }
        // the digits, each run before the nonzero value ending it
        {
            uint32_t dsum = 0;  // digits of the runs ending before i
            for (uint64_t r = R; r; r &= r - 1ull) {
                const uint32_t i = (uint32_t)__builtin_ctzll(r), z = run_len(i);
                digits(wr + (uint32_t)__popcll(NZ & ((1ull << i) - 1ull)) + dsum, z);
                dsum += run_digits(z);
            }
        }
        if (has_last) {
            if (zend) digits(wr + w - 1u - dend, zend);
            tile_out[rle2_swz(wr + w - 1u)] = (uint16_t)EOB;
            atomicAdd(&freq[EOB], 1u);
        }
        __syncthreads();
        const uint32_t base = s_wr;
        for (uint32_t i = t; i < tile_total; i += kRle2Threads) out[base + i] = tile_out[rle2_swz(i)];
        __syncthreads();
        if (t == 0) {
            s_wr = base + tile_total;
            s_carry = tile_end_zeros;
        }
        __syncthreads();
    }
    static_assert(kRunA == 0 && kRunB == 1, "RUNA / RUNB are symbols 0 and 1");
    // wave sums of the register counters, one atomic per wave and symbol
    uint32_t cnts[6] = {nrunA, nrunB, (uint32_t)(hot & 0xFFFFu), (uint32_t)((hot >> 16) & 0xFFFFu),
                        (uint32_t)((hot >> 32) & 0xFFFFu), (uint32_t)(hot >> 48)};
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        uint32_t c = cnts[r];
        for (int d = 32; d > 0; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d);
        if (lane == 0 && c) atomicAdd(&freq[r], c);
    }
    __syncthreads();
    if (t == 0) {
        B.nmtf[s] = s_wr;
        if (!heap_narrow(B, s, (int)nin + 2)) B.wide[atomicAdd(B.wide_cnt, 1u)] = s;  // u64 Huffman heaps
    }
    for (uint32_t v = t; v < kMaxAlpha; v += kRle2Threads) B.mtf_freq[(size_t)s * kMaxAlpha + v] = freq[v];
}

// --------------------------------------------------------------- huffman --
constexpr int kHuffThreads = 256;

// sendMTFValues split across launches so the sequential part (the heap of
// BZ2_hbMakeCodeLengths) runs SIMT, one table per lane:
//   huff_select   x4: selector per 50 symbols (first minimum cost, all tables
//                 summed at once in 10-bit fields), then symbol frequencies
//                 per selected table; the first one starts with nGroups and
//                 the initial partition (lengths 0 / 15)
//   huff_lengths  x4: BZ2_hbMakeCodeLengths (huffman.c, restated: nodes and
//                 heap from 1, entry 0 the sentinel, weights carry the depth
//                 in the low byte), one lane per (stream, table)
//   huff_final    selector MTF and the codes (BZ2_hbAssignCodes)
__device__ __forceinline__ uint32_t stream_nin(const Batch& B, uint32_t s)
{
    uint32_t nin = 0;
    for (int q = 0; q < 8; ++q) nin += __popc(B.inuse[s * 8 + q]);
    return nin;
}

// compress.c's initial partition, the prologue of the first huff_select_reg
// launch: the frequencies go to LDS (the greedy walk is sequential and would
// otherwise wait on a global load per symbol), one lane walks them; table q
// then prices symbols pgs[q] .. pge[q] at 0 and the others at 15.  Writes
// nGroups and nSel for the later launches.
__device__ __forceinline__ void huff_partition(const Batch& B, uint32_t s, uint32_t t, uint32_t nthreads, uint32_t nMTF,
                                               int alphaSize, int nGroups, int* mf, int* pgs, int* pge)
{
    const uint32_t* mfreq = B.mtf_freq + (size_t)s * kMaxAlpha;
    for (int v = t; v < kMaxAlpha; v += nthreads) mf[v] = v < alphaSize ? (int)mfreq[v] : 0;
    __syncthreads();
    if (t == 0) {
        int nPart = nGroups, remF = (int)nMTF, gs = 0;
        while (nPart > 0) {
            const int tFreq = remF / nPart;
            int ge = gs - 1, aFreq = 0;
            while (aFreq < tFreq && ge < alphaSize - 1) {
                ++ge;
                aFreq += mf[ge];
            }
            if (ge > gs && nPart != nGroups && nPart != 1 && ((nGroups - nPart) % 2 == 1)) {
                aFreq -= mf[ge];
                --ge;
            }
            pgs[nPart - 1] = gs;
            pge[nPart - 1] = ge;
            --nPart;
            gs = ge + 1;
            remF -= aFreq;
        }
        B.ngroups[s] = (uint32_t)nGroups;
        B.nsel[s] = (nMTF + kGSize - 1) / kGSize;
    }
    __syncthreads();
}

// huff_select with a group's 50 symbols loaded straight into registers (25
// dword loads from its 100 bytes; a row is 16-byte aligned and 100 is a
// multiple of 4): no LDS tile, so ~8 KiB of LDS per workgroup and more
// workgroups per CU to hide the loads.  The last, partial group pads with
// symbol kMaxAlpha, whose packed lengths are 0 and which is not counted.
// (A 25 KiB LDS tile of the symbols measured 3.4x slower: fewer workgroups per CU.)
// FIRST: the first of the kIters launches prices the symbols by the initial
// partition (huff_partition, walked here: no launch of its own and no 0 / 15
// length table in memory, which nothing else reads); the later ones by the
// code lengths huff_lengths_heap left.
template <bool FIRST>
__global__ __launch_bounds__(kHuffThreads) void huff_select_reg(Batch B)
{
    __shared__ uint32_t rfreq[kMaxGroups][kMaxAlpha];
    __shared__ uint64_t lpack[kMaxAlpha + 1];
    __shared__ uint32_t junk[kHuffThreads];
    __shared__ int pgs[kMaxGroups], pge[kMaxGroups];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (B.flags[s] & kFlagHost) return;
    const uint32_t nMTF = B.nmtf[s];
    const uint32_t nSel = FIRST ? (nMTF + kGSize - 1) / kGSize : B.nsel[s];
    int nGroups;
    if constexpr (FIRST) nGroups = nMTF < 200 ? 2 : nMTF < 600 ? 3 : nMTF < 1200 ? 4 : nMTF < 2400 ? 5 : 6;
    else nGroups = (int)B.ngroups[s];
    const int alphaSize = (int)stream_nin(B, s) + 2;
    const uint8_t* len = B.len + (size_t)s * kMaxGroups * kMaxAlpha;
    const uint16_t* mtfv = B.mtfv + (size_t)s * (B.cap + 8);
    uint8_t* sel = B.sel + (size_t)s * B.sel_cap;
    // (the walk's frequencies lie in rfreq's first row until it is cleared)
    if constexpr (FIRST) huff_partition(B, s, t, kHuffThreads, nMTF, alphaSize, nGroups, (int*)&rfreq[0][0], pgs, pge);
    for (int v = t; v <= kMaxAlpha; v += kHuffThreads) {
        uint64_t lp = 0;
        if (v < alphaSize)
            for (int q = 0; q < nGroups; ++q) {
                const uint32_t l = FIRST ? (v >= pgs[q] && v <= pge[q] ? 0u : 15u) : (uint32_t)len[q * kMaxAlpha + v];
                lp |= (uint64_t)l << (10 * q);
            }
        lpack[v] = lp;
    }
    for (int i = t; i < kMaxGroups * kMaxAlpha; i += kHuffThreads) rfreq[i / kMaxAlpha][i % kMaxAlpha] = 0;
    __syncthreads();
    uint64_t lp_hot[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) lp_hot[f] = lpack[f];
    for (uint32_t g = t; g < nSel; g += kHuffThreads) {
        const uint32_t gs = g * kGSize, cnt = min(nMTF - gs, (uint32_t)kGSize);
        uint32_t w[kGSize / 2];
        if (cnt == (uint32_t)kGSize) {
            const uint32_t* p = (const uint32_t*)(mtfv + gs);
#pragma unroll
            for (int q = 0; q < kGSize / 2; ++q) w[q] = p[q];
        } else {
#pragma unroll
            for (int q = 0; q < kGSize / 2; ++q) {
                const uint32_t lo = 2u * q < cnt ? mtfv[gs + 2 * q] : (uint32_t)kMaxAlpha;
                const uint32_t hi = 2u * q + 1 < cnt ? mtfv[gs + 2 * q + 1] : (uint32_t)kMaxAlpha;
                w[q] = lo | (hi << 16);
            }
        }
        // a group's cost under every table at once (10-bit fields, as
        // huff_select); symbols 0 .. 3 (most of them) are counted in 8-bit
        // fields and priced from registers, their lanes read the pad entry
        // (one broadcast address instead of bank conflicts on 4 hot words)
        uint32_t hot = 0;
        uint64_t acc = 0;
#pragma unroll
        for (int q = 0; q < kGSize / 2; ++q) {
            const uint32_t lo = w[q] & 0xFFFFu, hi = w[q] >> 16;
            hot += lo < 4u ? 1u << (8u * lo) : 0u;
            hot += hi < 4u ? 1u << (8u * hi) : 0u;
            acc += lpack[lo < 4u ? (uint32_t)kMaxAlpha : lo] + lpack[hi < 4u ? (uint32_t)kMaxAlpha : hi];
        }
#pragma unroll
        for (uint32_t f = 0; f < 4; ++f) acc += (uint64_t)((hot >> (8u * f)) & 0xFFu) * lp_hot[f];
        int bt = -1;
        uint32_t bc = 999999999u;
        for (int q = 0; q < nGroups; ++q) {
            const uint32_t cq = (uint32_t)(acc >> (10 * q)) & 1023u;
            if (cq < bc) { bc = cq; bt = q; }
        }
        sel[g] = (uint8_t)bt;
        // symbols 0 .. 3 (RUNA, RUNB and the two smallest values: most of
        // them) go to rfreq from their 8-bit fields, the others by LDS atomics
        // (the hot bins' atomics serialised on bank conflicts); a lane's other
        // symbols land in its own junk word
#pragma unroll
        for (int q = 0; q < kGSize / 2; ++q) {
            const uint32_t lo = w[q] & 0xFFFFu, hi = w[q] >> 16;
            atomicAdd(lo >= 4u && lo != (uint32_t)kMaxAlpha ? &rfreq[bt][lo] : &junk[t], 1u);
            atomicAdd(hi >= 4u && hi != (uint32_t)kMaxAlpha ? &rfreq[bt][hi] : &junk[t], 1u);
        }
#pragma unroll
        for (uint32_t f = 0; f < 4; ++f)
            if ((hot >> (8u * f)) & 0xFFu) atomicAdd(&rfreq[bt][f], (hot >> (8u * f)) & 0xFFu);
    }
    __syncthreads();
    uint32_t* rf = B.rfreq + (size_t)s * kMaxGroups * kMaxAlpha;
    for (int i = t; i < kMaxGroups * kMaxAlpha; i += kHuffThreads) rf[i] = rfreq[i / kMaxAlpha][i % kMaxAlpha];
}

// BZ2_hbMakeCodeLengths, kL (stream, table) heaps per wave, one per lane,
// with wave-uniform heap walks.  A heap entry is one word: the weight as
// (freq << 5 | height) above bit 10, the node in bits 0..9; the order of
// (freq << 5 | height) is huffman.c's order of (freq << 8 | depth) because
// height <= 17 -- a node of height 18 already means a code longer than
// maxLen 17, so the lane keeps going on garbage and then redoes the tree with
// halved weights, the retry huffman.c takes after building it.  Narrow heaps
// (heap_narrow: weights < 2^17) use u32 entries (~1 KB of LDS per heap, so
// many heaps are resident), the others u64 entries in a second launch over the
// list the first one built (kList).
//   * Entries are entry-major: entry e of every lane in one row of kL words,
//     so a read or write of one entry index by all lanes has no bank conflict,
//     an address is one multiply-add and a children pair one ds_read2.
//   * The merges run in lockstep over the wave, one merge per trip, and a
//     sift's path comes from the lane's pref bits (lfm_huff_heap.h), not from
//     a walk: its levels are read in one LDS round trip and rewritten without
//     a branch.  The level count is the wave's: from the largest heap, which
//     shrinks by one entry per trip.
//   * Parents go to global memory (the stream's code table, unused until
//     huff_final) and come back for the depth pass, whose depths overlay the
//     lane's own entries.

// Diagnostic build (-DLFM_HUFF_STAMPS, off by default: nothing of it is in the
// library otherwise): the wave's clock (s_memtime) is read between the phases
// of heap_code_lengths and around the two halves of huff_final, the time each
// phase took is summed over a lane's rounds and its largest value over the
// workgroup's lanes (and over the launches since the last read) is left in
// g_huff_stamps, which lfm_hip_huff_stamps copies out and clears
// (scripts/huff_stamps_probe.py).
// A phase's value is thus a maximum taken apart from the other phases', not one
// launch's chain: shares of their sum are approximate.
//   row 0, huff_lengths_heap (all launches since the last read): 0 sentinel fill and frequency
//          loads, 1 inserts, 2 heap_pref_build, 3 merge trips, 4 depth pass,
//          5 length stores
//   row 1, huff_final: 0 the selector wave, 1 the wave of table 0
#ifdef LFM_HUFF_STAMPS
constexpr uint32_t kStampWgs = 4096, kStampSlots = 8;
__device__ unsigned long long g_huff_stamps[2][kStampWgs][kStampSlots];
struct HuffStamps {
    unsigned long long last, d[kStampSlots];
    __device__ __forceinline__ void start()
    {
        for (uint32_t p = 0; p < kStampSlots; ++p) d[p] = 0;
        __builtin_amdgcn_sched_barrier(0);
        last = __builtin_amdgcn_s_memtime();
    }
    __device__ __forceinline__ void mark(uint32_t p)
    {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        d[p] += now - last;
        last = now;
    }
    __device__ __forceinline__ void store(uint32_t row, uint32_t p0, uint32_t np) const
    {
        if (blockIdx.x < kStampWgs)
            for (uint32_t p = p0; p < p0 + np; ++p) atomicMax(&g_huff_stamps[row][blockIdx.x][p], d[p]);
    }
};
#define HUFF_STAMPS(x) x
#else
#define HUFF_STAMPS(x)
#endif

template <typename Ent, int kL>
struct LdsHeap {
    static constexpr uint32_t RS = sizeof(Ent) * kL;  // bytes per entry row
    char* base;                                       // the lane's word of row 0
    uint16_t* parent;
    __device__ __forceinline__ Ent ld(uint32_t e) const { return *(const Ent*)(base + e * RS); }
    __device__ __forceinline__ void st(uint32_t e, Ent v) const { *(Ent*)(base + e * RS) = v; }
    __device__ __forceinline__ void ld_pair(uint32_t e, Ent& a, Ent& b) const
    {
        const char* q = base + e * RS;
        a = *(const Ent*)q;
        b = *(const Ent*)(q + RS);
    }
    __device__ __forceinline__ void fence() const { __builtin_amdgcn_sched_barrier(0); }
    __device__ __forceinline__ void set_parent(uint32_t node, uint32_t p) const { parent[node] = (uint16_t)p; }
    __device__ __forceinline__ bool any(bool b) const { return __builtin_amdgcn_ballot_w64(b) != 0; }
    __device__ __forceinline__ void note_sift(uint32_t, uint32_t) const {}
    __device__ __forceinline__ void note_push(uint32_t, uint32_t) const {}
    __device__ __forceinline__ void check(const HeapPref&, uint32_t) const {}
};

// halvings after which every weight is 1 (the tree of equal weights is never
// too long): the retry loop's bound
template <typename Ent>
constexpr int kHeapMaxRetries = sizeof(Ent) == 4 ? 17 : 32;

// kL heaps with Ent entries in the LDS area hb (kHeapEntries rows of kL
// entries); this lane's heap is (stream s, table tb)
template <typename Ent, int kL>
__device__ __forceinline__ void heap_code_lengths(const Batch& B, char* hb, uint32_t lane, uint32_t s, uint32_t tb)
{
    constexpr uint32_t ES = sizeof(Ent);
    static_assert(kHeapEntries * sizeof(Ent) * kL <= 33792, "the heaps' LDS grew");
    static_assert(kHeapEntries >= kMaxAlpha + 2 && 2 * kMaxAlpha / (int)(ES / 2) < kHeapEntries, "heap entries");
    {
        const int A = (int)stream_nin(B, s) + 2;
        const uint32_t* freq = B.rfreq + ((size_t)s * kMaxGroups + tb) * kMaxAlpha;
        uint8_t* len = B.len + ((size_t)s * kMaxGroups + tb) * kMaxAlpha;
        uint16_t* parent = (uint16_t*)(B.code + ((size_t)s * kMaxGroups + tb) * kMaxAlpha);  // nodes 1 .. 2A - 2
        LdsHeap<Ent, kL> acc{hb + lane * ES, parent};
        auto ent = [&](uint32_t e) -> Ent& { return *(Ent*)(acc.base + e * LdsHeap<Ent, kL>::RS); };
        // depth of node k (<= 515): u16 number k % (ES / 2) of the lane's entry k / (ES / 2)
        auto dep = [&](uint32_t k) -> uint16_t& {
            return *(uint16_t*)((char*)&ent(k / (ES / 2)) + 2 * (k % (ES / 2)));
        };
        // rows are 8-byte aligned (258 words): pairs of words, a few loads ahead
        auto ld2 = [](const void* p, int i) { return *(const uint2*)((const uint32_t*)p + (i > 0 ? i : 0)); };
        // every position past the heap holds kSent (greater than any entry:
        // heights stop at 30), so the sift needs no bounds: a pop writes kSent
        // where the last entry was, a push overwrites the first one
        constexpr Ent kSent = ~(Ent)0;
        // 8-byte global loads per round trip.  32 (five round trips for the
        // frequencies and the parents instead of nine) measured slower,
        // 409.3 against 406.8 us per launch: DESIGN 4b
        constexpr int kLoads = 16;
        // Rounds of the wave: a lane builds its heap (again, with halved
        // weights, after a tree that came out too long), then all merge in
        // lockstep; lanes whose heap is done sit the trips out.  Every loop's
        // trip count is bounded by constants, whatever the entries hold.
        int retries = 0;
        uint32_t nMerged = (uint32_t)A;  // nodes so far
        bool build = true;
        HUFF_STAMPS(HuffStamps ts; ts.start();)
        for (int round = 0; round <= kHeapMaxRetries<Ent>; ++round) {
            uint32_t nHeap = 1, tooLong = 0;
            Ent top = 0;
            HeapPref m;
            if (build) {
                // leaves at heap positions 1 .. A first (an insertion's upheap only
                // touches positions below it), then inserted in order; sentinels
                // past them
                ent(0) = 0;
                for (int e = A + 1; e < kHeapEntries; ++e) ent((uint32_t)e) = kSent;
                // 32 frequencies per batch of kLoads loads (one memory latency
                // per batch, not per load: the compiler drains vmcnt at loop
                // edges)
                for (int i0 = 1; i0 <= A; i0 += 2 * kLoads) {
                    uint2 f[kLoads];
#pragma unroll
                    for (int q = 0; q < kLoads; ++q) f[q] = ld2(freq, min(i0 - 1 + 2 * q, kMaxAlpha - 2));
#pragma unroll
                    for (int q = 0; q < kLoads; ++q) {
                        const int i = i0 + 2 * q;
                        uint32_t w0 = f[q].x ? f[q].x : 1u, w1 = f[q].y ? f[q].y : 1u;
                        for (int r = 0; r < retries; ++r) {
                            w0 = 1u + w0 / 2u;
                            w1 = 1u + w1 / 2u;
                        }
                        if (i <= A) ent(i) = ((Ent)w0 << 15) | (Ent)i;
                        if (i + 1 <= A) ent(i + 1) = ((Ent)w1 << 15) | (Ent)(i + 1);
                    }
                }
                HUFF_STAMPS(ts.mark(0);)
                // the inserts, level by level (position z is the same in
                // every lane still inserting): an insert reads its own
                // ancestors only, seven positions on average, not ten
                heap_insert_levels<Ent>(acc, (uint32_t)A);
                HUFF_STAMPS(ts.mark(1);)
                heap_pref_build<Ent>(acc, m, (uint32_t)A);
                HUFF_STAMPS(ts.mark(2);)
                nHeap = (uint32_t)A;
                nMerged = (uint32_t)A;
                top = ent(1);
            }
            // the wave's largest heap, bit by bit
            uint32_t hmax = 0;
            for (int b = 8; b >= 0; --b) {
                const uint32_t a = build ? (uint32_t)A : 0u;
                if (__builtin_amdgcn_ballot_w64((a >> b & 1u) && (a >> (b + 1)) == (hmax >> (b + 1)))) hmax |= 1u << b;
            }
            hmax = min(__builtin_amdgcn_readfirstlane(hmax), (uint32_t)kMaxAlpha);
            for (; hmax > 1u; --hmax)
                if (build && nHeap > 1u) heap_merge_step_at<Ent>(acc, m, hmax, nHeap, nMerged, top, tooLong);
            HUFF_STAMPS(ts.mark(3);)
            build = build && tooLong && retries < kHeapMaxRetries<Ent>;
            if (build) ++retries;
            if (!__builtin_amdgcn_ballot_w64(build)) break;
        }
        const int nNodes = (int)nMerged;
        if (retries) atomicAdd(B.wide_cnt + 1, (uint32_t)retries);  // statistics (LFM_BZ2_STATS)
        // depths top-down (a parent is created after its children)
        dep(nNodes) = 0;
        // 64 parents per batch of kLoads loads, highest nodes first
        for (int kc = (nNodes - 1) & ~(4 * kLoads - 1); kc >= 0; kc -= 4 * kLoads) {
            uint2 pw[kLoads];
#pragma unroll
            for (int q = 0; q < kLoads; ++q) pw[q] = ld2(parent, min(kc / 2 + 2 * q, (2 * kMaxAlpha) / 2 - 2));
            // four nodes b .. b + 3 per LDS round trip: their parents' depths
            // are read together, a parent inside the four (the root included)
            // is taken from registers instead
#pragma unroll
            for (int q = kLoads - 1; q >= 0; --q) {
                const int b = kc + 4 * q;
                const uint32_t p4[4] = {pw[q].x & 0xFFFFu, pw[q].x >> 16, pw[q].y & 0xFFFFu, pw[q].y >> 16};
                uint32_t d[4], dn[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) d[r] = dep(min(p4[r], 2u * kMaxAlpha));
#pragma unroll
                for (int r = 3; r >= 0; --r) {
                    const int k = b + r;
                    uint32_t x = d[r];
#pragma unroll
                    for (int u = r + 1; u < 4; ++u) x = p4[r] == (uint32_t)(b + u) ? dn[u] : x;
                    dn[r] = k == nNodes ? 0u : x + 1u;
                    if (k >= 1 && k < nNodes) dep(k) = (uint16_t)dn[r];
                }
            }
        }
        HUFF_STAMPS(ts.mark(4);)
        for (int i = 1; i <= A; ++i) len[i - 1] = (uint8_t)dep(i);
        HUFF_STAMPS(ts.mark(5); ts.store(0, 0, 6);)
    }
}

// Workgroups [0, nwg_wide): kL / 2 heaps of the wide streams (B.wide,
// listed by rle2 and counted by the host) with u64 entries, first so their
// chains start first; the rest: kL (stream, table) heaps each with u32
// entries (lanes of wide streams exit).  One launch, so a wide heap's chain
// runs beside the narrow ones.
template <int kL>
__global__ __launch_bounds__(64) void huff_lengths_heap(Batch B, uint32_t nwg_wide, uint32_t nwide_streams)
{
    __shared__ uint32_t hq[kHeapEntries * kL];
    char* hb = (char*)hq;
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x >= nwg_wide) {
        const uint32_t task = (blockIdx.x - nwg_wide) * kL + lane;
        const uint32_t s = task / kMaxGroups, tb = task % kMaxGroups;
        if (lane >= (uint32_t)kL || s >= B.nstreams || (B.flags[s] & kFlagHost) || tb >= B.ngroups[s]) return;
        if (!heap_narrow(B, s, (int)stream_nin(B, s) + 2)) return;
        heap_code_lengths<uint32_t, kL>(B, hb, lane, s, tb);
    } else {
        constexpr int kW = kL / 2;
        const uint32_t i = blockIdx.x * kW + lane;
        if (lane >= (uint32_t)kW || i >= nwide_streams * kMaxGroups) return;
        const uint32_t s = B.wide[i / kMaxGroups], tb = i % kMaxGroups;
        if ((B.flags[s] & kFlagHost) || tb >= B.ngroups[s]) return;
        heap_code_lengths<uint64_t, kW>(B, hb, lane, s, tb);
    }
}

// Seven waves per stream, each with a chain of its own and nothing shared.
// Waves 0 .. 5: the codes of table `wave` (BZ2_hbAssignCodes): code = (codes
// of all shorter lengths, doubled per length) + rank of the symbol among the
// same-length symbols before it (ballots per length).  Wave 6: the selector
// MTF (compress.c, 6 entries) as a scan (lfm_sel_mtf.h): a lane holds
// kSelChunk selectors in registers, sums them up, the wave composes the
// summaries on top of the carry, the lane replays its chunk from its own list.
// A pass covers 64 * kSelChunk selectors: a config-3 stream (1 900 .. 2 000)
// in one, a level-9 block's 18 002 in nine with the list carried.
constexpr uint32_t kSelChunk = 32;
constexpr uint32_t kFinalWaves = kMaxGroups + 1;
static_assert(kSelChunk % 16 == 0, "a lane's chunk is loaded and stored in 16-byte pieces");

__device__ __forceinline__ void sel_mtf_scan(const uint8_t* __restrict__ sel, uint8_t* __restrict__ sm, uint32_t nSel,
                                             uint32_t lane)
{
    constexpr uint32_t NQ = kSelChunk / 16;
    uint32_t carry = kSelMtfStart;
    for (uint32_t i0 = 0; i0 < nSel; i0 += kSelMtfLanes * kSelChunk) {
        const uint32_t b = i0 + lane * kSelChunk;
        const uint32_t n = selmtf_chunk_count(nSel, i0, lane, kSelChunk);
        // the selector arrays start 256-byte aligned in the workspace and a
        // stream's selectors at s * sel_cap, a multiple of 64 (layout()), and
        // nSel <= sel_cap: a 16-byte piece that starts below nSel is aligned
        // and lies inside the stream's sel_cap bytes
        uint32_t w[4 * NQ];
#pragma unroll
        for (uint32_t q = 0; q < NQ; ++q) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (b + 16u * q < nSel) v = *(const uint4*)(sel + b + 16u * q);
            w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
        }
        auto get = [&](uint32_t g) { return (w[g >> 2] >> (8u * (g & 3u))) & 0xFFu; };
        uint32_t incl = selmtf_summary(get, n, kSelChunk);
        if (lane == 0) incl = selmtf_compose(carry, incl);
#pragma unroll
        for (uint32_t d = 1; d < kSelMtfLanes; d <<= 1) {
            const uint32_t prev = (uint32_t)__shfl_up((int)incl, d);
            const uint32_t both = selmtf_compose(prev, incl);
            incl = lane >= d ? both : incl;
        }
        const uint32_t before = (uint32_t)__shfl_up((int)incl, 1);
        uint32_t o[4 * NQ];
#pragma unroll
        for (uint32_t q = 0; q < 4 * NQ; ++q) o[q] = 0;
        selmtf_replay(lane ? before : carry, get, [&](uint32_t g, uint32_t j) { o[g >> 2] |= j << (8u * (g & 3u)); }, n,
                      kSelChunk);
        // (the bytes of a last piece past nSel: zeros inside sel_cap, never read)
#pragma unroll
        for (uint32_t q = 0; q < NQ; ++q)
            if (b + 16u * q < nSel) *(uint4*)(sm + b + 16u * q) = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        carry = (uint32_t)__builtin_amdgcn_readlane((int)incl, kSelMtfLanes - 1);
    }
}

__global__ __launch_bounds__(64 * kFinalWaves) void huff_final(Batch B)
{
    const uint32_t s = blockIdx.x, lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (B.flags[s] & kFlagHost) return;
    const uint32_t nGroups = B.ngroups[s];
    HUFF_STAMPS(HuffStamps ts; ts.start();)
    if (wave == (uint32_t)kMaxGroups) {
        sel_mtf_scan(B.sel + (size_t)s * B.sel_cap, B.sel_mtf + (size_t)s * B.sel_cap, B.nsel[s], lane);
        HUFF_STAMPS(ts.mark(0); ts.store(1, 0, 1);)
        return;
    }
    if (wave >= nGroups) return;
    const uint32_t alphaSize = stream_nin(B, s) + 2;
    const uint8_t* len = B.len + (size_t)s * kMaxGroups * kMaxAlpha;
    const uint64_t lt = (1ull << lane) - 1ull;
    {
        const uint32_t q = wave;
        const uint8_t* lq = len + q * kMaxAlpha;
        uint32_t* code = B.code + ((size_t)s * kMaxGroups + q) * kMaxAlpha;
        uint32_t L[5], c[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint32_t i = 64 * k + lane;
            L[k] = i < alphaSize ? lq[i] : 0u;
            c[k] = 0;
        }
        uint32_t vec = 0;
        for (uint32_t nl = 1; nl <= 20; ++nl) {
            uint32_t before = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const uint64_t b = __ballot(L[k] == nl);
                if (L[k] == nl) c[k] = vec + before + (uint32_t)__popcll(b & lt);
                before += (uint32_t)__popcll(b);
            }
            // BZ2_hbAssignCodes: vec <<= 1 after every length from minLen on
            vec = (vec + before) << 1;
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const uint32_t i = 64 * k + lane;
            if (i < alphaSize) code[i] = c[k];
        }
    }
    HUFF_STAMPS(ts.mark(1); if (wave == 0) ts.store(1, 1, 1);)
}

// ------------------------------------------------------------------ emit --
constexpr int kEmitThreads = 256;

// MSB-first bit writer into 32-bit words (bit p is bit 31 - p%32 of word p/32)
__device__ __forceinline__ void put_bits_atomic(uint32_t* words, uint64_t pos, uint32_t nbits, uint32_t v)
{
    if (!nbits) return;
    const uint32_t w = (uint32_t)(pos >> 5), o = (uint32_t)(pos & 31);
    const uint64_t sh = ((uint64_t)v << (64 - nbits)) >> o;  // bits aligned at the top of a 64-bit window
    const uint32_t hi = (uint32_t)(sh >> 32), lo = (uint32_t)sh;
    if (hi) atomicOr(&words[w], hi);
    if (lo) atomicOr(&words[w + 1], lo);
}

constexpr uint32_t kSelLds = 8192;  // selectors cached in LDS (level <= 4 always fits)

// header bits are assembled in LDS (one writer, no atomics; a global atomic
// per header field serialised the lane on memory latency), then copied out
constexpr uint32_t kHdrWords = 4096;  // 128 kbit: every level-1..9 header but extreme ones

__device__ __forceinline__ void put_bits_hdr(uint32_t* hdr, uint32_t* words, uint64_t pos, uint32_t nbits, uint32_t v)
{
    if (!nbits) return;
    const uint32_t w = (uint32_t)(pos >> 5), o = (uint32_t)(pos & 31);
    const uint64_t sh = ((uint64_t)v << (64 - nbits)) >> o;
    const uint32_t hi = (uint32_t)(sh >> 32), lo = (uint32_t)sh;
    if (w + 1 < kHdrWords) {
        hdr[w] |= hi;
        hdr[w + 1] |= lo;
    } else {  // overflow past the LDS buffer: straight to memory
        if (hi) atomicOr(&words[w], hi);
        if (lo) atomicOr(&words[w + 1], lo);
    }
}

// header items written by many threads: neighbours share words (atomicOr)
__device__ __forceinline__ void put_bits_hdr_atomic(uint32_t* hdr, uint32_t* words, uint64_t pos, uint32_t nbits,
                                                    uint32_t v)
{
    if (!nbits) return;
    const uint32_t w = (uint32_t)(pos >> 5), o = (uint32_t)(pos & 31);
    const uint64_t sh = ((uint64_t)v << (64 - nbits)) >> o;
    const uint32_t hi = (uint32_t)(sh >> 32), lo = (uint32_t)sh;
    if (w + 1 < kHdrWords) {
        if (hi) atomicOr(&hdr[w], hi);
        if (lo) atomicOr(&hdr[w + 1], lo);
    } else {
        if (hi) atomicOr(&words[w], hi);
        if (lo) atomicOr(&words[w + 1], lo);
    }
}

// up to 64 bits, MSB first
__device__ __forceinline__ void put_bits64_hdr_atomic(uint32_t* hdr, uint32_t* words, uint64_t pos, uint32_t nbits,
                                                      uint64_t v)
{
    if (nbits > 32) {
        put_bits_hdr_atomic(hdr, words, pos, nbits - 32, (uint32_t)(v >> 32));
        put_bits_hdr_atomic(hdr, words, pos + nbits - 32, 32, (uint32_t)v);
    } else {
        put_bits_hdr_atomic(hdr, words, pos, nbits, (uint32_t)v);
    }
}

// exclusive scan over the workgroup (wave shuffles, then the waves); *total = sum
template <int NT>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t* total)
{
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if ((int)lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (uint32_t w = 0; w < NT / 64; ++w) {
        const uint32_t x = wsum[w];
        pre += w < wave ? x : 0u;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return pre + inc - v;
}

// The header: the fixed fields and the mapping table by one lane, then the
// selectors (unary MTF values) and the delta-coded code lengths as items
// written by all threads at prefix-summed bit offsets.
constexpr uint32_t kEmitC = 16;  // symbols per thread and round
constexpr uint32_t kEmitBufWords = (kEmitThreads * kEmitC * 17 + 31) / 32 + 2;  // code lengths <= 17 bits

// MULTI (Batch::parts > 1): a slot emits its part by role -- the stream header
// only in a stream's first slot, then the block from its magic through its
// last symbol, the exact bit count in out_bits; join_parts adds the trailer.
template <bool MULTI>
__global__ __launch_bounds__(kEmitThreads) void emit_stream(Batch B)
{
    __shared__ uint32_t wsum[kEmitThreads / 64];
    __shared__ uint32_t obuf[kEmitBufWords];
    __shared__ uint64_t s_hdr_bits;
    __shared__ uint32_t hdr[kHdrWords];
    __shared__ uint32_t lc[kMaxGroups * kMaxAlpha];  // code | len << 24 per (table, symbol)
    __shared__ uint8_t sel_l[kSelLds];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    if (B.flags[s] & kFlagHost) {
        if (t == 0) (MULTI ? B.out_bits : B.out_bytes)[s] = 0;
        return;
    }
    uint32_t* words = B.words + (size_t)s * (B.out_cap / 4);
    const uint32_t nMTF = B.nmtf[s], nSel = B.nsel[s], nGroups = B.ngroups[s];
    const uint8_t* len = B.len + (size_t)s * kMaxGroups * kMaxAlpha;
    const uint32_t* code = B.code + (size_t)s * kMaxGroups * kMaxAlpha;
    const uint8_t* sel = B.sel + (size_t)s * B.sel_cap;
    const uint16_t* mtfv = B.mtfv + (size_t)s * (B.cap + 8);
    uint32_t inu[8];
    uint32_t nin = 0;
    for (int q = 0; q < 8; ++q) {
        inu[q] = B.inuse[s * 8 + q];
        nin += __popc(inu[q]);
    }
    const uint32_t alphaSize = nin + 2;
    for (uint32_t w = t; w < kHdrWords; w += kEmitThreads) hdr[w] = 0;
    {
        // the word buffer is not cleared: a header that could spill past the
        // LDS copy (OR-ed straight into memory) gets its spill words zeroed here
        const uint64_t bound = 32 + 48 + 32 + 1 + 24 + 16 + 256 + 3 + 15 + (uint64_t)nSel * (kMaxGroups + 1) +
                               (uint64_t)nGroups * (5 + 33ull * alphaSize);
        if (bound >= (uint64_t)(kHdrWords - 1) * 32)
            for (uint64_t w = kHdrWords - 1 + t; w < (bound >> 5) + 2; w += kEmitThreads) words[w] = 0;
    }
    for (uint32_t i = t; i < nGroups * kMaxAlpha; i += kEmitThreads) lc[i] = code[i] | ((uint32_t)len[i] << 24);
    for (uint32_t i = t; i < min(nSel, kSelLds); i += kEmitThreads) sel_l[i] = sel[i];
    __syncthreads();
    // header (thread 0, sequential, into LDS)
    if (t == 0) {
        uint64_t p = 0;
        auto put = [&](uint32_t nb, uint32_t v) {
            put_bits_hdr(hdr, words, p, nb, v);
            p += nb;
        };
        if (!MULTI || s % B.parts == 0) {
            put(8, 'B'); put(8, 'Z'); put(8, 'h'); put(8, '0' + B.level);
        }
        put(8, 0x31); put(8, 0x41); put(8, 0x59); put(8, 0x26); put(8, 0x53); put(8, 0x59);
        put(32, B.crc[s]);
        put(1, 0);
        put(24, B.orig_ptr[s]);
        uint32_t in16 = 0;
        for (int i = 0; i < 16; ++i) {
            const uint32_t bits16 = (inu[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
            if (bits16) in16 |= 1u << i;
        }
        for (int i = 0; i < 16; ++i) put(1, (in16 >> i) & 1u);
        for (int i = 0; i < 16; ++i)
            if ((in16 >> i) & 1u)
                for (int j = 0; j < 16; ++j) {
                    const uint32_t c = i * 16 + j;
                    put(1, (inu[c >> 5] >> (c & 31)) & 1u);
                }
        put(3, nGroups);
        put(15, nSel);
        s_hdr_bits = p;
    }
    __syncthreads();
    {
        uint64_t p = s_hdr_bits;
        uint32_t total = 0;
        // selectors: MTF value k as k ones and a zero (k < nGroups <= 6)
        {
            const uint8_t* sm = B.sel_mtf + (size_t)s * B.sel_cap;
            const uint32_t per = (nSel + kEmitThreads - 1) / kEmitThreads;
            const uint32_t a = min(nSel, t * per), b = min(nSel, a + per);
            uint32_t nb = 0;
            for (uint32_t i = a; i < b; ++i) nb += sm[i] + 1u;
            uint64_t q = p + block_excl_scan<kEmitThreads>(nb, wsum, &total);
            for (uint32_t i = a; i < b; ++i) {
                const uint32_t k = sm[i];
                put_bits_hdr_atomic(hdr, words, q, k + 1, ((1u << k) - 1u) << 1);
                q += k + 1;
            }
            p += total;
        }
        // code lengths: per table 5 bits of the first length, then per symbol
        // |d| x ("10" up / "11" down) and a zero, d = change from the previous
        {
            const uint32_t nl = nGroups * alphaSize;
            const uint32_t per = (nl + kEmitThreads - 1) / kEmitThreads;
            const uint32_t a = min(nl, t * per), b = min(nl, a + per);
            auto item = [&](uint32_t e, uint32_t& nbits, uint64_t& v) {
                const uint32_t q = e / alphaSize, i = e - q * alphaSize;
                const uint8_t* lq = len + q * kMaxAlpha;
                const int cur = lq[i], prev = i ? lq[i - 1] : cur;
                const int d = cur - prev;
                const uint32_t ad = (uint32_t)(d < 0 ? -d : d);
                v = 0;
                for (uint32_t r = 0; r < ad; ++r) v = (v << 2) | (d > 0 ? 2u : 3u);
                v <<= 1;
                nbits = 2 * ad + 1;
                if (i == 0) {
                    v |= (uint64_t)cur << nbits;
                    nbits += 5;
                }
            };
            uint32_t nb = 0;
            for (uint32_t e = a; e < b; ++e) {
                uint32_t k;
                uint64_t v;
                item(e, k, v);
                nb += k;
            }
            uint64_t q = p + block_excl_scan<kEmitThreads>(nb, wsum, &total);
            for (uint32_t e = a; e < b; ++e) {
                uint32_t k;
                uint64_t v;
                item(e, k, v);
                put_bits64_hdr_atomic(hdr, words, q, k, v);
                q += k;
            }
            p += total;
        }
        if (t == 0) s_hdr_bits = p;
    }
    __syncthreads();
    // data bits, in rounds of kEmitC symbols per thread (thread t codes
    // symbols r0 + t * kEmitC ..): a round's bits are contiguous across the
    // threads, so they are assembled in LDS and leave in coalesced word
    // stores; the round's partial last word carries into the next round.
    // (Each thread writing its own stretch of the stream straight to memory
    // made every store instruction touch 64 scattered lines.)
    const uint64_t hb = s_hdr_bits;
    {
        // header words; the word holding the data's first bit starts the carry
        const uint32_t full = (uint32_t)min<uint64_t>(hb >> 5, kHdrWords - 1);
        for (uint32_t w = t; w < full; w += kEmitThreads) words[w] = hdr[w];
        if (t == 0 && (hb >> 5) >= kHdrWords - 1) atomicOr(&words[kHdrWords - 1], hdr[kHdrWords - 1]);
        for (uint32_t i = t; i < kEmitBufWords; i += kEmitThreads) obuf[i] = 0;
    }
    __syncthreads();
    if (t == 0)  // a spilled header's last word is in memory (OR-ed there), else in LDS
        obuf[0] = (hb >> 5) < kHdrWords - 1 ? hdr[hb >> 5] : atomicOr(&words[hb >> 5], 0u);
    __syncthreads();
    auto sym_lc = [&](uint32_t i, uint32_t v) {
        const uint32_t g = i / kGSize;
        const uint32_t tb = g < kSelLds ? sel_l[g] : sel[g];
        return lc[tb * kMaxAlpha + v];
    };
    uint64_t bitpos = hb;
    for (uint32_t r0 = 0; r0 < nMTF; r0 += kEmitThreads * kEmitC) {
        const uint32_t i0 = min(nMTF, r0 + t * kEmitC), i1 = min(nMTF, i0 + kEmitC);
        uint32_t e[kEmitC];
        uint32_t nb = 0;
        {
            const uint4 v0 = i0 < i1 ? *(const uint4*)(mtfv + i0) : make_uint4(0, 0, 0, 0);
            const uint4 v1 = i0 + 8 < i1 ? *(const uint4*)(mtfv + i0 + 8) : make_uint4(0, 0, 0, 0);
            const uint32_t w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
            for (uint32_t k = 0; k < kEmitC; ++k) {
                e[k] = i0 + k < i1 ? sym_lc(i0 + k, (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu) : 0u;
                nb += e[k] >> 24;
            }
        }
        uint32_t rbits = 0;
        const uint32_t lb0 = (uint32_t)(bitpos & 31) + block_excl_scan<kEmitThreads>(nb, wsum, &rbits);
        if (nb) {
            uint64_t acc = 0;      // pending bits, left aligned at bit 63
            uint32_t wpos = lb0 >> 5, nacc = lb0 & 31;
            bool first_word = true;
#pragma unroll
            for (uint32_t k = 0; k < kEmitC; ++k) {
                const uint32_t l = e[k] >> 24;
                if (l) {
                    acc |= ((uint64_t)(e[k] & 0xFFFFFFu) << (64 - l)) >> nacc;
                    nacc += l;
                    if (nacc >= 32) {
                        const uint32_t wv = (uint32_t)(acc >> 32);
                        if (first_word) atomicOr(&obuf[wpos], wv);
                        else obuf[wpos] = wv;
                        first_word = false;
                        ++wpos;
                        acc <<= 32;
                        nacc -= 32;
                    }
                }
            }
            if (nacc > 0) atomicOr(&obuf[wpos], (uint32_t)(acc >> 32));
        }
        __syncthreads();
        const uint32_t nfull = (uint32_t)(((bitpos & 31) + rbits) >> 5);
        uint32_t* dst = words + (bitpos >> 5);
        // non-temporal: the stream words are read once more (compaction), and
        // dirty lines left in the caches slow the next encode's predictor
        for (uint32_t i = t; i < nfull; i += kEmitThreads) __builtin_nontemporal_store(obuf[i], &dst[i]);
        const uint32_t cv = obuf[nfull];
        __syncthreads();
        for (uint32_t i = 1 + t; i <= nfull; i += kEmitThreads) obuf[i] = 0;
        if (t == 0) obuf[0] = cv;
        __syncthreads();
        bitpos += rbits;
    }
    const uint64_t data_end = bitpos;
    if (t == 0) {  // the last partial word, and zeros under the end marker
        words[data_end >> 5] = (data_end & 31) ? obuf[0] : 0u;
        for (uint64_t w = (data_end >> 5) + 1; w <= ((data_end + 80) >> 5) + 1; ++w) words[w] = 0;
    }
    if (MULTI) {
        if (t == 0) B.out_bits[s] = (uint32_t)data_end;
        return;
    }
    if (t == 0) {
        uint64_t p = data_end;
        auto put = [&](uint32_t nb2, uint32_t v) {
            put_bits_atomic(words, p, nb2, v);
            p += nb2;
        };
        put(8, 0x17); put(8, 0x72); put(8, 0x45); put(8, 0x38); put(8, 0x50); put(8, 0x90);
        put(32, B.crc[s]);  // combined CRC of a one-block stream: rotl(0, 1) ^ blockCRC
        B.out_bytes[s] = (uint32_t)((p + 7) >> 3);
    }
}

// MULTI: a stream's parts joined at bit offsets into its jwords row, then the
// end magic and the combined CRC (rotl(combined, 1) ^ blockCRC over the
// parts).  One workgroup per stream, part after part: destination word i of a
// part is a funnel shift of its source words i - 1 and i, and the word on a
// part boundary also keeps the previous part's last bits.  A stream with a
// periodic part (flagged by the BWT) goes to the host as a whole.
__global__ __launch_bounds__(256) void join_parts(Batch B)
{
    const uint32_t s = blockIdx.x, t = threadIdx.x, s0 = s * B.parts;
    const uint32_t np = B.nparts[s];
    uint32_t host = B.sflags[s];
    for (uint32_t k = 0; k < np; ++k) host |= B.flags[s0 + k] & kFlagHost;
    if (host) {
        if (t == 0) {
            B.sflags[s] = kFlagHost;
            B.sbytes[s] = 0;
        }
        return;
    }
    uint32_t* dst = B.jwords + (size_t)s * (B.jcap / 4);
    uint64_t D = 0;
    uint32_t comb = 0;
    for (uint32_t k = 0; k < np; ++k) {
        const uint32_t bits = B.out_bits[s0 + k], nsw = (bits + 31) >> 5;
        const uint32_t* src = B.words + (size_t)(s0 + k) * (B.out_cap / 4);
        const uint32_t sh = (uint32_t)(D & 31), ndw = (sh + bits + 31) >> 5;
        const uint64_t wd0 = D >> 5;
        auto sw = [&](uint32_t j) -> uint32_t {  // source word j, zero past the part's last bit
            if (j >= nsw) return 0u;
            const uint32_t v = src[j];
            return (j == nsw - 1 && (bits & 31)) ? v & (~0u << (32 - (bits & 31))) : v;
        };
        for (uint32_t i = t; i < ndw; i += 256) {
            uint32_t v = sw(i) >> sh;
            if (sh && i) v |= sw(i - 1) << (32 - sh);
            if (sh && !i) v |= dst[wd0];
            dst[wd0 + i] = v;
        }
        __syncthreads();
        D += bits;
        comb = ((comb << 1) | (comb >> 31)) ^ B.crc[s0 + k];
    }
    if (t == 0) {
        for (uint64_t w = (D + 31) >> 5; w <= ((D + 80) >> 5) + 1; ++w) dst[w] = 0;
        uint64_t p = D;
        auto put = [&](uint32_t nb2, uint32_t v) {
            put_bits_atomic(dst, p, nb2, v);
            p += nb2;
        };
        put(8, 0x17); put(8, 0x72); put(8, 0x45); put(8, 0x38); put(8, 0x50); put(8, 0x90);
        put(32, comb);
        const uint32_t nbytes = (uint32_t)((p + 7) >> 3);
        B.sbytes[s] = nbytes <= B.pay_cap ? nbytes : 0u;
        if (nbytes > B.pay_cap) B.sflags[s] = kFlagHost;
    }
}

// copy the streams (MSB-first words) to their byte offsets in the payload:
// one workgroup per stream; the payload words wholly inside the stream are
// assembled from two source words (byte-swapped) and stored 4 bytes at a
// time, the at most 3 + 3 edge bytes one by one
__global__ __launch_bounds__(256) void compact_streams(Batch B, const uint64_t* __restrict__ offs,
                                                       uint8_t* __restrict__ payload)
{
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const uint32_t nbytes = B.out_bytes[s];
    if (!nbytes) return;
    const uint32_t* words = B.words + (size_t)s * (B.out_cap / 4);
    const uint64_t o = offs[s], e = o + nbytes;
    const uint64_t a0 = (o + 3) >> 2, a1 = e >> 2;
    auto byte_at = [&](uint64_t k) { return (uint8_t)(words[k >> 2] >> (24 - 8 * (k & 3))); };
    if (a0 >= a1) {  // no whole word: bytes only
        for (uint64_t k = t; k < nbytes; k += 256) payload[o + k] = byte_at(k);
        return;
    }
    if (t < 4 && o + t < 4 * a0) payload[o + t] = byte_at(t);
    if (t >= 4 && t < 8 && 4 * a1 + (t - 4) < e) payload[4 * a1 + (t - 4)] = byte_at(4 * a1 + (t - 4) - o);
    uint32_t* p32 = (uint32_t*)payload;
    const uint32_t r = (uint32_t)((4 * a0 - o) & 3), sh = 8 * r;
    const uint64_t j0 = (4 * a0 - o) >> 2;  // source word of the first whole payload word
    for (uint64_t a = a0 + t; a < a1; a += 256) {
        const uint64_t w = j0 + (a - a0);
        const uint32_t x = r ? (words[w] << sh) | (words[w + 1] >> (32 - sh)) : words[w];
        __builtin_nontemporal_store(__builtin_bswap32(x), &p32[a]);  // read next by the SDMA copy
    }
}

// exclusive offsets of the streams' byte counts: one workgroup, every thread
// sums a contiguous run, one block scan, then every thread writes its run
__global__ __launch_bounds__(1024) void scan_offsets(const uint32_t* __restrict__ nbytes, uint32_t n,
                                                     uint64_t* __restrict__ offs)
{
    __shared__ uint64_t wsum64[16];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t a = min(n, t * per), b = min(n, a + per);
    uint64_t sum = 0;
    for (uint32_t i = a; i < b; ++i) sum += nbytes[i];
    uint64_t inc = sum;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(inc, d);
        if ((int)lane >= d) inc += o;
    }
    if (lane == 63) wsum64[wave] = inc;
    __syncthreads();
    uint64_t acc = inc - sum;
    for (uint32_t w = 0; w < wave; ++w) acc += wsum64[w];
    for (uint32_t i = a; i < b; ++i) {
        offs[i] = acc;
        acc += nbytes[i];
    }
    if (b == n && a < b) offs[n] = acc;
    if (n == 0 && t == 0) offs[0] = 0;
}

} // namespace bz
} // namespace lfm

// =============================================================== host side
using namespace lfm::bz;

namespace {

uint32_t host_crc_table[256];
uint32_t host_crc4[4][256];
uint32_t host_crc_shift[kCrcLevels][32];
uint32_t host_crc_unshift[kCrcUnshift][32];
uint32_t host_crc_shb[kCrcLevels][4][256];  // host_crc_shift as byte tables

// runs once per process (crc_tables_on_device)
bool build_crc_tables()
{
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i << 24;
        for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04c11db7u : (c << 1);
        host_crc_table[i] = c;
    }
    // slicing-by-4 tables: 4 zero feeds of a register holding byte v at byte k
    auto feed0 = [](uint32_t c) { return (c << 8) ^ host_crc_table[c >> 24]; };
    for (uint32_t k = 0; k < 4; ++k)
        for (uint32_t v = 0; v < 256; ++v) {
            uint32_t c = v << (8 * k);
            for (int r = 0; r < 4; ++r) c = feed0(c);
            host_crc4[k][v] = c;
        }
    // one zero feed and its inverse (the table's low byte identifies its index)
    uint32_t inv_low[256];
    bool seen[256] = {};
    for (uint32_t x = 0; x < 256; ++x) {
        const uint32_t lo = host_crc_table[x] & 0xFFu;
        if (seen[lo]) std::abort();  // never for CRC-32: the map is a bijection
        seen[lo] = true;
        inv_low[lo] = x;
    }
    auto unfeed0 = [&](uint32_t c) {
        const uint32_t x = inv_low[c & 0xFFu];
        return ((c ^ host_crc_table[x]) >> 8) | (x << 24);
    };
    auto mat_apply = [](const uint32_t* m, uint32_t v) {
        uint32_t r = 0;
        for (int k = 0; k < 32; ++k)
            if ((v >> k) & 1u) r ^= m[k];
        return r;
    };
    auto mat_square = [&](const uint32_t* m, uint32_t* out) {
        for (int k = 0; k < 32; ++k) out[k] = mat_apply(m, m[k]);
    };
    uint32_t z[32];
    for (int k = 0; k < 32; ++k) z[k] = feed0(1u << k);
    for (uint32_t b = 1; b < kRleChunk; b <<= 1) {  // Z^kRleChunk
        uint32_t t2[32];
        mat_square(z, t2);
        std::memcpy(z, t2, sizeof(z));
    }
    std::memcpy(host_crc_shift[0], z, sizeof(z));
    for (int l = 1; l < kCrcLevels; ++l) mat_square(host_crc_shift[l - 1], host_crc_shift[l]);
    for (int l = 0; l < kCrcLevels; ++l)
        for (uint32_t j = 0; j < 4; ++j)
            for (uint32_t v = 0; v < 256; ++v) host_crc_shb[l][j][v] = mat_apply(host_crc_shift[l], v << (8 * j));
    for (int k = 0; k < 32; ++k) host_crc_unshift[0][k] = unfeed0(1u << k);
    for (int l = 1; l < kCrcUnshift; ++l) mat_square(host_crc_unshift[l - 1], host_crc_unshift[l]);
    return true;
}

// Every caller passes here before its first rle1_crc launch on `dev` (the
// current device): the first one uploads, under the mutex, so a later caller
// returns only once the tables are there; nobody writes them again while
// another stream's rle1_crc may be reading them.
bool crc_tables_on_device(int dev)
{
    static const bool built = build_crc_tables();  // function-local static: once, thread-safely
    static std::mutex mu;
    static std::vector<char> uploaded;  // per device
    std::lock_guard<std::mutex> lock(mu);
    if (!built || dev < 0) return false;
    if ((size_t)dev >= uploaded.size()) uploaded.resize((size_t)dev + 1, 0);
    if (uploaded[dev]) return true;
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_crc4), host_crc4, sizeof(host_crc4)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(c_crc_shb), host_crc_shb, sizeof(host_crc_shb)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(c_crc_unshift), host_crc_unshift, sizeof(host_crc_unshift)) != hipSuccess)
        return false;
    uploaded[dev] = 1;
    return true;
}

// stage boundary events of the calling thread (lfm_hip_bzip2_last_stage_ms)
struct StageEvents {
    int dev = -1;
    hipEvent_t ev[6] = {};
    float last_ms[5] = {};
    bool valid = false;
    ~StageEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    bool ready(int d)
    {
        if (dev == d) return true;
        for (hipEvent_t& e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return false;
        }
        dev = d;
        return true;
    }
};
thread_local StageEvents t_stage;
thread_local void (*t_hook)(void*, int) = nullptr;
thread_local void* t_hook_ctx = nullptr;
thread_local uint64_t t_last_blocks = 0;  // bzip2 blocks the calling thread's last call produced (lfm_hip_bzip2_last_blocks)
thread_local uint32_t t_last_place = 0;  // how its sorted rotations were placed (lfm_hip_bzip2_last_place_path)
thread_local uint32_t t_last_bwt[12] = {};  // the path its BWT took (lfm_hip_bzip2_last_bwt_stats)
thread_local uint32_t t_last_jobs[4] = {};  // its sort jobs per sorter capacity (lfm_hip_bzip2_last_sort_jobs)

// rocPRIM temporary storage for the largest use of each primitive in a batch
// of `count` streams (size queries only: no device work).  Carved out of the
// caller's workspace: a per-call stream-ordered allocation of these
// gigabyte-sized buffers stalled every stream of the device for ~0.3 s.
size_t prim_tmp_bytes(uint32_t count, uint32_t cap)
{
    const size_t N = (size_t)count * cap;
    uint64_t* k = nullptr;
    uint32_t* v = nullptr;
    uint8_t* f = nullptr;
    size_t tmp = 0, q = 0;
    const size_t max_seg = (size_t)count * (cap / kBigCap + 1);
    (void)rocprim::segmented_radix_sort_pairs(nullptr, q, k, k, v, v, (unsigned)N, (unsigned)max_seg, v, v, 0,
                                              64 - kBucketBits);
    tmp = std::max(tmp, q);
    (void)rocprim::radix_sort_pairs(nullptr, q, k, k, v, v, (unsigned)N, 0, 64);
    tmp = std::max(tmp, q);

    (void)rocprim::select(nullptr, q, rocprim::counting_iterator<uint32_t>(0), f, v, v, N);
    tmp = std::max(tmp, q);
    (void)rocprim::select(nullptr, q, v, f, v, v, N);
    tmp = std::max(tmp, q);
    (void)rocprim::inclusive_scan(nullptr, q, v, v, N, rocprim::maximum<uint32_t>());
    tmp = std::max(tmp, q);
    return tmp;
}

// The parts of the workspace that are not per-stream kernel buffers.
// cnt: eight device counters, zeroed at the start of every BWT attempt:
//   [0]    chunks of class 0 (<= kSmallCap) from the bucket pass; from the
//          placing chunk sorts (which count up from 0) or tie_offsets on, the
//          length of the tied list (rewritten by every round's compaction)
//   [1]    chunks of class 1 (<= kBigCap); then the length of the compacted
//          group keys of a text round
//   [2]    chunks of class 2 (rocPRIM segmented sort)
//   [3]    sort jobs <= kMiniCap from the bucket pass; zeroed once the host has
//          read them, then streams whose Huffman heaps need u64 entries (rle2;
//          Batch::wide_cnt)
//   [4]    sort jobs <= kTinyCap; zeroed with [3], then Huffman code-length
//          retries (statistics only)
//   [5]    chunks of class 3 (<= kTinyCap)
//   [6]    sort jobs <= kSmallCap (the jobs <= kBigCap and the segmented
//          ones are the chunks of classes 1 and 2: [1], [2])
//   [7]    tied runs tie_runs_direct left to the tie rounds
struct Scratch {
    uint64_t* offs;    // nstreams + 1 byte offsets of the compacted streams
    uint32_t* cnt;     // the counters above (right after offs)
    void* tmp;         // rocPRIM temporary storage (prim_tmp_bytes)
    size_t tmp_bytes;
};

// What LFM_BZ2_STATS=1 reports about the BWT (its first_ties and left_runs)
// and lfm_hip_bzip2_last_bwt_stats about the path bwt_sort took.  Every value is
// a count the host has read back anyway or a host loop counter; chunks to
// text_rounds are those of the last attempt (the one after a restart, if any).
struct BwtStats {
    uint32_t chunks[4] = {};      // chunks per class: <= kTinyCap, <= kSmallCap, <= kBigCap, segmented sort
    uint32_t jobs[4] = {};        // sort jobs per sorter: <= kMiniCap, <= kTinyCap, <= kSmallCap, <= kBigCap
                                  // (lfm_hip_bzip2_last_sort_jobs; not part of the report above)
    uint32_t first_ties = 0;      // tied slots after the chunk sorts
    uint32_t left_runs = 0;       // runs tie_runs_direct left
    uint32_t text_rounds = 0;     // text rounds run
    uint32_t restarted = 0;       // the batch was sorted again with every rotation in the sort
    uint32_t rank_form = 0;       // rank_rebuild: 0 not run, 1 bwt_rank0, 2 from the gathered group keys
    uint32_t doubling_rounds = 0;
    uint32_t flag_periodic = 0;   // bwt_flag_periodic ran
    bool fused_sorts = false;     // the last attempt's chunk sorts placed their rotations (not part of the report above)

    // How the sorted rotations get placed (lfm_hip_bzip2_last_place_path):
    // 0 not at all (restarted: mtf_last reads sa), 1 by the chunk sorts and
    // bwt_place_tied, 2 by bwt_place_sorted over the whole batch -- when the
    // sorts did not place (segmented chunks), or a run was left to the text
    // rounds, whose scratch is where the sorts had placed.
    uint32_t place_path(bool it_full) const
    {
        return it_full ? 0u : (fused_sorts && left_runs == 0 && text_rounds == 0) ? 1u : 2u;
    }
};

// The workspace, described once: every buffer in order, 256-byte aligned.
// With base == nullptr this only sums (lfm_hip_bzip2_workspace_bytes); with
// the workspace base it also points B and S into it.  Either way it sets the
// capacities of B the sizes derive from.  Returns the bytes needed.
//
// level == 0: one slot per stream, sized for the whole block (the layout
// lfm_hip_bzip2_workspace_bytes has always described).  level >= 1: the
// stream owns max_parts(block_bytes, level) slots, each sized for one bzip2
// block of that level; with one part that is the same layout, byte for byte.
size_t layout(uint8_t* base, uint32_t streams, uint32_t block_bytes, uint32_t level, Batch& B, Scratch& S)
{
    B.parts = level ? max_parts(block_bytes, level) : 1u;
    const uint32_t count = streams * B.parts;  // slots
    B.nstreams = count;
    B.raw_cap = (uint32_t)align_up(block_bytes, 16);  // stream stride of the raw blocks (16-byte loads)
    B.cap = rle_cap(block_bytes);
    B.out_cap = out_cap(block_bytes);
    B.sel_cap = sel_cap(block_bytes);
    B.full_cap = B.cap;
    if (B.parts > 1) {
        // a part's text is at most nblockMAX + 5 bytes: the slack rle_cap adds
        // for the 16-byte loads, the same alignment
        const uint32_t part_max = 100000u * level - 19u + 5u;
        B.cap = std::min(B.cap, (uint32_t)align_up((size_t)part_max + 64, 256));
        B.out_cap = std::min(B.out_cap, out_cap(part_max));
        B.sel_cap = (uint32_t)align_up(B.cap / kGSize + 8, 64);
    }
    B.jcap = B.parts * B.out_cap;
    B.pay_cap = out_cap(block_bytes);
    const size_t n = count, N = n * B.cap;
    size_t off = 0;
    auto take = [&](auto*& p, size_t bytes) {
        using P = std::remove_reference_t<decltype(p)>;
        p = base ? (P)(base + off) : nullptr;
        off += align_up(bytes, 256);
    };
    take(B.raw, (size_t)streams * B.raw_cap);
    take(B.T, N);
    take(B.keys_a, N * 8);
    take(B.keys_b, N * 8);
    take(B.vals_a, N * 4);
    take(B.sa, N * 4);
    take(B.rank, N * 4);
    take(B.vals_b, N * 4);
    take(B.cl0, N * 4);
    take(B.cl1, N * 4);
    take(B.uflag, N);
    take(B.mtfv, n * (B.cap + 8) * 2);
    take(B.sel, n * B.sel_cap);
    take(B.sel_mtf, n * B.sel_cap);
    take(B.len, n * kMaxGroups * kMaxAlpha);
    take(B.code, n * kMaxGroups * kMaxAlpha * 4);
    take(B.rfreq, n * kMaxGroups * kMaxAlpha * 4);
    take(B.words, n * B.out_cap);
    take(B.mtf_freq, n * kMaxAlpha * 4);
    take(B.inuse, n * 8 * 4);
    take(B.wide, n * kMaxGroups * 4 + 64);
    take(B.abcnt, n * 512 * 4);
    take(B.itab, n * 1024 * 4);
    // one u32 per stream each
    uint32_t** small[] = {&B.raw_len, &B.n, &B.crc, &B.flags, &B.done, &B.seg_begin, &B.seg_end, &B.nmtf,
                          &B.orig_ptr, &B.nsel, &B.ngroups, &B.out_bytes, &B.nsub, &B.bwt_mode};
    for (uint32_t** q : small) take(*q, n * 4 + 64);
    // pad: two more such arrays that nothing uses.  The engine sizes its
    // batches from the total, so the total stays what it has always been.
    off += 2 * align_up(n * 4 + 64, 256);
    take(S.offs, (n + 1) * 8 + 32);  // the offsets, then the 8 counters
    S.cnt = base ? (uint32_t*)(S.offs + n + 1) : nullptr;
    B.wide_cnt = base ? S.cnt + 3 : nullptr;
    S.tmp_bytes = prim_tmp_bytes(count, B.cap);
    take(S.tmp, S.tmp_bytes);
    if (B.parts > 1) {
        take(B.Tfull, (size_t)streams * B.full_cap);
        uint32_t** per_slot[] = {&B.part_toff, &B.part_roff, &B.part_rlen, &B.out_bits};
        for (uint32_t** q : per_slot) take(*q, n * 4 + 64);
        uint32_t** per_stream[] = {&B.nparts, &B.sflags, &B.sbytes};
        for (uint32_t** q : per_stream) take(*q, (size_t)streams * 4 + 64);
        take(B.jwords, (size_t)streams * B.jcap);
    }
    return off;
}

// What the steps of one bwt_sort call share.  The tied list (slots whose
// rotations still compare equal) lives in `cl`, its length in cnt[0] on the
// device (slot map at Scratch); every round compacts
// it into cl_next and swaps the two.
struct TieRounds {
    hipStream_t st;
    size_t N;            // nstreams * cap
    uint32_t* cnt;       // device counters
    void* tmp;           // rocPRIM temporary storage
    size_t tmp_bytes;
    uint32_t* cl;
    uint32_t* cl_next;
    uint32_t covered;    // bytes of every rotation the order so far accounts for
    bool none_left;      // a count read 0 and no kernel ran since: skip the later reads
    BwtStats stats;
    uint64_t* gk;        // text rounds' group keys: u64 per entry in the rank area, free until the ranks are built
    uint32_t first[8] = {};   // the counters after placing sorts that left no run, read by first_round
    bool first_read = false;  // ... and valid: text_rounds does not read them again

    // the tied list's length, read back: one host synchronisation
    hipError_t read_count(uint32_t* out, size_t bytes = 4)
    {
        hipError_t e = hipMemcpyAsync(out, cnt, bytes, hipMemcpyDeviceToHost, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    }
};

uint32_t list_grid(uint32_t cnt) { return std::min<uint32_t>(4096, (cnt + 255) / 256); }

// the nc sort jobs of list `list`, in XCD-aware order: workgroup b runs on XCD b % 8
// (place: the sorts also append their tied slots to tl, at most tcap of them, and count them in W.cnt[0])
template <int TH, int IPT>
void chunk_sorts(const Batch& B, const ChunkLists& CL, int list, uint32_t nc, bool place, const TieRounds& W, uint32_t* tl,
                 uint32_t tcap)
{
    const uint32_t per = (nc + 7) / 8;
    if (!nc) return;
    if (place)
        hipLaunchKernelGGL((bwt_chunk_sort<TH, IPT, true>), dim3(8 * per), dim3(TH), 0, W.st, B, CL.b[list], CL.e[list], nc,
                           per, tl, W.cnt, tcap);
    else
        hipLaunchKernelGGL((bwt_chunk_sort<TH, IPT, false>), dim3(8 * per), dim3(TH), 0, W.st, B, CL.b[list], CL.e[list],
                           nc, per, nullptr, nullptr, 0u);
}

// Round 0: the bucket pass, the chunk sorts by the 8-byte prefix (one host
// synchronisation between them, for the chunk and job counts), then the tied
// list and the runs short enough to order directly.
hipError_t first_round(const Batch& B, TieRounds& W)
{
    hipStream_t st = W.st;
    const uint32_t count = B.nstreams;
    hipError_t e;
    ChunkLists CL;
    // job lists in the cl0 / cl1 areas: a stream has at most 3 n / kChunk + 1
    // chunks, twice as many jobs, and cap / 8 entries in each list
    const size_t q = W.N / (2 * 4);
    for (int c = 0; c < kJobLists; ++c) {
        CL.b[c] = B.cl0 + c * q;
        CL.e[c] = B.cl1 + c * q;
    }
    CL.cnt = W.cnt;
    uint32_t nch[8] = {};
    if ((e = hipMemsetAsync(W.cnt, 0, 32, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(bwt_bucket<kBucketBits>, dim3(count), dim3(kBucketThreads), 0, st, B, CL);
    if ((e = hipGetLastError()) != hipSuccess || (e = W.read_count(nch, 32)) != hipSuccess) return e;
    // Words 0 to 4 have been read: zero again.  [0] becomes the tied list's
    // length, [3] and [4] (job counts here) are the Huffman stage's counters.
    if ((e = hipMemsetAsync(W.cnt, 0, 20, st)) != hipSuccess) return e;
    W.stats.chunks[0] = nch[5];
    W.stats.chunks[1] = nch[0];
    W.stats.chunks[2] = nch[1];
    W.stats.chunks[3] = nch[2];
    const uint32_t jobs[kJobLists] = {nch[job_cnt_word(0)], nch[job_cnt_word(1)], nch[job_cnt_word(2)],
                                      nch[job_cnt_word(3)], nch[job_cnt_word(4)]};
    W.stats.jobs[0] = jobs[4];
    W.stats.jobs[1] = jobs[3];
    W.stats.jobs[2] = jobs[0];
    W.stats.jobs[3] = jobs[1];
    W.stats.first_ties = W.stats.left_runs = W.stats.text_rounds = 0;
    // The sorts place their rotations themselves (PLACE) when the batch is
    // induced and every chunk goes through them: the segmented sort's keys
    // lie in keys_a, where the entries go.  Between the sorts and bwt_induce
    // only tie_runs_direct (sa at tied slots, cnt[7]) and the two small
    // kernels below run on that path, and none of them writes keys_a or mtfv
    // (the symbols); a text round would (its scratch is both), which is why a
    // call that runs one places the whole batch again.
    const bool fused = !B.it_full && nch[2] == 0;
    W.stats.fused_sorts = fused;
    W.first_read = false;
    auto sorts = [&](bool place, uint32_t* tl) {
        chunk_sorts<kMiniCap / kCsItems, kCsItems>(B, CL, 4, jobs[4], place, W, tl, (uint32_t)W.N);
        chunk_sorts<kTinyCap / kCsItems, kCsItems>(B, CL, 3, jobs[3], place, W, tl, (uint32_t)W.N);
        chunk_sorts<kCsThreads, kCsItems>(B, CL, 0, jobs[0], place, W, tl, (uint32_t)W.N);
        chunk_sorts<kBigThreads, kBigItems>(B, CL, 1, jobs[1], place, W, tl, (uint32_t)W.N);
    };
    W.covered = kKeyBytes;
    W.none_left = false;
    if (fused) {
        // The placing sorts list their tied slots themselves, in the vals_b
        // area (N entries; the text rounds' and free here: the job lists in
        // cl0 / cl1 are still being read), and write sa at those slots only;
        // cnt[0] is the list's length.
        uint32_t* tl = B.vals_b;
        sorts(true, tl);
        hipLaunchKernelGGL(tie_runs_direct, dim3(1024), dim3(256), 0, st, B, tl, W.cnt, W.cnt + 7);
        // queued ahead of the host's read of the counts; void if a run was left (place_path)
        hipLaunchKernelGGL(bwt_place_tied, dim3(256), dim3(256), 0, st, B, tl, W.cnt);
        hipLaunchKernelGGL(bwt_pend_live, dim3(count), dim3(256), 0, st, B);
        if ((e = hipGetLastError()) != hipSuccess || (e = W.read_count(W.first, 32)) != hipSuccess) return e;
        W.stats.first_ties = W.first[0];
        W.stats.left_runs = W.first[7];
        if (W.first[7] == 0) {  // every run sorted: text_rounds takes the counts from W.first
            W.first_read = true;
            return hipSuccess;
        }
        // A run was left to the text rounds, which read sa and uflag at every
        // slot: the sorts once more without PLACE, from vals_a and the job
        // lists (both intact), then the tied list as on the unfused path.
        if ((e = hipMemsetAsync(W.cnt + 7, 0, 4, st)) != hipSuccess) return e;
    }
    if ((e = hipMemsetAsync(B.done, 0, (size_t)count * 4, st)) != hipSuccess) return e;
    sorts(false, nullptr);
    if (nch[2]) {
        hipLaunchKernelGGL(bwt_chunk_keys, dim3(nch[2]), dim3(256), 0, st, B, CL.b[2], CL.e[2]);
        e = rocprim::segmented_radix_sort_pairs(W.tmp, W.tmp_bytes, B.keys_a, B.keys_b, B.vals_a, B.sa,
                                                (unsigned)W.N, nch[2], CL.b[2], CL.e[2], 0, 64 - kBucketBits, st);
        if (e == hipSuccess)
            hipLaunchKernelGGL(bwt_chunk_flags, dim3(nch[2]), dim3(256), 0, st, B, CL.b[2], CL.e[2]);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    W.cl = B.cl0;
    W.cl_next = B.cl1;
    hipLaunchKernelGGL(tie_offsets, dim3(1), dim3(1024), 0, st, B, W.cnt);
    hipLaunchKernelGGL(tie_compact, dim3(count), dim3(256), 0, st, B, B.cl0);
    hipLaunchKernelGGL(tie_runs_direct, dim3(1024), dim3(256), 0, st, B, B.cl0, W.cnt, W.cnt + 7);
    return hipGetLastError();
}

// Text rounds over the tied list (group index / bounds in the mtfv area,
// free here); each starts with a read of the list's length.  Leaves
// none_left set when a read found nothing to do.
hipError_t text_rounds(const Batch& B, TieRounds& W)
{
    hipStream_t st = W.st;
    uint32_t* bnd = (uint32_t*)B.mtfv;
    for (int r = 0; r < kTextRounds; ++r) {
        // counters: [0] tied slots, [7] runs tie_runs_direct left (read with the first round's count)
        uint32_t c8[8] = {};
        hipError_t e = hipSuccess;
        if (r == 0 && W.first_read) std::copy(W.first, W.first + 8, c8);  // first_round has read them (placing sorts)
        else e = W.read_count(c8, r == 0 ? 32 : 4);
        if (e != hipSuccess) return e;
        const uint32_t cnt = c8[0];
        if (r == 0 && !W.stats.fused_sorts) {  // (placing sorts: the first attempt's, set by first_round)
            W.stats.first_ties = cnt;
            W.stats.left_runs = c8[7];
        }
        if (cnt == 0 || (r == 0 && c8[7] == 0)) {  // nothing tied, or tie_runs_direct sorted every run
            W.none_left = true;
            break;
        }
        if ((size_t)cnt * 4 > W.N) break;
        unsigned gbits = 1;
        while ((1u << gbits) < cnt) ++gbits;
        // group index above the text bytes in one 64-bit key: fewer text
        // bytes when the tied list is longer than 2^24
        const uint32_t tb = std::min<uint32_t>(kTextBytes, (64 - gbits) / 8);
        uint32_t* gidx = bnd + cnt;
        const uint32_t grid = list_grid(cnt);
        if (r == 0) hipLaunchKernelGGL(text_gather_keys, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, W.gk);
        hipLaunchKernelGGL(text_bounds, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, W.gk, bnd);
        e = rocprim::inclusive_scan(W.tmp, W.tmp_bytes, bnd, gidx, (size_t)cnt, rocprim::plus<uint32_t>(), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(text_keys, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, gidx, W.covered, tb);
        e = rocprim::radix_sort_pairs(W.tmp, W.tmp_bytes, B.keys_a, B.keys_b, B.vals_a, B.vals_b, cnt, 0,
                                      8 * tb + gbits, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(text_write, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt);
        W.covered += tb;
        ++W.stats.text_rounds;
        e = rocprim::select(W.tmp, W.tmp_bytes, B.keys_b, B.uflag, W.gk, W.cnt + 1, (size_t)cnt, st);
        if (e == hipSuccess) e = rocprim::select(W.tmp, W.tmp_bytes, W.cl, B.uflag, W.cl_next, W.cnt, (size_t)cnt, st);
        if (e != hipSuccess) return e;
        std::swap(W.cl, W.cl_next);
    }
    return hipSuccess;
}

// Ranks of every rotation for doubling (only with every rotation sorted):
// group bounds of the remaining `cnt` tied slots from the last text keys, or
// from the first-round keys when no text round ran.
hipError_t rank_rebuild(const Batch& B, TieRounds& W, uint32_t cnt)
{
    hipStream_t st = W.st;
    hipError_t e = hipSuccess;
    uint64_t* gsrc = W.gk;
    const uint32_t grid = list_grid(cnt);
    if (W.covered == kKeyBytes) gsrc = (uint64_t*)B.vals_b;  // cnt * 8 <= N * 4 when cnt <= N / 2: rank0 otherwise
    if (W.covered == kKeyBytes && (size_t)cnt * 2 > W.N) {
        W.stats.rank_form = 1;
        hipLaunchKernelGGL(bwt_rank0, dim3(B.nstreams), dim3(1024), 0, st, B);
    } else {
        W.stats.rank_form = 2;
        if (W.covered == kKeyBytes)
            hipLaunchKernelGGL(text_gather_keys, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, gsrc);
        uint32_t* bnd2 = (uint32_t*)B.keys_a;  // 2 * cnt u32 fit the keys area
        uint32_t* hv = bnd2 + cnt;
        uint32_t* hvs = B.cl1 == W.cl ? B.cl0 : B.cl1;
        hipLaunchKernelGGL(text_bounds, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, gsrc, bnd2);
        hipLaunchKernelGGL(text_head_slots, dim3(grid), dim3(256), 0, st, W.cl, W.cnt, bnd2, hv);
        e = rocprim::inclusive_scan(W.tmp, W.tmp_bytes, hv, hvs, (size_t)cnt, rocprim::maximum<uint32_t>(), st);
        hipLaunchKernelGGL(bwt_rank_all, dim3(8192), dim3(256), 0, st, B, W.N);
        hipLaunchKernelGGL(text_rank_tied, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, hvs);
        W.cl_next = hvs;
    }
    return e;
}

// Doubling rounds over what the text rounds left (long repeats only), each
// after a read of the list's length, until nothing is tied or h covers the
// block (what is still tied then are the equal rotations of a periodic block).
hipError_t doubling_rounds(const Batch& B, TieRounds& W)
{
    hipStream_t st = W.st;
    uint32_t h = W.covered;
    const uint32_t max_n = B.cap;
    while (!W.none_left) {
        uint32_t cnt = 0;
        hipError_t e = W.read_count(&cnt);
        if (e != hipSuccess) return e;
        if (cnt == 0) break;
        if (h >= max_n) {  // every remaining tie is a pair of equal rotations
            hipLaunchKernelGGL(bwt_flag_periodic, dim3(256), dim3(256), 0, st, B, W.cl, W.cnt);
            W.stats.flag_periodic = 1;
            break;
        }
        const uint32_t grid = list_grid(cnt);
        hipLaunchKernelGGL(bwt_comp_keys, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, h);
        e = rocprim::radix_sort_pairs(W.tmp, W.tmp_bytes, B.keys_a, B.keys_b, B.vals_a, B.vals_b, cnt, 0, 52, st);
        if (e != hipSuccess) return e;
        uint32_t* hv = (uint32_t*)B.keys_a;  // the sort has consumed keys_a
        uint32_t* hvs = hv + cnt;
        hipLaunchKernelGGL(bwt_comp_heads, dim3(grid), dim3(256), 0, st, B, W.cl, W.cnt, hv);
        e = rocprim::inclusive_scan(W.tmp, W.tmp_bytes, hv, hvs, (size_t)cnt, rocprim::maximum<uint32_t>(), st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bwt_comp_rank, dim3(grid), dim3(256), 0, st, B, W.cnt, hvs);
        e = rocprim::select(W.tmp, W.tmp_bytes, W.cl, B.uflag, W.cl_next, W.cnt, (size_t)cnt, st);
        if (e != hipSuccess) return e;
        std::swap(W.cl, W.cl_next);
        h *= 2;
        ++W.stats.doubling_rounds;
    }
    return hipSuccess;
}

// The rotations to sort, sorted: round 0 (bucket pass + chunk sorts by the
// 8-byte prefix), then the tie rounds.  Ties that would need prefix doubling
// (long repeats) restart the batch with every rotation sorted (B.it_full:
// doubling ranks every rotation), which also finds the periodic blocks.
hipError_t bwt_sort(Batch& B, const Scratch& S, hipStream_t st, BwtStats* stats)
{
    TieRounds W{st, (size_t)B.nstreams * B.cap, S.cnt, S.tmp, S.tmp_bytes, B.cl0, B.cl1, kKeyBytes, false, {},
                (uint64_t*)B.rank};
    hipError_t e;
    for (B.it_full = LFM_BWT_FORCE_FULL;; B.it_full = 1) {
        if ((e = first_round(B, W)) != hipSuccess || (e = text_rounds(B, W)) != hipSuccess) return e;
        // ties left (long repeats)
        uint32_t cnt = 0;
        if (!W.none_left && (e = W.read_count(&cnt)) != hipSuccess) return e;
        if (cnt == 0) {
            W.none_left = true;
            break;
        }
        if (!B.it_full) {  // doubling needs the rank of every rotation: sort them all
            W.stats.restarted = 1;
            continue;
        }
        if ((e = rank_rebuild(B, W, cnt)) != hipSuccess) return e;
        break;
    }
    if ((e = doubling_rounds(B, W)) != hipSuccess) return e;
    if (stats) *stats = W.stats;
    return hipSuccess;
}

} // namespace

extern "C" size_t lfm_hip_bzip2_workspace_bytes(uint32_t nstreams, uint32_t block_bytes)
{
    Batch B{};
    Scratch S{};
    return layout(nullptr, nstreams, block_bytes, 0, B, S);
}

extern "C" size_t lfm_hip_bzip2_workspace_bytes_multi(uint32_t nstreams, uint32_t block_bytes, uint32_t level)
{
    if (level < 1 || level > 9) return 0;
    Batch B{};
    Scratch S{};
    return layout(nullptr, nstreams, block_bytes, level, B, S);
}

extern "C" uint32_t lfm_hip_bzip2_max_count_multi(uint32_t block_bytes, uint32_t level)
{
    if (level < 1 || level > 9) return 0;
    Batch B{};
    Scratch S{};
    (void)layout(nullptr, 0, block_bytes, level, B, S);
    return (uint32_t)(((1ull << 32) - 1) / ((uint64_t)B.parts * B.cap));
}

extern "C" size_t lfm_hip_bzip2_out_cap(uint32_t block_bytes) { return out_cap(block_bytes); }

// Compress streams [first, first + count) of the block grid of `img`
// (device, image layout) into `payload` (device, contiguous in block order);
// sizes[i] = compressed size of stream i, flags[i] != 0 -> the stream must be
// produced by the host library (its bytes are absent from the payload).
namespace {
// multi: a stream may take several slots (layout with the level)
int bzip2_blocks(const void* d_img, const uint32_t dims[5], const uint32_t bs[5], uint32_t bpp, uint32_t first,
                 const uint32_t streams, uint32_t level, void* d_ws, size_t ws_bytes, void* d_payload,
                 uint64_t* h_sizes, uint32_t* h_flags, void* stream_, bool multi)
{
    uint32_t count = streams;  // slots, once the layout is known
    hipStream_t st = (hipStream_t)stream_;
    if (!d_img || !dims || !bs || !bpp || !count || level < 1 || level > 9 || !d_ws || !d_payload) return LFM_HIP_EINVAL;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!crc_tables_on_device(dev)) return LFM_HIP_ERUNTIME;
    StageEvents& SE = t_stage;
    SE.valid = false;
    const bool timed = SE.ready(dev);
    auto mark = [&](int i) {
        if (timed) (void)hipEventRecord(SE.ev[i], st);
    };
    Batch B{};
    B.img = (const uint8_t*)d_img;
    uint32_t raw_cap = bpp;
    for (int d = 0; d < 5; ++d) {
        B.g.dims[d] = dims[d];
        B.g.bs[d] = bs[d];
        B.g.nb[d] = (uint32_t)((dims[d] + bs[d] - 1) / bs[d]);
        raw_cap *= bs[d];
    }
    B.g.bpp = bpp;
    B.first_block = first;
    B.level = level;
    B.nblock_max = 100000u * level - 19u;
    Scratch S{};
    if (ws_bytes < layout((uint8_t*)d_ws, streams, raw_cap, multi ? level : 0u, B, S)) return LFM_HIP_EINVAL;
    count = B.nstreams;
    if ((size_t)count * B.cap >= (1ull << 32)) return LFM_HIP_EINVAL;
    // huff_final moves a stream's selectors in 16-byte pieces
    if (B.sel_cap % 16 || ((uintptr_t)d_ws & 15)) return LFM_HIP_EINVAL;
    const bool parts = B.parts > 1;

    hipError_t e = hipSuccess;
    auto ok = [&]() { return (e = hipGetLastError()) == hipSuccess; };
    // RLE1 reads the image directly when every block row is whole 16-byte
    // pieces at 16-byte aligned addresses (the default uint16 96-pixel
    // blocks); other geometries gather the blocks first
    const bool from_img = ((uintptr_t)d_img & 15) == 0 && (bs[0] * bpp) % 16 == 0 && (dims[0] * bpp) % 16 == 0 &&
                          ((dims[0] % bs[0]) * bpp) % 16 == 0;
    mark(0);
    if (!from_img) hipLaunchKernelGGL(gather_blocks, dim3(64, streams), dim3(256), 0, st, B);
    if (!parts) {
        if (from_img) hipLaunchKernelGGL((rle1_crc<true, false>), dim3(count), dim3(kRleThreads), 0, st, B);
        else hipLaunchKernelGGL((rle1_crc<false, false>), dim3(count), dim3(kRleThreads), 0, st, B);
    } else {
        if (from_img) hipLaunchKernelGGL((rle1_crc<true, true>), dim3(streams), dim3(kRleThreads), 0, st, B);
        else hipLaunchKernelGGL((rle1_crc<false, true>), dim3(streams), dim3(kRleThreads), 0, st, B);
        hipLaunchKernelGGL(place_parts, dim3(16, count), dim3(256), 0, st, B);
    }
    if (!ok()) return LFM_HIP_ERUNTIME;
    mark(1);
    // BWT: the rotations of one type sorted (bwt_sort), every other rotation
    // placed by bwt_induce unless bwt_sort had to sort them all (B.it_full)
    BwtStats bwt_stats;
    B.ent = (uint2*)B.keys_a;  // (free after the sorts; the chunk sorts themselves write it when they place)
    if (bwt_sort(B, S, st, &bwt_stats) != hipSuccess) return LFM_HIP_ERUNTIME;
    t_last_place = bwt_stats.place_path(B.it_full != 0);
    {
        const uint32_t v[12] = {bwt_stats.chunks[0], bwt_stats.chunks[1], bwt_stats.chunks[2], bwt_stats.chunks[3],
                                bwt_stats.first_ties, bwt_stats.left_runs, bwt_stats.text_rounds, bwt_stats.restarted,
                                bwt_stats.rank_form, bwt_stats.doubling_rounds, bwt_stats.flag_periodic, 0u};
        std::copy(v, v + 12, t_last_bwt);
        std::copy(bwt_stats.jobs, bwt_stats.jobs + 4, t_last_jobs);
    }
    if (!B.it_full) {
        // the other type placed by one scan, which writes the symbols ll[]
        const uint32_t chunks = (B.cap + kPlaceChunk - 1) / kPlaceChunk;
        if (t_last_place == 2)
            hipLaunchKernelGGL(bwt_place_sorted, dim3(8 * chunks * ((count + 7) / 8)), dim3(256), 0, st, B, chunks);
        hipLaunchKernelGGL(bwt_induce, dim3(count), dim3(64), 0, st, B);
        if (!ok()) return LFM_HIP_ERUNTIME;
    }
    mark(2);
    if (t_hook) t_hook(t_hook_ctx, 1);  // the tie rounds of bwt_sort end with a host synchronisation
    {
        const uint32_t nseg_max = (B.cap + kSeg - 1) / kSeg;
        int32_t* seg_last = (int32_t*)B.keys_a;  // free after the BWT (count * nseg_max KiB << N * 8 bytes)
        const dim3 g((nseg_max + 3) / 4, count);
        if (B.it_full) hipLaunchKernelGGL(mtf_last<false>, g, dim3(256), 0, st, B, nseg_max, seg_last);
        else hipLaunchKernelGGL(mtf_last<true>, g, dim3(256), 0, st, B, nseg_max, seg_last);
        hipLaunchKernelGGL(mtf_prefix, dim3(count), dim3(256), 0, st, B, nseg_max, seg_last);
        hipLaunchKernelGGL(mtf_win, g, dim3(256), 0, st, B, nseg_max, (const int32_t*)seg_last);
        hipLaunchKernelGGL(rle2, dim3(count), dim3(kRle2Threads), 0, st, B);
    }
    // streams whose Huffman weights need u64 heap entries (listed by rle2)
    uint32_t nwide = 0;
    if (!ok() || hipMemcpyAsync(&nwide, B.wide_cnt, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess || nwide > count)
        return LFM_HIP_ERUNTIME;
    mark(3);
    if (t_hook) t_hook(t_hook_ctx, 2);  // after the wide-stream count's synchronisation: rle2 has run
    // stage hook 3 once the Huffman tables are done (emission and compaction
    // still queued): a caller may start its next work beside this tail
    // (earlier, after the second or third code-length round, measured slower:
    // the next encode's kernels then slow these latency-bound rounds)
    // (one per thread, destroyed when the thread exits: gpu_compress starts
    // its slot threads per call)
    static thread_local struct TablesEvent {
        hipEvent_t ev = nullptr;
        int dev = -1;
        ~TablesEvent()
        {
            if (ev) (void)hipEventDestroy(ev);
        }
    } tables_ev;
    if (t_hook && tables_ev.dev != dev) {
        if (tables_ev.ev) (void)hipEventDestroy(tables_ev.ev);
        tables_ev.ev = nullptr;
        tables_ev.dev = -1;
        if (hipEventCreateWithFlags(&tables_ev.ev, hipEventDisableTiming) == hipSuccess) tables_ev.dev = dev;
    }
    hipEvent_t ev_tables = tables_ev.ev;
    for (int it = 0; it < kIters; ++it) {
        if (it == 0) hipLaunchKernelGGL(huff_select_reg<true>, dim3(count), dim3(kHuffThreads), 0, st, B);
        else hipLaunchKernelGGL(huff_select_reg<false>, dim3(count), dim3(kHuffThreads), 0, st, B);
        // uniform heaps, 32 per workgroup: u32 entries for the narrow tables,
        // u64 for the streams rle2 listed, in one launch
        constexpr uint32_t kPlane = 32;  // (stream, table) heaps per wave
        const uint32_t nn = (count * kMaxGroups + kPlane - 1) / kPlane;
        const uint32_t nw = (nwide * kMaxGroups + kPlane / 2 - 1) / (kPlane / 2);
        hipLaunchKernelGGL(huff_lengths_heap<kPlane>, dim3(nn + nw), dim3(64), 0, st, B, nw, nwide);
    }
    hipLaunchKernelGGL(huff_final, dim3(count), dim3(64 * kFinalWaves), 0, st, B);
    mark(4);
    const bool hook3 = t_hook && ev_tables && hipEventRecord(ev_tables, st) == hipSuccess;
    Batch J = B;  // what compaction reads: the slots' streams, or the joined ones
    if (!parts) {
        hipLaunchKernelGGL(emit_stream<false>, dim3(count), dim3(kEmitThreads), 0, st, B);
    } else {
        hipLaunchKernelGGL(emit_stream<true>, dim3(count), dim3(kEmitThreads), 0, st, B);
        hipLaunchKernelGGL(join_parts, dim3(streams), dim3(256), 0, st, B);
        J.words = B.jwords;
        J.out_cap = B.jcap;
        J.out_bytes = B.sbytes;
        J.flags = B.sflags;
    }
    hipLaunchKernelGGL(scan_offsets, dim3(1), dim3(1024), 0, st, J.out_bytes, streams, S.offs);
    hipLaunchKernelGGL(compact_streams, dim3(streams), dim3(256), 0, st, J, S.offs, (uint8_t*)d_payload);
    mark(5);
    if (!ok()) return LFM_HIP_ERUNTIME;
    if (hook3 && hipEventSynchronize(ev_tables) == hipSuccess) t_hook(t_hook_ctx, 3);
    static const bool stats = std::getenv("LFM_BZ2_STATS") && std::atoi(std::getenv("LFM_BZ2_STATS")) != 0;
    if (stats) {
        uint32_t c[8] = {};
        if (hipMemcpyAsync(c, S.cnt, 32, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess)
            std::fprintf(stderr, "lfm_bzip2 stats: %u streams, %u with u64 Huffman heaps, Huffman retries %u, "
                         "tied after the chunk sorts %u, runs left to the tie rounds %u\n", count, c[3], c[4],
                         bwt_stats.first_ties, bwt_stats.left_runs);
    }
    std::vector<uint32_t> nbytes(streams), np(streams, 1u);  // np: bzip2 blocks per stream
    if (hipMemcpyAsync(nbytes.data(), J.out_bytes, streams * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(h_flags, J.flags, streams * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (parts && hipMemcpyAsync(np.data(), B.nparts, streams * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return LFM_HIP_ERUNTIME;
    for (uint32_t i = 0; i < streams; ++i) h_sizes[i] = nbytes[i];
    t_last_blocks = 0;
    for (uint32_t i = 0; i < streams; ++i) t_last_blocks += h_flags[i] ? 0u : np[i];
    if (timed) {
        SE.valid = true;
        for (int i = 0; i < 5; ++i)
            if (hipEventElapsedTime(&SE.last_ms[i], SE.ev[i], SE.ev[i + 1]) != hipSuccess) SE.valid = false;
    }
    return LFM_HIP_OK;
}
} // namespace

extern "C" int lfm_hip_bzip2_blocks(const void* d_img, const uint32_t dims[5], const uint32_t bs[5], uint32_t bpp,
                                    uint32_t first, uint32_t count, uint32_t level, void* d_ws, size_t ws_bytes,
                                    void* d_payload, uint64_t* h_sizes, uint32_t* h_flags, void* stream)
{
    return bzip2_blocks(d_img, dims, bs, bpp, first, count, level, d_ws, ws_bytes, d_payload, h_sizes, h_flags, stream,
                        false);
}

extern "C" int lfm_hip_bzip2_blocks_multi(const void* d_img, const uint32_t dims[5], const uint32_t bs[5],
                                          uint32_t bpp, uint32_t first, uint32_t count, uint32_t level, void* d_ws,
                                          size_t ws_bytes, void* d_payload, uint64_t* h_sizes, uint32_t* h_flags,
                                          void* stream)
{
    return bzip2_blocks(d_img, dims, bs, bpp, first, count, level, d_ws, ws_bytes, d_payload, h_sizes, h_flags, stream,
                        true);
}

extern "C" void lfm_hip_bzip2_set_stage_hook(void (*fn)(void*, int), void* ctx)
{
    t_hook = fn;
    t_hook_ctx = ctx;
}

extern "C" uint64_t lfm_hip_bzip2_last_blocks(void) { return t_last_blocks; }

extern "C" void lfm_hip_bzip2_last_bwt_stats(uint32_t out[12])
{
    if (out) std::copy(t_last_bwt, t_last_bwt + 12, out);
}

extern "C" void lfm_hip_bzip2_last_sort_jobs(uint32_t out[4])
{
    if (out) std::copy(t_last_jobs, t_last_jobs + 4, out);
}

extern "C" uint32_t lfm_hip_bzip2_last_place_path(void) { return t_last_place; }

extern "C" int lfm_hip_bzip2_last_stage_ms(float ms[5])
{
    if (!ms || !t_stage.valid) return 3;
    for (int i = 0; i < 5; ++i) ms[i] = t_stage.last_ms[i];
    return 0;
}

#ifdef LFM_HUFF_STAMPS
// the stamps since the last call, 2 x 4096 x 8 values (HuffStamps), then cleared
extern "C" int lfm_hip_huff_stamps(unsigned long long* out)
{
    if (!out || hipDeviceSynchronize() != hipSuccess) return 3;
    const size_t bytes = sizeof(unsigned long long) * 2 * kStampWgs * kStampSlots;
    void* d = nullptr;
    if (hipGetSymbolAddress(&d, HIP_SYMBOL(g_huff_stamps)) != hipSuccess) return 3;
    if (hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost) != hipSuccess || hipMemset(d, 0, bytes) != hipSuccess) return 3;
    return 0;
}
#endif
