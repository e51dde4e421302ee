// lfm_bz_caps.h -- per-stream capacities of the GPU bzip2 encoder, from the
// bytes of one 5-D block.  The only place these formulas are written: the
// encoder (lfm_bzip2.hip), the host engine (lfm_internal.h) and, through
// lfm_hip_bzip2_out_cap, the Python binding all read them here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lfm::bz {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// RLE1 block (elements): bzip2's first run-length stage can grow a block by a
// quarter (4 bytes + count per run of 4), plus slack for the 16-byte loads
inline uint32_t rle_cap(uint32_t block_bytes) { return (uint32_t)align_up((size_t)block_bytes + block_bytes / 4 + 64, 256); }

// compressed stream (bytes): what the payload reserves per stream
inline uint32_t out_cap(uint32_t block_bytes) { return (uint32_t)align_up((size_t)block_bytes + block_bytes / 50 + 4096, 256); }

constexpr int kGSize = 50;  // symbols per Huffman selector (compress.c BZ_G_SIZE)

// selectors of a stream
inline uint32_t sel_cap(uint32_t block_bytes) { return (uint32_t)align_up(rle_cap(block_bytes) / kGSize + 8, 64); }

// bzip2 blocks libbzip2 can cut a block of block_bytes into at `level` (1..9):
// the RLE1 text is at most 5/4 of the block, and every part but the last holds
// at least nblockMAX = 100000 * level - 19 bytes of it.  The slots a stream
// owns in the encoder's (lfm_bzip2.hip) and the decoder's (lfm_bunzip2.hip)
// multi-block workspaces.
inline uint32_t max_parts(uint32_t block_bytes, uint32_t level)
{
    const uint64_t worst = (uint64_t)block_bytes + block_bytes / 4 + 1;
    return (uint32_t)(worst / (100000u * level - 19u)) + 1u;
}

} // namespace lfm::bz
