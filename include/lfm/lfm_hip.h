/*
 * lfm_hip.h -- extern "C" HIP shim of the LFM predictor path (gfx950).
 *
 * This is the internal kernel boundary the host encoder (klb_imageIO) calls;
 * it replaces the reference's CUDA launchers and their call sites:
 *   predictorK_{tiles,angle,space}_GPU + symbolize_GPU
 *       (lfm_Predictors.h:16-40, called at klb_imageIO.cpp:1270-1300, :1696-1737)
 *       -> lfm_hip_predict  (all frames of a stack in one launch, fused symbolize)
 *   bwt_GPU + static_bwt_GPU + sum_bwt_GPU inside bwt_entropy_2D and the
 *   candidate loop of predict_and_2DEntropy / writeImage
 *       (lfm_Predictors.h:33-43; klb_imageIO.cpp:2030-2093, :2197-2225, :2273-2306)
 *       -> lfm_hip_select / lfm_hip_entropy2d
 *
 * Conventions: plain device pointers owned by the caller, explicit stream
 * (a hipStream_t passed as void*, NULL = default stream), asynchronous unless
 * stated, status code return.  The caller selects the device (hipSetDevice).
 */
#ifndef LFM_HIP_H
#define LFM_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum lfm_hip_status {
    LFM_HIP_OK = 0,
    LFM_HIP_EINVAL = 1,    /* bad argument                                   */
    LFM_HIP_ERUNTIME = 2,  /* HIP runtime error (launch / alloc / copy)      */
    LFM_HIP_ENOTINV = 3,   /* frame is not invertible (angle/space temporal) */
    LFM_HIP_ENODEV = 4     /* no usable GPU                                  */
};

/* families: 0 = tiles ("ANGLE_AND_SPACE", LFM_PREDICTOR_WAY 0), 1 = angle, 2 = space */

/* Forward predictor + symbolize for nframes consecutive frames of one volume.
 * d_in holds frames z0 .. z0+nframes-1 (W*H uint16 each, x fastest); frame
 * z is temporal when (video_bit & z) is odd, and then uses the raw frame z-1
 * (d_in of the previous frame, or d_prev for the first one).  predictor 0
 * copies the raw frames.  d_out receives uint16 symbols in the same layout.
 * Alignment: any 2-byte aligned pointers are legal.  The ring, vec and
 * frame-pair kernels move 16 bytes per lane between d_in / d_prev / d_out and
 * LDS, so they run only when d_in, d_out and (where frame 0 is temporal: video
 * bit and odd z0) d_prev are 16-byte aligned; with any other base the call
 * takes predict_generic, which makes 2-byte accesses only and is several times
 * slower.  lfm_hip_predict_candidates follows the same rule for d_frame and
 * d_out7 and then runs one generic launch per predictor. */
int lfm_hip_predict(const uint16_t* d_in, const uint16_t* d_prev, uint16_t* d_out, int W, int H, int nframes,
                    int T, int family, int predictor, int video_bit, int z0, void* stream);

/* One kernel launch of a forward-predictor call, as lfm_hip_predict_plan reports it. */
enum lfm_predict_kernel {
    LFM_PK_COPY = 0,      /* predictor 0: a device-to-device copy, no kernel */
    LFM_PK_GENERIC = 1,   /* predict_generic: one thread per pixel            */
    LFM_PK_RING = 2,      /* predict_ring: T <= 31, W % 8 == 0, W >= 32       */
    LFM_PK_VEC = 3,       /* predict_vec: T 13 / 15                           */
    LFM_PK_VEC_PAIR = 4,  /* predict_vec_pair: video volumes, T 13 / 15       */
    LFM_PK_CANDS = 5      /* predict_cands: seven candidates, grid_y = 7      */
};
typedef struct lfm_predict_launch {
    int kernel;         /* enum lfm_predict_kernel */
    int first;          /* first frame of the call that this launch codes */
    int nframes;        /* frames it codes (vec_pair: 2 * pairs) */
    int pairs;          /* vec_pair: (spatial, temporal) frame pairs, else 0 */
    int strip;          /* pixels per strip (0: copy / generic, as all fields to xcd_map) */
    int nstrip;         /* strips per row, the last one may be partial */
    int rows_per_step;  /* rows (of each frame) a workgroup codes between two barriers */
    int rows_per_piece; /* rows per row piece, a whole number of steps */
    int npiece;         /* row pieces per frame */
    int R;              /* row slots of the LDS ring */
    int RP;             /* row slots of the previous-frame ring (temporal frames), else 0 */
    int halo;           /* pixels left of a strip kept per ring slot: 16 or 32 */
    int xcd_map;        /* 1: the strips of a (frame, piece) are workgroups b, b + 8, ... */
    int grid_x, grid_y; /* workgroups */
    int threads;        /* per workgroup */
    int lds_bytes;      /* dynamic LDS per workgroup */
} lfm_predict_launch;
#define LFM_PREDICT_MAX_LAUNCHES 7

/* The launches lfm_hip_predict would make for these arguments, or with
 * `candidates` lfm_hip_predict_candidates for one W x H frame (nframes,
 * predictor, video_bit and z0 are then ignored), in launch order, without
 * launching anything: at most three (a video volume's temporal first frame,
 * its frame pairs, its unpaired last frame), and seven for the candidates'
 * per-predictor generic loop.  `aligned` says whether the call's pointers are
 * 16-byte aligned (see lfm_hip_predict).  Both entries launch exactly this
 * list.  Returns the number of launches written to out[0 .. cap), or -1 for
 * arguments lfm_hip_predict refuses or a cap that is too small.  With the
 * automatic piece count it asks the HIP runtime for the kernel's occupancy and
 * the device's CU count (256 CUs x 1 workgroup without a device); with a
 * forced piece count (below) it is pure: no HIP call. */
int lfm_hip_predict_plan(int W, int H, int nframes, int T, int family, int predictor, int video_bit, int z0,
                         int candidates, int aligned, lfm_predict_launch* out, int cap);
/* Test hook, process-wide: n > 0 replaces the planner's "resident workgroups /
 * (frames x strips)" piece count by n, for every later plan of every thread;
 * the cap of H / (2 (T + 1)) pieces and the rounding of a piece to whole steps
 * still apply.  0 (the default) restores the automatic count.  Returns the
 * previous value.  Production code never calls it. */
int lfm_hip_predict_set_pieces(int n);

/* Inverse of lfm_hip_predict (decode): symbols -> pixels for nframes frames
 * starting at global frame z0; a temporal first frame (video, odd z0) needs
 * the decoded frame z0-1 in d_prev.  ENOTINV for temporal frames of the
 * angle / space families (their residual is not invertible). */
int lfm_hip_unpredict(const uint16_t* d_sym, const uint16_t* d_prev, uint16_t* d_out, int W, int H, int nframes,
                      int T, int family, int predictor, int video_bit, int z0, void* stream);
/* lfm_hip_unpredict without the synchronisation: the kernels are queued on
 * `stream` and the launch's status word is copied into *h_status (pinned host
 * memory) behind them; once the stream has passed that point the caller hands
 * it to lfm_hip_unpredict_check.  The pipelined decode (gpu_decode) checks
 * each chunk's words at the event its download already waits for. */
int lfm_hip_unpredict_async(const uint16_t* d_sym, const uint16_t* d_prev, uint16_t* d_out, int W, int H,
                            int nframes, int T, int family, int predictor, int video_bit, int z0, int* h_status,
                            void* stream);
/* LFM_HIP_OK when a status word says the pixels are valid (0, or a band
 * hand-over timeout repaired on the device, reported on stderr), else
 * LFM_HIP_ERUNTIME. */
int lfm_hip_unpredict_check(int status);
/* Which kernel lfm_hip_unpredict runs for W x H frames of lenslet size T:
 * 0 the chain (one wave per 64-row band, bands hand rows over in memory),
 * 1 the frame wave (one wave per frame, the band above's rows kept in LDS),
 * 2 the one-wave kernel (rows of earlier bands from memory); -1 for
 * T <= 0, T > 31, W <= 0 or H <= 0.  Pure: no HIP call. */
int lfm_hip_unpredict_path(int W, int H, int T);

/* The seven spatial candidates of one frame (predictors 1..7, symbolized) in
 * one launch: candidate k goes to d_out7 + (k-1)*W*H. */
int lfm_hip_predict_candidates(const uint16_t* d_frame, uint16_t* d_out7, int W, int H, int T, int family,
                               void* stream);

/* 2D entropy of a candidate buffer of npix uint16 symbols (450000-pixel
 * chunks, klb_imageIO.cpp:2030-2093).  Synchronous: writes the float result
 * (without the 0.96 raw-candidate factor) to *entropy. */
int lfm_hip_entropy2d(const uint16_t* d_cand, uint64_t npix, float* entropy, void* stream);
/* Test / diagnostic entry: the integer bigram histograms the selection kernels
 * count for d_cands[0..ncand) (a host array of 1..8 device buffers of npix
 * symbols each, any 2-byte alignment), before any float arithmetic:
 * d_hist[ncand][nchunks][65536] with nchunks = ceil(npix / 450000) and bin =
 * (val << 8) | partner.  Bins 0 and 0xFFFF and the sentinel's bigram are
 * included; the end-of-L element has none.  Same launches and counting code as
 * lfm_hip_entropy2d / lfm_hip_select.  Synchronous. */
int lfm_hip_entropy2d_hist(const uint16_t* const* d_cands, int ncand, uint64_t npix, uint32_t* d_hist, void* stream);

/* Predictor selection on one frame: builds the 8 candidates (0 = raw,
 * k = predictor k, spatial), their 2D entropies (candidate 0 scaled by 0.96)
 * and the reference argmin (exact ties -> highest index).  Synchronous.
 * d_workspace may be NULL (allocated internally) or hold
 * lfm_hip_select_workspace_bytes(W, H) bytes. */
size_t lfm_hip_select_workspace_bytes(int W, int H);
int lfm_hip_select(const uint16_t* d_frame, int W, int H, int T, int family, float entropy[8], int* chosen,
                   void* d_workspace, void* stream);

/* bzip2 (libbzip2 1.0.6 byte-exact) of the blocks [first, first + count) of
 * the x-fastest block grid of a device image (dims / bs as in the .lfm
 * header, bpp bytes per sample) at `level`: the compressed streams land
 * back to back in d_payload (block order); h_sizes[i] / h_flags[i] per
 * stream (flag != 0: the stream is NOT in the payload and must be produced by
 * the host library -- RLE1 block reaching nblockMAX, a periodic block, or a
 * block above about 350 000 sorted rotations whose sort would need 1 024 chunk
 * cuts or more).
 * d_ws: lfm_hip_bzip2_workspace_bytes(count, blockBytes); d_payload: count *
 * lfm_hip_bzip2_out_cap(blockBytes) bytes.  Synchronous. */
size_t lfm_hip_bzip2_workspace_bytes(uint32_t count, uint32_t block_bytes);
size_t lfm_hip_bzip2_out_cap(uint32_t block_bytes);
int lfm_hip_bzip2_blocks(const void* d_img, const uint32_t dims[5], const uint32_t bs[5], uint32_t bpp,
                         uint32_t first, uint32_t count, uint32_t level, void* d_ws, size_t ws_bytes,
                         void* d_payload, uint64_t* h_sizes, uint32_t* h_flags, void* stream);
/* The same for streams that libbzip2 cuts into several bzip2 blocks (RLE1 text
 * reaching nblockMAX = 100000 * level - 19): the device finds the cuts as
 * libbzip2 does, compresses every part as a block of its own and joins them
 * at bit offsets behind one stream header, so only periodic streams (any
 * periodic part) come back flagged.  A stream takes max_parts slots of the
 * workspace, max_parts from the worst-case RLE1 length (5/4 of blockBytes) and
 * nblockMAX(level), each slot sized for one block of that level.  Where
 * max_parts is 1 (the default 96x96x8 uint16 block at its level 2) the size,
 * the layout and the launches are those of lfm_hip_bzip2_blocks, and a stream
 * that would need a second block is flagged.  Arguments, payload capacity,
 * stage times and the stage hook as for lfm_hip_bzip2_blocks; the workspace is
 * lfm_hip_bzip2_workspace_bytes_multi(count, blockBytes, level) (0 for a
 * level outside 1..9).  lfm_hip_bzip2_max_count_multi: the largest count one
 * call takes (the slots' texts are indexed in 32 bits). */
size_t lfm_hip_bzip2_workspace_bytes_multi(uint32_t count, uint32_t block_bytes, uint32_t level);
uint32_t lfm_hip_bzip2_max_count_multi(uint32_t block_bytes, uint32_t level);
int lfm_hip_bzip2_blocks_multi(const void* d_img, const uint32_t dims[5], const uint32_t bs[5], uint32_t bpp,
                               uint32_t first, uint32_t count, uint32_t level, void* d_ws, size_t ws_bytes,
                               void* d_payload, uint64_t* h_sizes, uint32_t* h_flags, void* stream);
/* bzip2 blocks in the payload of the calling thread's last lfm_hip_bzip2_blocks
 * or lfm_hip_bzip2_blocks_multi (one per unflagged stream for the former). */
uint64_t lfm_hip_bzip2_last_blocks(void);
/* The path the BWT sort of the calling thread's last lfm_hip_bzip2_blocks or
 * lfm_hip_bzip2_blocks_multi took (read-only; counts the call had read back
 * anyway and its host loop counters, no further synchronisation):
 * [0..3] chunks sorted per class (at most 1 024 rotations, at most 2 048, one
 * bucket of at most 4 096, segmented sort), [4] slots tied on their 8-byte
 * prefix after the chunk sorts, [5] tied runs left to the tie rounds (more than
 * 32 members, or two that agree on 72 bytes), [6] text rounds run -- [0..6] of
 * the last attempt --, [7] 1 when the batch was sorted again with every rotation
 * in the sort, [8] how the doubling ranks were built (0 not at all, 1 from the
 * whole sorted order, 2 from the tied list's group keys), [9] doubling rounds
 * run, [10] 1 when streams still tied after the last round were flagged as
 * periodic, [11] 0. */
void lfm_hip_bzip2_last_bwt_stats(uint32_t out[12]);
/* The sort jobs of that call's last attempt: slot ranges of whole buckets
 * sorted by one workgroup each, per sorter capacity (at most 512 rotations, at
 * most 1 024, at most 2 048, at most 4 096).  A chunk is one job, or two where
 * a chunk of several buckets and more than 512 rotations is sorted as its
 * slots before its last bucket and that bucket; the segmented-sort class is
 * not among them. */
void lfm_hip_bzip2_last_sort_jobs(uint32_t out[4]);
/* How the sorted rotations of the calling thread's last lfm_hip_bzip2_blocks
 * or lfm_hip_bzip2_blocks_multi were placed in the final order (read-only,
 * decided from the counts above): 0 not at all (the batch was sorted again
 * with every rotation in the sort), 1 by the chunk sorts themselves, 2 by the
 * placement kernel over the whole batch (segmented chunks, or a tied run left
 * to the text rounds). */
uint32_t lfm_hip_bzip2_last_place_path(void);
/* Stage times (HIP events on its stream, ms) of the calling thread's last
 * lfm_hip_bzip2_blocks / lfm_hip_bzip2_blocks_multi: [0] RLE1 + CRC, [1] BWT (buckets, chunk sorts, tie
 * rounds), [2] MTF + RUNA/RUNB, [3] Huffman tables, [4] bit emission +
 * compaction.  Returns 0, or 3 when no call has completed on this thread. */
int lfm_hip_bzip2_last_stage_ms(float ms[5]);
/* Progress hook of the calling thread's lfm_hip_bzip2_blocks calls: fn(ctx,
 * stage) once the device has finished stage 1 (BWT) and stage 2 (MTF + RUNA/
 * RUNB), at the host synchronisations that follow them, and stage 3 (the
 * Huffman tables; emission and compaction still queued behind them); fn ==
 * NULL removes it.  The pipelined encoder releases the next stack's GPU
 * bzip2 at stage 3 of each slot's last batch. */
void lfm_hip_bzip2_set_stage_hook(void (*fn)(void* ctx, int stage), void* ctx);

/* GPU bzip2 decode of `count` single-block streams (the .lfm block payloads,
 * SURVEY.md 8(f2); replaces the per-block BZ2_bzBuffToBuffDecompress of
 * klb_imageIO.cpp:1748-1821).  d_payload: device copy of the payload, 4-byte
 * aligned, readable 8 bytes past its end; stream i is h_offs[i] .. h_offs[i+1]
 * (host array of count + 1 byte offsets) and decodes into d_out + i *
 * out_stride.  h_lens[i] = decoded bytes; h_flags[i]: 0 ok, 1 decode this
 * stream with the host library (several blocks, randomised, malformed,
 * larger than out_stride, or periodic: lfm_hip_bunzip2_set_periodic below),
 * 2 block CRC mismatch.  d_ws:
 * lfm_hip_bunzip2_workspace_bytes(count, out_stride).  Synchronous. */
size_t lfm_hip_bunzip2_workspace_bytes(uint32_t count, uint32_t out_stride);
int lfm_hip_bunzip2_blocks(const void* d_payload, const uint64_t* h_offs, uint32_t count, void* d_out,
                           uint32_t out_stride, void* d_ws, size_t ws_bytes, uint32_t* h_lens, uint32_t* h_flags,
                           void* stream);
/* lfm_hip_bunzip2_blocks without the final synchronisation: returns once the
 * kernels and the copies into h_lens / h_flags are queued on `stream`
 * (h_lens / h_flags must be pinned host memory; read them after the stream or
 * an event recorded behind the call has completed).  The pipelined decode
 * (gpu_decode) overlaps one chunk's kernels with another's copies. */
int lfm_hip_bunzip2_issue(const void* d_payload, const uint64_t* h_offs, uint32_t count, void* d_out,
                          uint32_t out_stride, void* d_ws, size_t ws_bytes, uint32_t* h_lens, uint32_t* h_flags,
                          void* stream);
/* The same pair for streams of several bzip2 blocks (what libbzip2 and
 * lfm_hip_bzip2_blocks_multi write for a block above ~900 kB, or a smaller one
 * that grows under RLE1).  `level` (1..9) is the batch's bzip2 level: a stream
 * takes lfm_hip_bunzip2_max_parts(out_stride, level) slots of the workspace
 * (the encoder's bound: the worst-case RLE1 length, 5/4 of out_stride, over
 * nblockMAX(level)), each sized for one bzip2 block of that level.  One wave
 * still reads a stream's blocks one after the other (a block's start is known
 * once the block before it is decoded); the inverse BWT and the RLE1 decode
 * run per block, each block's bytes landing behind those of the blocks before
 * it, each checked against its own CRC and the stream's combined CRC against
 * their fold.  h_lens[i] is the stream's decoded length and h_flags[i] as
 * above: 1 for a stream with more blocks than slots, a block above the
 * level's size, a periodic block (unless lfm_hip_bunzip2_set_periodic(1), see
 * below), a damaged magic or combined CRC or more than out_stride decoded bytes (nothing of a part that does not fit is
 * written); 2 when a block's bytes do not match its CRC.  Where max_parts is 1
 * (the default 96x96x8 uint16 block at its level 2) the size, the layout and
 * the launches are those of the single-block pair.  The workspace is
 * lfm_hip_bunzip2_workspace_bytes_multi(count, out_stride, level); a level
 * outside 1..9 gives 0 there, 0 parts and LFM_HIP_EINVAL here. */
uint32_t lfm_hip_bunzip2_max_parts(uint32_t out_stride, uint32_t level);
size_t lfm_hip_bunzip2_workspace_bytes_multi(uint32_t count, uint32_t out_stride, uint32_t level);
int lfm_hip_bunzip2_blocks_multi(const void* d_payload, const uint64_t* h_offs, uint32_t count, void* d_out,
                                 uint32_t out_stride, uint32_t level, void* d_ws, size_t ws_bytes, uint32_t* h_lens,
                                 uint32_t* h_flags, void* stream);
int lfm_hip_bunzip2_issue_multi(const void* d_payload, const uint64_t* h_offs, uint32_t count, void* d_out,
                                uint32_t out_stride, uint32_t level, void* d_ws, size_t ws_bytes, uint32_t* h_lens,
                                uint32_t* h_flags, void* stream);
/* bzip2 blocks whose text after RLE1 is exactly periodic (w w ... w: a constant
 * 16-bit value with two different bytes, for one).  Their LF permutation has
 * several cycles, and libbzip2's n steps from origPtr go n / q times round
 * the one of the start, of the period's length q.  One process-wide switch
 * for the four entries above, read once per call, when the call is issued.
 * 0 (the default; env LFM_BUNZIP2_PERIODIC=1 starts with 1): such a block's
 * stream comes back with flag 1, as before this switch existed.  1: the
 * inverse BWT places the q bytes of one trip and repeats them up to n, the
 * same bytes libbzip2 gives, whatever q and n are; the block's CRC decides
 * as for any other block (flag 2 for an origPtr that names a row of another
 * cycle).  The setter returns the previous value.  Neither makes a device
 * call. */
int lfm_hip_bunzip2_set_periodic(int on);
int lfm_hip_bunzip2_get_periodic(void);

/* Decoded blocks first .. first + count - 1 (block i at d_blocks + (i -
 * first) * stride, x fastest) back into the device image (the inverse of the
 * writer's block gather, klb_imageIO.cpp:133-140).  Asynchronous. */
int lfm_hip_scatter_blocks(const void* d_blocks, uint32_t stride, uint32_t first, uint32_t count,
                           const uint32_t dims[5], const uint32_t bs[5], uint32_t bpp, void* d_img, void* stream);

/* The box lb .. lb + n - 1 (xyzct, x fastest) of a device image of src_dims
 * (bpp = 1, 2, 4 or 8 bytes per sample) into the dense device array d_dst of
 * n[4] * ... * n[0] samples; d_dst must not overlap the image.  Rows are
 * copied in 16-byte accesses where a row's two addresses differ by a multiple
 * of 16 (single bytes up to the first boundary and after the last), else in
 * 4-, 2- or 1-byte accesses.  EINVAL for a zero extent, a box that leaves the
 * image or another bpp.  Asynchronous. */
int lfm_hip_crop_region(const void* d_src, const uint32_t src_dims[5], const uint32_t lb[5], const uint32_t n[5],
                        uint32_t bpp, void* d_dst, void* stream);

/* Synthetic light-field stack of SURVEY.md 8(d) (integer generator) written
 * straight into device memory: frames z0 .. z0+Z-1 (X*Y pixels each) of
 * volume (c, t) = (0, t_index), global pixel index offset idx0 (a z-slab of a
 * c = t = 1 stack: z0 = first frame, idx0 = z0*X*Y). */
int lfm_hip_synth(uint16_t* d_out, int X, int Y, int Z, int T, int t_index, int z0, uint64_t idx0, uint64_t seed,
                  void* stream);

/* number of visible HIP devices (0 when no GPU / no runtime) */
int lfm_hip_device_count(void);

/* debug switch (env LFM_FORCE_GENERIC=1): route predictor launches to the
 * one-thread-per-pixel kernel instead of the LDS-ring kernel */
int lfm_hip_force_generic(void);

#ifdef __cplusplus
}
#endif
#endif
