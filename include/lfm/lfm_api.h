/*
 * lfm_api.h -- liblfm extensions beyond the reference C ABI.
 *
 *  - lfm_set_family / lfm_get_family: the predictor family (0 tiles,
 *    1 angle, 2 space), a compile-time constant in the reference
 *    (src/common.h:19 LFM_PREDICTOR_WAY); default from env LFM_PREDICTOR_WAY.
 *  - writeLFMstack_c / readLFMstack_c: the MEX writeLFMstack / readLFMstack
 *    argument set (predictor request, Nnum, video flag) as plain C, for
 *    ctypes / cgo / JNI callers (matlabWrapper/writeLFMstack.cpp:360-433).
 *  - lfm_encoder_*: reusable encoder context that encodes to memory from a
 *    host or a DEVICE-resident stack and reports per-stage timings (bench).
 *  - lfm_writer_* / lfm_reader_*: stacks larger than memory -- block layers
 *    appended over time to one .lfm file, and region reads that fetch only
 *    the bytes of the blocks they need (at the end of this file); the writer
 *    checkpoints its table, so lfm_recover saves the complete layers of a
 *    file that was never closed and a live reader reads them meanwhile.
 */
#ifndef LFM_API_H
#define LFM_API_H

#include <stdint.h>
#include <stddef.h>
#include "common.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LFM_API __attribute__((visibility("default")))

LFM_API int lfm_set_family(int family);
LFM_API int lfm_get_family(void);
/* Interface version of this header (also in lfm_version()'s string).
 * 2: lfm_decode_memory_roi takes out_bytes before numThreads (round 5; a
 *    caller built against version 1 passed numThreads third-to-last). */
#define LFM_API_VERSION 2
LFM_API const char* lfm_version(void);
LFM_API int lfm_api_version(void);

/* predictor_request: header bits 0-6 (0..7 auto, 8..15 forced k = request-8);
 * video: header bit 7.  Returns the writeKLBstack codes. */
LFM_API int writeLFMstack_c(const void* im, const char* filename, const uint32_t xyzct[KLB_DATA_DIMS],
                            int dataType, int numThreads, const float pixelSize[KLB_DATA_DIMS],
                            const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                            const char metadata[KLB_METADATA_SIZE], int predictor_request, int Nnum, int video);

/* Decode into im (caller-allocated, getImageSizeBytes); the header fields are
 * returned through the optional out pointers (headerVersion, Nnum). */
LFM_API int readLFMstack_c(const char* filename, void* im, int numThreads, uint8_t* headerVersion, uint8_t* Nnum);

typedef struct lfm_encode_stats {
    double total_ms;      /* whole encode, wall clock                        */
    double h2d_ms;        /* host -> device upload (0 for device input)      */
    double select_ms;     /* predictor selection (kernels + sync), wall       */
    double predict_ms;    /* predictor kernels, HIP events                    */
    double d2h_ms;        /* symbols device -> host                           */
    double compress_ms;   /* block compression + in-order assembly, wall      */
    int chosen;           /* predictor written to the header (bits 0-6)       */
    int header_version;   /* final header byte                                */
    float entropy[8];     /* candidate entropies when auto-selected, else 0   */
    uint64_t out_bytes;   /* size of the .lfm produced                        */
    double bz_stage_ms[5];/* GPU bzip2 stages (lfm_hip_bzip2_last_stage_ms order), HIP events,
                             summed over a HIP stream's batches, max over the streams */
    uint64_t bz_in_bytes; /* block bytes the GPU bzip2 stage compressed       */
} lfm_encode_stats;

typedef struct lfm_encoder lfm_encoder;

/* device < 0: current device; numThreads <= 0: host CPU share */
LFM_API lfm_encoder* lfm_encoder_create(int device, int numThreads);
LFM_API void lfm_encoder_destroy(lfm_encoder* enc);

/* Encode a stack to an in-memory .lfm.  img_is_device != 0: `img` is a device
 * pointer on the encoder's device.  *out stays valid until the next call on
 * this encoder or its destruction. */
LFM_API int lfm_encoder_encode(lfm_encoder* enc, const void* img, int img_is_device,
                               const uint32_t xyzct[KLB_DATA_DIMS], int dataType, int headerVersion, int Nnum,
                               const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                               const char metadata[KLB_METADATA_SIZE], const uint8_t** out, uint64_t* out_len,
                               lfm_encode_stats* stats);

/* Pipelined encode of a stack (z0 = 0, prev_frame = NULL) or of a z-slab
 * (arguments as lfm_encoder_encode_slab).  An auto request (headerVersion &
 * 0x7F < 8) on a slab with z0 > 0 returns 3: use lfm_encoder_submit_select
 * with the stack's frame 0, or a forced request 8 + k.  Runs the predictor stage (img may
 * be released on return), then hands the GPU bzip2 stage, the .lfm assembly
 * and its payload copies (system DMA engine) to a finisher thread and
 * returns.  The next submit's GPU bzip2 starts once this encode's kernels are
 * done (its selection and predictor stage run before, beside this one).  At
 * most two encodes are in flight: a submit first joins the one before last.
 * *ticket names the encode for lfm_encoder_wait; errors of the finisher are
 * returned by lfm_encoder_wait. */
LFM_API int lfm_encoder_submit(lfm_encoder* enc, const void* img, int img_is_device, const void* prev_frame,
                               uint32_t z0, const uint32_t xyzct[KLB_DATA_DIMS], int dataType, int headerVersion,
                               int Nnum, const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                               const char metadata[KLB_METADATA_SIZE], uint64_t* ticket);
/* lfm_encoder_submit with the frame auto-selection runs on: select_frame
 * (X*Y samples, host or device like img) is the whole stack's frame 0 when img
 * is a z-slab of it (z0 > 0), so every slab selects what the whole-stack
 * encode selects (klb_imageIO.cpp:2316-2360); NULL = img's own frame 0.  An
 * auto request (headerVersion & 0x7F < 8) on a slab with z0 > 0 needs it
 * (returns 3 otherwise).  Selection then runs inside the submit, on the
 * encoder's high-priority stream, after the previous encode's kernels. */
LFM_API int lfm_encoder_submit_select(lfm_encoder* enc, const void* img, int img_is_device, const void* prev_frame,
                                      uint32_t z0, const void* select_frame, const uint32_t xyzct[KLB_DATA_DIMS],
                                      int dataType, int headerVersion, int Nnum,
                                      const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                                      const char metadata[KLB_METADATA_SIZE], uint64_t* ticket);
/* Wait for a submitted encode.  *out stays valid until the second submit
 * after it (or a synchronous encode on this encoder); returns its status.
 * On a nonzero status *out = NULL and *out_len = 0; 8 = the ticket was never
 * submitted on this encoder or its buffer set has been reused since. */
LFM_API int lfm_encoder_wait(lfm_encoder* enc, uint64_t ticket, const uint8_t** out, uint64_t* out_len,
                             lfm_encode_stats* stats);

/* Encode z-slab [z0, z0 + xyzct[2]) of a larger stack (c = t = 1) for
 * multi-GPU sharding: frame z of the slab is temporal when video & (z0 + z)
 * is odd, and the slab's first frame then uses prev_frame (the raw frame
 * z0 - 1, host or device like img).  Use a forced predictor request (8 + k,
 * k selected on the whole stack's frame 0) so every slab codes like the
 * whole stack would; slab depths must be multiples of the block depth except
 * the last.  The result is a valid .lfm of the slab (lfm_merge_slabs joins
 * them).  An auto request (headerVersion & 0x7F < 8) with z0 > 0 returns 3:
 * the slab's own frame 0 is not the stack's, so it cannot select what the
 * whole-stack encode selects. */
LFM_API int lfm_encoder_encode_slab(lfm_encoder* enc, const void* img, int img_is_device, const void* prev_frame,
                                    uint32_t z0, const uint32_t xyzct[KLB_DATA_DIMS], int dataType,
                                    int headerVersion, int Nnum, const uint32_t blockSize[KLB_DATA_DIMS],
                                    int compressionType, const char metadata[KLB_METADATA_SIZE],
                                    const uint8_t** out, uint64_t* out_len, lfm_encode_stats* stats);

/* Join the .lfm files of consecutive z-slabs into the whole stack's .lfm
 * (byte-identical to encoding the stack in one piece).  *out is malloc'ed:
 * release it with lfm_free.  Returns 0, or 3 when the slabs do not fit. */
LFM_API int lfm_merge_slabs(const uint8_t* const* slabs, const uint64_t* lens, int nslabs, uint8_t** out,
                            uint64_t* out_len);
LFM_API void lfm_free(void* p);

/* Multi-process writers (one process per GPU, e.g. torchrun): each rank
 * places its own z-slab .lfm into the whole stack's .lfm buffer `dst`
 * (shared memory), concurrently with the other ranks.  lfm_slab_info gives a
 * slab's payload bytes and block count (the values the ranks exchange);
 * lfm_place_slab copies the slab's payload to payload_offset (payload bytes
 * of the slabs before it), writes its block end offsets re-based into the
 * table at block_index (blocks before it) and, for block_index 0, the fixed
 * header with the stack's depth total_z.  The result equals lfm_merge_slabs. */
LFM_API int lfm_slab_info(const uint8_t* slab, uint64_t len, uint64_t* payload_bytes, uint64_t* nblocks);
LFM_API int lfm_place_slab(const uint8_t* slab, uint64_t slab_len, uint8_t* dst, uint64_t dst_len, uint32_t total_z,
                           uint64_t total_blocks, uint64_t block_index, uint64_t payload_offset, int numThreads);

/* Devices the writers farm block ranges to (klb_imageIO::writeImage,
 * writeKLBstack, writeLFMstack_c, lfm_encoder_encode_multi): n > 0 sets the
 * list (a device may repeat: several workers on one GPU); n = 0 restores the
 * default: env LFM_GPUS = "0,1,.." or a count; else, in a multi-process job,
 * one device when several processes share this node (LOCAL_WORLD_SIZE or
 * OMPI_COMM_WORLD_LOCAL_SIZE > 1, or only WORLD_SIZE > 1 known): LOCAL_RANK
 * (OMPI_COMM_WORLD_LOCAL_RANK) modulo the visible devices, the current device
 * when no local rank is set; else (one process on the node) every visible
 * device.  lfm_get_devices returns the count and fills up to cap entries. */
LFM_API int lfm_set_devices(const int* devices, int n);
LFM_API int lfm_get_devices(int* devices, int cap);
/* The default list above for n_visible devices and current device `current`
 * (no device call; what lfm_get_devices gives after lfm_set_devices(NULL, 0)
 * on such a machine).  Returns the count and fills up to cap entries. */
LFM_API int lfm_default_devices(int n_visible, int current, int* devices, int cap);

/* Encode a HOST stack on the device list above (one host thread per device,
 * block-layer ranges: z-slabs, or ranges of c / t), into the encoder's
 * in-memory .lfm (byte-identical to a one-device encode).  Falls back to the
 * encoder's own device when the list has one device or the stack one range. */
LFM_API int lfm_encoder_encode_multi(lfm_encoder* enc, const void* img, const uint32_t xyzct[KLB_DATA_DIMS],
                                     int dataType, int headerVersion, int Nnum,
                                     const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                                     const char metadata[KLB_METADATA_SIZE], const uint8_t** out, uint64_t* out_len,
                                     lfm_encode_stats* stats);

/* GPU bzip2 of streams that libbzip2 cuts into several bzip2 blocks: blocks
 * above about 900 kB (the level is capped at 9), or blocks whose data grows
 * under bzip2's first run-length stage.  1 (the default; env
 * LFM_BZ2_MULTIBLOCK=0 starts with 0): the device cuts, compresses and joins
 * them.  0: such streams are compressed by the host library, as before this
 * switch existed.  The .lfm bytes are the same either way.  The setter
 * returns the previous value; it applies to encodes started after it. */
LFM_API int lfm_set_bzip2_multiblock(int on);
LFM_API int lfm_get_bzip2_multiblock(void);
/* The reader's side of the same.  1 (the default; env
 * LFM_BUNZIP2_MULTIBLOCK=0 starts with 0): streams of several bzip2 blocks are
 * decoded on the GPU like single-block ones, in every reader that decodes on
 * the GPU (whole images and regions, host and device destinations, one device
 * or several); only streams with a periodic block (see
 * lfm_set_bunzip2_periodic) and malformed ones still go to the host library.
 * 0: every such stream is decoded by the host
 * library, one after the other, as before this switch existed.  The pixels
 * are the same either way; lfm_decode_stats.host_blocks tells the two apart.
 * The setter returns the previous value; it applies to decodes started after
 * it. */
LFM_API int lfm_set_bunzip2_multiblock(int on);
LFM_API int lfm_get_bunzip2_multiblock(void);
/* GPU decode of bzip2 blocks whose text after bzip2's first run-length stage
 * is exactly periodic (w w ... w): in an unpredicted file any 16-bit region of
 * one value whose two bytes differ, a camera offset of 100 for one.  0 (the
 * default; env LFM_BUNZIP2_PERIODIC=1 starts with 1): streams with such a
 * block are decoded by the host library, one after the other, as before this
 * switch existed.  1: they are decoded on the GPU like any other stream, in
 * every reader that decodes on the GPU (whole images and regions, host and
 * device destinations, one device or several).  The pixels are the same
 * either way; lfm_decode_stats.host_blocks tells the two apart.  The setter
 * returns the previous value; it applies to decodes started after it.
 * (lfm_hip_bunzip2_set_periodic, lfm_hip.h, is the same switch.) */
LFM_API int lfm_set_bunzip2_periodic(int on);
LFM_API int lfm_get_bunzip2_periodic(void);
/* How the bzip2 streams (one per 5-D block) of the last encode were compressed
 * that lfm_encoder_encode, lfm_encoder_encode_slab or lfm_encoder_wait
 * completed on this encoder: all streams, those the host library compressed,
 * and the bzip2 blocks the GPU produced (a stream may hold several).  Without
 * a GPU host_streams == streams.  lfm_encoder_encode_multi encodes on other
 * encoders: after it all three are 0.  Any pointer may be NULL. */
LFM_API int lfm_encoder_stream_counts(lfm_encoder* enc, uint64_t* streams, uint64_t* host_streams,
                                      uint64_t* bzip2_blocks);

/* Free the device / pinned buffers the writers keep between calls. */
LFM_API void lfm_release_encoders(void);

/* Decode an in-memory .lfm into `img` (host, getImageSizeBytes bytes). */
LFM_API int lfm_decode_memory(const uint8_t* buf, uint64_t len, void* img, int numThreads);
/* Decode the region lb .. ub (inclusive, xyzct) of an in-memory .lfm into
 * `out` (host, x fastest, out_bytes long): readKLBroiInPlace on memory.
 * Only the blocks the region depends on are decoded.  Returns 3 when the
 * region lies outside the image or out_bytes is less than the region's
 * pixels times the file's bytes per pixel (the header's data type). */
LFM_API int lfm_decode_memory_roi(const uint8_t* buf, uint64_t len, const uint32_t lb[KLB_DATA_DIMS],
                                  const uint32_t ub[KLB_DATA_DIMS], void* out, uint64_t out_bytes, int numThreads);

/* What a device-destination decode did (the two functions below). */
typedef struct lfm_decode_stats {
    double   total_ms;
    int      path;         /* 0: pipelined GPU decode wrote the caller's buffer; 1: host decode + upload */
    uint32_t chunks;       /* pipeline chunks (0 on path 1) */
    uint64_t blocks;       /* streams decoded */
    uint64_t host_blocks;  /* of them handed to the host library (all of them on path 1) */
    uint64_t d2h_bytes;    /* image bytes copied device -> host during the call */
    uint64_t staged_bytes; /* device sub-image the region read decoded before cropping (0: exact / whole) */
} lfm_decode_stats;

/* lfm_decode_memory / lfm_decode_memory_roi into DEVICE memory: d_img / d_out
 * is a device pointer (hipMalloc, a torch CUDA tensor's data_ptr) of at least
 * the image's / region's bytes in the file's data type, x fastest.  The
 * decode runs on the buffer's device (found with hipPointerGetAttributes; the
 * caller's current device is restored) and no image byte goes through host
 * memory: the inverse predictor, or for unpredicted files the block scatter,
 * writes the buffer, and a region that is not exactly a box of blocks is
 * cropped on the device from a sub-image the library keeps there.
 * Ordering: the library's first write to the buffer comes after all work
 * queued on the device's null stream when the call is made (a producer on
 * another stream must be synchronised by the caller); when the call returns
 * 0, all library work on the buffer is complete and host-synchronised, so any
 * stream may read it.  When it returns non-zero the buffer's contents are
 * unspecified.
 * Files the pipelined GPU decode does not take (compression NONE / ZLIB,
 * Nnum > 31, non-contiguous block offsets, blocks more than one channel or
 * time point deep, LFM_GPU_DECODE=0 or
 * LFM_GPU_BUNZIP2=0, device memory exhausted) are decoded on the host as
 * lfm_decode_memory does into a temporary and uploaded with one copy:
 * stats->path = 1.
 * Return codes as the host functions', and 3 for a host or unregistered
 * pointer or a buffer smaller than the image / region.  stats may be NULL. */
LFM_API int lfm_decode_memory_device(const uint8_t* buf, uint64_t len, void* d_img, uint64_t d_img_bytes,
                                     int numThreads, lfm_decode_stats* stats);
LFM_API int lfm_decode_memory_roi_device(const uint8_t* buf, uint64_t len, const uint32_t lb[KLB_DATA_DIMS],
                                         const uint32_t ub[KLB_DATA_DIMS], void* d_out, uint64_t out_bytes,
                                         int numThreads, lfm_decode_stats* stats);

/* Devices the whole-image readers farm block-layer ranges to, one host
 * thread per entry (a device may repeat: several workers on one GPU).  The
 * list is opt-in: n > 0 sets it, n = 0 restores the default, which is env
 * LFM_DECODE_GPUS = "0,1,.." or a count (the syntax of LFM_GPUS) and empty
 * without it.  With fewer than two entries every reader runs on the current
 * device exactly as before.  With two or more, lfm_decode_memory,
 * readLFMstack_c, readKLBstack, readKLBstackInPlace and
 * klb_imageIO::readImageFull decode as lfm_decode_memory_multi does; region
 * reads are never farmed.  lfm_get_decode_devices returns the count and fills
 * up to cap entries. */
LFM_API int lfm_set_decode_devices(const int* devices, int n);
LFM_API int lfm_get_decode_devices(int* devices, int cap);
/* The env parse alone, for n_visible devices (no device call). */
LFM_API int lfm_default_decode_devices(int n_visible, int* devices, int cap);
/* End the readers' kept worker threads: the device and pinned buffers they
 * hold between calls are freed (the next farmed decode starts them again).
 * lfm_release_encoders is about the writers only. */
LFM_API void lfm_release_decoders(void);

/* One shard of a farmed decode: indices [first, first + count) along the
 * shard axis, decoded on `device` with status rc. */
typedef struct lfm_decode_shard {
    uint32_t first, count;   /* along the axis */
    int device;              /* -1: no device (a host decode on a GPU-less machine) */
    int rc;
    lfm_decode_stats stats;  /* this shard's */
} lfm_decode_shard;

typedef struct lfm_decode_multi_stats {
    double total_ms;
    int axis;                /* 2 / 3 / 4: the shards are ranges of z / c / t */
    int workers;             /* shards decoded side by side; 1 = not farmed */
    uint64_t blocks, host_blocks, d2h_bytes;   /* summed over the shards */
} lfm_decode_multi_stats;

/* How a file is cut for nworkers readers: the writers' split.  The axis is t
 * when xyzct[4] > 1, else c when xyzct[3] > 1, else z; a shard is a range of
 * whole block layers along it (on the z axis of a predicted video file with an
 * odd block depth, of pairs of layers, so every shard starts at an even z):
 * per = ceil(layers / nworkers) layers each, ceil(layers / per) shards.
 * Fills *axis and up to cap entries of first / count (each may be NULL) and
 * returns the shard count (>= 1; asking for that many workers gives the same
 * shards again), or 0 on a bad header. */
LFM_API int lfm_decode_shard_plan(const uint8_t* buf, uint64_t len, int nworkers, int* axis, uint32_t* first,
                                  uint32_t* count, int cap);

/* lfm_decode_memory with one worker per entry of the decode device list:
 * shard w of lfm_decode_shard_plan(.., list length, ..) is decoded by its own
 * host thread (numThreads / shards host threads each, at least 1) on device
 * list[w], straight into its slice of img; no data crosses between devices and
 * no block is decoded twice.  One plain decode on the current device instead
 * (stats->workers = 1) when the list has fewer than two entries, the file is
 * one shard, or the pipelined GPU decode does not take it (compression NONE /
 * ZLIB, Nnum > 31, non-contiguous block offsets, LFM_GPU_DECODE=0 or
 * LFM_GPU_BUNZIP2=0, no GPU).  Returns the first non-zero shard status in
 * shard order, after every worker has finished.  The workers keep their
 * device buffers between calls (lfm_release_decoders).  stats and shards may
 * be NULL; up to shard_cap shards are filled. */
LFM_API int lfm_decode_memory_multi(const uint8_t* buf, uint64_t len, void* img, int numThreads,
                                    lfm_decode_multi_stats* stats, lfm_decode_shard* shards, int shard_cap);

/* The same into DEVICE memory, one buffer per shard: d_out[w] (out_bytes[w]
 * bytes) takes shard w of lfm_decode_shard_plan(.., nshards, ..), x fastest.
 * nshards must be the count that plan returns for nshards workers; anything
 * else returns 3.  Each shard runs on its buffer's device, found as
 * lfm_decode_memory_device finds it (the decode device list is not used), and
 * that function's ordering and failure rules hold per buffer. */
LFM_API int lfm_decode_memory_multi_device(const uint8_t* buf, uint64_t len, void* const* d_out,
                                           const uint64_t* out_bytes, int nshards, int numThreads,
                                           lfm_decode_multi_stats* stats, lfm_decode_shard* shards, int shard_cap);

/* ---- stream writer: one .lfm file from block layers that arrive over time ----
 * The stream axis is the writers' shard axis: t when xyzct[4] > 1, else c
 * when xyzct[3] > 1, else z (lfm_writer_axis: 4, 3 or 2).  xyzct[axis] at open
 * is the CAPACITY: the most indices that may be appended.  The other
 * arguments are lfm_encoder_encode's (headerVersion = predictor request |
 * video << 7) and writeLFMstack_c's (pixelSize, metadata; NULL = defaults).
 *
 * lfm_writer_append takes count >= 1 consecutive indices along the axis (host
 * memory, or device memory on the writer's device; x fastest; any count).
 * The writer encodes whole block layers, blockSize[axis] indices each, on an
 * encoder of its own on `device` (< 0: the current one), pipelined like
 * lfm_encoder_submit, two encodes in flight; every full layer one append
 * completes goes into one encode.  Fewer than one layer is held back, in
 * memory of the input's kind (stats.staged_peak_bytes); an append that starts
 * and ends on a layer boundary is encoded from the caller's memory without a
 * copy.  When append returns, the library has finished reading img; the
 * compressed bytes may reach the file later, and an error of a background
 * encode is returned by the next append or by close.  A device input is read
 * after the work queued on the device's null stream, as lfm_encoder_submit
 * reads its input.  The predictor is selected once, on frame 0 of the first
 * append, and forced for every encode; the bzip2 level is the level of the
 * stack's nominal block.  Returns 3 and takes nothing: count 0, an append
 * past the capacity, host and device appends mixed in one writer.  After any
 * other non-zero return the writer is failed: every later call returns that
 * code and close removes the file.
 *
 * File: the fixed header and a zero offset table sized for the capacity are
 * written at open, the payload follows in block order, and close writes the
 * table and the final xyzct[axis].  When fewer indices than the capacity were
 * appended the final table is shorter by 8 * (Nb_capacity - Nb_final) bytes:
 * close moves the payload down by that much (a forward chunked copy,
 * stats.moved_bytes) and truncates the file.  After close the file is
 * byte-identical to what writeLFMstack_c / lfm_encoder_encode produce for the
 * appended stack with the same arguments and xyzct[axis] = what was appended
 * (a final extent below blockSize[axis] included: that single layer is
 * encoded at close, with the block and the bzip2 level the one-shot writer
 * would clamp to).
 *
 * Checkpoints: whenever an encode of whole layers has finished and its payload
 * is in the file, the writer also writes that range's entries into the
 * capacity-sized table (payload first, then the entries; the first time also
 * the chosen header byte at offset 0).  A file that was never closed is still
 * NOT a valid .lfm -- its header says xyzct[axis] = capacity, its table ends in
 * zeros, and lfm_reader_open refuses it with 2 -- but its complete layers are
 * not lost: see lfm_recover, and lfm_reader_open_live to read them while the
 * writer runs.
 * lfm_writer_flush waits until every whole layer appended so far is encoded and
 * its payload and table entries are in the file (both in-flight encodes are
 * joined; the part of a layer the writer holds back stays in memory and is NOT
 * covered).  sync != 0: fdatasync after that.  *committed (may be NULL) =
 * indices along the stream axis a recovery would now keep.  A failed writer
 * returns its code.
 * lfm_writer_close finalises and frees the writer whatever it returns; a
 * close with nothing appended returns 3 and removes the file.
 * lfm_writer_abort frees the writer and removes the file.  One writer is
 * used by one thread at a time. */
typedef struct lfm_writer lfm_writer;
typedef struct lfm_writer_stats {
    uint64_t appended;       /* indices along the stream axis taken so far            */
    uint64_t ranges;         /* encodes run                                           */
    uint64_t streams, host_streams, bzip2_blocks;   /* summed over the ranges         */
    uint64_t bytes_written;  /* final file size (after close)                         */
    uint64_t moved_bytes;    /* payload bytes moved at close (0 when capacity reached) */
    uint64_t staged_peak_bytes; /* most input bytes the writer held back at one time  */
    int chosen, header_version; float entropy[8];
    double total_ms;         /* wall clock spent inside append, flush and close       */
    uint64_t committed;      /* indices a recovery would keep (at close: appended); last: the
                                fields before it lie where they lay before it existed  */
} lfm_writer_stats;

LFM_API int lfm_writer_open(lfm_writer** w, const char* filename, const uint32_t xyzct[KLB_DATA_DIMS], int dataType,
                            int headerVersion, int Nnum, const float pixelSize[KLB_DATA_DIMS],
                            const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                            const char metadata[KLB_METADATA_SIZE], int device, int numThreads);
LFM_API int lfm_writer_axis(const lfm_writer* w);   /* 4, 3 or 2 */
LFM_API int lfm_writer_append(lfm_writer* w, const void* img, int img_is_device, uint32_t count);
LFM_API int lfm_writer_flush(lfm_writer* w, int sync, uint64_t* committed);
LFM_API int lfm_writer_close(lfm_writer* w, lfm_writer_stats* stats);   /* finalises and frees */
LFM_API void lfm_writer_abort(lfm_writer* w);                           /* frees, removes the file */

/* ---- recovery: the .lfm of the complete layers of a file that was never closed ----
 * Turns a file its writer never closed (a crash, a kill, a power loss) into
 * the .lfm of its complete layers.  out_filename NULL: in place -- NOT atomic:
 * an in-place recovery that is itself interrupted (while the payload moves
 * down over the unused table entries, or before the truncate) can leave the
 * file beyond repair, so recover into out_filename when the data matters and
 * the space is there.  Else the input is only read and the result is written
 * to out_filename.
 * Committed prefix: the longest run of leading table entries that are
 * non-zero, strictly increasing and end at or below the file's payload bytes
 * (the payload starts behind the capacity-sized table), floored to whole
 * layers along the stream axis.
 * verify != 0: every stream of the committed layers is decoded, one layer at a
 * time (memory is bounded by a layer): bzip2 streams are checked against their
 * CRCs and the block's byte count, on the GPU decoder when a device is visible
 * (with lfm_set_bunzip2_multiblock / lfm_set_bunzip2_periodic as set; streams
 * the device hands back, and all of them without a device, go through the host
 * library: stats.host_streams), ZLIB streams are inflated, and of NONE only the
 * stored size can be checked.  The longest prefix of layers whose streams all
 * pass is kept.  No inverse predictor runs: the file does not record the
 * predictor family, and verification does not depend on lfm_set_family.
 * verify == 0 trusts the table: safe after a process crash (the page cache
 * survived), not after a power loss, where entries can reach the disk before
 * their payload.
 * The result is finalised as lfm_writer_close finalises (the same code) and is
 * byte-identical to what the one-shot writer produces for the first
 * stats.kept indices with the same arguments.
 * Returns 0 on success -- also for a file that already is a closed .lfm:
 * stats.already_valid = 1, nothing is done and no output is written; 2 when
 * the file cannot be opened or is shorter than its table; 3 when no complete
 * layer survives (the input is untouched, no output is created); 5 on write
 * errors.  stats may be NULL. */
typedef struct lfm_recover_stats {
    int axis, header_version, already_valid;   /* already_valid: the file was a closed .lfm, nothing done */
    uint64_t capacity, kept;                   /* indices along the axis: at open / in the result */
    uint64_t committed_blocks;                 /* leading table entries that are plausible (above) */
    uint64_t dropped_layers;                   /* committed layers not kept (torn, or failed verification) */
    uint64_t verified_streams, host_streams;   /* streams decoded for verification; of them by the host library */
    uint64_t bytes_written, moved_bytes;
    double total_ms;
} lfm_recover_stats;
LFM_API int lfm_recover(const char* filename, const char* out_filename, int verify, int numThreads,
                        lfm_recover_stats* stats);

/* ---- ranged reader: region reads that fetch only the bytes they need ----
 * lfm_reader_open reads the fixed header and the offset table, nothing else
 * (2: the file cannot be opened, is truncated, or its table points past its
 * end -- a file its writer never closed: see lfm_recover and
 * lfm_reader_open_live).  lfm_reader_read decodes the region
 * lb .. ub (inclusive, xyzct) as lfm_decode_memory_roi (out_is_device == 0)
 * or lfm_decode_memory_roi_device (!= 0) do -- the same blocks, return codes,
 * device ordering and lfm_decode_stats (stats may be NULL) -- but the streams
 * of those blocks are read from the file: one pread per run of blocks that
 * lie one after the other in it, no byte between the runs.  The blocks are
 * the ones the region depends on: with a predictor the corner up and left of
 * the region in its frames, plus the frame before an odd z of a video stack.
 * A region equal to the whole image is allowed.  lfm_reader_bytes_read is the
 * cumulative count of bytes read from the file, header and table included.
 * One reader is used by one thread at a time.
 *
 * Live reader.  lfm_reader_open_live also takes a file its writer has not
 * closed (on a closed file it is lfm_reader_open).  The reader then shows the
 * committed whole layers, found by lfm_recover's rule: lfm_reader_info reports
 * xyzct[axis] as that extent, which may be 0; a region past it returns 3, and
 * inside it lfm_reader_read works as on a closed file, host and device
 * destinations alike (the same blocks, lfm_decode_stats and bytes_read
 * accounting; the payload starts behind the capacity-sized table).
 * lfm_reader_refresh re-reads the fixed header and the table entries not yet
 * accepted (one pread each, both counted in bytes_read) and gives the extent
 * now readable.  If the writer has closed the file meanwhile (the header's
 * extent differs from the capacity, or the table is complete) the reader
 * re-parses it as a closed file; on a closed file refresh only reports the
 * extent.  A reader MUST refresh after the writer's close before it reads
 * again, and reads that overlap the close (its payload move) are unsupported;
 * after a refresh that returns non-zero (2: the file could not be read as
 * either) the reader is good for lfm_reader_close only.
 * A stream that is bad although its entry is plausible (entries that reached
 * the disk before their payload) surfaces as return code 2 through the bzip2
 * CRC, never as wrong pixels; files of compression NONE carry no checksum and
 * lack this guarantee.  One reader is used by one thread; a writer and a
 * reader of the same file may live in different threads or processes. */
typedef struct lfm_reader lfm_reader;
LFM_API int lfm_reader_open(lfm_reader** r, const char* filename);        /* header + table only */
LFM_API int lfm_reader_open_live(lfm_reader** r, const char* filename);
LFM_API int lfm_reader_refresh(lfm_reader* r, uint32_t* extent);
LFM_API int lfm_reader_info(const lfm_reader* r, uint32_t xyzct[KLB_DATA_DIMS], int* dataType,
                            uint32_t blockSize[KLB_DATA_DIMS], uint8_t* headerVersion, uint8_t* Nnum,
                            uint64_t* file_bytes);
LFM_API int lfm_reader_read(lfm_reader* r, const uint32_t lb[KLB_DATA_DIMS], const uint32_t ub[KLB_DATA_DIMS],
                            void* out, uint64_t out_bytes, int out_is_device, int numThreads,
                            lfm_decode_stats* stats);
LFM_API uint64_t lfm_reader_bytes_read(const lfm_reader* r);              /* cumulative, header + table included */
LFM_API void lfm_reader_close(lfm_reader* r);

#ifdef __cplusplus
}
#endif
#endif
