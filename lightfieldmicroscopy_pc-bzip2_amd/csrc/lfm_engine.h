// lfm_engine.h -- encode / decode engine behind klb_imageIO, the C ABI and
// the lfm_encoder API.
#pragma once
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
#include "klb_imageHeader.h"
#include "lfm_api.h"
#include "lfm_buffers.h"
#include "lfm_transfer.h"

namespace lfm {

// error codes beyond the reference's 2 / 3 / 5
constexpr int kErrBadPredictor = 6;
constexpr int kErrNoGpu = 7;
constexpr int kErrUnknownTicket = 8;  // lfm_encoder_wait: ticket never submitted or already recycled

bool gpu_bzip2_enabled();   // env LFM_GPU_BZIP2 (default on)
bool gpu_decode_enabled();  // env LFM_GPU_DECODE (default on): inverse predictor on the GPU
bool gpu_bunzip2_enabled(); // env LFM_GPU_BUNZIP2 (default on): bzip2 decode on the GPU
int default_threads();      // env LFM_NUM_THREADS, else OMP_NUM_THREADS, else hardware_concurrency
int current_family();       // lfm_set_family / env LFM_PREDICTOR_WAY / LFM_PREDICTOR_WAY
void set_family(int fam);

// x-fastest decomposition of the 5-D image into blocks (klb_imageIO.cpp:98-160)
struct BlockGrid {
    uint64_t dims[5], bs[5], nb[5], stride[5], nblocks;
    explicit BlockGrid(const klb_image_header& h);
    void block(uint64_t id, uint64_t origin[5], uint64_t size[5]) const;
};
void gather_block(const uint8_t* img, const BlockGrid& g, uint64_t id, size_t bpp, uint8_t* dst, size_t* nbytes);
void scatter_block(const uint8_t* blk, const BlockGrid& g, uint64_t id, size_t bpp, uint8_t* img);

// output of an encode: a file (reference writer order: header, blocks, then
// the offset table rewritten) or a memory buffer
class Sink {
public:
    virtual ~Sink() = default;
    virtual int begin(const klb_image_header& h) = 0;
    virtual int append(const uint8_t* p, size_t n) = 0;
    virtual int finish(const klb_image_header& h) = 0;
    // sinks backed by pinned host memory hand out the next n bytes of the
    // output so a device buffer can be copied straight into place
    virtual bool direct_capable() const { return false; }
    virtual uint8_t* direct(size_t) { return nullptr; }
    virtual void reserve_hint(size_t) {}
};

// growable pinned host buffer (the in-memory .lfm): device-to-host copies land
// in it at full DMA speed, and it is kept between encodes
class PinnedBuffer {
public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer();
    bool reserve(size_t n);
    bool resize(size_t n);
    void clear() { size_ = 0; }
    uint8_t* data() { return p_; }
    const uint8_t* data() const { return p_; }
    size_t size() const { return size_; }
    size_t capacity() const { return cap_; }
private:
    uint8_t* p_ = nullptr;
    size_t size_ = 0, cap_ = 0;
    bool malloced_ = false;
};
class FileSink : public Sink {
public:
    explicit FileSink(FILE* f) : f_(f) {}
    int begin(const klb_image_header& h) override;
    int append(const uint8_t* p, size_t n) override;
    int finish(const klb_image_header& h) override;
private:
    FILE* f_;
    std::vector<char> vbuf_;
};
class MemSink : public Sink {
public:
    explicit MemSink(PinnedBuffer* out) : out_(out) {}
    int begin(const klb_image_header& h) override;
    int append(const uint8_t* p, size_t n) override;
    int finish(const klb_image_header& h) override;
    bool direct_capable() const override { return true; }
    uint8_t* direct(size_t n) override;
    // n is the worst case (every block stored at its raw size + bzip2's
    // overhead); beyond 8 GiB only 60 % of it is pinned up front (ratio >= 1.67
    // fits): a 100-volume config-5 stack (107 GB raw, 52 GB .lfm) would
    // otherwise pin 110 GB of host memory for its output.  A stack that
    // compresses worse grows the buffer once, straight to the worst case
    // (direct()): the peak is the old buffer plus n, 1.6 n; if n cannot be
    // pinned, the buffer grows by half its capacity at a time instead (first
    // step: 0.6 n + 0.9 n = 1.5 n).
    void reserve_hint(size_t n) override
    {
        const size_t big = (size_t)8 << 30;
        worst_ = n;
        (void)out_->reserve(n <= big ? n : std::max(big, n / 10 * 6));
    }
private:
    PinnedBuffer* out_;
    size_t worst_ = 0;
};

// Compress every block of `sym` (image layout, bpp bytes per pixel) in
// parallel and hand them to the sink in block order.  `h` must already hold
// the clamped block size; its blockOffset table is filled.
int compress_blocks(const uint8_t* sym, klb_image_header& h, Sink& sink, int threads, int level = -1);

// z-slab [z0, z0 + xyzct[2]) of a larger stack (c = t = 1): the temporal
// flag of frame z is video & (z0 + z), and the first frame's previous raw
// frame is `prev` (host or device like the image) when z0 is odd.
// level >= 1 overrides the bzip2 level rule (min(9, ceil(nominal block
// bytes / 1e5)), klb_imageIO.cpp:108): a range of a larger stack codes at the
// level of the whole stack's nominal block even when its own last block layer
// is shallower.
// select_frame: the frame auto-selection runs on (host or device like the
// image) instead of the image's own frame 0 -- the whole stack's frame 0 when
// this encode is a slab of it (klb_imageIO.cpp:2316-2360 selects on frame 0).
struct SlabSpec {
    uint32_t z0 = 0;
    const void* prev = nullptr;
    int level = -1;
    const void* select_frame = nullptr;
};

// clamp the block size to the dims and check the types (klb_imageIO.cpp:2402-2404)
int normalize_header(klb_image_header& h);
// bzip2 level of the reference's rule for the header's nominal block
int bzip2_level(const klb_image_header& h);
// GPU bzip2 of streams that libbzip2 cuts into several blocks (1, the default;
// env LFM_BZ2_MULTIBLOCK) or their hand-back to the host library (0); the
// setter returns the previous value
int bzip2_multiblock();
int set_bzip2_multiblock(int on);
// the reader's side of the same: GPU decode of streams of several bzip2 blocks
// (1, the default; env LFM_BUNZIP2_MULTIBLOCK) or their decode by the host
// library (0); read once by every decode as it starts, the setter returns the
// previous value
int bunzip2_multiblock();
int set_bunzip2_multiblock(int on);
// multi-threaded memcpy (1 MiB pieces)
void par_memcpy(void* dst, const void* src, size_t n, int threads);

// Encoder: GPU predictor stage + block compression.  One per device; keeps
// device / pinned buffers between calls.
class Encoder {
public:
    explicit Encoder(int device);
    ~Encoder();
    // img: host pointer (dev=false) or device pointer on this encoder's device
    int encode(const void* img, bool dev, klb_image_header& h, Sink& sink, lfm_encode_stats* st, int threads,
               const SlabSpec* slab = nullptr);
    PinnedBuffer mem_out;
    int device() const { return device_; }
    // Pipelined encodes (lfm_encoder_submit / lfm_encoder_wait), two buffer
    // sets (symbols, bzip2 slots and workspaces, pinned output) used in turn:
    // submit runs the predictor stage of its stack into one set and hands the
    // GPU bzip2 + in-order assembly + payload copies to a finisher thread.
    // The next submit's GPU bzip2 starts once the previous encode's kernels
    // are done, so the next stack's kernels overlap its assembly and payload
    // copies (releasing it after its BWT or its MTF, so they also overlap its
    // latency-bound tail, measured 8 943 / 9 035 vs 9 098 Mpixel/s: the heap
    // chains slow down as much as the head gains).  At most two encodes are
    // in flight.  The input may be released when submit returns (the
    // predictor stage has consumed it).
    int submit(const void* img, bool dev, klb_image_header& h, int threads, const SlabSpec* slab, uint64_t* ticket);
    // wait for a submitted encode: its .lfm is *out (valid until the second
    // submit after it); stats as encode() reports them, d2h_ms including the
    // deferred copies
    int wait(uint64_t ticket, const PinnedBuffer** out, lfm_encode_stats* st);
    PinnedBuffer mem_ring[2];
    // bzip2 streams of the last encode that encode() or wait() completed
    // (lfm_encoder_stream_counts): all of them, those the host library
    // compressed, and the bzip2 blocks the GPU produced
    struct StreamCounts {
        uint64_t streams = 0, host_streams = 0, bzip2_blocks = 0;
    };
    StreamCounts last_counts;
    // predictor selection on one host frame (uploaded to this encoder's device)
    int select_host_frame(const void* frame, int W, int H, int T, int family, int* chosen, float entropy[8]);
    // predictor selection on one frame of h's x / y size, host or device
    // (a device frame is read after the null stream's queued work, as submit
    // reads its input): the stream writer selects once, on its first frame
    int select_frame(const void* frame, bool dev, const klb_image_header& h, int* chosen, float entropy[8]);

private:
    // an encode in flight (submit): its finisher thread and the release point
    struct Inflight {
        uint64_t ticket = 0;  // 0: none
        std::thread th;       // GPU bzip2, in-order assembly, payload copies
        int rc = 0;
        lfm_encode_stats st{};
        std::mutex mu;
        std::condition_variable cv;
        int reached = 0;      // batches of the last round past the release stage
        int need = 0;         // ... needed to release the next submit (0: not yet known)
        bool released = true;
        int reached2 = 0;     // batches of the last round past the MTF stage (stage 2)
        bool mtf_done = true; // every last-round batch is past stage 2 (or released)
        void release();
        void wait_release();
        void reach();         // one last-round batch passed the release stage
        void reach2();        // one last-round batch passed its MTF stage
        void wait_mtf();
    };
    // Host stacks for the GPU bzip2 path go up in chunks of whole frames on
    // up_stream_ (one uploader thread per encode), each chunk predicted on
    // stream_ as soon as it has landed; the GPU bzip2 batches wait (event)
    // only for the chunks that hold their blocks, so the PCIe upload overlaps
    // the compression of the layers already predicted.  Chunks pass through a
    // ring of device slots (LFM_H2D_RING_MB), so the stack's size is not
    // bounded by it.  LFM_H2D_PIPE=0: the whole volume is uploaded first.
    struct UploadPipe {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        std::vector<hipEvent_t> ev;  // pool: 2 per chunk (predict start / end), kept between encodes
        std::vector<uint64_t> end;   // per chunk: flattened frame index (v * Z + z) past its last frame
        size_t nchunks = 0, recorded = 0;  // chunks whose "predicted" event is recorded
        int rc = 0;
        bool active = false;
        double h2d_ms = 0.0, predict_ms = 0.0;
        // SDMA copies (HSA async copies, not a blit kernel beside the GPU
        // bzip2): completion signals and, for pageable sources, two pinned
        // staging chunks; kept between encodes
        SdmaPair sdma;
        HostBuffer stage[2];
        // make `st` wait until frames [0, f_end) are predicted (0 or 3)
        int wait_frames(uint64_t f_end, hipStream_t st);
        void join();
    };
    int start_upload(const void* img, klb_image_header& h, const SlabSpec& slab, int k, int set);
    bool upload_pipe_ok(bool dev, const klb_image_header& h) const;
    int predictor_stage(const void* img, bool dev, klb_image_header& h, const uint8_t** sym, const uint8_t** dsym,
                        lfm_encode_stats* st, const SlabSpec& slab, int set);
    int gpu_compress(const uint8_t* d_sym, klb_image_header& h, Sink& sink, lfm_encode_stats* st, int level, int set,
                     Inflight* fly);
    int encode_set(const void* img, bool dev, klb_image_header& h, Sink& sink, lfm_encode_stats* st, int threads,
                   const SlabSpec* slab, int set);
    int preselect(const void* img, bool dev, const klb_image_header& h, const SlabSpec& slab, int* k, float ent[8]);
    int ensure_gpu();
    int after_caller(bool dev);
    void join_inflight();
    Inflight fly_[2];                         // by buffer set
    StreamCounts counts_[2];                  // by buffer set: what its last encode compressed
    UploadPipe up_[2];                        // by buffer set
    hipStream_t up_stream_ = nullptr;         // host -> device chunk copies
    uint64_t next_ticket_ = 1;
    int par_ = 0;                             // buffer set of the next submit
    hipStream_t copy_stream_ = nullptr;       // payload copies the SDMA path cannot take
    int device_;
    bool gpu_ready_ = false;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    hipEvent_t caller_ev_ = nullptr;          // the null stream's work before a device input
    DeviceBuffer d_in_;
    DeviceBuffer d_sym_[2];  // by buffer set
    DeviceBuffer d_ws_;
    DeviceBuffer d_prev_;
    DeviceBuffer d_sel_;     // host select_frame uploaded
    // GPU bzip2 pipeline slots (stream, workspace, device + pinned output),
    // kBzSlots per buffer set (LFM_BZ2_SLOTS picks how many run, at most that)
    static constexpr int kBzSlots = 4;
    struct BzSlot {
        hipStream_t stream = nullptr;
        DeviceBuffer d_ws, d_out;
        HostBuffer h_out;
    };
    BzSlot bz_[2][kBzSlots];
    static int bz_slot_count();  // slots that run (env LFM_BZ2_SLOTS, default 2)
    HostBuffer h_sym_[2];  // pinned, by buffer set
};

// process-wide encoders for the C ABI / klb_imageIO, one per (device, worker
// slot), kept between calls; `lock` holds the entry while it is used
Encoder& shared_encoder(std::unique_lock<std::mutex>& lock);
Encoder& pooled_encoder(int dev, int slot, std::unique_lock<std::mutex>& lock);
void release_pooled_encoders();

// devices the writer farms block ranges to: lfm_set_devices, else env
// LFM_GPUS ("0,1,2" or a count), else the current device when the process is one
// rank of a one-process-per-GPU job (WORLD_SIZE / LOCAL_WORLD_SIZE > 1), else
// every visible device
std::vector<int> encode_devices();
// the default device list for n visible devices, `current` the caller's device (-1: unknown)
std::vector<int> default_devices(int n, int current);
void set_encode_devices(const std::vector<int>& devs);

// Multi-GPU writer (lfm_multigpu.cpp): host image, block-layer ranges farmed
// to `devs` (one host thread each), selection once on frame 0, in-order
// append to `sink`.  Returns -1 when the image does not split into two or
// more ranges (the caller then encodes on one device).
int encode_multi(const void* img, klb_image_header& h, Sink& sink, lfm_encode_stats* st, int threads,
                 const std::vector<int>& devs);

// Assemble one .lfm from the .lfm files of consecutive z-slabs of a stack
// (each encoded with the same forced predictor, slab i starting at the sum of
// the previous depths, depths multiples of the block depth except the last):
// the blocks of a slab are a contiguous id range of the whole stack's blocks,
// so the payloads concatenate and the offset table is re-accumulated.
int merge_slabs(const uint8_t* const* slabs, const uint64_t* lens, int n, std::vector<uint8_t>* out);

// A decode whose destination is device memory (lfm_decode_memory_device,
// lfm_decode_memory_roi_device): `img` / `out` of decode_payload / decode_roi
// is then a device pointer on the current device.  The pipelined GPU decode
// writes it directly (the inverse predictor's output, or the block scatter of
// an unpredicted file): no second device image, no prefault thread, no pinned
// download staging, no device -> host copy of image bytes.  Every library
// stream waits for `after_caller` (recorded on the null stream when the call
// came in) before its first write; on a successful return all library work on
// the buffer is complete and host-synchronised.  On failure the buffer's
// contents are unspecified.  Files the pipelined decode does not take are
// decoded on the host as ever into a temporary and uploaded with one copy
// (stats.path = 1).
struct DeviceDest {
    lfm_decode_stats stats{};
    hipEvent_t after_caller = nullptr;
};

// Decode the payload of a .lfm (bytes after the header) into img (host memory,
// or device memory when dd is given).  hstats (optional, host destination):
// what the decode did, as dd->stats reports it for a device destination
// (path 1: the host reader); total_ms and staged_bytes are the caller's.
int decode_payload(const uint8_t* payload, size_t len, const klb_image_header& h, uint8_t* img, int threads,
                   int family, DeviceDest* dd = nullptr, lfm_decode_stats* hstats = nullptr);
int decode_file(const char* filename, klb_image_header& h, std::vector<uint8_t>* img_out, uint8_t* img_into,
                int threads);
// ROI read: only the blocks the ROI depends on are decoded (lb / ub inclusive).
// With dd, `out` is device memory: an exact region decodes straight into it,
// any other decodes its sub-image into a kept device buffer and
// lfm_hip_crop_region writes `out` (stats.staged_bytes = that sub-image).
int decode_roi(const uint8_t* payload, size_t len, const klb_image_header& h, const uint32_t lb[5],
               const uint32_t ub[5], uint8_t* out, int threads, int family, DeviceDest* dd = nullptr,
               lfm_decode_stats* hstats = nullptr);
// Where a region read takes the streams of its blocks from: the payload in
// memory (`mem`, the bytes after the header), or a file it is fetched from by
// byte range (`fd`, the payload starting at file offset `base`): one pread per
// run of blocks that lie one after the other, nothing between the runs.  The
// block list, the sub-header and the decode are the same for both.
struct PayloadSource {
    const uint8_t* mem = nullptr;
    int fd = -1;
    uint64_t base = 0;
    uint64_t len = 0;              // payload bytes
    uint64_t* fetched = nullptr;   // file source: the bytes read are added here
};
int decode_roi(const PayloadSource& src, const klb_image_header& h, const uint32_t lb[5], const uint32_t ub[5],
               uint8_t* out, int threads, int family, DeviceDest* dd = nullptr, lfm_decode_stats* hstats = nullptr);
// The two device-destination readers behind the C ABI: find the buffer's
// device (3 for a host or unregistered pointer), run the decode there with the
// ordering of DeviceDest and restore the caller's current device.
int decode_memory_device(const uint8_t* buf, uint64_t len, const uint32_t* lb, const uint32_t* ub, void* d_out,
                         uint64_t out_bytes, int threads, lfm_decode_stats* stats);
// the same for a parsed header and a payload source (a file source reads a region: lb / ub given)
int decode_source_device(const PayloadSource& src, const klb_image_header& h, const uint32_t* lb, const uint32_t* ub,
                         void* d_out, uint64_t out_bytes, int threads, lfm_decode_stats* stats);
int decode_file_roi(const char* filename, klb_image_header& h, const uint32_t lb[5], const uint32_t ub[5],
                    uint8_t* out, int threads);

// ---- multi-GPU reader (lfm_decode_multi.cpp) ----
// Devices the whole-image readers farm block-layer ranges to.  Opt-in:
// lfm_set_decode_devices, else env LFM_DECODE_GPUS (the syntax of LFM_GPUS),
// else empty.  Fewer than two entries: the reader runs on the current device
// as ever.
std::vector<int> decode_devices();
void set_decode_devices(const std::vector<int>& devs);
// env LFM_DECODE_GPUS for n visible devices (no device call)
std::vector<int> default_decode_devices(int n);
// "0,1,2" (a device may repeat) or a count, entries outside [0, n) dropped:
// the value of LFM_GPUS / LFM_DECODE_GPUS
std::vector<int> parse_device_list(const char* s, int n);

// How a whole image is cut for `nworkers` readers: the writer's split
// (encode_multi) along t, else c, else z, in whole block layers; on the z axis
// of a predicted video file with an odd block depth in pairs of layers, so
// every shard starts at an even z and decode_roi decodes exactly the shard's
// blocks.  One shard = the whole axis when the image does not split.
struct ShardPlan {
    int axis = 2;
    std::vector<std::pair<uint32_t, uint32_t>> shards;  // (first, count) along the axis
};
ShardPlan decode_shard_plan(const klb_image_header& h, int nworkers);

// Decode the .lfm at buf (header h already parsed from it) with one host
// thread per shard of decode_shard_plan(h, devs.size()), each on its device
// with its own kept decode state, into img (host, the whole image) or, when
// d_out is given, into d_out[w] (device, out_bytes[w] bytes, shard w alone;
// the plan is then that of n_out workers and each shard runs on its
// buffer's device).  A file that does not split, or that the pipelined GPU
// decode does not take, is one plain decode_payload into img.  Returns the
// first non-zero shard status in shard order.
int decode_multi(const uint8_t* buf, size_t len, const klb_image_header& h, uint8_t* img, void* const* d_out,
                 const uint64_t* out_bytes, int n_out, int threads, const std::vector<int>& devs,
                 lfm_decode_multi_stats* stats, lfm_decode_shard* shards, int shard_cap);
// The whole-image host readers' decode (lfm_decode_memory, decode_file):
// decode_multi when decode_devices() names two or more, else decode_payload.
int decode_image(const uint8_t* buf, size_t len, const klb_image_header& h, uint8_t* img, int threads);
// stop the kept decode workers; their device and pinned buffers are freed
void release_decode_workers();

// ---- streaming (lfm_stream.cpp) ----
// lfm_writer: block layers along the shard axis (t, else c, else z) arrive
// over time and go into one .lfm file.  Each range of whole layers is encoded
// as encode_multi encodes its ranges (predictor selected once on frame 0 and
// forced, the stack's nominal bzip2 level, z0 / prev on the z axis) through
// Encoder::submit / wait on an encoder of its own, two in flight; the calling
// thread is the in-order writer: a finished range's payload is appended to
// the file and its block sizes re-accumulated into the offset table, which
// close writes with the final extent.  A range of whole layers is also a
// checkpoint: once its payload is in the file, its table entries go into the
// capacity-sized table (and, the first time, the chosen header byte to offset
// 0), so a file that is never closed holds what recover_file and a live
// FileReader need to find its complete layers.
class StreamWriter {
public:
    // h: the stack as lfm_writer_open describes it, xyzct[axis] the capacity
    StreamWriter(const klb_image_header& h, int device, int threads);
    ~StreamWriter();
    int open(const char* filename);
    int axis() const { return axis_; }
    int append(const void* img, bool dev, uint32_t count);
    // joins the encodes in flight (their payload and table entries are then in
    // the file), fdatasync when asked; *committed = indices a recovery keeps
    int flush(bool sync, uint64_t* committed);
    int close(lfm_writer_stats* st);  // the writer is finished either way
    void abort();                     // closes and removes the file

private:
    int submit_range(const void* data, bool dev, uint64_t n);
    int drain_one();
    int stage_copy(void* dst, const void* src, size_t n, bool dev);
    void* stage_buffer(bool dev, int which, size_t n);
    int finish_file();
    Encoder enc_;
    klb_image_header cap_;       // block size as asked for, xyzct[axis] the capacity
    int threads_, axis_;
    uint64_t unit_, stride_;     // indices per block layer; bytes per index
    std::string path_;
    int fd_ = -1;
    int rc_ = 0;                 // sticky failure
    int kind_ = -1;              // -1 none yet, 0 host appends, 1 device appends
    bool selected_ = false;
    uint8_t hv_;                 // the request every range is encoded with (forced once selected)
    uint8_t hv_final_ = 0;       // the header byte the ranges produced
    uint64_t appended_ = 0, submitted_ = 0, staged_ = 0;  // indices: taken, handed to the encoder, held back
    bool have_prev_ = false;
    std::vector<uint8_t> h_buf_[3];  // host: held-back part, assembled range, raw frame before the next range
    DeviceBuffer d_buf_[3];          // device: the same
    std::vector<uint64_t> pending_;  // tickets in flight, oldest first
    std::vector<uint64_t> pending_n_;  // their indices along the axis
    std::vector<uint64_t> table_;    // block end offsets so far
    uint64_t payload_ = 0, payload_base_ = 0, nb_cap_ = 0;
    bool hv_on_disk_ = false;        // the chosen header byte has been checkpointed
    lfm_writer_stats st_{};
};

// What an unclosed file's table says (recover_file and the live FileReader
// apply the same rule): the committed prefix is the longest run of leading
// entries that are non-zero, strictly increasing and end inside the payload
// bytes the file holds (`payload_bytes` = file size - payload base); only
// whole block layers of it count.  `from`: entries below it are known good.
struct CommittedPrefix {
    uint64_t blocks = 0;        // plausible leading entries
    uint64_t layer_blocks = 0;  // blocks of one layer along the stream axis
    uint64_t layers = 0;        // whole layers among `blocks`
};
CommittedPrefix committed_prefix(const klb_image_header& capacity_header, int axis, const uint64_t* table, uint64_t nb,
                                 uint64_t payload_bytes, uint64_t from = 0);

// lfm_recover: the .lfm of the complete layers of a file its writer never
// closed, finalised by the code StreamWriter::close finalises with.
int recover_file(const char* filename, const char* out_filename, bool verify, int threads, lfm_recover_stats* st);

// lfm_reader: header and table in memory, the streams of a region's blocks
// fetched from the file by byte range (PayloadSource) for each read.  A live
// reader (open with live = true) takes a file its writer has not closed: `h` is
// then the view of the committed whole layers (xyzct[axis] may be 0), the
// payload starts behind the capacity-sized table, and refresh() extends the
// view by what the writer has checkpointed since.
class FileReader {
public:
    ~FileReader();
    int open(const char* filename, bool live = false);
    int refresh(uint32_t* extent);
    int read(const uint32_t lb[5], const uint32_t ub[5], void* out, uint64_t out_bytes, bool dev, int threads,
             lfm_decode_stats* stats);
    klb_image_header h;
    uint64_t file_bytes = 0, bytes_read = 0;

private:
    int load(bool* closed);          // header and table into h; *closed: the table is a closed file's
    void make_view();                // live: h from cap_ and the entries accepted so far
    int fd_ = -1;
    bool live_ = false;              // the file was unclosed when last looked at
    int axis_ = 2;
    klb_image_header cap_;           // live: the header as on disk (xyzct[axis] the capacity) and its table as far as read
    uint64_t known_ = 0;             // live: leading entries of cap_'s table accepted so far (whole layers)
    uint64_t payload_base_ = 0;      // file offset of the payload
};

} // namespace lfm
