// lfm_decode.cpp -- the readers: host inverse predictor, the pipelined GPU
// decode of a BZIP2 payload, whole-image and region reads into host or device
// memory, the file readers.
#include "lfm_engine.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <sys/mman.h>
#include <unistd.h>

#include "lfm_cases.h"
#include "lfm_hip.h"
#include "lfm_internal.h"

namespace lfm {

// ---------------------------------------------------------------- decode --
namespace {
template <int FAM, int K, bool TEMP>
void unpredict_frame(const uint16_t* sym, const uint16_t* prev, uint16_t* out, int W, int H, int T)
{
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            GlobalNb g{out, W, T, x, y};
            const int r = unsymbolize16(sym[(size_t)y * W + x]);
            const int P = TEMP ? (int)prev[(size_t)y * W + x] : 0;
            const int val = with_case(tile_case(x / T, y / T), pos_case(x % T, y % T), [&](auto TC, auto UC) {
                return inverse_case<FAM, K, TC.value, UC.value, TEMP>(g, r, P);
            });
            out[(size_t)y * W + x] = (uint16_t)val;
        }
}

template <int FAM>
int unpredict_dispatch_k(int k, bool temp, const uint16_t* sym, const uint16_t* prev, uint16_t* out, int W, int H,
                         int T)
{
#define LFM_K(K_)                                                                          \
    case K_:                                                                               \
        if (temp) unpredict_frame<FAM, K_, true>(sym, prev, out, W, H, T);                 \
        else unpredict_frame<FAM, K_, false>(sym, prev, out, W, H, T);                     \
        return 0;
    switch (k) { LFM_K(1) LFM_K(2) LFM_K(3) LFM_K(4) LFM_K(5) LFM_K(6) LFM_K(7) }
#undef LFM_K
    return 3;
}

int unpredict_one(int fam, int k, bool temp, const uint16_t* sym, const uint16_t* prev, uint16_t* out, int W, int H,
                  int T)
{
    if (temp && fam != 0) return LFM_HIP_ENOTINV;  // r = ((I - pred) + P) >> 1 drops a bit
    switch (fam) {
    case 0: return unpredict_dispatch_k<0>(k, temp, sym, prev, out, W, H, T);
    case 1: return unpredict_dispatch_k<1>(k, temp, sym, prev, out, W, H, T);
    case 2: return unpredict_dispatch_k<2>(k, temp, sym, prev, out, W, H, T);
    }
    return 3;
}

// frames whose temporal residual the reference wrote lossily
int not_invertible()
{
    std::printf("ERROR: frames of this file cannot be inverted (temporal angle/space predictor)\n");
    return 3;
}

// Device buffers, streams and pinned status arrays of the GPU decode, kept
// per host thread and device between calls (LFM_DECODE_KEEP=0 releases them
// after every call): fresh device allocations are cleared by the driver
// before first use, which showed up as 20-40 ms stalls of the first upload.
// Two slots (stream, workspace, block buffer, lens / flags) for the pipelined
// chunks of gpu_decode.
struct DecodeBuffers {
    static constexpr int kSlots = 3;
    enum { PAY, SYM, OUT, WS0, BLK0 = WS0 + kSlots, N = BLK0 + kSlots };
    int dev = -1;
    hipStream_t st[kSlots] = {};
    hipStream_t dl = nullptr;                // the downloads' device -> pinned copies
    DeviceBuffer p[N];
    // the sub-image a device-destination region read crops from: decode_roi
    // takes it out of here between its sub-image's decode and the crop, so a
    // release() in between (LFM_DECODE_KEEP=0, a failed allocation) spares it
    DeviceBuffer roi;
    HostBuffer hs[kSlots];  // pinned: lens then flags, per slot
    HostBuffer us;          // pinned: the inverse predictor's status words, per (chunk, volume piece)
    Staging down;                            // the download thread's pinned chunks
    ~DecodeBuffers() { release(); }  // a worker thread that exits frees its device buffers
    void release()
    {
        for (DeviceBuffer& b : p) b.release();
        roi.release();
        us.release();
        for (int k = 0; k < kSlots; ++k) {
            hs[k].release();
            if (st[k]) (void)hipStreamDestroy(st[k]);
            st[k] = nullptr;
        }
        if (dl) (void)hipStreamDestroy(dl);
        dl = nullptr;
        down.release();
        dev = -1;
    }
    bool begin()
    {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) return false;
        if (dev != d) {
            release();
            // LFM_DECODE_PRIO=1: slot 0's stream at the highest priority, the
            // others at the lowest, so the first chunk finishes (and its
            // download starts) while the second one still decodes
            static const bool prio = env_int("LFM_DECODE_PRIO", 0) != 0;
            int least = 0, greatest = 0;
            if (prio) (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            for (int k = 0; k < kSlots; ++k)
                if ((prio ? hipStreamCreateWithPriority(&st[k], hipStreamNonBlocking, k == 0 ? greatest : least)
                          : hipStreamCreateWithFlags(&st[k], hipStreamNonBlocking)) != hipSuccess) {
                    release();
                    return false;
                }
            if (hipStreamCreateWithFlags(&dl, hipStreamNonBlocking) != hipSuccess) {
                release();
                return false;
            }
            dev = d;
        }
        return true;
    }
    // (a failed device allocation is not an error of the decode: the caller
    // falls back, so the HIP error is cleared)
    static void* device(DeviceBuffer& b, size_t bytes)
    {
        void* q = b.reserve(bytes);
        if (!q) (void)hipGetLastError();
        return q;
    }
    void* get(int i, size_t bytes) { return device(p[i], bytes); }
    uint32_t* status(int k, size_t count) { return (uint32_t*)hs[k].reserve(count * 8); }  // 2 * count words: lens, flags
    int* ustatus(size_t count) { return (int*)us.reserve(count * sizeof(int)); }
};

DecodeBuffers& decode_buffers()
{
    static thread_local DecodeBuffers b;
    return b;
}

// LFM_DECODE_KEEP=0: the decode's buffers and the thread's pinned chunks are
// released after every call
void release_unless_kept(DecodeBuffers& DB)
{
    static const bool keep = env_int("LFM_DECODE_KEEP", 1) != 0;
    if (!keep) {
        DB.release();
        staging().release();
    }
}

// image bytes this thread's decodes have copied device -> host (lfm_decode_stats.d2h_bytes)
thread_local uint64_t tl_d2h_bytes = 0;

// LFM_DECODE_TIMING: a timeline of the pipeline's steps (ms since start);
// nothing is recorded when timing is off
struct Timeline {
    const clk::time_point t_start = clk::now();
    std::mutex mu;
    std::vector<std::pair<std::string, double>> steps;
    void mark(const char* what, uint64_t c)
    {
        if (!decode_timing()) return;
        std::lock_guard<std::mutex> lk(mu);
        steps.emplace_back(std::string(what) + " " + std::to_string(c), ms_since(t_start));
    }
};

std::atomic<int>& bunzip2_multiblock_flag()
{
    static std::atomic<int> on{env_int("LFM_BUNZIP2_MULTIBLOCK", 1) != 0 ? 1 : 0};
    return on;
}

// How a payload is cut into chunks, computed once from header, grid and
// switches.
// chunks: whole slabs, at least two and about LFM_DECODE_CHUNK_BLOCKS
// blocks each (default 4096, about the streams the Huffman kernel holds
// resident at once: config 3's 3 872 streams in two chunks, a config-5
// volume's 7 396 in two); 0 = one chunk.  With two slots a third chunk
// cannot start before the first is finished, so smaller chunks lose (four
// chunks of 968 streams: 75.6 vs 54.3 ms on config 3)
struct DecodePlan {
    uint64_t nslabs, nbz, bz, Z;  // block slabs (one z-block row of one volume), z-block rows and frames per volume
    uint64_t spc;                 // slabs per chunk
    uint64_t batch, nch;          // blocks per chunk, chunks
    int nslot;                    // slots in use
    // inverse predictor status words: chunk c's volume pieces at us[c * (spc + 1) ..]
    // (a chunk's slabs lie in at most spc volumes)
    uint64_t us_per;
    size_t ws;                    // a slot's workspace
    // streams of several bzip2 blocks on the device (bunzip2_multiblock(), read
    // once per decode): the bzip2 level the writer chose for the nominal block
    // (klb_imageIO.cpp:108), which sizes a stream's slots; 0: the single-block
    // entries, such streams go to the host library
    uint32_t level;
    size_t ws_bytes(uint32_t n, uint32_t block_bytes) const
    {
        return level ? lfm_hip_bunzip2_workspace_bytes_multi(n, block_bytes, level)
                     : lfm_hip_bunzip2_workspace_bytes(n, block_bytes);
    }
    DecodePlan(const BlockGrid& g, uint32_t block_bytes)
    {
        level = bunzip2_multiblock() ? std::min<uint32_t>(9, std::max<uint32_t>(1, (block_bytes + 99999) / 100000)) : 0;
        const uint64_t nb = g.nblocks, slab = g.nb[0] * g.nb[1];
        nslabs = nb / slab;
        nbz = g.nb[2];
        bz = g.bs[2];
        Z = g.dims[2];
        const long target = env_int("LFM_DECODE_CHUNK_BLOCKS", 4096);
        static const int slots = std::max(2, std::min(env_int("LFM_DECODE_SLOTS", 2), (int)DecodeBuffers::kSlots));
        spc = nslabs;
        if (target > 0) {
            const uint64_t want = std::max<uint64_t>(slots, (nb + (uint64_t)target - 1) / (uint64_t)target);
            spc = std::max<uint64_t>(1, (nslabs + want - 1) / want);
        }
        const size_t per = ws_bytes(1, block_bytes) + block_bytes;
        const size_t budget = (size_t)env_int("LFM_BUNZIP2_GPU_BUDGET_MB", 16 * 1024) << 20;
        spc = std::max<uint64_t>(1, std::min<uint64_t>(spc, budget / slots / per / slab));
        batch = spc * slab;
        nch = (nslabs + spc - 1) / spc;
        ws = ws_bytes((uint32_t)batch, block_bytes);
        nslot = (int)std::min<uint64_t>(nch, (uint64_t)slots);
        us_per = spc + 1;
    }
    // the frames (volume-major) a chunk's slabs cover: [f0, f1)
    void frames(uint64_t c, uint64_t& f0, uint64_t& f1) const
    {
        const uint64_t s0 = c * spc, s1 = std::min(nslabs, s0 + spc) - 1;
        f0 = (s0 / nbz) * Z + (s0 % nbz) * bz;
        f1 = (s1 / nbz) * Z + std::min<uint64_t>(Z, (s1 % nbz + 1) * bz);
    }
};

// One pipelined decode: what its steps (finish_chunk on the calling thread,
// download_chunks on the downloader thread) read, fixed before the first
// chunk is issued, and the few figures each of the two threads adds up.
struct DecodeJob {
    const uint8_t* payload;
    const klb_image_header& h;
    const BlockGrid& g;
    const DecodePlan& P;
    const std::vector<uint64_t>& offs;  // payload offset of every block, and the end
    uint8_t* img;
    DeviceDest* dd;
    bool predicted;
    int family, k, video, threads;
    DecodeBuffers& DB;
    Timeline& tl;
    void *d_pay = nullptr, *d_sym = nullptr, *d_out = nullptr;
    void *d_ws[DecodeBuffers::kSlots] = {}, *d_blk[DecodeBuffers::kSlots] = {};
    uint32_t* hs[DecodeBuffers::kSlots] = {};
    int* us = nullptr;
    uint32_t dims[5], bs[5];
    // per chunk: its scatter + inverse predictor done (the download waits for it)
    std::vector<hipEvent_t> cev;
    std::vector<uint8_t> hb;  // one block from the host library
    // the calling thread's
    double t_wait = 0, t_host = 0;
    uint64_t host_blocks = 0;
    // the downloader's (read after its join)
    double t_down = 0;
    uint64_t d2h_bytes = 0;
    int drc = 0;
    std::thread prefault;  // joined by the downloader before its first copy
};

// host side of chunk c once its streams are decoded: host-library blocks,
// then scatter and inverse predictor queued behind them (no wait)
int finish_chunk(DecodeJob& J, uint64_t c)
{
    const DecodePlan& P = J.P;
    const klb_image_header& h = J.h;
    const size_t bpp = h.getBytesPerPixel();
    const uint32_t block_bytes = h.getBlockSizeBytes();
    const uint64_t W = h.xyzct[0], H = h.xyzct[1], Z = h.xyzct[2];
    const int q = (int)(c % P.nslot);
    hipStream_t st = J.DB.st[q];
    const uint64_t b0 = c * P.batch, cnt = std::min<uint64_t>(P.batch, J.g.nblocks - b0);
    auto t0 = clk::now();
    if (hipStreamSynchronize(st) != hipSuccess) return 3;
    auto t1 = clk::now();
    J.t_wait += ms_between(t0, t1);
    const uint32_t* lens = J.hs[q];
    const uint32_t* flags = J.hs[q] + P.batch;
    for (uint64_t i = 0; i < cnt; ++i) {
        uint64_t o[5], sz[5];
        J.g.block(b0 + i, o, sz);
        const uint64_t expect = bpp * sz[0] * sz[1] * sz[2] * sz[3] * sz[4];
        if (flags[i] == 1) {  // the host library decodes this stream
            ++J.host_blocks;
            const int r = decompress_one(BZIP2, J.payload + J.offs[b0 + i],
                                         (uint32_t)(J.offs[b0 + i + 1] - J.offs[b0 + i]), J.hb.data(), (uint32_t)expect);
            if (r) return r;
            if (hipMemcpyAsync((uint8_t*)J.d_blk[q] + (size_t)i * block_bytes, J.hb.data(), expect,
                               hipMemcpyHostToDevice, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                return 3;
        } else if (flags[i] != 0 || lens[i] != expect) {
            std::printf("ERROR: block %llu of the payload does not decode to its %llu bytes (bzip2 CRC / length)\n",
                        (unsigned long long)(b0 + i), (unsigned long long)expect);
            return 2;
        }
    }
    // a device destination is first written by the scatter (unpredicted)
    // or the inverse predictor: after the caller's null-stream work
    if (J.dd && !J.predicted && hipStreamWaitEvent(st, J.dd->after_caller, 0) != hipSuccess) return 3;
    if (lfm_hip_scatter_blocks(J.d_blk[q], block_bytes, (uint32_t)b0, (uint32_t)cnt, J.dims, J.bs, (uint32_t)bpp,
                               J.d_sym, st) != LFM_HIP_OK)
        return 3;
    if (J.predicted) {
        uint64_t f0, f1;
        P.frames(c, f0, f1);
        if (J.dd && hipStreamWaitEvent(st, J.dd->after_caller, 0) != hipSuccess) return 3;
        // a temporal first frame (video, odd z) reads the previous chunk's
        // last decoded frame: wait for that chunk's inverse predictor
        if (J.video && c > 0 && hipStreamWaitEvent(st, J.cev[c - 1], 0) != hipSuccess) return 3;
        uint64_t piece = 0;
        for (uint64_t f = f0; f < f1; ++piece) {  // per volume
            const uint64_t v = f / Z, z0 = f % Z, n = std::min<uint64_t>(f1, (v + 1) * Z) - f;
            const uint16_t* prev = z0 > 0 ? (const uint16_t*)J.d_out + (f - 1) * W * H : nullptr;
            if (piece >= P.us_per) return 3;  // (cannot happen: see us_per)
            // queued only: its status word is checked with the download
            const int hr = lfm_hip_unpredict_async((const uint16_t*)J.d_sym + f * W * H, prev,
                                                   (uint16_t*)J.d_out + f * W * H, (int)W, (int)H, (int)n, h.Nnum,
                                                   J.family, J.k, J.video, (int)z0, J.us + c * P.us_per + piece, st);
            if (hr == LFM_HIP_ENOTINV) return not_invertible();
            if (hr != LFM_HIP_OK) return 3;
            f += n;
        }
    }
    if (hipEventRecord(J.cev[c], st) != hipSuccess) return 3;
    J.t_host += ms_since(t1);
    return 0;
}

// which chunks the downloader may take: the calling thread hands them over in order
struct HandOver {
    std::mutex mu;
    std::condition_variable cv;
    uint64_t ready = 0;  // chunks [0, ready) may be downloaded
    bool stop = false;
    void hand(uint64_t c) { update(c + 1, false); }  // chunk c is finished
    void finish() { update(ready, true); }           // no more will be (only the calling thread writes `ready`)
    void update(uint64_t r, bool s)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            ready = r;
            stop = s;
        }
        cv.notify_all();
    }
    bool wait(uint64_t c)  // false: stopped before chunk c was handed over
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return ready > c || stop; });
        return ready > c;
    }
};

// the downloads run on their own thread (own pinned chunks), in chunk
// order, each once its chunk's event fires: the calling thread goes on queueing
// the next chunks meanwhile
void download_chunks(DecodeJob& J, HandOver& ho)
{
    const DecodePlan& P = J.P;
    const size_t frame_bytes = (size_t)J.h.xyzct[0] * J.h.xyzct[1] * J.h.getBytesPerPixel();
    for (uint64_t c = 0; c < P.nch; ++c) {
        if (!ho.wait(c)) return;  // stopped
        // (started before chunk 0 was handed over; done long before it is decoded)
        if (c == 0 && J.prefault.joinable()) J.prefault.join();
        auto t0 = clk::now();
        J.tl.mark("dl-start", c);
        uint64_t f0, f1;
        P.frames(c, f0, f1);
        const size_t o0 = f0 * frame_bytes, n = (f1 - f0) * frame_bytes;
        const uint8_t* src = (const uint8_t*)(J.predicted ? J.d_out : J.d_sym) + o0;
        // (its own stream: on the chunk's slot stream the copies would
        // queue behind the kernels of chunk c + nslot, issued meanwhile)
        hipStream_t st = J.DB.dl;
        if (hipEventSynchronize(J.cev[c]) != hipSuccess) {
            J.drc = 3;
            return;
        }
        J.tl.mark("dl-ready", c);
        // the chunk's inverse predictor launches: a hand-over that timed
        // out and was not repaired on the device fails the read
        if (J.predicted)
            for (uint64_t i = 0; i < P.us_per; ++i)
                if (lfm_hip_unpredict_check(J.us[c * P.us_per + i]) != LFM_HIP_OK) {
                    std::printf("ERROR: the inverse predictor did not complete (band hand-over timed out)\n");
                    J.drc = 3;
                    return;
                }
        if (J.dd) {  // the pixels are where they belong
            J.tl.mark("dl-end", c);
            continue;
        }
        // the device -> pinned copies: the runtime's (57 GB/s) or an SDMA
        // engine's (28 GB/s).  The runtime's copies slow the kernels of
        // chunks still decoding (config 5, 8 chunks: 403-427 vs 325-349
        // ms), so LFM_DECODE_D2H=1 (default) takes them only for the last
        // nslot chunks, whose downloads are the decode's exposed tail
        // (config 3: 55-57 vs 62-64 ms); 2: always, 0: never
        // (profiles/r06_ab_decode_d2h*.jsonl)
        static const int d2h_mode = env_int("LFM_DECODE_D2H", 1);
        const bool rt = d2h_mode == 2 || (d2h_mode == 1 && c + P.nslot >= P.nch);
        if (((rt || !sdma_staged_d2h(J.img + o0, src, n, J.threads, J.DB.down)) &&
             (!staged_d2h(J.img + o0, src, n, st, J.threads, J.DB.down) || hipStreamSynchronize(st) != hipSuccess))) {
            J.drc = 3;
            return;
        }
        J.t_down += ms_since(t0);
        J.d2h_bytes += n;
        J.tl.mark("dl-end", c);
    }
}

// The image comes down into the caller's buffer, usually fresh pages (a
// new numpy array, readKLBstack's malloc): the download's host copies used
// to take a first-touch fault per 4 KiB page (config 3: 131 072 faults,
// download 11-24 ms for 537 MB).  While the GPU decodes, a helper thread
// asks for huge pages and touches one byte per page of the destination, so
// the downloads copy into mapped memory (LFM_DECODE_PREFAULT=0: off).
void prefault(uint8_t* img, size_t img_bytes, int threads)
{
    const size_t pg = (size_t)sysconf(_SC_PAGESIZE), huge = (size_t)2 << 20;
    const uintptr_t a0 = ((uintptr_t)img + huge - 1) & ~(uintptr_t)(huge - 1);
    const uintptr_t a1 = ((uintptr_t)img + img_bytes) & ~(uintptr_t)(huge - 1);
    if (a1 > a0) (void)madvise((void*)a0, a1 - a0, MADV_HUGEPAGE);
    const size_t piece = (size_t)8 << 20;
    const uint64_t np = (img_bytes + piece - 1) / piece;
    parallel_for(np, std::max(1, threads / 2), [&](uint64_t i) {
        volatile uint8_t* q = (volatile uint8_t*)img;
        const size_t e = std::min(img_bytes, (size_t)(i + 1) * piece);
        for (size_t o = (size_t)i * piece; o < e; o += pg) q[o] = 0;
    });
}

// payload bytes [lo, hi) of the job go up.
// payload upload: the SDMA engine through the pinned chunks (LFM_DECODE_H2D
// = 0, default; falls back to 1 when HSA cannot take it), 1 one runtime
// copy, 2 the pinned chunks with hipMemcpyAsync -- the blit-kernel copies
// took 5-47 ms for config 3's 277 MB depending on the process's state
bool upload_payload(const DecodeJob& J, uint64_t lo, uint64_t hi, hipStream_t st)
{
    static const int up_mode = env_int("LFM_DECODE_H2D", 0);
    lo &= ~(uint64_t)3;  // (4-byte aligned pieces; neighbours rewrite the same bytes)
    const size_t n = hi - lo;
    uint8_t* dst = (uint8_t*)J.d_pay + lo;
    if (up_mode == 0 && sdma_staged_h2d(dst, J.payload + lo, n, J.threads)) return true;
    (void)hipGetLastError();
    const bool ok = up_mode == 2 ? staged_h2d(dst, J.payload + lo, n, st, J.threads)
                                 : hipMemcpyAsync(dst, J.payload + lo, n, hipMemcpyHostToDevice, st) == hipSuccess;
    return ok && hipStreamSynchronize(st) == hipSuccess;
}

// the decode's device buffers, pinned status arrays and streams; false: the
// GPU path does not apply
bool decode_job_buffers(DecodeJob& J, size_t pay_bytes, size_t img_bytes, uint32_t block_bytes)
{
    const DecodePlan& P = J.P;
    DecodeBuffers& DB = J.DB;
    if (DB.begin()) {
        J.d_pay = DB.get(DecodeBuffers::PAY, pay_bytes + 64);
        J.d_sym = J.dd && !J.predicted ? J.img : DB.get(DecodeBuffers::SYM, img_bytes);
        J.d_out = !J.predicted ? nullptr : J.dd ? J.img : DB.get(DecodeBuffers::OUT, img_bytes);
        for (int q = 0; q < P.nslot; ++q) {
            J.d_ws[q] = DB.get(DecodeBuffers::WS0 + q, P.ws);
            J.d_blk[q] = DB.get(DecodeBuffers::BLK0 + q, P.batch * block_bytes);
            J.hs[q] = DB.status(q, P.batch);
        }
        if (J.predicted) {
            J.us = DB.ustatus(P.nch * P.us_per);
            if (J.us) std::fill(J.us, J.us + P.nch * P.us_per, 0);
        }
    }
    bool have = DB.st[0] && J.d_pay && J.d_sym && (!J.predicted || (J.d_out && J.us));
    for (int q = 0; q < P.nslot; ++q) have = have && J.d_ws[q] && J.d_blk[q] && J.hs[q];
    return have;
}
} // namespace

int bunzip2_multiblock() { return bunzip2_multiblock_flag().load(); }
int set_bunzip2_multiblock(int on) { return bunzip2_multiblock_flag().exchange(on ? 1 : 0); }

// GPU decode of a BZIP2 payload (lfm_bunzip2.hip), pipelined over chunks of
// whole block slabs (the blocks of one z-block row of one volume, so a chunk's
// pixels are a contiguous run of frames of the image): per chunk the payload
// bytes go up (SDMA), its streams are decoded (the few flagged ones by the
// host library), scattered into the device symbol image, run through the
// inverse predictor and come down (SDMA) into the caller's image.  Chunks
// alternate between two HIP streams, and the host works one chunk behind the
// device: while chunk c's kernels run, chunk c - 1 is finished and copied
// down and chunk c + 1's payload goes up.  Returns -1 when the GPU path does
// not apply (the caller decodes on the host).
// With dd, img is device memory on the current device and takes the place of
// the device image the pixels are finished in (OUT of a predicted file, SYM of
// an unpredicted one, which is then not allocated): nothing comes down, the
// downloader thread only waits for each chunk's event and checks its status
// words, and every slot stream waits for dd->after_caller before the chunk's
// first kernel that writes img.
// stats (optional): chunks, blocks and host_blocks are set and the image
// bytes copied down are added to d2h_bytes.
static int gpu_decode(const uint8_t* payload, size_t len, const klb_image_header& h, uint8_t* img, int family,
                      bool predicted, int k, int video, int threads, DeviceDest* dd, lfm_decode_stats* stats)
{
    const BlockGrid g(h);
    const uint64_t nb = g.nblocks;
    const uint32_t block_bytes = h.getBlockSizeBytes();
    if (!nb || !block_bytes || nb >= (1ull << 31)) return -1;
    // (a chunk's frames, DecodePlan::frames, are those of blocks one channel and one time point deep)
    if (g.bs[3] != 1 || g.bs[4] != 1) return -1;
    // (the scatter's and the inverse predictor's 16-byte rows)
    if (dd && ((uintptr_t)img & 15)) return -1;
    Timeline tl;
    double t_up = 0;
    std::vector<uint64_t> offs(nb + 1);
    for (uint64_t i = 0; i < nb; ++i) {
        offs[i] = h.getBlockOffset(i);
        if (i && offs[i] != offs[i - 1] + h.getBlockCompressedSizeBytes(i - 1)) return -1;  // not contiguous
    }
    offs[nb] = offs[nb - 1] + h.getBlockCompressedSizeBytes(nb - 1);
    if (offs[nb] > len) return 3;
    const size_t img_bytes = h.getImageSizeBytes();
    const DecodePlan P(g, block_bytes);
    const uint64_t nch = P.nch;
    DecodeBuffers& DB = decode_buffers();
    DecodeJob J{payload, h, g, P, offs, img, dd, predicted, family, k, video, threads, DB, tl};
    if (!decode_job_buffers(J, offs[nb], img_bytes, block_bytes)) {
        DB.release();
        return -1;
    }
    const auto t_alloc = clk::now();
    for (int d = 0; d < 5; ++d) {
        J.dims[d] = h.xyzct[d];
        J.bs[d] = (uint32_t)g.bs[d];
    }
    J.hb.resize(block_bytes);
    int rc = 0;
    const double t_hb = ms_since(tl.t_start);
    // LFM_DECODE_DMA_PROBE=1 (diagnosis): a 64 KiB staged SDMA upload, timed,
    // before the decode's own steps start
    if (env_int("LFM_DECODE_DMA_PROBE", 0) == 1 && offs[nb] >= 65536) {
        const auto p0 = clk::now();
        const bool pok = sdma_staged_h2d(J.d_pay, payload, 65536, 1);
        std::fprintf(stderr, "dma probe: 64 KiB upload %.3f ms (%s)\n", ms_since(p0), pok ? "ok" : "failed");
    }
    static const int prefault_mode = env_int("LFM_DECODE_PREFAULT", 1);  // 2: started after the first upload
    auto start_prefault = [&]() {
        J.prefault = std::thread([img, img_bytes, threads, &tl]() {
            prefault(img, img_bytes, threads);
            tl.mark("prefault-done", 0);
        });
        tl.mark("prefault-started", 0);
    };
    if (prefault_mode == 1 && !dd) start_prefault();
    // the 64 zero bytes past the payload (the bit window's lookahead of the
    // last stream): LFM_DECODE_SLACK=1 queues them on the last chunk's stream
    // (stream order puts them before its kernels), 0 synchronises here
    static const int slack_mode = env_int("LFM_DECODE_SLACK", 1);
    {
        hipStream_t sst = slack_mode ? DB.st[(nch - 1) % P.nslot] : DB.st[0];
        if (hipMemsetAsync((uint8_t*)J.d_pay + offs[nb], 0, 64, sst) != hipSuccess) rc = 3;
        tl.mark("memset-issued", 0);
        if (!slack_mode && hipStreamSynchronize(sst) != hipSuccess) rc = 3;
    }
    tl.mark("memset", 0);
    J.cev.assign(nch, nullptr);
    for (uint64_t c = 0; c < nch && !rc; ++c)
        if (hipEventCreateWithFlags(&J.cev[c], hipEventDisableTiming) != hipSuccess) rc = 3;
    tl.mark("events", 0);
    HandOver ho;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::thread downloader([&J, &ho, dev]() {
        (void)hipSetDevice(dev);
        download_chunks(J, ho);
    });
    tl.mark("downloader-started", 0);
    for (uint64_t c = 0; c < nch && !rc; ++c) {
        const int q = (int)(c % P.nslot);
        const uint64_t b0 = c * P.batch, cnt = std::min<uint64_t>(P.batch, nb - b0);
        auto t0 = clk::now();
        if (!upload_payload(J, offs[b0], offs[b0 + cnt], DB.st[q])) {
            rc = 3;
            break;
        }
        t_up += ms_since(t0);
        tl.mark("uploaded", c);
        if (c == 0 && prefault_mode == 2 && !dd) start_prefault();
        const int irc = P.level ? lfm_hip_bunzip2_issue_multi(J.d_pay, offs.data() + b0, (uint32_t)cnt, J.d_blk[q],
                                                              block_bytes, P.level, J.d_ws[q], P.ws, J.hs[q],
                                                              J.hs[q] + P.batch, DB.st[q])
                                : lfm_hip_bunzip2_issue(J.d_pay, offs.data() + b0, (uint32_t)cnt, J.d_blk[q],
                                                        block_bytes, J.d_ws[q], P.ws, J.hs[q], J.hs[q] + P.batch,
                                                        DB.st[q]);
        if (irc != LFM_HIP_OK) {
            rc = 3;
            break;
        }
        tl.mark("issued", c);
        if (c > 0) {
            rc = finish_chunk(J, c - 1);
            tl.mark("finished", c - 1);
            if (!rc) ho.hand(c - 1);
        }
    }
    if (!rc) rc = finish_chunk(J, nch - 1);
    tl.mark("finished", nch - 1);
    if (!rc) ho.hand(nch - 1);
    ho.finish();
    downloader.join();
    tl_d2h_bytes += J.d2h_bytes;
    tl.mark("joined", nch);
    if (J.prefault.joinable()) J.prefault.join();  // (not reached: the downloader joins it first)
    if (!rc) rc = J.drc;
    for (int q = 0; q < P.nslot; ++q) (void)hipStreamSynchronize(DB.st[q]);  // nothing may still run on the buffers
    for (hipEvent_t e : J.cev)
        if (e) (void)hipEventDestroy(e);
    if (decode_timing()) {
        std::string line = "decode timeline: alloc@" + std::to_string(ms_between(tl.t_start, t_alloc)).substr(0, 6) +
                           " hb@" + std::to_string(t_hb).substr(0, 6);
        for (auto& e : tl.steps) line += " " + e.first + "@" + std::to_string(e.second).substr(0, 6);
        std::fprintf(stderr, "%s\n", line.c_str());
        std::fprintf(stderr,
                     "decode: %llu chunks of <= %llu blocks, alloc %.2f ms, upload %.2f, wait %.2f, host + kernels "
                     "after wait %.2f, download %.2f, total %.2f ms\n",
                     (unsigned long long)nch, (unsigned long long)P.batch, ms_between(tl.t_start, t_alloc), t_up,
                     J.t_wait, J.t_host, J.t_down, ms_since(tl.t_start));
    }
    if (stats) {
        stats->chunks = (uint32_t)nch;
        stats->blocks = nb;
        stats->host_blocks = J.host_blocks;
        stats->d2h_bytes += J.d2h_bytes;
    }
    release_unless_kept(DB);
    return rc;
}

int decode_payload(const uint8_t* payload, size_t len, const klb_image_header& h, uint8_t* img, int threads,
                   int family, DeviceDest* dd, lfm_decode_stats* hstats)
{
    if (threads <= 0) threads = default_threads();
    const BlockGrid g(h);
    if (g.nblocks != h.Nb) return 3;
    const size_t bpp = h.getBytesPerPixel();
    if (!bpp) return 5;
    const int k = h.headerVersion & 0x7F;
    const int video = (h.headerVersion >> 7) & 1;
    const bool predicted = bpp == 2 && k != 0;
    if (predicted && (k > 7 || h.Nnum == 0)) {
        std::printf("ERROR: unknown predictor %d in header\n", k);
        return 3;
    }
    if (dd) {
        // device destination: the pipelined decode writes img itself, or the
        // host reader below (this function without dd) fills a temporary that
        // one copy uploads, on the null stream and so behind the caller's work
        if (h.compressionType == BZIP2 && gpu_decode_enabled() && gpu_bunzip2_enabled() &&
            (!predicted || h.Nnum <= 31)) {
            const int rc = gpu_decode(payload, len, h, img, family, predicted, k, video, threads, dd, &dd->stats);
            if (rc != -1) {
                dd->stats.path = 0;
                return rc;
            }
        }
        const size_t n = h.getImageSizeBytes();
        std::unique_ptr<uint8_t[]> tmp(new uint8_t[n]);  // (no zero fill: every byte is decoded)
        const uint64_t down0 = tl_d2h_bytes;
        const int rc = decode_payload(payload, len, h, tmp.get(), threads, family);
        if (rc) return rc;
        dd->stats.path = 1;
        dd->stats.chunks = 0;
        dd->stats.blocks = dd->stats.host_blocks = g.nblocks;
        // (the host reader's inverse predictor runs on the GPU when one is
        // visible: its pixels came down before they go up again here)
        dd->stats.d2h_bytes += tl_d2h_bytes - down0;
        return hipMemcpy(img, tmp.get(), n, hipMemcpyHostToDevice) == hipSuccess ? 0 : 3;
    }
    if (h.compressionType == BZIP2 && gpu_decode_enabled() && gpu_bunzip2_enabled() && lfm_hip_device_count() > 0 &&
        (!predicted || h.Nnum <= 31)) {
        const int rc = gpu_decode(payload, len, h, img, family, predicted, k, video, threads, nullptr, hstats);
        if (rc != -1) {
            if (hstats) hstats->path = 0;
            return rc;
        }
    }
    // what the host reader below does, for a caller that asked (its image
    // bytes that come down are the GPU inverse predictor's)
    struct HostStats {
        lfm_decode_stats* s;
        uint64_t nb, down0;
        ~HostStats()
        {
            if (!s) return;
            s->path = 1;
            s->chunks = 0;
            s->blocks = s->host_blocks = nb;
            s->d2h_bytes += tl_d2h_bytes - down0;
        }
    } host_stats{hstats, g.nblocks, tl_d2h_bytes};
    std::vector<uint16_t> symbuf;
    uint8_t* sym = img;
    if (predicted) {
        symbuf.resize(h.getImageSizePixels());
        sym = (uint8_t*)symbuf.data();
    }
    std::atomic<int> err{0};
    const uint32_t block_bytes = h.getBlockSizeBytes();
    parallel_for(g.nblocks, threads, [&](uint64_t id) {
        thread_local std::vector<uint8_t> scratch;
        uint64_t o[5], s[5];
        g.block(id, o, s);
        const uint64_t expect = bpp * s[0] * s[1] * s[2] * s[3] * s[4];
        const uint64_t off = h.getBlockOffset(id), n = h.getBlockCompressedSizeBytes(id);
        if (off + n > len) { err.store(3); return; }
        scratch.resize(std::max<uint64_t>(expect, block_bytes));
        int rc = decompress_one(h.compressionType, payload + off, (uint32_t)n, scratch.data(), (uint32_t)expect);
        if (rc) { err.store(rc); return; }
        scatter_block(scratch.data(), g, id, bpp, sym);
    });
    if (err.load()) return err.load();
    if (!predicted) return 0;
    const int W = h.xyzct[0], H = h.xyzct[1], Z = h.xyzct[2];
    const uint64_t V = (uint64_t)h.xyzct[3] * h.xyzct[4];
    const size_t fs = (size_t)W * H;
    const uint16_t* s16 = symbuf.data();
    uint16_t* o16 = (uint16_t*)img;
    // inverse predictor on the GPU (lfm_unpredict.hip) whenever one is
    // visible; the host loop below is the reader of GPU-less machines (the
    // reference decoder itself is host code, klb_imageIO.cpp:1748-1821)
    if (gpu_decode_enabled() && lfm_hip_device_count() > 0 && h.Nnum <= 31) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        hipStream_t st = nullptr;
        DeviceBuffer sym_buf, out_buf;  // one volume each, for this call only
        const size_t vb = fs * Z * 2;
        int rc = 0;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) rc = 3;
        void* d_s = rc ? nullptr : sym_buf.reserve(vb);
        void* d_o = d_s ? out_buf.reserve(vb) : nullptr;
        if (!d_o) rc = 3;
        for (uint64_t v = 0; v < V && !rc; ++v) {
            if (hipMemcpyAsync(d_s, s16 + v * Z * fs, vb, hipMemcpyHostToDevice, st) != hipSuccess) { rc = 3; break; }
            const int hr = lfm_hip_unpredict((const uint16_t*)d_s, nullptr, (uint16_t*)d_o, W, H, Z, h.Nnum, family, k,
                                             video, 0, st);
            if (hr == LFM_HIP_ENOTINV) {
                rc = not_invertible();
                break;
            }
            if (hr != LFM_HIP_OK || hipMemcpyAsync(o16 + v * Z * fs, d_o, vb, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess)
                rc = 3;
            tl_d2h_bytes += vb;
        }
        sym_buf.release();
        out_buf.release();
        if (st) (void)hipStreamDestroy(st);
        return rc;
    }
    // host inverse (frames in parallel; on video stacks the odd frames need
    // the decoded even frame before them)
    for (int pass = 0; pass < (video ? 2 : 1); ++pass) {
        std::vector<uint64_t> frames;
        for (uint64_t v = 0; v < V; ++v)
            for (int z = 0; z < Z; ++z) {
                const bool temp = video && (z & 1);
                if (video ? (pass == (temp ? 1 : 0)) : true) frames.push_back(v * Z + z);
            }
        parallel_for(frames.size(), threads, [&](uint64_t i) {
            const uint64_t fidx = frames[i];
            const int z = (int)(fidx % Z);
            const bool temp = video && (z & 1);
            int rc = unpredict_one(family, k, temp, s16 + fidx * fs, temp ? o16 + (fidx - 1) * fs : nullptr,
                                   o16 + fidx * fs, W, H, h.Nnum);
            if (rc) err.store(rc);
        });
        if (err.load() == LFM_HIP_ENOTINV) return not_invertible();
        if (err.load()) return err.load();
    }
    return 0;
}

// ROI read: decode only the blocks the ROI depends on, then
// crop.  Every predictor neighbour is up and / or left in its frame, so a
// predicted ROI needs x in [0, ub0] and y in [0, ub1] of its frames (the
// inverse on that corner computes the same pixels as on the whole frame);
// a temporal (odd z) frame of a video stack also needs the frame before it.
// The blocks of that region (whole blocks, origin z even on video stacks so
// the temporal parity is unchanged) are described by a sub-header whose block
// grid is exactly those blocks in file order, their streams are gathered into
// a sub-payload, and the ordinary decode (GPU or host) runs on it.  The
// reference's own ROI path decodes the ROI's blocks and then un-predicts them
// as if they were the whole frame, which is wrong with predictors
// (klb_imageIO.cpp:2614-2682).
int decode_roi(const uint8_t* payload, size_t len, const klb_image_header& h, const uint32_t lb[5],
               const uint32_t ub[5], uint8_t* out, int threads, int family, DeviceDest* dd, lfm_decode_stats* hstats)
{
    PayloadSource src;
    src.mem = payload;
    src.len = len;
    return decode_roi(src, h, lb, ub, out, threads, family, dd, hstats);
}

int decode_roi(const PayloadSource& src, const klb_image_header& h, const uint32_t lb[5], const uint32_t ub[5],
               uint8_t* out, int threads, int family, DeviceDest* dd, lfm_decode_stats* hstats)
{
    const uint8_t* const payload = src.mem;
    const uint64_t len = src.len;
    if (!payload && src.fd < 0) return 3;
    const BlockGrid g(h);
    if (g.nblocks != h.Nb) return 3;
    const size_t bpp = h.getBytesPerPixel();
    if (!bpp) return 5;
    for (int d = 0; d < 5; ++d)
        if (ub[d] < lb[d] || ub[d] >= h.xyzct[d]) return 3;
    const int k = h.headerVersion & 0x7F;
    const bool video = (h.headerVersion >> 7) & 1;
    const bool predicted = bpp == 2 && k != 0;
    uint64_t b0[5], b1[5], o[5], n[5];
    for (int d = 0; d < 5; ++d) {
        uint64_t lo = lb[d];
        if (predicted && d < 2) lo = 0;
        if (predicted && video && d == 2 && (lo & 1)) lo -= 1;
        b0[d] = lo / g.bs[d];
        b1[d] = ub[d] / g.bs[d] + 1;
    }
    if (predicted && video)
        while (b0[2] > 0 && ((b0[2] * g.bs[2]) & 1)) --b0[2];
    klb_image_header sub(h);
    for (int d = 0; d < 5; ++d) {
        o[d] = b0[d] * g.bs[d];
        n[d] = std::min<uint64_t>(g.dims[d], b1[d] * g.bs[d]) - o[d];
        sub.xyzct[d] = (uint32_t)n[d];
    }
    const uint64_t cnt = (b1[0] - b0[0]) * (b1[1] - b0[1]) * (b1[2] - b0[2]) * (b1[3] - b0[3]) * (b1[4] - b0[4]);
    sub.resizeBlockOffset(cnt);
    std::vector<uint64_t> ids;
    ids.reserve(cnt);
    uint64_t total = 0;
    for (uint64_t t = b0[4]; t < b1[4]; ++t)
        for (uint64_t c = b0[3]; c < b1[3]; ++c)
            for (uint64_t z = b0[2]; z < b1[2]; ++z)
                for (uint64_t y = b0[1]; y < b1[1]; ++y)
                    for (uint64_t x = b0[0]; x < b1[0]; ++x) {
                        const uint64_t id = x + g.nb[0] * (y + g.nb[1] * (z + g.nb[2] * (c + g.nb[3] * t)));
                        const uint64_t e = h.getBlockOffset(id) + h.getBlockCompressedSizeBytes(id);
                        if (e > len) return 3;
                        total += h.getBlockCompressedSizeBytes(id);
                        sub.blockOffset[ids.size()] = total;
                        ids.push_back(id);
                    }
    // the region's streams: a run of consecutive blocks (whole t-volumes, a
    // z-range of whole frames) is read where it lies in the payload; anything
    // else is gathered into a buffer (no zero fill: every byte is copied)
    bool run = true;
    for (size_t i = 1; i < ids.size() && run; ++i)
        run = ids[i] == ids[i - 1] + 1 && h.getBlockOffset(ids[i]) == h.getBlockOffset(ids[i - 1]) +
                                                                         h.getBlockCompressedSizeBytes(ids[i - 1]);
    std::unique_ptr<uint8_t[]> gathered;
    const uint8_t* spay = (ids.empty() || !payload) ? payload : payload + h.getBlockOffset(ids[0]);
    if (!payload) {
        // the payload is a file: each run of blocks that lie one after the
        // other in it is fetched with one read into its place in the
        // sub-payload; the bytes between the runs are never read
        struct Run {
            uint64_t from, to, bytes;  // file offset, sub-payload offset
        };
        std::vector<Run> runs;
        for (size_t i = 0; i < ids.size(); ++i) {
            const uint64_t off = h.getBlockOffset(ids[i]), sz = h.getBlockCompressedSizeBytes(ids[i]);
            if (!runs.empty() && runs.back().from + runs.back().bytes == off) runs.back().bytes += sz;
            else runs.push_back(Run{off, sub.blockOffset[i] - sz, sz});
        }
        gathered.reset(new uint8_t[total ? total : 1]);
        std::atomic<bool> bad{false};
        parallel_for(runs.size(), threads, [&](uint64_t r) {
            if (!pread_all(src.fd, gathered.get() + runs[r].to, runs[r].bytes, src.base + runs[r].from)) bad.store(true);
        });
        if (bad.load()) return 3;
        if (src.fetched) *src.fetched += total;
        spay = gathered.get();
    } else if (!run) {
        gathered.reset(new uint8_t[total]);
        parallel_for(ids.size(), threads, [&](uint64_t i) {
            const uint64_t id = ids[i], sz = h.getBlockCompressedSizeBytes(id);
            std::memcpy(gathered.get() + (sub.blockOffset[i] - sz), payload + h.getBlockOffset(id), sz);
        });
        spay = gathered.get();
    }
    // a region that is exactly its blocks' box (e.g. whole t-volumes) is
    // decoded straight into `out`: no temporary image, no crop
    bool exact = true;
    for (int d = 0; d < 5; ++d) exact = exact && o[d] == lb[d] && n[d] == (uint64_t)ub[d] - lb[d] + 1;
    if (exact) return decode_payload(spay, total, sub, out, threads, family, dd, hstats);
    if (dd) {
        // the sub-image is decoded into a device buffer kept between calls and
        // the region copied out of it on the device, behind the caller's work
        DecodeBuffers& DB = decode_buffers();
        const size_t sbytes = sub.getImageSizeBytes();
        if (!DB.begin()) return 3;
        // (out of DB's hands until the crop is done: the decode below may release DB)
        DeviceBuffer roi = std::move(DB.roi);
        void* d_sub = DecodeBuffers::device(roi, sbytes);
        if (!d_sub) return 3;
        dd->stats.staged_bytes = sbytes;
        int rc = decode_payload(spay, total, sub, (uint8_t*)d_sub, threads, family, dd);
        if (!rc && !DB.begin()) rc = 3;  // (its streams again, had the decode released them)
        uint32_t sdims[5], slb[5], sn[5];
        for (int d = 0; d < 5; ++d) {
            sdims[d] = (uint32_t)n[d];
            slb[d] = (uint32_t)(lb[d] - o[d]);
            sn[d] = ub[d] - lb[d] + 1;
        }
        hipStream_t st = DB.st[0];
        if (!rc && (hipStreamWaitEvent(st, dd->after_caller, 0) != hipSuccess ||
                    lfm_hip_crop_region(d_sub, sdims, slb, sn, (uint32_t)bpp, out, st) != LFM_HIP_OK ||
                    hipStreamSynchronize(st) != hipSuccess))
            rc = 3;
        DB.roi = std::move(roi);
        release_unless_kept(DB);
        return rc;
    }
    std::unique_ptr<uint8_t[]> simg(new uint8_t[sub.getImageSizeBytes()]);  // (no zero fill: every byte is decoded)
    const int rc = decode_payload(spay, total, sub, simg.get(), threads, family, nullptr, hstats);
    if (rc) return rc;
    const size_t row = (size_t)(ub[0] - lb[0] + 1) * bpp;
    const uint64_t ny = (uint64_t)ub[1] - lb[1] + 1, nz = (uint64_t)ub[2] - lb[2] + 1, nc = (uint64_t)ub[3] - lb[3] + 1;
    const uint64_t nrows = ny * nz * nc * ((uint64_t)ub[4] - lb[4] + 1);
    parallel_for(nrows, threads, [&](uint64_t r) {  // output row r = ((t * nc + c) * nz + z) * ny + y
        const uint64_t y = lb[1] + r % ny, z = lb[2] + (r / ny) % nz, c = lb[3] + (r / ny / nz) % nc,
                       t = lb[4] + r / ny / nz / nc;
        const uint64_t e = (lb[0] - o[0]) +
                           n[0] * ((y - o[1]) + n[1] * ((z - o[2]) + n[2] * ((c - o[3]) + n[3] * (t - o[4]))));
        std::memcpy(out + r * row, simg.get() + e * bpp, row);
    });
    return 0;
}

int decode_memory_device(const uint8_t* buf, uint64_t len, const uint32_t* lb, const uint32_t* ub, void* d_out,
                         uint64_t out_bytes, int threads, lfm_decode_stats* stats)
{
    if (!buf || !d_out || (lb == nullptr) != (ub == nullptr)) return 3;
    klb_image_header h;
    int rc = h.parseHeader(buf, len);
    if (rc) return rc;
    const size_t hs = h.getSizeInBytes();
    PayloadSource src;
    src.mem = buf + hs;
    src.len = len - hs;
    return decode_source_device(src, h, lb, ub, d_out, out_bytes, threads, stats);
}

int decode_source_device(const PayloadSource& src, const klb_image_header& h, const uint32_t* lb, const uint32_t* ub,
                         void* d_out, uint64_t out_bytes, int threads, lfm_decode_stats* stats)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!d_out || (lb == nullptr) != (ub == nullptr) || (!src.mem && (src.fd < 0 || !lb))) return 3;
    int rc = 0;
    uint64_t need = h.getImageSizeBytes();
    if (lb) {
        need = h.getBytesPerPixel();  // the region in the file's own data type
        for (int d = 0; d < KLB_DATA_DIMS; ++d) {
            if (ub[d] < lb[d] || ub[d] >= h.xyzct[d]) return 3;
            need *= (uint64_t)(ub[d] - lb[d] + 1);
        }
    }
    if (!need || out_bytes < need || lfm_hip_device_count() <= 0) return 3;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_out) != hipSuccess) {
        (void)hipGetLastError();  // (a pointer the runtime has never seen)
        return 3;
    }
    if (attr.type != hipMemoryTypeDevice) return 3;
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) return 3;
    if (attr.device != cur && hipSetDevice(attr.device) != hipSuccess) return 3;
    DeviceDest dd;
    // what the caller has queued on the buffer's device (its null stream)
    // comes before the library's first write
    if (hipEventCreateWithFlags(&dd.after_caller, hipEventDisableTiming) != hipSuccess ||
        hipEventRecord(dd.after_caller, nullptr) != hipSuccess)
        rc = 3;
    if (!rc)
        rc = lb ? decode_roi(src, h, lb, ub, (uint8_t*)d_out, threads, current_family(), &dd)
                : decode_payload(src.mem, src.len, h, (uint8_t*)d_out, threads, current_family(), &dd);
    if (dd.after_caller) (void)hipEventDestroy(dd.after_caller);
    if (attr.device != cur) (void)hipSetDevice(cur);
    dd.stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (stats) *stats = dd.stats;
    return rc;
}

// the whole file in memory and its header parsed (3: it cannot be opened or read)
static int read_whole_file(const char* filename, std::vector<uint8_t>* buf, klb_image_header& h)
{
    FILE* f = std::fopen(filename, "rb");
    if (!f) {
        std::printf("ERROR: file %s could not be opened\n", filename);
        return 3;
    }
    std::fseek(f, 0, SEEK_END);
    const long size = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    buf->resize(size > 0 ? (size_t)size : 0);
    const size_t got = buf->empty() ? 0 : std::fread(buf->data(), 1, buf->size(), f);
    std::fclose(f);
    return got == buf->size() ? h.parseHeader(buf->data(), buf->size()) : 3;
}

int decode_file_roi(const char* filename, klb_image_header& h, const uint32_t lb[5], const uint32_t ub[5],
                    uint8_t* out, int threads)
{
    std::vector<uint8_t> buf;
    if (int rc = read_whole_file(filename, &buf, h)) return rc;
    const size_t hs = h.getSizeInBytes();
    return decode_roi(buf.data() + hs, buf.size() - hs, h, lb, ub, out, threads, current_family());
}

int decode_file(const char* filename, klb_image_header& h, std::vector<uint8_t>* img_out, uint8_t* img_into,
                int threads)
{
    std::vector<uint8_t> buf;
    if (int rc = read_whole_file(filename, &buf, h)) return rc;
    uint8_t* dst = img_into;
    if (!dst) {
        img_out->resize(h.getImageSizeBytes());
        dst = img_out->data();
    }
    return decode_image(buf.data(), buf.size(), h, dst, threads);
}

} // namespace lfm
