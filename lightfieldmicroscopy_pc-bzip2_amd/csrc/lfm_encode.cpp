// lfm_encode.cpp -- the Encoder: submit pipeline, upload pipe, predictor
// stage and the GPU bzip2 driver.
#include "lfm_engine.h"

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstring>
#include <numeric>

#include "lfm_hip.h"
#include "lfm_internal.h"

namespace lfm {

// --------------------------------------------------------------- encoder --
// GPU bzip2 for an encode: on unless disabled (LFM_GPU_BZIP2=0), not bzip2 or
// no device; a host image of at most kHostBz2Bytes goes to the host library
// (its predictor stage, if any, still runs on the GPU): a GPU batch costs
// about a millisecond of launches and host synchronisations, more than
// libbzip2 needs on the host threads for such an image (config 1's
// 101 x 151 page: 1.3 ms through the GPU batch, 0.18 ms on the host).
constexpr uint64_t kHostBz2Bytes = 1u << 20;
static bool use_gpu_bzip2(const klb_image_header& h, bool dev)
{
    if (!gpu_bzip2_enabled() || h.compressionType != BZIP2 || lfm_hip_device_count() <= 0) return false;
    return dev || h.getImageSizeBytes() > kHostBz2Bytes;
}

// the payload copy of gpu_compress: SDMA if possible, else hipMemcpyAsync
static bool payload_d2h(void* dst, const void* src, size_t n, hipStream_t st)
{
    if (hipStreamSynchronize(st) != hipSuccess) return false;
    if (sdma_d2h(dst, src, n)) return true;
    return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}

// the bzip2 level of a slab's encode (-1: the header's own rule).
// a z-slab that starts past frame 0 lies in a stack at least one nominal
// block deeper than its start, so the stack's nominal block keeps the
// requested depth even where the slab's own last layer is shallower
static int slab_level(const klb_image_header& h, const SlabSpec* slab)
{
    int level = slab ? slab->level : -1;
    if (level < 1 && slab && slab->z0 > 0 && h.getBytesPerPixel()) {
        klb_image_header nominal(h);
        for (int d = 0; d < KLB_DATA_DIMS; ++d)
            if (d != 2 && nominal.blockSize[d]) nominal.blockSize[d] = std::min(nominal.blockSize[d], h.xyzct[d]);
        if (nominal.blockSize[2] == 0) nominal.blockSize[2] = 1;
        level = bzip2_level(nominal);
    }
    return level;
}

// the reference writes these bytes (reproduced), but its temporal
// residual ((I - pred) + P) >> 1 drops a bit: no reader can restore
// the odd frames (lfm_Predictors_space.cu:114-177, _angle.cu:136-192)
static void warn_lossy_video(int fam)
{
    std::fprintf(stderr, "WARNING: video stack with the %s predictor family: the odd frames are coded with the "
                         "reference's lossy temporal residual and cannot be decoded exactly\n",
                 fam == 1 ? "angle" : "space");
}

Encoder::Encoder(int device) : device_(device) {}

Encoder::~Encoder()
{
    join_inflight();
    for (UploadPipe& u : up_) u.join();
    // (the buffers free themselves after this body, on the device set here;
    // a buffer exists only if its allocation succeeded, so an encoder that
    // never reached the GPU makes no HIP call)
    if (gpu_ready_) {
        for (UploadPipe& u : up_)
            for (hipEvent_t e : u.ev) (void)hipEventDestroy(e);
        if (up_stream_) (void)hipStreamDestroy(up_stream_);
        (void)hipSetDevice(device_);
        for (auto& set : bz_)
            for (BzSlot& sl : set)
                if (sl.stream) (void)hipStreamDestroy(sl.stream);
        if (ev0_) (void)hipEventDestroy(ev0_);
        if (ev1_) (void)hipEventDestroy(ev1_);
        if (caller_ev_) (void)hipEventDestroy(caller_ev_);
        if (stream_) (void)hipStreamDestroy(stream_);
        if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
    }
}

void Encoder::join_inflight()
{
    for (Inflight& f : fly_)
        if (f.th.joinable()) f.th.join();
}

void Encoder::Inflight::release()
{
    {
        std::lock_guard<std::mutex> lk(mu);
        released = true;
        mtf_done = true;
    }
    cv.notify_all();
}

void Encoder::Inflight::reach()
{
    {
        std::lock_guard<std::mutex> lk(mu);
        ++reached;
        if (need > 0 && reached >= need) released = mtf_done = true;
    }
    cv.notify_all();
}

void Encoder::Inflight::reach2()
{
    {
        std::lock_guard<std::mutex> lk(mu);
        ++reached2;
        if (need > 0 && reached2 >= need) mtf_done = true;
    }
    cv.notify_all();
}

void Encoder::Inflight::wait_mtf()
{
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return mtf_done || released; });
}

void Encoder::Inflight::wait_release()
{
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return released; });
}

int Encoder::submit(const void* img, bool dev, klb_image_header& h, int threads, const SlabSpec* slab,
                    uint64_t* ticket)
{
    static const SlabSpec whole;
    if (threads <= 0) threads = default_threads();
    if (int rc = after_caller(dev)) return rc;
    const int p = par_;
    Inflight& f = fly_[p];
    if (f.th.joinable()) f.th.join();  // the encode before last used this buffer set
    // Auto-selection (klb_imageIO.cpp:2316-2360) on the encoder's stream; the
    // request then becomes the forced 8 + k (video bit kept) for the
    // predictor stage, the bytes are the same.
    const bool gpu_bz = use_gpu_bzip2(h, dev);
    const int req0 = h.headerVersion & 0x7F;
    int pre_k = -1;
    float pre_ent[8] = {0};
    double pre_ms = 0.0;
    auto select_now = [&]() -> int {
        auto ts0 = clk::now();
        if (int rc = preselect(img, dev, h, slab ? *slab : whole, &pre_k, pre_ent)) return rc;
        pre_ms = ms_since(ts0);
        h.headerVersion = (uint8_t)((h.headerVersion & 0x80) | (8 + pre_k));
        return 0;
    };
    const bool pre = gpu_bz && req0 < NUM_PREDICTORS && h.getBytesPerPixel() == 2 && h.Nnum > 0;
    // a host stack starts its chunked upload (and the predictor on the chunks
    // that have landed) before the previous encode is released: the PCIe
    // upload runs under the previous encode's GPU bzip2.  A device stack, too,
    // runs its selection and predictor stage before that wait, beside the
    // previous encode's tail (its own buffer set; the selection then queues
    // behind that tail and the predictor kernel shares the CUs): config 3
    // pipelined 12 068-12 158 vs 11 797-11 872 Mpixel/s waiting for the
    // release first, same box (profiles/r04_ab_predict_early.txt)
    const bool host_early = gpu_bz && (upload_pipe_ok(dev, h) || dev);
    f.ticket = next_ticket_++;
    f.rc = 0;
    std::memset(&f.st, 0, sizeof(f.st));
    {
        std::lock_guard<std::mutex> lk(f.mu);
        f.reached = 0;
        f.reached2 = 0;
        f.need = 0;
        f.released = false;
        f.mtf_done = false;
    }
    if (ticket) *ticket = f.ticket;
    par_ ^= 1;
    auto fail = [&](int rc) {
        up_[p].join();
        f.rc = rc;
        f.release();
        return rc;
    };
    // LFM_SELECT_AT=2: a device stack's selection and predictor stage wait
    // until the previous encode is past its MTF stage, i.e. in its
    // latency-bound Huffman rounds, instead of sharing the CUs with its sorts
    static const int select_at = env_int("LFM_SELECT_AT", 0);
    if (select_at == 2 && dev && host_early) fly_[p ^ 1].wait_mtf();
    if (pre && host_early)
        if (int rc = select_now()) return fail(rc);
    if (pre_k >= 0) {
        f.st.select_ms = pre_ms;
        std::memcpy(f.st.entropy, pre_ent, sizeof(pre_ent));
    }
    auto t0 = clk::now();
    const int level = slab_level(h, slab);
    const uint8_t* dsym = nullptr;
    if (host_early) {
        if (int rc = normalize_header(h)) return fail(rc);
        if (int rc = predictor_stage(img, dev, h, nullptr, &dsym, &f.st, slab ? *slab : whole, p)) return fail(rc);
    }
    fly_[p ^ 1].wait_release();        // the previous encode is in its tail
    if (pre && !host_early) {
        if (int rc = select_now()) return fail(rc);
        f.st.select_ms = pre_ms;
        std::memcpy(f.st.entropy, pre_ent, sizeof(pre_ent));
    }
    if (!gpu_bz) {  // no GPU bzip2: the whole encode here
        MemSink sink(&mem_ring[p]);
        f.rc = encode_set(img, dev, h, sink, &f.st, threads, slab, p);
        f.release();
        return f.rc;
    }
    if (!host_early &&
        ((f.rc = normalize_header(h)) || (f.rc = predictor_stage(img, dev, h, nullptr, &dsym, &f.st, slab ? *slab : whole, p))))
        return fail(f.rc);
    if ((f.rc = ensure_gpu())) return fail(f.rc);
    if (dev && dsym == (const uint8_t*)img) {
        // no predictor stage (forced predictor 0, non-16-bit data): the symbols
        // ARE the caller's image, which the caller may release or refill once
        // submit returns -- the finisher must compress a copy of it
        const size_t bytes = h.getImageSizeBytes();
        void* copy = d_sym_[p].reserve(bytes);
        if (!copy || hipMemcpyAsync(copy, img, bytes, hipMemcpyDeviceToDevice, stream_) != hipSuccess ||
            hipStreamSynchronize(stream_) != hipSuccess) {
            f.rc = 3;
            f.release();
            return f.rc;
        }
        dsym = (const uint8_t*)copy;
    }
    auto hh = std::make_shared<klb_image_header>(h);
    f.th = std::thread([this, &f, hh, dsym, level, p, t0]() {
        (void)hipSetDevice(device_);
        MemSink sink(&mem_ring[p]);
        auto tc = clk::now();
        f.rc = gpu_compress(dsym, *hh, sink, &f.st, level, p, &f);
        f.st.compress_ms = ms_since(tc);
        f.st.total_ms = ms_since(t0);
        f.st.header_version = hh->headerVersion;
        f.st.chosen = hh->headerVersion & 0x7F;
        f.st.out_bytes = hh->getCompressedFileSizeInBytes();
        f.release();  // in case the release stage was never reached (host paths)
    });
    UploadPipe& up = up_[p];
    if (up.active) {
        // the caller may release a host stack once submit returns: wait for
        // its upload (the finisher's GPU bzip2 already runs on the chunks)
        up.join();
        f.st.h2d_ms += up.h2d_ms;
        f.st.predict_ms += up.predict_ms;
        if (up.rc) return up.rc;  // the finisher's batches fail too; wait() reports it
    }
    return 0;
}

int Encoder::wait(uint64_t ticket, const PinnedBuffer** out, lfm_encode_stats* st)
{
    for (int p = 0; p < 2; ++p) {
        Inflight& f = fly_[p];
        if (f.ticket != ticket || ticket == 0) continue;
        if (f.th.joinable()) f.th.join();
        last_counts = counts_[p];
        if (out) *out = &mem_ring[p];
        if (st) *st = f.st;
        return f.rc;
    }
    return kErrUnknownTicket;  // never submitted, already recycled (two submits ago), or 0
}

int Encoder::ensure_gpu()
{
    if (gpu_ready_) return 0;
    int n = lfm_hip_device_count();
    if (n <= 0) {
        std::printf("ERROR: the LFM predictor stage needs a HIP GPU (gfx950) and none is visible\n");
        return kErrNoGpu;
    }
    if (device_ < 0) {
        if (hipGetDevice(&device_) != hipSuccess) device_ = 0;
    }
    if (device_ >= n || hipSetDevice(device_) != hipSuccess) return kErrNoGpu;
    // the predictor stage's stream (a high-priority one measured 10 % slower
    // end to end: it took a hardware queue from the bzip2 slots)
    if (hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking) != hipSuccess) return kErrNoGpu;
    // the first buffer set's GPU bzip2 slot streams are created right after
    // the predictor stream, so each lands on a hardware queue of its own
    // (GPU_MAX_HW_QUEUES is 4, the null stream holding one): streams created
    // later share queues, and two slots sharing one run their batches in
    // series (measured: the upload pipe's extra stream, created first, put
    // both slots on one queue, +19 ms per 2 GiB encode)
    for (int k = 0; k < bz_slot_count(); ++k)
        if (hipStreamCreateWithFlags(&bz_[0][k].stream, hipStreamNonBlocking) != hipSuccess) return kErrNoGpu;
    (void)hipEventCreate(&ev0_);
    (void)hipEventCreate(&ev1_);
    gpu_ready_ = true;
    return 0;
}

// ---------------------------------------------------------- upload pipe --
int Encoder::UploadPipe::wait_frames(uint64_t f_end, hipStream_t st)
{
    std::unique_lock<std::mutex> lk(mu);
    if (!active) return 0;
    size_t c = (size_t)(std::lower_bound(end.begin(), end.begin() + nchunks, f_end) - end.begin());
    if (c >= nchunks) c = nchunks - 1;
    cv.wait(lk, [&] { return recorded > c || rc != 0; });
    if (rc) return 3;
    return hipStreamWaitEvent(st, ev[3 * c + 2], 0) == hipSuccess ? 0 : 3;
}

void Encoder::UploadPipe::join()
{
    if (th.joinable()) th.join();
    std::lock_guard<std::mutex> lk(mu);
    active = false;
}

int Encoder::bz_slot_count()
{
    static const int n = [] {
        const int v = env_int("LFM_BZ2_SLOTS", 0);
        return v > 0 ? std::min(v, (int)kBzSlots) : 2;
    }();
    return n;
}

bool Encoder::upload_pipe_ok(bool dev, const klb_image_header& h) const
{
    static const bool on = env_int("LFM_H2D_PIPE", 1) != 0;
    return on && !dev && h.getBytesPerPixel() == 2 && h.Nnum > 0;
}

// The uploader's copies on an SDMA engine (LFM_H2D_SDMA=0: hipMemcpyAsync, whose blit
// kernel measured ~25 ms slower for the GPU bzip2 running beside a 2 GiB
// upload); a pinned (HSA-allocated) source goes straight to the engine,
// a pageable one through two pinned staging chunks (host copy of one
// overlapping the engine's copy of the other).  Returns the HSA CPU agent
// with the signals (and, for a pageable source, the staging chunks of cbytes)
// ready, or null: the hipMemcpyAsync loop.
static const hsa_agent_t* upload_sdma_setup(const void* d_in, const void* img, size_t cbytes, SdmaPair& sdma,
                                            HostBuffer stage[2], hsa_agent_t* gpu, bool* direct)
{
    static const bool sdma_on = env_int("LFM_H2D_SDMA", 1) != 0;
    const hsa_agent_t* cpu = sdma_on ? hsa_cpu_agent() : nullptr;
    if (!cpu || !hsa_owner(d_in, gpu)) return nullptr;
    hsa_agent_t src_owner;
    *direct = hsa_owner(img, &src_owner);
    if (!sdma.create()) return nullptr;
    if (!*direct && (!stage[0].reserve(cbytes) || !stage[1].reserve(cbytes))) return nullptr;
    return cpu;
}

// Upload the host stack in chunks of whole frames through a ring of device
// slots and predict each chunk (forced predictor k >= 1) into the set's
// symbol buffer as it lands (see UploadPipe).  Returns once the uploader
// thread runs; UploadPipe::join waits for it (the host image is read until
// then).  The chunk's first frame takes its temporal predecessor from the
// previous chunk's slot (or the slab's prev frame), which the ring keeps
// until the chunk after it has been predicted.
int Encoder::start_upload(const void* img, klb_image_header& h, const SlabSpec& slab, int k, int set)
{
    UploadPipe& up = up_[set];
    up.join();
    const uint64_t W = h.xyzct[0], H = h.xyzct[1], Z = h.xyzct[2];
    const uint64_t V = (uint64_t)h.xyzct[3] * h.xyzct[4];
    const size_t fpx = W * H, fs = fpx * 2;
    const int video = (h.headerVersion >> 7) & 1;
    // (<= 0 means the default)
    static const long chunk_mb = env_long("LFM_H2D_CHUNK_MB", 0), ring_mb = env_long("LFM_H2D_RING_MB", 0);
    static const size_t chunk_target = (size_t)(chunk_mb > 0 ? chunk_mb : 32) << 20;
    static const size_t ring_target = (size_t)(ring_mb > 0 ? ring_mb : 1024) << 20;
    // >= chunk_target bytes of whole frames; an even count on video stacks
    // (a spatial and its temporal frame go through the pair kernel together)
    uint64_t cz = std::max<uint64_t>(1, (chunk_target + fs - 1) / fs);
    if (video && (cz & 1)) ++cz;
    cz = std::min<uint64_t>(cz, Z);
    const uint64_t per_vol = (Z + cz - 1) / cz, nch = V * per_vol;
    const size_t cbytes = cz * fs;
    // at least 3 slots: the SDMA loop issues copy c before chunk c - 1 is
    // predicted, and slot c % nslot must no longer be read by chunk
    // c - nslot + 1 (its last frame is that chunk's temporal predecessor), so
    // that chunk's predictor must already be issued when copy c waits for it
    const uint64_t nslot = std::min<uint64_t>(nch, std::max<uint64_t>(3, ring_target / cbytes));
    uint16_t* const d_in = (uint16_t*)d_in_.reserve(nslot * cbytes);
    uint16_t* const d_sym = (uint16_t*)d_sym_[set].reserve(V * Z * fs);
    if (!d_in || !d_sym) return 3;
    while (up.ev.size() < 3 * nch) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return 3;
        up.ev.push_back(e);
    }
    const uint16_t* d_prev = nullptr;
    if (slab.z0 > 0 && video && (slab.z0 & 1)) {
        if (V != 1 || !slab.prev) return 3;
        d_prev = (const uint16_t*)d_prev_.reserve(fs);
        if (!d_prev) return 3;
        if (hipMemcpyAsync(d_prev_.get(), slab.prev, fs, hipMemcpyHostToDevice, stream_) != hipSuccess) return 3;
    }
    up.end.assign(nch, 0);
    for (uint64_t c = 0; c < nch; ++c) up.end[c] = (c / per_vol) * Z + std::min<uint64_t>(Z, (c % per_vol + 1) * cz);
    {
        std::lock_guard<std::mutex> lk(up.mu);
        up.nchunks = nch;
        up.recorded = 0;
        up.rc = 0;
        up.active = true;
        up.h2d_ms = up.predict_ms = 0.0;
    }
    const int fam = current_family(), T = h.Nnum;
    const uint32_t z0 = slab.z0;
    const uint8_t* const src = (const uint8_t*)img;
    hsa_agent_t gpu{};
    bool direct = false;
    const hsa_agent_t* cpu = upload_sdma_setup(d_in, img, cbytes, up.sdma, up.stage, &gpu, &direct);
    // (the stream of the hipMemcpyAsync copies only: SDMA copies need none)
    if (!cpu && !up_stream_ && hipStreamCreateWithFlags(&up_stream_, hipStreamNonBlocking) != hipSuccess) return 3;
    const int cthreads = default_threads();
    up.th = std::thread([=, &up]() {
        (void)hipSetDevice(device_);
        auto t0 = clk::now();
        int rc = 0;
        auto predict = [&](uint64_t c, uint16_t* slot) -> int {
            const uint64_t v = c / per_vol, za = (c % per_vol) * cz, zb = std::min<uint64_t>(Z, za + cz);
            hipEvent_t* e = &up.ev[3 * c];
            const uint16_t* prev = nullptr;
            if (video) prev = za > 0 ? d_in + ((c - 1) % nslot) * cz * fpx + (cz - 1) * fpx : d_prev;
            (void)hipEventRecord(e[1], stream_);
            if (lfm_hip_predict(slot, prev, d_sym + (v * Z + za) * fpx, (int)W, (int)H, (int)(zb - za), T, fam, k,
                                video, (int)(z0 + za), stream_) != LFM_HIP_OK ||
                hipEventRecord(e[2], stream_) != hipSuccess)
                return 3;
            {
                std::lock_guard<std::mutex> lk(up.mu);
                up.recorded = c + 1;
            }
            up.cv.notify_all();
            return 0;
        };
        uint8_t* const stage[2] = {(uint8_t*)up.stage[0].get(), (uint8_t*)up.stage[1].get()};
        // SDMA: copy c is issued before chunk c - 1 (copied) is predicted,
        // so the engine always has the next chunk while a chunk is predicted
        for (uint64_t c = 0; cpu && c < nch && !rc; ++c) {
            const uint64_t v = c / per_vol, za = (c % per_vol) * cz, zb = std::min<uint64_t>(Z, za + cz);
            const size_t len = (zb - za) * fs;
            const int b = (int)(c & 1);
            uint16_t* slot = d_in + (c % nslot) * cz * fpx;
            // the slot's last readers (chunk c - nslot and the chunk after
            // it, which reads its last frame) are predicted
            if (c >= nslot && hipEventSynchronize(up.ev[3 * (c - nslot + 1) + 2]) != hipSuccess) rc = 3;
            if (!rc && c >= 2 && !up.sdma.wait(b)) rc = 3;  // (chunk c - 2's copy: staging chunk b is free)
            const uint8_t* from = src + (v * Z + za) * fs;
            if (!rc && !direct) {
                par_memcpy(stage[b], from, len, cthreads);
                from = stage[b];
            }
            if (!rc && !up.sdma.issue(b, slot, gpu, from, *cpu, len)) rc = 3;
            if (!rc && c >= 1) {
                if (!up.sdma.wait((int)((c - 1) & 1))) rc = 3;
                else rc = predict(c - 1, d_in + ((c - 1) % nslot) * cz * fpx);
            }
        }
        if (cpu && !rc) {
            if (!up.sdma.wait((int)((nch - 1) & 1))) rc = 3;
            else rc = predict(nch - 1, d_in + ((nch - 1) % nslot) * cz * fpx);
        }
        if (cpu) {  // no copy still reads the caller's image or a staging chunk
            for (int b = 0; b < 2; ++b) (void)up.sdma.wait(b);
        }
        for (uint64_t c = 0; !cpu && c < nch && !rc; ++c) {
            const uint64_t v = c / per_vol, za = (c % per_vol) * cz, zb = std::min<uint64_t>(Z, za + cz);
            uint16_t* slot = d_in + (c % nslot) * cz * fpx;
            hipEvent_t* e = &up.ev[3 * c];
            // the slot was chunk c - nslot's; chunk c - nslot + 1 (predicted
            // after it) also reads that slot's last frame as its temporal prev
            if (c >= nslot && hipStreamWaitEvent(up_stream_, up.ev[3 * (c - nslot + 1) + 2], 0) != hipSuccess) rc = 3;
            if (!rc && hipMemcpyAsync(slot, src + (v * Z + za) * fs, (zb - za) * fs, hipMemcpyHostToDevice,
                                      up_stream_) != hipSuccess)
                rc = 3;
            if (!rc && (hipEventRecord(e[0], up_stream_) != hipSuccess ||
                        hipStreamWaitEvent(stream_, e[0], 0) != hipSuccess))
                rc = 3;
            if (!rc) rc = predict(c, slot);
            if (rc) {  // (this loop publishes a failure per chunk, the SDMA loop at the end)
                {
                    std::lock_guard<std::mutex> lk(up.mu);
                    up.rc = rc;
                }
                up.cv.notify_all();
            }
        }
        // the host image is no longer read once the copies are done
        if (!cpu && hipStreamSynchronize(up_stream_) != hipSuccess) rc = 3;
        const double h2d = ms_since(t0);
        double pms = 0.0;
        if (!rc && hipEventSynchronize(up.ev[3 * (nch - 1) + 2]) == hipSuccess) {
            for (uint64_t c = 0; c < nch; ++c) {
                float ms = 0.f;
                if (hipEventElapsedTime(&ms, up.ev[3 * c + 1], up.ev[3 * c + 2]) == hipSuccess) pms += ms;
            }
        }
        {
            std::lock_guard<std::mutex> lk(up.mu);
            if (rc) up.rc = rc;
            up.h2d_ms = h2d;
            up.predict_ms = pms;
        }
        up.cv.notify_all();
    });
    return 0;
}

int Encoder::predictor_stage(const void* img, bool dev, klb_image_header& h, const uint8_t** sym,
                             const uint8_t** dsym, lfm_encode_stats* st, const SlabSpec& slab, int set)
{
    DeviceBuffer& d_sym_ = this->d_sym_[set];
    HostBuffer& h_sym_ = this->h_sym_[set];
    // dsym != nullptr: the caller compresses on the GPU -- leave the symbols
    // of every volume in device memory (*dsym) and skip the host copy.
    const bool keep = dsym != nullptr;
    const size_t bpp = h.getBytesPerPixel();
    const uint8_t hv = h.headerVersion;
    const int req = hv & 0x7F;
    const int video = (hv >> 7) & 1;
    const uint64_t W = h.xyzct[0], H = h.xyzct[1], Z = h.xyzct[2];
    const uint64_t V = (uint64_t)h.xyzct[3] * h.xyzct[4];
    const uint64_t vol = W * H * Z;
    const uint64_t total_bytes = h.getImageSizeBytes();
    const bool autosel = req < NUM_PREDICTORS;
    int k = autosel ? 0 : (hv & 0x77);  // `headerVersion & 0x7F - 8` parses as & 0x77 (klb_imageIO.cpp:2380)
    if (st) st->chosen = 0;
    if (sym) *sym = nullptr;
    if (dsym) *dsym = nullptr;

    // one copy on stream_, waited for, its time added to the stats (h2d_ms / d2h_ms)
    auto timed_copy = [&](void* dst, const void* src, size_t bytes, hipMemcpyKind kind) -> bool {
        auto t0 = clk::now();
        if (hipMemcpyAsync(dst, src, bytes, kind, stream_) != hipSuccess || hipStreamSynchronize(stream_) != hipSuccess)
            return false;
        if (st) (kind == hipMemcpyHostToDevice ? st->h2d_ms : st->d2h_ms) += ms_since(t0);
        return true;
    };
    auto host_symbols_from_device = [&](const void* d, size_t bytes) -> int {
        void* hs = h_sym_.reserve(bytes);
        if (!hs || !timed_copy(hs, d, bytes, hipMemcpyDeviceToHost)) return 3;
        *sym = (const uint8_t*)hs;
        return 0;
    };

    // data without a 16-bit sample: no predictor stage (the reference would
    // reinterpret the buffer as uint16, klb_imageIO.cpp:2365)
    const bool predictable = (bpp == 2) && h.Nnum > 0;
    if (!predictable || (!autosel && k == 0)) {
        if (!autosel && k > 7) return kErrBadPredictor;
        h.headerVersion = (uint8_t)(hv & 0x80);
        if (keep) {  // the raw image is the symbol stream
            if (dev) {
                *dsym = (const uint8_t*)img;
                return 0;
            }
            void* ds = d_sym_.reserve(total_bytes);
            if (!ds || !timed_copy(ds, img, total_bytes, hipMemcpyHostToDevice)) return 3;
            *dsym = (const uint8_t*)ds;
            return 0;
        }
        if (!dev) {
            *sym = (const uint8_t*)img;
            return 0;
        }
        return host_symbols_from_device(img, total_bytes);
    }
    if (!autosel && k > 7) {
        std::printf("ERROR: predictor request %d is not valid (use 0-7 for auto, 8-15 for predictor 0-7)\n", req);
        return kErrBadPredictor;
    }
    if (int rc = ensure_gpu()) return rc;
    (void)hipSetDevice(device_);
    const int fam = current_family();
    const int T = h.Nnum;

    if (keep && upload_pipe_ok(dev, h)) {
        // host stack, GPU bzip2: chunked upload overlapped with the predictor
        // and the compression (start_upload); selection first, on frame 0 of
        // volume (0, 0) or the stack's frame 0 handed in for a slab
        if (autosel) {
            auto t0 = clk::now();
            const void* frame = slab.select_frame ? slab.select_frame : (slab.z0 > 0 ? nullptr : img);
            if (!frame) return 3;  // a slab's own frame 0 is not the stack's
            float ent[8];
            if (int rc = select_host_frame(frame, (int)W, (int)H, T, fam, &k, ent)) return rc;
            if (st) {
                st->select_ms += ms_since(t0);
                std::memcpy(st->entropy, ent, sizeof(ent));
            }
        }
        if (int rc = start_upload(img, h, slab, k, set)) {
            up_[set].join();
            return rc;
        }
        h.headerVersion = (uint8_t)((hv & 0x80) | k);
        if (st) st->chosen = k;
        if (video && fam != 0 && Z > 1) warn_lossy_video(fam);
        *dsym = (const uint8_t*)d_sym_.get();
        return 0;
    }

    const uint16_t* d_img = (const uint16_t*)img;
    // slab of a larger stack: its first frame may need the raw frame z0 - 1
    const uint16_t* d_prev = nullptr;
    if (slab.z0 > 0) {
        if (V != 1) return 3;  // slabs are z ranges of a single (c, t) volume
        if (video && (slab.z0 & 1)) {
            if (!slab.prev) return 3;
            if (dev) {
                d_prev = (const uint16_t*)slab.prev;
            } else {
                d_prev = (const uint16_t*)d_prev_.reserve(W * H * 2);
                if (!d_prev) return 3;
                if (hipMemcpyAsync(d_prev_.get(), slab.prev, W * H * 2, hipMemcpyHostToDevice, stream_) != hipSuccess)
                    return 3;
            }
        }
    }
    // every volume's symbols stay on the device when they are needed there
    // (device input, or GPU compression); otherwise one volume at a time
    const bool all_on_device = dev || keep;
    if (!dev && !d_in_.reserve(vol * 2)) return 3;
    uint16_t* const d_sym = (uint16_t*)d_sym_.reserve((all_on_device ? V * vol : vol) * 2);
    if (!d_sym) return 3;
    uint8_t* const h_sym = keep ? nullptr : (uint8_t*)h_sym_.reserve(total_bytes);
    if (!keep && !h_sym) return 3;
    float pred_ms_total = 0.f;
    for (uint64_t v = 0; v < V; ++v) {
        const uint16_t* src;
        if (dev) {
            src = d_img + v * vol;
        } else {
            if (!timed_copy(d_in_.get(), (const uint16_t*)img + v * vol, vol * 2, hipMemcpyHostToDevice)) return 3;
            src = (const uint16_t*)d_in_.get();
        }
        if (v == 0 && autosel) {
            // selection on frame 0 of volume (c=0, t=0) (klb_imageIO.cpp:2316-2360),
            // or on the whole stack's frame 0 handed in for a slab
            auto t0 = clk::now();
            const size_t need = lfm_hip_select_workspace_bytes((int)W, (int)H);
            void* ws = d_ws_.reserve(need);
            if (!ws) return 3;
            const uint16_t* sel = src;
            if (slab.select_frame) {
                if (dev) {
                    sel = (const uint16_t*)slab.select_frame;
                } else {
                    sel = (const uint16_t*)d_sel_.reserve(W * H * 2);
                    if (!sel) return 3;
                    if (hipMemcpyAsync(d_sel_.get(), slab.select_frame, W * H * 2, hipMemcpyHostToDevice, stream_) !=
                        hipSuccess)
                        return 3;
                }
            } else if (slab.z0 > 0) {
                return 3;  // a slab's own frame 0 is not the stack's: the caller must hand that frame in
            }
            float ent[8];
            int chosen = 0;
            int rc = lfm_hip_select(sel, (int)W, (int)H, T, fam, ent, &chosen, ws, stream_);
            if (rc != LFM_HIP_OK) return 3;
            k = chosen;
            if (st) {
                st->select_ms += ms_since(t0);
                std::memcpy(st->entropy, ent, sizeof(ent));
            }
        }
        uint16_t* dst = d_sym + (all_on_device ? v * vol : 0);
        (void)hipEventRecord(ev0_, stream_);
        int rc = lfm_hip_predict(src, d_prev, dst, (int)W, (int)H, (int)Z, T, fam, k, video, (int)slab.z0, stream_);
        (void)hipEventRecord(ev1_, stream_);
        if (rc != LFM_HIP_OK) return 3;
        if (!all_on_device) {
            if (!timed_copy(h_sym + v * vol * 2, dst, vol * 2, hipMemcpyDeviceToHost)) return 3;
        } else if (hipEventSynchronize(ev1_) != hipSuccess) {
            return 3;
        }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev0_, ev1_);
        pred_ms_total += ms;
    }
    if (st) st->predict_ms += pred_ms_total;
    h.headerVersion = (uint8_t)((hv & 0x80) | k);
    if (st) st->chosen = k;
    if (video && fam != 0 && k != 0 && Z > 1) warn_lossy_video(fam);
    if (keep) {
        *dsym = (const uint8_t*)d_sym;
        return 0;
    }
    if (dev && !timed_copy(h_sym, d_sym, total_bytes, hipMemcpyDeviceToHost)) return 3;
    *sym = h_sym;
    return 0;
}

namespace {
std::atomic<int>& multiblock_flag()
{
    static std::atomic<int> on{env_int("LFM_BZ2_MULTIBLOCK", 1) != 0 ? 1 : 0};
    return on;
}
} // namespace

int bzip2_multiblock() { return multiblock_flag().load(); }
int set_bzip2_multiblock(int on) { return multiblock_flag().exchange(on ? 1 : 0); }

// GPU bzip2 of every block (lfm_bzip2.hip), streams batched to bound the
// workspace; streams the device hands back (periodic blocks; with
// bzip2_multiblock() off also every stream libbzip2 cuts into several blocks)
// are compressed by libbz2 here.  Same bytes either way.
int Encoder::gpu_compress(const uint8_t* d_sym, klb_image_header& h, Sink& sink, lfm_encode_stats* st, int level,
                          int set, Inflight* fly)
{
    HostBuffer& h_sym_ = this->h_sym_[set];
    BzSlot* bz_ = this->bz_[set];
    const BlockGrid g(h);
    const uint64_t nblocks = g.nblocks;
    h.resizeBlockOffset(nblocks);
    const size_t bpp = h.getBytesPerPixel();
    const uint32_t block_bytes = h.getBlockSizeBytes();
    if (level < 1) level = bzip2_level(h);
    const size_t out_cap = bz::out_cap(block_bytes), rle_cap = bz::rle_cap(block_bytes);
    // Batches run in a pipeline of kBzSlots HIP streams (one host thread
    // each): one batch's latency-bound stages (MTF, Huffman tables, the
    // host-synchronised doubling rounds) overlap another batch's sorts.  The
    // workspace budget (env LFM_BZ2_GPU_BUDGET_MB, default 48 GiB) is split
    // between the slots.
    static const long budget_mb = env_long("LFM_BZ2_GPU_BUDGET_MB", 0);  // (<= 0 means the default)
    static const size_t budget = (size_t)(budget_mb > 0 ? budget_mb : 48 * 1024) << 20;
    // several bzip2 blocks per stream on the device: a stream takes one slot
    // of the batch per block libbzip2 could cut (one for the default geometry:
    // then both entry pairs are the same layout and launches)
    const bool multi = bzip2_multiblock() != 0;
    auto ws_bytes = [&](uint32_t n) {
        return multi ? lfm_hip_bzip2_workspace_bytes_multi(n, block_bytes, (uint32_t)level)
                     : lfm_hip_bzip2_workspace_bytes(n, block_bytes);
    };
    const size_t per_stream = ws_bytes(1) + out_cap;
    // one batch per slot (smaller batches, so the in-order writer's copies
    // overlap later batches' kernels, measured slower: the latency-bound
    // stages cost per batch)
    const int slots = bz_slot_count();
    const uint64_t nway = slots;
    uint64_t batch = std::max<uint64_t>(1, std::min<uint64_t>((nblocks + nway - 1) / nway,
                                                                budget / slots / per_stream));
    // the slots' texts are indexed in 32 bits
    batch = std::min<uint64_t>(batch, multi ? std::max<uint32_t>(1, lfm_hip_bzip2_max_count_multi(block_bytes, (uint32_t)level))
                                            : ((1ull << 32) - 1) / rle_cap);
    const uint64_t nbatch = (nblocks + batch - 1) / batch;
    const int nslots = (int)std::min<uint64_t>(slots, nbatch);
    const size_t ws = ws_bytes((uint32_t)batch);
    std::vector<uint64_t> gpu_blocks(nslots, 0);  // per slot, summed over its batches
    for (int k = 0; k < nslots; ++k) {
        BzSlot& sl = bz_[k];
        if (!sl.stream && hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess) return 3;
        if (!sl.d_ws.reserve(ws) || !sl.d_out.reserve(batch * out_cap) || !sl.h_out.reserve(batch * out_cap)) return 3;
    }
    uint32_t dims[5], bs[5];
    for (int d = 0; d < 5; ++d) {
        dims[d] = h.xyzct[d];
        bs[d] = h.blockSize[d];
    }
    // per batch: sizes / flags, and the ready / consumed hand-shake with the
    // in-order writer below (slot k reuses its buffers for batch b + kBzSlots)
    std::vector<std::vector<uint64_t>> sizes(nbatch);
    std::vector<std::vector<uint32_t>> flags(nbatch);
    std::vector<int> state(nbatch, 0);  // 0 pending, 1 ready, 2 consumed, -1 failed
    // a sink backed by pinned memory takes each batch's payload straight from
    // the device, in order, at its final offset (no host copy of the blocks)
    const bool direct = sink.direct_capable();
    std::vector<char> staged(nbatch, 1);
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<bool> abort_all{false};
    std::vector<double> d2h(nslots, 0.0);
    std::vector<std::array<double, 5>> stage_ms(nslots);  // per slot, summed over its batches
    for (auto& a : stage_ms) a.fill(0.0);
    // pipelined encodes: the next submit starts once every batch of the last
    // round has run its kernels (releasing it after the BWT or the MTF of
    // those batches measured equal or slower: the next stack's kernels slow
    // this one's latency-bound Huffman chains as much as they gain; staggering
    // the two slots measured slower too, their latency-bound stages overlap
    // each other in lockstep)
    // host stack still uploading (start_upload): a batch waits for the chunks
    // holding its last block (blocks run x -> y -> z -> c -> t, so that block
    // reaches furthest into the flattened (t, c, z) frame order)
    UploadPipe* up = nullptr;
    {
        std::lock_guard<std::mutex> lk(up_[set].mu);
        if (up_[set].active) up = &up_[set];
    }
    auto frames_needed = [&](uint64_t last_block) -> uint64_t {
        uint64_t o[5], sz[5];
        g.block(last_block, o, sz);
        return ((o[4] + sz[4] - 1) * h.xyzct[3] + (o[3] + sz[3] - 1)) * (uint64_t)h.xyzct[2] + o[2] + sz[2];
    };
    if (fly) {
        std::lock_guard<std::mutex> lk(fly->mu);
        fly->need = (int)std::min<uint64_t>(nslots, nbatch);
    }
    auto payload_bytes = [&](uint64_t b) { return std::accumulate(sizes[b].begin(), sizes[b].end(), (uint64_t)0); };
    auto worker = [&](int k) {
        (void)hipSetDevice(device_);
        BzSlot& sl = bz_[k];
        for (uint64_t b = k; b < nbatch; b += nslots) {
            if (b >= (uint64_t)nslots) {  // wait until the writer consumed batch b - nslots
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return state[b - nslots] != 1 || abort_all.load(); });
                if (abort_all.load() || state[b - nslots] < 0) break;
            }
            const uint64_t b0 = b * batch;
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, nblocks - b0);
            sizes[b].assign(cnt, 0);
            flags[b].assign(cnt, 0);
            if (up && up->wait_frames(frames_needed(b0 + cnt - 1), sl.stream)) {
                std::lock_guard<std::mutex> lk(mu);
                state[b] = -1;
                cv.notify_all();
                break;
            }
            // the slot's last batch releases the next encode once its Huffman
            // tables are done (stage hook 3), so the next encode's first
            // kernels queue while this one's emission and copies finish
            const bool last = fly && b + nslots >= nbatch;
            struct ReachOnce {
                Inflight* f;
                bool done;
            } ro{fly, false};
            // (measured +2.6 % end to end against the release after the
            // batch's last copy: the ~0.45 ms host turnaround between two
            // encodes' kernels is hidden, profiles/r05_ab_early_release.jsonl)
            if (last)
                lfm_hip_bzip2_set_stage_hook(
                    [](void* c, int stage) {
                        auto* r = (ReachOnce*)c;
                        if (stage == 2) r->f->reach2();
                        if (stage == 3 && !r->done) {
                            r->done = true;
                            r->f->reach();
                        }
                    },
                    &ro);
            int ok = (multi ? lfm_hip_bzip2_blocks_multi : lfm_hip_bzip2_blocks)(
                         d_sym, dims, bs, (uint32_t)bpp, (uint32_t)b0, cnt, (uint32_t)level, sl.d_ws.get(), ws,
                         sl.d_out.get(), sizes[b].data(), flags[b].data(), sl.stream) == LFM_HIP_OK;
            if (ok) gpu_blocks[k] += lfm_hip_bzip2_last_blocks();
            if (last) {
                lfm_hip_bzip2_set_stage_hook(nullptr, nullptr);
                if (!ro.done) fly->reach();
            }
            float sm[5];
            if (ok && lfm_hip_bzip2_last_stage_ms(sm) == 0)
                for (int i = 0; i < 5; ++i) stage_ms[k][i] += sm[i];
            bool any_flag = false;
            for (uint32_t i = 0; i < cnt; ++i) any_flag |= flags[b][i] != 0;
            staged[b] = !direct || any_flag;
            if (ok && staged[b]) {  // through the pinned staging buffer (the writer copies block by block)
                auto t0 = clk::now();
                ok = payload_d2h(sl.h_out.get(), sl.d_out.get(), payload_bytes(b), sl.stream);
                d2h[k] += ms_since(t0);
            }
            {
                std::lock_guard<std::mutex> lk(mu);
                state[b] = ok ? 1 : -1;
            }
            cv.notify_all();
            if (!ok) break;
        }
    };
    std::vector<std::thread> pool;
    for (int k = 0; k < nslots; ++k) pool.emplace_back(worker, k);

    const uint8_t* h_all = nullptr;  // host copy of the symbols, only if a stream needs the host library
    std::vector<uint8_t> in(block_bytes), out((size_t)std::ceil((float)block_bytes * 2.0f + 50.0f));
    int rc = sink.begin(h);
    if (direct) sink.reserve_hint(h.getSizeInBytes() + nblocks * out_cap);
    uint64_t offset = 0, host_streams = 0;
    for (uint64_t b = 0; b < nbatch && !rc; ++b) {
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return state[b] != 0; });
            if (state[b] < 0) rc = 3;
        }
        if (rc) break;
        const uint64_t b0 = b * batch;
        const uint32_t cnt = (uint32_t)sizes[b].size();
        if (!staged[b]) {
            const uint64_t tot = payload_bytes(b);
            BzSlot& sl = bz_[b % nslots];
            uint8_t* dst = sink.direct(tot);
            if (!dst) {
                rc = 3;
            } else {
                auto t0 = clk::now();
                if (!payload_d2h(dst, sl.d_out.get(), tot, sl.stream)) rc = 3;
                if (st) st->d2h_ms += ms_since(t0);
            }
            for (uint32_t i = 0; i < cnt; ++i) {
                offset += sizes[b][i];
                h.blockOffset[b0 + i] = offset;
            }
        }
        const uint8_t* p = (const uint8_t*)bz_[b % nslots].h_out.get();
        for (uint32_t i = 0; i < cnt && !rc && staged[b]; ++i) {
            if (flags[b][i]) {
                if (!h_all) {
                    const size_t bytes = h.getImageSizeBytes();
                    void* hs = h_sym_.reserve(bytes);
                    if (!hs) { rc = 3; break; }
                    // on this batch's own HIP stream: stream_ belongs to the
                    // caller thread's next submit (its predictor stage)
                    hipStream_t fs = bz_[b % nslots].stream;
                    if ((up && up->wait_frames(~0ull, fs)) ||
                        hipMemcpyAsync(hs, d_sym, bytes, hipMemcpyDeviceToHost, fs) != hipSuccess ||
                        hipStreamSynchronize(fs) != hipSuccess) {
                        rc = 3;
                        break;
                    }
                    h_all = (const uint8_t*)hs;
                }
                size_t n = 0;
                ++host_streams;
                gather_block(h_all, g, b0 + i, bpp, in.data(), &n);
                uint32_t len = 0;
                rc = compress_one(BZIP2, in.data(), (uint32_t)n, out.data(), (uint32_t)out.size(), &len, level);
                if (!rc) rc = sink.append(out.data(), len);
                offset += len;
            } else {
                rc = sink.append(p, sizes[b][i]);
                p += sizes[b][i];
                offset += sizes[b][i];
            }
            h.blockOffset[b0 + i] = offset;
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            state[b] = 2;
            if (rc) abort_all = true;
        }
        cv.notify_all();
    }
    if (rc) {
        std::lock_guard<std::mutex> lk(mu);
        abort_all = true;
    }
    cv.notify_all();
    for (auto& t : pool) t.join();
    counts_[set] = StreamCounts{nblocks, host_streams, std::accumulate(gpu_blocks.begin(), gpu_blocks.end(), (uint64_t)0)};
    if (st) {
        for (double v : d2h) st->d2h_ms += v;
        for (int i = 0; i < 5; ++i)
            for (int k = 0; k < nslots; ++k) st->bz_stage_ms[i] = std::max(st->bz_stage_ms[i], stage_ms[k][i]);
        st->bz_in_bytes = nblocks * (uint64_t)block_bytes;
    }
    if (rc) return rc;
    return sink.finish(h);
}

// selection for submit: on the slab's select_frame, else on frame 0 of the image
// A device input was written by the caller's kernels, typically on the null
// stream (torch's default stream, lfm_hip_synth without a stream); the
// encoder's streams are non-blocking, so they would not wait for that work:
// the encoder's stream waits for an event recorded on the null stream.  (A
// producer on another stream must be synchronised by the caller; the Python
// binding does that for torch's current stream.)
int Encoder::after_caller(bool dev)
{
    if (!dev) return 0;
    if (int rc = ensure_gpu()) return rc;
    (void)hipSetDevice(device_);
    if (!caller_ev_ && hipEventCreateWithFlags(&caller_ev_, hipEventDisableTiming) != hipSuccess) {
        caller_ev_ = nullptr;
        return 3;
    }
    return hipEventRecord(caller_ev_, nullptr) == hipSuccess && hipStreamWaitEvent(stream_, caller_ev_, 0) == hipSuccess
               ? 0
               : 3;
}

int Encoder::preselect(const void* img, bool dev, const klb_image_header& h, const SlabSpec& slab, int* k,
                       float ent[8])
{
    if (int rc = ensure_gpu()) return rc;
    (void)hipSetDevice(device_);
    const int W = (int)h.xyzct[0], H = (int)h.xyzct[1];
    if (W <= 0 || H <= 0) return 3;
    const void* frame = slab.select_frame ? slab.select_frame : (slab.z0 > 0 ? nullptr : img);
    if (!frame) return 3;  // a slab's own frame 0 is not the stack's
    if (!dev) return select_host_frame(frame, W, H, h.Nnum, current_family(), k, ent);
    void* ws = d_ws_.reserve(lfm_hip_select_workspace_bytes(W, H));
    if (!ws) return 3;
    return lfm_hip_select((const uint16_t*)frame, W, H, h.Nnum, current_family(), ent, k, ws, stream_) ==
                   LFM_HIP_OK
               ? 0
               : 3;
}

int Encoder::select_frame(const void* frame, bool dev, const klb_image_header& h, int* chosen, float entropy[8])
{
    static const SlabSpec whole;
    if (int rc = after_caller(dev)) return rc;
    return preselect(frame, dev, h, whole, chosen, entropy);
}

int Encoder::select_host_frame(const void* frame, int W, int H, int T, int family, int* chosen, float entropy[8])
{
    if (int rc = ensure_gpu()) return rc;
    (void)hipSetDevice(device_);
    const size_t bytes = (size_t)W * H * 2;
    void* in = d_in_.reserve(bytes);
    void* ws = in ? d_ws_.reserve(lfm_hip_select_workspace_bytes(W, H)) : nullptr;
    if (!ws) return 3;
    if (hipMemcpyAsync(in, frame, bytes, hipMemcpyHostToDevice, stream_) != hipSuccess) return 3;
    return lfm_hip_select((const uint16_t*)in, W, H, T, family, entropy, chosen, ws, stream_) == LFM_HIP_OK ? 0 : 3;
}

int Encoder::encode(const void* img, bool dev, klb_image_header& h, Sink& sink, lfm_encode_stats* st, int threads,
                    const SlabSpec* slab)
{
    join_inflight();  // a synchronous encode may use either buffer set
    const int rc = encode_set(img, dev, h, sink, st, threads, slab, 0);
    last_counts = counts_[0];
    return rc;
}

int Encoder::encode_set(const void* img, bool dev, klb_image_header& h, Sink& sink, lfm_encode_stats* st,
                        int threads, const SlabSpec* slab, int set)
{
    static const SlabSpec whole;
    if (threads <= 0) threads = default_threads();
    auto t0 = clk::now();
    if (st) std::memset(st, 0, sizeof(*st));
    const int level = slab_level(h, slab);
    counts_[set] = StreamCounts{};
    if (int rc = normalize_header(h)) return rc;
    if (int rc = after_caller(dev)) return rc;
    const uint8_t* sym = nullptr;
    const uint8_t* dsym = nullptr;
    const bool gpu_bz = use_gpu_bzip2(h, dev);
    int rc = predictor_stage(img, dev, h, &sym, gpu_bz ? &dsym : nullptr, st, slab ? *slab : whole, set);
    if (rc) return rc;
    auto tc = clk::now();
    if (gpu_bz) {
        if ((rc = ensure_gpu())) {
            up_[set].join();
            return rc;
        }
        rc = gpu_compress(dsym, h, sink, st, level, set, nullptr);
        UploadPipe& up = up_[set];
        if (up.active) {  // the host image is read until the uploader is done
            up.join();
            if (!rc) rc = up.rc;
            if (st) {
                st->h2d_ms += up.h2d_ms;
                st->predict_ms += up.predict_ms;
            }
        }
    } else {
        rc = compress_blocks(sym, h, sink, threads, level);
        const uint64_t nb = BlockGrid(h).nblocks;
        counts_[set] = StreamCounts{nb, nb, 0};
    }
    if (st) {
        st->compress_ms = ms_since(tc);
        st->total_ms = ms_since(t0);
        st->header_version = h.headerVersion;
        st->chosen = h.headerVersion & 0x7F;
        st->out_bytes = h.getCompressedFileSizeInBytes();
    }
    return rc;
}

} // namespace lfm
