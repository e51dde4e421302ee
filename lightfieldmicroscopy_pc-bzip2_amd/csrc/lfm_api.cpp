// lfm_api.cpp -- liblfm extensions (lfm_api.h).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "lfm_api.h"
#include <cstdlib>
#include <cstring>
#include <string>
#include "klb_imageIO.h"
#include "lfm_engine.h"
#include "lfm_hip.h"
#include <vector>

struct lfm_encoder {
    lfm::Encoder enc;
    int threads;
    lfm_encoder(int device, int threads_) : enc(device), threads(threads_) {}
};

extern "C" int lfm_set_family(int family)
{
    if (family < 0 || family > 2) return 1;
    lfm::set_family(family);
    return 0;
}
extern "C" int lfm_get_family(void) { return lfm::current_family(); }
extern "C" const char* lfm_version(void) { return "lfm-mi355x 0.2 (gfx950, api 2)"; }
extern "C" int lfm_api_version(void) { return LFM_API_VERSION; }

extern "C" int writeLFMstack_c(const void* im, const char* filename, const uint32_t xyzct[KLB_DATA_DIMS],
                               int dataType, int numThreads, const float pixelSize[KLB_DATA_DIMS],
                               const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                               const char metadata[KLB_METADATA_SIZE], int predictor_request, int Nnum, int video)
{
    klb_imageIO io{std::string(filename)};
    io.header.setHeader(xyzct, (KLB_DATA_TYPE)dataType, pixelSize, blockSize, (KLB_COMPRESSION_TYPE)compressionType,
                        metadata);
    // matlabWrapper/writeLFMstack.cpp:360-433: headerVersion |= predictor; Nnum; |= video << 7
    io.header.headerVersion = (uint8_t)(io.header.headerVersion | (uint8_t)predictor_request);
    io.header.Nnum = (uint8_t)Nnum;
    io.header.headerVersion = (uint8_t)(io.header.headerVersion | ((uint8_t)video << 7));
    return io.writeImage((const char*)im, numThreads);
}

extern "C" int readLFMstack_c(const char* filename, void* im, int numThreads, uint8_t* headerVersion, uint8_t* Nnum)
{
    klb_imageIO io{std::string(filename)};
    int e = io.readHeader();
    if (e) return e;
    e = io.readImageFull((char*)im, numThreads);
    if (headerVersion) *headerVersion = io.header.headerVersion;
    if (Nnum) *Nnum = io.header.Nnum;
    return e;
}

extern "C" lfm_encoder* lfm_encoder_create(int device, int numThreads)
{
    return new lfm_encoder(device, numThreads);
}
extern "C" void lfm_encoder_destroy(lfm_encoder* e) { delete e; }

extern "C" int lfm_encoder_encode(lfm_encoder* e, const void* img, int img_is_device,
                                  const uint32_t xyzct[KLB_DATA_DIMS], int dataType, int headerVersion, int Nnum,
                                  const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                                  const char metadata[KLB_METADATA_SIZE], const uint8_t** out, uint64_t* out_len,
                                  lfm_encode_stats* stats)
{
    if (!e || !img || !out || !out_len) return 3;
    klb_image_header h;
    h.setHeader(xyzct, (KLB_DATA_TYPE)dataType, nullptr, blockSize, (KLB_COMPRESSION_TYPE)compressionType, metadata,
                (uint8_t)headerVersion, (uint8_t)Nnum);
    lfm::MemSink sink(&e->enc.mem_out);
    int rc = e->enc.encode(img, img_is_device != 0, h, sink, stats, e->threads);
    *out = e->enc.mem_out.data();
    *out_len = e->enc.mem_out.size();
    return rc;
}

extern "C" int lfm_encoder_encode_slab(lfm_encoder* e, const void* img, int img_is_device, const void* prev_frame,
                                       uint32_t z0, const uint32_t xyzct[KLB_DATA_DIMS], int dataType,
                                       int headerVersion, int Nnum, const uint32_t blockSize[KLB_DATA_DIMS],
                                       int compressionType, const char metadata[KLB_METADATA_SIZE],
                                       const uint8_t** out, uint64_t* out_len, lfm_encode_stats* stats)
{
    if (!e || !img || !out || !out_len) return 3;
    klb_image_header h;
    h.setHeader(xyzct, (KLB_DATA_TYPE)dataType, nullptr, blockSize, (KLB_COMPRESSION_TYPE)compressionType, metadata,
                (uint8_t)headerVersion, (uint8_t)Nnum);
    lfm::SlabSpec slab;
    slab.z0 = z0;
    slab.prev = prev_frame;
    lfm::MemSink sink(&e->enc.mem_out);
    int rc = e->enc.encode(img, img_is_device != 0, h, sink, stats, e->threads, &slab);
    *out = e->enc.mem_out.data();
    *out_len = e->enc.mem_out.size();
    return rc;
}

extern "C" int lfm_encoder_submit(lfm_encoder* e, const void* img, int img_is_device, const void* prev_frame,
                                  uint32_t z0, const uint32_t xyzct[KLB_DATA_DIMS], int dataType, int headerVersion,
                                  int Nnum, const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                                  const char metadata[KLB_METADATA_SIZE], uint64_t* ticket)
{
    if (!e || !img || !ticket) return 3;
    klb_image_header h;
    h.setHeader(xyzct, (KLB_DATA_TYPE)dataType, nullptr, blockSize, (KLB_COMPRESSION_TYPE)compressionType, metadata,
                (uint8_t)headerVersion, (uint8_t)Nnum);
    lfm::SlabSpec slab;
    slab.z0 = z0;
    slab.prev = prev_frame;
    return e->enc.submit(img, img_is_device != 0, h, e->threads, &slab, ticket);
}

extern "C" int lfm_encoder_submit_select(lfm_encoder* e, const void* img, int img_is_device, const void* prev_frame,
                                         uint32_t z0, const void* select_frame, const uint32_t xyzct[KLB_DATA_DIMS],
                                         int dataType, int headerVersion, int Nnum,
                                         const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                                         const char metadata[KLB_METADATA_SIZE], uint64_t* ticket)
{
    if (!e || !img || !ticket) return 3;
    klb_image_header h;
    h.setHeader(xyzct, (KLB_DATA_TYPE)dataType, nullptr, blockSize, (KLB_COMPRESSION_TYPE)compressionType, metadata,
                (uint8_t)headerVersion, (uint8_t)Nnum);
    lfm::SlabSpec slab;
    slab.z0 = z0;
    slab.prev = prev_frame;
    slab.select_frame = select_frame;
    return e->enc.submit(img, img_is_device != 0, h, e->threads, &slab, ticket);
}

extern "C" int lfm_encoder_wait(lfm_encoder* e, uint64_t ticket, const uint8_t** out, uint64_t* out_len,
                                lfm_encode_stats* stats)
{
    if (!e || !out || !out_len) return 3;
    const lfm::PinnedBuffer* b = nullptr;
    const int rc = e->enc.wait(ticket, &b, stats);
    // a failed encode leaves an earlier encode's bytes in that buffer set:
    // hand out nothing rather than a stale .lfm
    *out = (b && rc == 0) ? b->data() : nullptr;
    *out_len = (b && rc == 0) ? b->size() : 0;
    return rc;
}

extern "C" int lfm_set_devices(const int* devices, int n)
{
    if (n < 0 || (n > 0 && !devices)) return 3;
    std::vector<int> d(devices, devices + n);
    const int count = lfm_hip_device_count();
    for (int v : d)
        if (v < 0 || v >= count) return 3;
    lfm::set_encode_devices(d);
    return 0;
}

extern "C" int lfm_get_devices(int* devices, int cap)
{
    const std::vector<int> d = lfm::encode_devices();
    for (int i = 0; i < cap && i < (int)d.size(); ++i) devices[i] = d[i];
    return (int)d.size();
}

extern "C" int lfm_default_devices(int n_visible, int current, int* devices, int cap)
{
    const std::vector<int> d = lfm::default_devices(n_visible, current);
    for (int i = 0; i < cap && i < (int)d.size(); ++i) devices[i] = d[i];
    return (int)d.size();
}

extern "C" int lfm_encoder_encode_multi(lfm_encoder* e, const void* img, const uint32_t xyzct[KLB_DATA_DIMS],
                                        int dataType, int headerVersion, int Nnum,
                                        const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                                        const char metadata[KLB_METADATA_SIZE], const uint8_t** out,
                                        uint64_t* out_len, lfm_encode_stats* stats)
{
    if (!e || !img || !out || !out_len) return 3;
    klb_image_header h;
    h.setHeader(xyzct, (KLB_DATA_TYPE)dataType, nullptr, blockSize, (KLB_COMPRESSION_TYPE)compressionType, metadata,
                (uint8_t)headerVersion, (uint8_t)Nnum);
    lfm::MemSink sink(&e->enc.mem_out);
    int rc = lfm::encode_multi(img, h, sink, stats, e->threads, lfm::encode_devices());
    if (rc == -1) rc = e->enc.encode(img, false, h, sink, stats, e->threads);
    e->enc.last_counts = {};
    *out = e->enc.mem_out.data();
    *out_len = e->enc.mem_out.size();
    return rc;
}

extern "C" int lfm_set_bzip2_multiblock(int on) { return lfm::set_bzip2_multiblock(on); }
extern "C" int lfm_get_bzip2_multiblock(void) { return lfm::bzip2_multiblock(); }
extern "C" int lfm_set_bunzip2_multiblock(int on) { return lfm::set_bunzip2_multiblock(on); }
extern "C" int lfm_get_bunzip2_multiblock(void) { return lfm::bunzip2_multiblock(); }
extern "C" int lfm_set_bunzip2_periodic(int on) { return lfm_hip_bunzip2_set_periodic(on); }
extern "C" int lfm_get_bunzip2_periodic(void) { return lfm_hip_bunzip2_get_periodic(); }

extern "C" int lfm_encoder_stream_counts(lfm_encoder* e, uint64_t* streams, uint64_t* host_streams,
                                         uint64_t* bzip2_blocks)
{
    if (!e) return 3;
    if (streams) *streams = e->enc.last_counts.streams;
    if (host_streams) *host_streams = e->enc.last_counts.host_streams;
    if (bzip2_blocks) *bzip2_blocks = e->enc.last_counts.bzip2_blocks;
    return 0;
}

extern "C" void lfm_release_encoders(void) { lfm::release_pooled_encoders(); }

extern "C" int lfm_merge_slabs(const uint8_t* const* slabs, const uint64_t* lens, int nslabs, uint8_t** out,
                               uint64_t* out_len)
{
    if (!out || !out_len) return 3;
    *out = nullptr;
    *out_len = 0;
    std::vector<uint8_t> v;
    int rc = lfm::merge_slabs(slabs, lens, nslabs, &v);
    if (rc) return rc;
    *out = (uint8_t*)std::malloc(v.size() ? v.size() : 1);
    if (!*out) return 3;
    std::memcpy(*out, v.data(), v.size());
    *out_len = v.size();
    return 0;
}

extern "C" void lfm_free(void* p) { std::free(p); }

extern "C" int lfm_slab_info(const uint8_t* slab, uint64_t len, uint64_t* payload_bytes, uint64_t* nblocks)
{
    klb_image_header h;
    if (!slab || h.parseHeader(slab, len)) return 3;
    const uint64_t body = h.Nb ? h.blockOffset[h.Nb - 1] : 0;
    if (h.getSizeInBytes() + body > len) return 3;
    if (payload_bytes) *payload_bytes = body;
    if (nblocks) *nblocks = h.Nb;
    return 0;
}

extern "C" int lfm_place_slab(const uint8_t* slab, uint64_t slab_len, uint8_t* dst, uint64_t dst_len,
                              uint32_t total_z, uint64_t total_blocks, uint64_t block_index, uint64_t payload_offset,
                              int numThreads)
{
    klb_image_header h;
    if (!slab || !dst || h.parseHeader(slab, slab_len)) return 3;
    if (h.xyzct[3] != 1 || h.xyzct[4] != 1 || block_index + h.Nb > total_blocks) return 3;
    const uint64_t body = h.Nb ? h.blockOffset[h.Nb - 1] : 0;
    const uint64_t hsz = 320 + 8 * total_blocks;
    if (h.getSizeInBytes() + body > slab_len || hsz + payload_offset + body > dst_len) return 3;
    if (block_index == 0) {  // the whole stack's fixed header (the offset table follows from every rank)
        klb_image_header H(h);
        H.xyzct[2] = total_z;
        H.resizeBlockOffset(0);
        if (H.calculateNumBlocks() != total_blocks) return 3;
        H.serialize(dst, 320);
    }
    uint64_t* table = (uint64_t*)(dst + 320);  // little-endian host (x86-64)
    for (size_t j = 0; j < h.Nb; ++j) table[block_index + j] = payload_offset + h.blockOffset[j];
    lfm::par_memcpy(dst + hsz + payload_offset, slab + h.getSizeInBytes(), body,
                    numThreads > 0 ? numThreads : lfm::default_threads());
    return 0;
}

extern "C" int lfm_decode_memory(const uint8_t* buf, uint64_t len, void* img, int numThreads)
{
    const auto t0 = std::chrono::steady_clock::now();
    klb_image_header h;
    int rc = h.parseHeader(buf, len);
    if (rc) return rc;
    rc = lfm::decode_image(buf, len, h, (uint8_t*)img, numThreads);
    if (std::getenv("LFM_DECODE_TIMING"))
        std::fprintf(stderr, "decode total (C)     %8.2f ms\n",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}

extern "C" int lfm_set_decode_devices(const int* devices, int n)
{
    if (n < 0 || (n > 0 && !devices)) return 3;
    std::vector<int> d(devices, devices + n);
    const int count = n > 0 ? lfm_hip_device_count() : 0;
    for (int v : d)
        if (v < 0 || v >= count) return 3;
    lfm::set_decode_devices(d);
    return 0;
}

extern "C" int lfm_get_decode_devices(int* devices, int cap)
{
    const std::vector<int> d = lfm::decode_devices();
    for (int i = 0; devices && i < cap && i < (int)d.size(); ++i) devices[i] = d[i];
    return (int)d.size();
}

extern "C" int lfm_default_decode_devices(int n_visible, int* devices, int cap)
{
    const std::vector<int> d = lfm::default_decode_devices(n_visible);
    for (int i = 0; devices && i < cap && i < (int)d.size(); ++i) devices[i] = d[i];
    return (int)d.size();
}

extern "C" void lfm_release_decoders(void) { lfm::release_decode_workers(); }

extern "C" int lfm_decode_shard_plan(const uint8_t* buf, uint64_t len, int nworkers, int* axis, uint32_t* first,
                                     uint32_t* count, int cap)
{
    klb_image_header h;
    if (!buf || h.parseHeader(buf, len)) return 0;
    const lfm::ShardPlan p = lfm::decode_shard_plan(h, nworkers);
    if (axis) *axis = p.axis;
    for (int w = 0; w < cap && w < (int)p.shards.size(); ++w) {
        if (first) first[w] = p.shards[w].first;
        if (count) count[w] = p.shards[w].second;
    }
    return (int)p.shards.size();
}

extern "C" int lfm_decode_memory_multi(const uint8_t* buf, uint64_t len, void* img, int numThreads,
                                       lfm_decode_multi_stats* stats, lfm_decode_shard* shards, int shard_cap)
{
    if (!buf || !img) return 3;
    klb_image_header h;
    if (int rc = h.parseHeader(buf, len)) return rc;
    return lfm::decode_multi(buf, len, h, (uint8_t*)img, nullptr, nullptr, 0, numThreads, lfm::decode_devices(), stats,
                             shards, shard_cap);
}

extern "C" int lfm_decode_memory_multi_device(const uint8_t* buf, uint64_t len, void* const* d_out,
                                              const uint64_t* out_bytes, int nshards, int numThreads,
                                              lfm_decode_multi_stats* stats, lfm_decode_shard* shards, int shard_cap)
{
    if (!buf || !d_out || !out_bytes || nshards < 1 || lfm_hip_device_count() <= 0) return 3;
    klb_image_header h;
    if (int rc = h.parseHeader(buf, len)) return rc;
    return lfm::decode_multi(buf, len, h, nullptr, d_out, out_bytes, nshards, numThreads, {}, stats, shards, shard_cap);
}

extern "C" int lfm_decode_memory_device(const uint8_t* buf, uint64_t len, void* d_img, uint64_t d_img_bytes,
                                        int numThreads, lfm_decode_stats* stats)
{
    const int rc = lfm::decode_memory_device(buf, len, nullptr, nullptr, d_img, d_img_bytes, numThreads, stats);
    if (std::getenv("LFM_DECODE_TIMING") && stats)
        std::fprintf(stderr, "decode total (C, device) %8.2f ms\n", stats->total_ms);
    return rc;
}

extern "C" int lfm_decode_memory_roi_device(const uint8_t* buf, uint64_t len, const uint32_t lb[KLB_DATA_DIMS],
                                            const uint32_t ub[KLB_DATA_DIMS], void* d_out, uint64_t out_bytes,
                                            int numThreads, lfm_decode_stats* stats)
{
    if (!lb || !ub) return 3;
    return lfm::decode_memory_device(buf, len, lb, ub, d_out, out_bytes, numThreads, stats);
}

// ---- stream writer / ranged reader (lfm_stream.cpp) ----
struct lfm_writer {
    lfm::StreamWriter w;
    lfm_writer(const klb_image_header& h, int device, int threads) : w(h, device, threads) {}
};
struct lfm_reader {
    lfm::FileReader r;
};

extern "C" int lfm_writer_open(lfm_writer** w, const char* filename, const uint32_t xyzct[KLB_DATA_DIMS], int dataType,
                               int headerVersion, int Nnum, const float pixelSize[KLB_DATA_DIMS],
                               const uint32_t blockSize[KLB_DATA_DIMS], int compressionType,
                               const char metadata[KLB_METADATA_SIZE], int device, int numThreads)
{
    if (!w) return 3;
    *w = nullptr;
    if (!filename || !xyzct) return 3;
    klb_image_header h;
    h.setHeader(xyzct, (KLB_DATA_TYPE)dataType, pixelSize, blockSize, (KLB_COMPRESSION_TYPE)compressionType, metadata,
                (uint8_t)headerVersion, (uint8_t)Nnum);
    lfm_writer* p = new lfm_writer(h, device, numThreads);
    if (int rc = p->w.open(filename)) {
        p->w.abort();
        delete p;
        return rc;
    }
    *w = p;
    return 0;
}

extern "C" int lfm_writer_axis(const lfm_writer* w) { return w ? w->w.axis() : -1; }

extern "C" int lfm_writer_append(lfm_writer* w, const void* img, int img_is_device, uint32_t count)
{
    return w ? w->w.append(img, img_is_device != 0, count) : 3;
}

extern "C" int lfm_writer_flush(lfm_writer* w, int sync, uint64_t* committed)
{
    if (!w) return 3;
    return w->w.flush(sync != 0, committed);
}

extern "C" int lfm_recover(const char* filename, const char* out_filename, int verify, int numThreads,
                           lfm_recover_stats* stats)
{
    return lfm::recover_file(filename, out_filename, verify != 0, numThreads, stats);
}

extern "C" int lfm_writer_close(lfm_writer* w, lfm_writer_stats* stats)
{
    if (!w) return 3;
    const int rc = w->w.close(stats);
    delete w;
    return rc;
}

extern "C" void lfm_writer_abort(lfm_writer* w)
{
    if (!w) return;
    w->w.abort();
    delete w;
}

static int reader_open(lfm_reader** r, const char* filename, bool live)
{
    if (!r) return 3;
    *r = nullptr;
    if (!filename) return 3;
    lfm_reader* p = new lfm_reader;
    if (int rc = p->r.open(filename, live)) {
        delete p;
        return rc;
    }
    *r = p;
    return 0;
}

extern "C" int lfm_reader_open(lfm_reader** r, const char* filename) { return reader_open(r, filename, false); }

extern "C" int lfm_reader_open_live(lfm_reader** r, const char* filename) { return reader_open(r, filename, true); }

extern "C" int lfm_reader_refresh(lfm_reader* r, uint32_t* extent) { return r ? r->r.refresh(extent) : 3; }

extern "C" int lfm_reader_info(const lfm_reader* r, uint32_t xyzct[KLB_DATA_DIMS], int* dataType,
                               uint32_t blockSize[KLB_DATA_DIMS], uint8_t* headerVersion, uint8_t* Nnum,
                               uint64_t* file_bytes)
{
    if (!r) return 3;
    const klb_image_header& h = r->r.h;
    if (xyzct) std::memcpy(xyzct, h.xyzct, sizeof(h.xyzct));
    if (dataType) *dataType = (int)h.dataType;
    if (blockSize) std::memcpy(blockSize, h.blockSize, sizeof(h.blockSize));
    if (headerVersion) *headerVersion = h.headerVersion;
    if (Nnum) *Nnum = h.Nnum;
    if (file_bytes) *file_bytes = r->r.file_bytes;
    return 0;
}

extern "C" int lfm_reader_read(lfm_reader* r, const uint32_t lb[KLB_DATA_DIMS], const uint32_t ub[KLB_DATA_DIMS],
                               void* out, uint64_t out_bytes, int out_is_device, int numThreads,
                               lfm_decode_stats* stats)
{
    return r ? r->r.read(lb, ub, out, out_bytes, out_is_device != 0, numThreads, stats) : 3;
}

extern "C" uint64_t lfm_reader_bytes_read(const lfm_reader* r) { return r ? r->r.bytes_read : 0; }

extern "C" void lfm_reader_close(lfm_reader* r) { delete r; }

extern "C" int lfm_decode_memory_roi(const uint8_t* buf, uint64_t len, const uint32_t lb[KLB_DATA_DIMS],
                                     const uint32_t ub[KLB_DATA_DIMS], void* out, uint64_t out_bytes, int numThreads)
{
    if (!buf || !lb || !ub || !out) return 3;
    klb_image_header h;
    int rc = h.parseHeader(buf, len);
    if (rc) return rc;
    uint64_t need = h.getBytesPerPixel();  // the region in the file's own data type
    for (int d = 0; d < KLB_DATA_DIMS; ++d) {
        if (ub[d] < lb[d] || ub[d] >= h.xyzct[d]) return 3;
        need *= (uint64_t)(ub[d] - lb[d] + 1);
    }
    if (!need || out_bytes < need) return 3;
    const size_t hs = h.getSizeInBytes();
    return lfm::decode_roi(buf + hs, len - hs, h, lb, ub, (uint8_t*)out, numThreads, lfm::current_family());
}
