// lfm_engine.cpp -- MI355X-native encode / decode engine: what its parts
// share (switches and threads, predictor family, block grid, sinks, the
// pinned output buffer, the host block compressors, header rules, the z-slab
// merge).  The Encoder is lfm_encode.cpp, the readers lfm_decode.cpp, the
// host <-> device copies lfm_transfer.cpp.
//
// Encode = predictor stage (GPU, lfm_hip.h) + block compression (host worker
// pool, in-order sink).  The reference equivalents:
//   writeImage               klb_imageIO.cpp:2248-2492
//   predictor selection      :2273-2360 (8 candidates on frame 0, argmin)
//   Predictor_both/_angle/_space :1227-1670 (one launch + 2 PCIe copies per frame)
//   blockCompressor          :78-295    (x-fastest gather, BZ2 level rule, workFactor 30)
//   blockWriter              :1145-1225 (in-order append, offset table rewritten at the end)
// Here the whole stack is predicted by one kernel launch per (c,t) volume,
// symbols come back with one D2H copy into pinned memory, and the block
// compressors run on all host cores while the calling thread appends the
// finished blocks in order.
#include "lfm_engine.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <zlib.h>

#include "bz2_sys.h"
#include "lfm_hip.h"
#include "lfm_internal.h"

namespace lfm {

namespace {
std::atomic<int> g_family{-1};
} // namespace

int default_threads()
{
    int n = env_int("LFM_NUM_THREADS", 0);
    if (n <= 0) n = env_int("OMP_NUM_THREADS", 0);
    if (n <= 0) n = (int)std::thread::hardware_concurrency();
    return std::max(n, 1);
}

int current_family()
{
    int f = g_family.load();
    if (f < 0) {
        f = env_int("LFM_PREDICTOR_WAY", LFM_PREDICTOR_WAY);
        if (f < 0 || f > 2) f = LFM_PREDICTOR_WAY;
        g_family.store(f);
    }
    return f;
}
void set_family(int fam) { g_family.store(fam); }

// ------------------------------------------------------------- block grid --
BlockGrid::BlockGrid(const klb_image_header& h)
{
    nblocks = 1;
    uint64_t s = 1;
    for (int d = 0; d < 5; ++d) {
        dims[d] = h.xyzct[d];
        bs[d] = h.blockSize[d];
        nb[d] = (uint64_t)std::ceil((float)h.xyzct[d] / (float)h.blockSize[d]);  // calculateNumBlocks
        nblocks *= nb[d];
        stride[d] = s;
        s *= dims[d];
    }
}

void BlockGrid::block(uint64_t id, uint64_t origin[5], uint64_t size[5]) const
{
    for (int d = 0; d < 5; ++d) {
        const uint64_t c = id % nb[d];
        id /= nb[d];
        origin[d] = c * bs[d];
        size[d] = std::min<uint64_t>(bs[d], dims[d] - origin[d]);
    }
}

template <bool GATHER>
static void walk_block(uint8_t* img, const BlockGrid& g, uint64_t id, size_t bpp, uint8_t* blk, size_t* nbytes)
{
    uint64_t o[5], s[5];
    g.block(id, o, s);
    const size_t row = s[0] * bpp;
    size_t k = 0;
    for (uint64_t t = 0; t < s[4]; ++t)
        for (uint64_t c = 0; c < s[3]; ++c)
            for (uint64_t z = 0; z < s[2]; ++z)
                for (uint64_t y = 0; y < s[1]; ++y) {
                    const uint64_t e = (o[0]) * g.stride[0] + (o[1] + y) * g.stride[1] + (o[2] + z) * g.stride[2] +
                                       (o[3] + c) * g.stride[3] + (o[4] + t) * g.stride[4];
                    if (GATHER) std::memcpy(blk + k, img + e * bpp, row);
                    else std::memcpy(img + e * bpp, blk + k, row);
                    k += row;
                }
    if (nbytes) *nbytes = k;
}

void gather_block(const uint8_t* img, const BlockGrid& g, uint64_t id, size_t bpp, uint8_t* dst, size_t* nbytes)
{
    walk_block<true>(const_cast<uint8_t*>(img), g, id, bpp, dst, nbytes);
}
void scatter_block(const uint8_t* blk, const BlockGrid& g, uint64_t id, size_t bpp, uint8_t* img)
{
    walk_block<false>(img, g, id, bpp, const_cast<uint8_t*>(blk), nullptr);
}

// ------------------------------------------------------------------ sinks --
int FileSink::begin(const klb_image_header& h)
{
    vbuf_.resize(32 << 20);
    setvbuf(f_, vbuf_.data(), _IOFBF, vbuf_.size());
    std::vector<uint8_t> head(h.getSizeInBytes(), 0);
    klb_image_header tmp(h);
    std::fill(tmp.blockOffset, tmp.blockOffset + tmp.Nb, 0);
    tmp.serialize(head.data(), head.size());
    return std::fwrite(head.data(), 1, head.size(), f_) == head.size() ? 0 : 5;
}
int FileSink::append(const uint8_t* p, size_t n)
{
    return std::fwrite(p, 1, n, f_) == n ? 0 : 5;
}
int FileSink::finish(const klb_image_header& h)
{
    if (std::fseek(f_, (long)h.getSizeInBytesFixPortion(), SEEK_SET) != 0) return 5;
    if (h.Nb && std::fwrite(h.blockOffset, sizeof(uint64_t), h.Nb, f_) != h.Nb) return 5;
    std::fflush(f_);
    return 0;
}

PinnedBuffer::~PinnedBuffer()
{
    if (p_ && malloced_) std::free(p_);
    else if (p_) (void)hipHostFree(p_);
}
bool PinnedBuffer::reserve(size_t n)
{
    if (n <= cap_) return true;
    const size_t cap = std::max(n, cap_ + cap_ / 2);
    void* q = nullptr;
    if (hipHostMalloc(&q, cap, hipHostMallocDefault) != hipSuccess) {
        // no HIP runtime (CPU-only paths): plain memory
        (void)hipGetLastError();
        q = std::malloc(cap);
        if (!q) return false;
        if (p_ && size_) std::memcpy(q, p_, size_);
        if (p_ && malloced_) std::free(p_);
        else if (p_) (void)hipHostFree(p_);
        p_ = (uint8_t*)q;
        cap_ = cap;
        malloced_ = true;
        return true;
    }
    if (p_ && size_) par_memcpy(q, p_, size_, default_threads());
    if (p_) {
        if (malloced_) std::free(p_);
        else (void)hipHostFree(p_);
    }
    p_ = (uint8_t*)q;
    cap_ = cap;
    malloced_ = false;
    return true;
}
bool PinnedBuffer::resize(size_t n)
{
    if (!reserve(n)) return false;
    size_ = n;
    return true;
}

int MemSink::begin(const klb_image_header& h)
{
    out_->clear();
    if (!out_->resize(h.getSizeInBytes())) return 3;
    std::memset(out_->data(), 0, out_->size());
    return 0;
}
int MemSink::append(const uint8_t* p, size_t n)
{
    uint8_t* d = direct(n);
    if (!d) return 3;
    std::memcpy(d, p, n);
    return 0;
}
uint8_t* MemSink::direct(size_t n)
{
    const size_t at = out_->size();
    // grow once to the worst case; if that reservation fails, the plain
    // resize below still grows by what this append needs
    if (at + n > out_->capacity() && worst_ > at + n) (void)out_->reserve(worst_);
    if (!out_->resize(at + n)) return nullptr;
    return out_->data() + at;
}
int MemSink::finish(const klb_image_header& h)
{
    h.serialize(out_->data(), h.getSizeInBytes());
    return 0;
}

// ------------------------------------------------------- block compression --
int compress_one(int ctype, uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint32_t* out_len, int level)
{
    switch (ctype) {
    case NONE:
        std::memcpy(out, in, n);
        *out_len = n;
        return 0;
    case BZIP2: {
        unsigned int len = cap;
        int rc = BZ2_bzBuffToBuffCompress((char*)out, &len, (char*)in, n, level, 0, 30);
        *out_len = len;
        return rc == LFM_BZ_OK ? 0 : 2;
    }
    case ZLIB: {
        z_stream s;
        std::memset(&s, 0, sizeof(s));
        if (deflateInit(&s, Z_DEFAULT_COMPRESSION) != Z_OK) return 3;
        s.next_in = in;
        s.avail_in = n;
        s.next_out = out;
        s.avail_out = cap;
        s.data_type = Z_BINARY;
        int rc = deflate(&s, Z_FINISH);
        *out_len = cap - s.avail_out;
        deflateEnd(&s);
        return (rc == Z_STREAM_END || rc == Z_OK) ? 0 : 3;
    }
    }
    return 5;
}

int decompress_one(int ctype, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t expect)
{
    switch (ctype) {
    case NONE:
        if (n != expect) return 3;
        std::memcpy(out, in, n);
        return 0;
    case BZIP2: {
        unsigned int len = expect;
        int rc = BZ2_bzBuffToBuffDecompress((char*)out, &len, (char*)in, n, 0, 0);
        return (rc == LFM_BZ_OK && len == expect) ? 0 : 2;
    }
    case ZLIB: {
        z_stream s;
        std::memset(&s, 0, sizeof(s));
        if (inflateInit(&s) != Z_OK) return 3;
        s.next_in = const_cast<uint8_t*>(in);
        s.avail_in = n;
        s.next_out = out;
        s.avail_out = expect;
        int rc = inflate(&s, Z_FINISH);
        const bool ok = (rc == Z_STREAM_END) && s.avail_out == 0;
        inflateEnd(&s);
        return ok ? 0 : 3;
    }
    }
    return 5;
}

int bzip2_level(const klb_image_header& h)
{
    return std::min(9, (int)((h.getBlockSizeBytes() + 99999) / 100000));  // klb_imageIO.cpp:108, nominal block
}

int compress_blocks(const uint8_t* sym, klb_image_header& h, Sink& sink, int threads, int level)
{
    const BlockGrid g(h);
    const uint64_t nblocks = g.nblocks;
    h.resizeBlockOffset(nblocks);
    const size_t bpp = h.getBytesPerPixel();
    const uint32_t block_bytes = h.getBlockSizeBytes();                 // nominal (clamped) block
    if (level < 1) level = bzip2_level(h);
    uint32_t cap = block_bytes;
    if (h.compressionType != NONE) cap = (uint32_t)std::ceil((float)block_bytes * 2.0f + 50.0f);
    if (h.compressionType != NONE && h.compressionType != BZIP2 && h.compressionType != ZLIB) {
        std::printf("ERROR: compression type not implemented\n");
        return 5;
    }
    threads = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), nblocks));

    std::vector<std::vector<uint8_t>> res(nblocks);
    std::vector<uint8_t> done(nblocks, 0);
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<uint64_t> next{0};
    std::atomic<int> err{0};

    auto worker = [&]() {
        std::vector<uint8_t> in(block_bytes), out(cap);
        for (;;) {
            const uint64_t id = next.fetch_add(1);
            if (id >= nblocks) break;
            size_t n = 0;
            gather_block(sym, g, id, bpp, in.data(), &n);
            uint32_t len = 0;
            int rc = err.load() ? 0 : compress_one(h.compressionType, in.data(), (uint32_t)n, out.data(), cap, &len, level);
            if (rc) {
                std::printf("ERROR: compressing block %llu failed (code %d)\n", (unsigned long long)id, rc);
                int z = 0;
                err.compare_exchange_strong(z, rc);
                len = 0;
            }
            std::vector<uint8_t> v(out.data(), out.data() + len);
            {
                std::lock_guard<std::mutex> lk(mu);
                res[id].swap(v);
                done[id] = 1;
            }
            cv.notify_all();
        }
    };
    std::vector<std::thread> pool;
    pool.reserve(threads);
    for (int i = 0; i < threads; ++i) pool.emplace_back(worker);

    int rc = sink.begin(h);
    uint64_t offset = 0;
    for (uint64_t id = 0; id < nblocks; ++id) {
        std::vector<uint8_t> blk;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return done[id] != 0; });
            blk.swap(res[id]);
        }
        if (!rc && !err.load()) rc = sink.append(blk.data(), blk.size());
        offset += blk.size();
        h.blockOffset[id] = offset;
    }
    for (auto& t : pool) t.join();
    if (err.load()) return err.load();
    if (rc) return rc;
    return sink.finish(h);
}

// --------------------------------------------------------------- switches --
// GPU bzip2 (default when a GPU is usable); env LFM_GPU_BZIP2=0 selects the
// host library for every block (the same bytes, for comparison).
bool gpu_decode_enabled()
{
    static const bool on = env_int("LFM_GPU_DECODE", 1) != 0;
    return on;
}

bool gpu_bzip2_enabled()
{
    static const bool on = env_int("LFM_GPU_BZIP2", 1) != 0;
    return on;
}

// the GPU bzip2 decoder (env LFM_GPU_BUNZIP2=0: host libbz2 per block)
bool gpu_bunzip2_enabled()
{
    static const bool on = env_int("LFM_GPU_BUNZIP2", 1) != 0;
    return on;
}

int normalize_header(klb_image_header& h)
{
    if (h.getBytesPerPixel() == 0) return 5;
    for (int d = 0; d < KLB_DATA_DIMS; ++d) {
        if (h.xyzct[d] == 0) return 3;
        if (h.blockSize[d] == 0) h.blockSize[d] = 1;
        h.blockSize[d] = std::min(h.blockSize[d], h.xyzct[d]);  // klb_imageIO.cpp:2402-2404
    }
    if (h.compressionType != NONE && h.compressionType != BZIP2 && h.compressionType != ZLIB) {
        std::printf("ERROR: compression type %d not implemented\n", (int)h.compressionType);
        return 5;
    }
    return 0;
}

// ------------------------------------------------------------ z-slab merge --
int merge_slabs(const uint8_t* const* slabs, const uint64_t* lens, int n, std::vector<uint8_t>* out)
{
    if (n <= 0 || !slabs || !lens || !out) return 3;
    std::vector<klb_image_header> hs(n);
    for (int i = 0; i < n; ++i)
        if (hs[i].parseHeader(slabs[i], lens[i])) return 3;
    const klb_image_header& h0 = hs[0];
    if (h0.xyzct[3] != 1 || h0.xyzct[4] != 1) return 3;
    const uint32_t bz = h0.blockSize[2];
    uint64_t Z = 0, nb = 0, payload = 0;
    for (int i = 0; i < n; ++i) {
        const klb_image_header& hi = hs[i];
        bool same = hi.xyzct[0] == h0.xyzct[0] && hi.xyzct[1] == h0.xyzct[1] && hi.xyzct[3] == 1 &&
                    hi.xyzct[4] == 1 && hi.dataType == h0.dataType && hi.compressionType == h0.compressionType &&
                    hi.headerVersion == h0.headerVersion && hi.Nnum == h0.Nnum &&
                    std::memcmp(hi.pixelSize, h0.pixelSize, sizeof(h0.pixelSize)) == 0 &&
                    std::memcmp(hi.metadata, h0.metadata, KLB_METADATA_SIZE) == 0 &&
                    hi.blockSize[0] == h0.blockSize[0] && hi.blockSize[1] == h0.blockSize[1];
        if (i + 1 < n) same = same && hi.blockSize[2] == bz && hi.xyzct[2] % bz == 0;
        else same = same && hi.blockSize[2] == std::min(bz, hi.xyzct[2]);
        if (!same) {
            std::printf("ERROR: slab %d does not continue slab 0 (dims, type, predictor or block depth)\n", i);
            return 3;
        }
        const uint64_t hsz = hi.getSizeInBytes();
        const uint64_t body = hi.Nb ? hi.blockOffset[hi.Nb - 1] : 0;
        if (hsz + body > lens[i]) return 3;
        Z += hi.xyzct[2];
        nb += hi.Nb;
        payload += body;
    }
    klb_image_header H = h0;
    H.xyzct[2] = (uint32_t)Z;
    H.resizeBlockOffset(H.calculateNumBlocks());
    if (H.Nb != nb) return 3;
    uint64_t acc = 0, b = 0;
    for (int i = 0; i < n; ++i) {
        uint64_t prev_end = 0;
        for (size_t j = 0; j < hs[i].Nb; ++j) {
            acc += hs[i].blockOffset[j] - prev_end;
            prev_end = hs[i].blockOffset[j];
            H.blockOffset[b++] = acc;
        }
    }
    const size_t hsz = H.getSizeInBytes();
    out->assign(hsz + payload, 0);
    H.serialize(out->data(), hsz);
    uint8_t* dst = out->data() + hsz;
    for (int i = 0; i < n; ++i) {
        const uint64_t body = hs[i].Nb ? hs[i].blockOffset[hs[i].Nb - 1] : 0;
        std::memcpy(dst, slabs[i] + hs[i].getSizeInBytes(), body);
        dst += body;
    }
    return 0;
}

} // namespace lfm
