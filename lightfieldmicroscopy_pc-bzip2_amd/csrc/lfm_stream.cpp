// lfm_stream.cpp -- stacks larger than memory: the append writer (lfm_writer)
// and the ranged file reader (lfm_reader).
//
// Writer.  encode_multi (lfm_multigpu.cpp) cuts a stack that lies in memory
// into ranges of whole block layers and appends their payloads in order; here
// the ranges arrive over time.  Block ids run x -> y -> z -> c -> t, so a range
// of layers along the stream axis is a contiguous id range of the file and the
// payloads concatenate; the offset table is a running sum of block sizes.  The
// table's length depends on the final extent, which is known only at close:
// the file is laid out for the capacity given at open, and a shorter stack
// has its payload moved down over the unused table entries at close.
//
// Reader.  The header and the table are read at open; a region read hands
// decode_roi a PayloadSource that preads the region's blocks.
#include <algorithm>
#include <cerrno>
#include <cstring>
#include <string>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "lfm_engine.h"
#include "lfm_hip.h"
#include "lfm_internal.h"

namespace lfm {

// every byte of [off, off + n) of the file written / read, or false
bool pwrite_all(int fd, const uint8_t* src, uint64_t n, uint64_t off)
{
    while (n) {
        const ssize_t put = ::pwrite(fd, src, (size_t)std::min<uint64_t>(n, (uint64_t)1 << 30), (off_t)off);
        if (put < 0 && errno == EINTR) continue;
        if (put <= 0) return false;
        src += put, off += (uint64_t)put, n -= (uint64_t)put;
    }
    return true;
}

bool pread_all(int fd, uint8_t* dst, uint64_t n, uint64_t off)
{
    while (n) {
        const ssize_t got = ::pread(fd, dst, (size_t)std::min<uint64_t>(n, (uint64_t)1 << 30), (off_t)off);
        if (got < 0 && errno == EINTR) continue;
        if (got <= 0) return false;
        dst += got, off += (uint64_t)got, n -= (uint64_t)got;
    }
    return true;
}

namespace {
int stream_axis(const klb_image_header& h) { return h.xyzct[4] > 1 ? 4 : (h.xyzct[3] > 1 ? 3 : 2); }
} // namespace

// ------------------------------------------------------------------ writer --
StreamWriter::StreamWriter(const klb_image_header& h, int device, int threads)
    : enc_(device), cap_(h), threads_(threads > 0 ? threads : default_threads()), axis_(stream_axis(h)),
      hv_(h.headerVersion)
{
    for (int d = 0; d < KLB_DATA_DIMS; ++d)
        if (cap_.blockSize[d] == 0) cap_.blockSize[d] = 1;
    unit_ = cap_.blockSize[axis_];
    stride_ = cap_.getBytesPerPixel();
    for (int d = 0; d < axis_; ++d) stride_ *= cap_.xyzct[d];
}

StreamWriter::~StreamWriter()
{
    if (fd_ >= 0) ::close(fd_);
}

int StreamWriter::open(const char* filename)
{
    klb_image_header hc(cap_);
    if (int rc = normalize_header(hc)) return rc;
    nb_cap_ = hc.calculateNumBlocks();
    payload_base_ = hc.getSizeInBytesFixPortion() + 8 * nb_cap_;
    path_ = filename;
    fd_ = ::open(filename, O_RDWR | O_CREAT | O_TRUNC, 0666);
    if (fd_ < 0) {
        std::printf("ERROR: file %s could not be opened\n", filename);
        return 5;
    }
    // the fixed header and a zero table for the capacity; close rewrites both
    hc.resizeBlockOffset(nb_cap_);
    std::vector<uint8_t> head(hc.getSizeInBytes(), 0);
    hc.serialize(head.data(), head.size());
    return pwrite_all(fd_, head.data(), head.size(), 0) ? 0 : 5;
}

// buffer `which` (0 held-back part, 1 assembled range, 2 raw frame before the
// next range) of at least n bytes, in memory of the input's kind.  A device
// buffer's contents do not survive its growth: 0 and 2 are asked for with
// their final size the first time.
void* StreamWriter::stage_buffer(bool dev, int which, size_t n)
{
    if (dev) return d_buf_[which].reserve(n);
    if (h_buf_[which].size() < n) h_buf_[which].resize(n);
    return h_buf_[which].data();
}

// copy n input bytes between the caller's memory and the staging buffers;
// done (host-synchronised) on return.  A device copy goes to the null stream,
// so it comes after the work the caller queued there.
int StreamWriter::stage_copy(void* dst, const void* src, size_t n, bool dev)
{
    if (!n) return 0;
    if (!dev) {
        par_memcpy(dst, src, n, threads_);
        return 0;
    }
    return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, nullptr) == hipSuccess &&
                   hipStreamSynchronize(nullptr) == hipSuccess
               ? 0
               : 3;
}

int StreamWriter::drain_one()
{
    const uint64_t ticket = pending_.front();
    pending_.erase(pending_.begin());
    const PinnedBuffer* b = nullptr;
    if (int rc = enc_.wait(ticket, &b, nullptr)) return rc;
    klb_image_header hs;
    if (!b || hs.parseHeader(b->data(), b->size())) return 3;
    const uint64_t hsz = hs.getSizeInBytes(), body = hs.Nb ? hs.blockOffset[hs.Nb - 1] : 0;
    if (hsz + body > b->size() || table_.size() + hs.Nb > nb_cap_) return 3;
    if (!table_.empty() && hs.headerVersion != hv_final_) return 3;
    hv_final_ = hs.headerVersion;
    uint64_t prev_end = 0;
    for (size_t j = 0; j < hs.Nb; ++j) {
        table_.push_back(payload_ + hs.blockOffset[j]);
        if (hs.blockOffset[j] < prev_end) return 3;
        prev_end = hs.blockOffset[j];
    }
    if (!pwrite_all(fd_, b->data() + hsz, body, payload_base_ + payload_)) return 5;
    payload_ += body;
    st_.streams += enc_.last_counts.streams;
    st_.host_streams += enc_.last_counts.host_streams;
    st_.bzip2_blocks += enc_.last_counts.bzip2_blocks;
    return 0;
}

// one encode of the n indices at `data` (whole layers, or the stack's last
// part at close): indices [submitted_, submitted_ + n) of the stack
int StreamWriter::submit_range(const void* data, bool dev, uint64_t n)
{
    // the buffer set the next submit encodes into is the oldest pending one's
    if (pending_.size() >= 2)
        if (int rc = drain_one()) return rc;
    const uint64_t first = submitted_;
    klb_image_header hs(cap_);
    hs.headerVersion = hv_;
    hs.xyzct[axis_] = (uint32_t)n;
    SlabSpec slab;
    // the bzip2 level of the stack's nominal block (klb_imageIO.cpp:108).  A
    // stack that reaches first + n >= one layer keeps the block depth asked
    // for; a range that ends below one layer is the whole stack (encoded at
    // close), whose block the one-shot writer clamps to its extent.
    klb_image_header nominal(cap_);
    nominal.xyzct[axis_] = (uint32_t)(first + n);
    if (int rc = normalize_header(nominal)) return rc;
    slab.level = bzip2_level(nominal);
    if (axis_ == 2 && first > 0) {
        slab.z0 = (uint32_t)first;
        if (have_prev_) slab.prev = dev ? d_buf_[2].get() : (const void*)h_buf_[2].data();
    }
    uint64_t ticket = 0;
    if (int rc = enc_.submit(data, dev, hs, threads_, &slab, &ticket)) return rc;
    pending_.push_back(ticket);
    submitted_ += n;
    ++st_.ranges;
    // a video stack's next range starts with a temporal frame when its z0 is
    // odd (odd block depth): that frame is predicted from the raw frame before it
    have_prev_ = false;
    const bool video = (hv_ >> 7) & 1;
    if (axis_ == 2 && video && (submitted_ & 1) && cap_.getBytesPerPixel() == 2 && cap_.Nnum > 0) {
        void* p = stage_buffer(dev, 2, stride_);
        if (!p) return 3;
        if (int rc = stage_copy(p, (const uint8_t*)data + (n - 1) * stride_, stride_, dev)) return rc;
        have_prev_ = true;
    }
    return 0;
}

int StreamWriter::append(const void* img, bool dev, uint32_t count)
{
    if (rc_) return rc_;
    if (!img || count == 0 || fd_ < 0) return 3;
    if (kind_ >= 0 && kind_ != (dev ? 1 : 0)) return 3;
    const uint64_t capacity = cap_.xyzct[axis_];
    if (appended_ + count > capacity) return 3;
    const auto t0 = clk::now();
    kind_ = dev ? 1 : 0;
    auto fail = [&](int rc) {
        st_.total_ms += ms_since(t0);
        return rc_ = rc;
    };
    int caller_dev = -1;
    if (dev) {  // copies and buffers on the encoder's device; the caller's is put back
        if (hipGetDevice(&caller_dev) != hipSuccess) return fail(3);
        if (enc_.device() >= 0 && enc_.device() != caller_dev && hipSetDevice(enc_.device()) != hipSuccess)
            return fail(3);
    }
    struct Restore {
        int dev;
        ~Restore()
        {
            if (dev >= 0) (void)hipSetDevice(dev);
        }
    } restore{caller_dev};
    if (!selected_) {
        // selection once, on frame 0 of the stream (klb_imageIO.cpp:2316-2360),
        // then forced (request 8 + k) for every range, as encode_multi does
        if (cap_.getBytesPerPixel() == 2 && cap_.Nnum > 0 && (hv_ & 0x7F) < NUM_PREDICTORS) {
            int k = 0;
            if (int rc = enc_.select_frame(img, dev, cap_, &k, st_.entropy)) return fail(rc);
            hv_ = (uint8_t)((hv_ & 0x80) | (8 + k));
        }
        selected_ = true;
    }
    const uint8_t* src = (const uint8_t*)img;
    const uint64_t nfull = (staged_ + count) / unit_ * unit_;
    const uint64_t max_staged = std::min<uint64_t>(unit_ - 1, capacity);
    if (nfull == 0) {
        uint8_t* stage = (uint8_t*)stage_buffer(dev, 0, max_staged * stride_);
        if (!stage) return fail(3);
        if (int rc = stage_copy(stage + staged_ * stride_, src, count * stride_, dev)) return fail(rc);
        staged_ += count;
    } else {
        const uint64_t take = nfull - staged_;  // of this append's indices
        const void* range = src;
        if (staged_) {
            uint8_t* whole = (uint8_t*)stage_buffer(dev, 1, nfull * stride_);
            const void* stage = dev ? d_buf_[0].get() : (const void*)h_buf_[0].data();
            if (!whole || !stage) return fail(3);
            if (int rc = stage_copy(whole, stage, staged_ * stride_, dev)) return fail(rc);
            if (int rc = stage_copy(whole + staged_ * stride_, src, take * stride_, dev)) return fail(rc);
            range = whole;
        }
        if (int rc = submit_range(range, dev, nfull)) return fail(rc);
        staged_ = 0;
        if (const uint64_t rest = count - take) {
            uint8_t* stage = (uint8_t*)stage_buffer(dev, 0, max_staged * stride_);
            if (!stage) return fail(3);
            if (int rc = stage_copy(stage, src + take * stride_, rest * stride_, dev)) return fail(rc);
            staged_ = rest;
        }
    }
    appended_ += count;
    st_.appended = appended_;
    st_.staged_peak_bytes = std::max<uint64_t>(st_.staged_peak_bytes, staged_ * stride_);
    st_.total_ms += ms_since(t0);
    return 0;
}

// the table and the final extent; a stack shorter than the capacity has a
// shorter table, and its payload moves down over the entries it does not use
int StreamWriter::finish_file()
{
    klb_image_header H(cap_);
    H.xyzct[axis_] = (uint32_t)appended_;
    H.headerVersion = hv_final_;
    if (int rc = normalize_header(H)) return rc;
    const uint64_t nb = H.calculateNumBlocks();
    if (nb != table_.size() || nb > nb_cap_) return 3;
    H.resizeBlockOffset(nb);
    std::memcpy(H.blockOffset, table_.data(), nb * sizeof(uint64_t));
    const uint64_t base = H.getSizeInBytes();
    if (base < payload_base_) {
        // forward chunked copy: a chunk is written below where it was read,
        // so no byte is overwritten before it has been read
        std::vector<uint8_t> chunk((size_t)std::min<uint64_t>(payload_ ? payload_ : 1, (uint64_t)32 << 20));
        for (uint64_t off = 0; off < payload_; off += chunk.size()) {
            const uint64_t n = std::min<uint64_t>(chunk.size(), payload_ - off);
            if (!pread_all(fd_, chunk.data(), n, payload_base_ + off) ||
                !pwrite_all(fd_, chunk.data(), n, base + off))
                return 5;
        }
        st_.moved_bytes = payload_;
    }
    std::vector<uint8_t> head(base, 0);
    H.serialize(head.data(), head.size());
    if (!pwrite_all(fd_, head.data(), head.size(), 0)) return 5;
    if (::ftruncate(fd_, (off_t)(base + payload_)) != 0) return 5;
    st_.bytes_written = base + payload_;
    st_.header_version = H.headerVersion;
    st_.chosen = H.headerVersion & 0x7F;
    return 0;
}

int StreamWriter::close(lfm_writer_stats* st)
{
    const auto t0 = clk::now();
    int rc = rc_;
    if (!rc && (fd_ < 0 || appended_ == 0)) rc = 3;
    if (!rc && staged_) {  // the stack's last, partial layer -- or the whole of a stack below one layer
        int caller_dev = -1;
        const bool dev = kind_ == 1;
        if (dev && hipGetDevice(&caller_dev) == hipSuccess && enc_.device() >= 0 && enc_.device() != caller_dev)
            (void)hipSetDevice(enc_.device());
        rc = submit_range(dev ? d_buf_[0].get() : (const void*)h_buf_[0].data(), dev, staged_);
        if (caller_dev >= 0) (void)hipSetDevice(caller_dev);
        staged_ = 0;
    }
    while (!rc && !pending_.empty()) rc = drain_one();
    if (!rc) rc = finish_file();
    if (fd_ >= 0) {
        if (::close(fd_) != 0 && !rc) rc = 5;
        fd_ = -1;
        if (rc) (void)::unlink(path_.c_str());
    }
    rc_ = rc ? rc : 3;  // finished: nothing more is taken
    st_.total_ms += ms_since(t0);
    if (st) *st = st_;
    return rc;
}

void StreamWriter::abort()
{
    if (fd_ >= 0) {
        (void)::close(fd_);
        fd_ = -1;
        (void)::unlink(path_.c_str());
    }
    rc_ = 3;
}

// ------------------------------------------------------------------ reader --
FileReader::~FileReader()
{
    if (fd_ >= 0) ::close(fd_);
}

int FileReader::open(const char* filename)
{
    fd_ = ::open(filename, O_RDONLY);
    if (fd_ < 0) {
        std::printf("ERROR: file %s could not be opened\n", filename);
        return 2;
    }
    struct stat sb;
    if (::fstat(fd_, &sb) != 0) return 2;
    file_bytes = (uint64_t)sb.st_size;
    // the fixed part tells the table's length
    const size_t fixed = h.getSizeInBytesFixPortion();
    std::vector<uint8_t> head(fixed);
    if (file_bytes < fixed || !pread_all(fd_, head.data(), fixed, 0)) return 2;
    klb_image_header f;
    uint32_t xs[KLB_DATA_DIMS], bs[KLB_DATA_DIMS];
    std::memcpy(xs, head.data() + 2, sizeof(xs));
    std::memcpy(bs, head.data() + 300, sizeof(bs));
    for (int d = 0; d < KLB_DATA_DIMS; ++d)
        if (!bs[d]) return 2;
    f.setHeader(xs, UINT8_TYPE, nullptr, bs);
    const uint64_t nb = f.calculateNumBlocks();
    if (file_bytes < fixed + 8 * nb) return 2;
    head.resize(fixed + 8 * nb);
    if (nb && !pread_all(fd_, head.data() + fixed, 8 * nb, fixed)) return 2;
    if (h.parseHeader(head.data(), head.size())) return 2;
    bytes_read = head.size();
    // a table that points past the file's end (or a zero one: the writer never closed it)
    const uint64_t end = h.Nb ? h.blockOffset[h.Nb - 1] : 0;
    if (head.size() + end > file_bytes || (h.Nb && end == 0)) return 2;
    return 0;
}

int FileReader::read(const uint32_t lb[5], const uint32_t ub[5], void* out, uint64_t out_bytes, bool dev, int threads,
                     lfm_decode_stats* stats)
{
    if (fd_ < 0 || !lb || !ub || !out) return 3;
    PayloadSource src;
    src.fd = fd_;
    src.base = h.getSizeInBytes();
    src.len = file_bytes - src.base;
    src.fetched = &bytes_read;
    if (dev) return decode_source_device(src, h, lb, ub, out, out_bytes, threads, stats);
    const auto t0 = clk::now();
    uint64_t need = h.getBytesPerPixel();  // the region in the file's own data type
    for (int d = 0; d < KLB_DATA_DIMS; ++d) {
        if (ub[d] < lb[d] || ub[d] >= h.xyzct[d]) return 3;
        need *= (uint64_t)(ub[d] - lb[d] + 1);
    }
    if (!need || out_bytes < need) return 3;
    lfm_decode_stats s{};
    const int rc = decode_roi(src, h, lb, ub, (uint8_t*)out, threads, current_family(), nullptr, &s);
    s.total_ms = ms_since(t0);
    if (stats) *stats = s;
    return rc;
}

} // namespace lfm
