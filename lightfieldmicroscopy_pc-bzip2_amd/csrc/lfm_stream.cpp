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
// Checkpoints: a finished range of whole layers also writes its entries into
// the capacity-sized table, behind its payload, so a file that is never closed
// still tells where its complete layers lie (committed_prefix): recover_file
// finalises such a file with the code close uses, and a live FileReader reads
// it while the writer runs.
//
// Reader.  The header and the table are read at open; a region read hands
// decode_roi a PayloadSource that preads the region's blocks.
#include <algorithm>
#include <cerrno>
#include <cmath>
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
    const uint64_t ticket = pending_.front(), n = pending_n_.front();
    pending_.erase(pending_.begin());
    pending_n_.erase(pending_n_.begin());
    const PinnedBuffer* b = nullptr;
    if (int rc = enc_.wait(ticket, &b, nullptr)) return rc;
    klb_image_header hs;
    if (!b || hs.parseHeader(b->data(), b->size())) return 3;
    const uint64_t hsz = hs.getSizeInBytes(), body = hs.Nb ? hs.blockOffset[hs.Nb - 1] : 0;
    if (hsz + body > b->size() || table_.size() + hs.Nb > nb_cap_) return 3;
    if (!table_.empty() && hs.headerVersion != hv_final_) return 3;
    hv_final_ = hs.headerVersion;
    const uint64_t first_block = table_.size();
    uint64_t prev_end = 0;
    for (size_t j = 0; j < hs.Nb; ++j) {
        table_.push_back(payload_ + hs.blockOffset[j]);
        if (hs.blockOffset[j] < prev_end) return 3;
        prev_end = hs.blockOffset[j];
    }
    if (!pwrite_all(fd_, b->data() + hsz, body, payload_base_ + payload_)) return 5;
    payload_ += body;
    // checkpoint, behind the payload: the header byte the ranges produce (once),
    // then the range's table entries as close will write them.  Not for the
    // stack's last, partial layer (encoded at close, which rewrites the table
    // right after): it has a whole layer's block count, and a recovery would
    // take it for one.
    if (n % unit_ == 0) {
        if (!hv_on_disk_ && !pwrite_all(fd_, &hv_final_, 1, 0)) return 5;
        hv_on_disk_ = true;
        if (!pwrite_all(fd_, (const uint8_t*)(table_.data() + first_block), 8 * hs.Nb,
                        cap_.getSizeInBytesFixPortion() + 8 * first_block))
            return 5;
        st_.committed += n;
    }
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
    pending_n_.push_back(n);
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

// The closing steps of a streamed file, for StreamWriter::close and
// recover_file alike: the header of the final extent (H: xyzct[axis] and
// headerVersion as they end up, the block size as asked for) with the table of
// its nb blocks, the payload (table[nb - 1] bytes at payload_base of src_fd)
// behind it in dst_fd, and the truncate.  In one file (src_fd == dst_fd) a
// shorter table means the payload moves down over the entries it does not use.
static int finalise_file(int src_fd, int dst_fd, klb_image_header& H, const uint64_t* table, uint64_t nb,
                         uint64_t payload_base, uint64_t* moved_bytes, uint64_t* bytes_written)
{
    if (int rc = normalize_header(H)) return rc;
    if (!nb || nb != H.calculateNumBlocks()) return 3;
    H.resizeBlockOffset(nb);
    std::memcpy(H.blockOffset, table, nb * sizeof(uint64_t));
    const uint64_t base = H.getSizeInBytes(), payload = table[nb - 1];
    if (src_fd != dst_fd || base < payload_base) {
        // forward chunked copy: a chunk is written below where it was read,
        // so no byte is overwritten before it has been read
        std::vector<uint8_t> chunk((size_t)std::min<uint64_t>(payload ? payload : 1, (uint64_t)32 << 20));
        for (uint64_t off = 0; off < payload; off += chunk.size()) {
            const uint64_t n = std::min<uint64_t>(chunk.size(), payload - off);
            if (!pread_all(src_fd, chunk.data(), n, payload_base + off) ||
                !pwrite_all(dst_fd, chunk.data(), n, base + off))
                return 5;
        }
        *moved_bytes = payload;
    }
    std::vector<uint8_t> head(base, 0);
    H.serialize(head.data(), head.size());
    if (!pwrite_all(dst_fd, head.data(), head.size(), 0)) return 5;
    if (::ftruncate(dst_fd, (off_t)(base + payload)) != 0) return 5;
    *bytes_written = base + payload;
    return 0;
}

// the table and the final extent; a stack shorter than the capacity has a
// shorter table, and its payload moves down over the entries it does not use
int StreamWriter::finish_file()
{
    klb_image_header H(cap_);
    H.xyzct[axis_] = (uint32_t)appended_;
    H.headerVersion = hv_final_;
    if (table_.size() > nb_cap_ || (!table_.empty() && table_.back() != payload_)) return 3;
    if (int rc = finalise_file(fd_, fd_, H, table_.data(), table_.size(), payload_base_, &st_.moved_bytes,
                               &st_.bytes_written))
        return rc;
    st_.header_version = H.headerVersion;
    st_.chosen = H.headerVersion & 0x7F;
    st_.committed = appended_;
    return 0;
}

int StreamWriter::flush(bool sync, uint64_t* committed)
{
    if (committed) *committed = st_.committed;
    if (rc_) return rc_;
    if (fd_ < 0) return 3;
    const auto t0 = clk::now();
    int rc = 0;
    while (!rc && !pending_.empty()) rc = drain_one();
    if (!rc && sync && ::fdatasync(fd_) != 0) rc = 5;
    st_.total_ms += ms_since(t0);
    if (committed) *committed = st_.committed;
    return rc_ = rc;
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

// ------------------------------------------------- what an open file holds --
namespace {
// the fixed header of an open file and the table its extent asks for, into h:
// 0, or 2 when the file is shorter than that
int read_header(int fd, uint64_t file_bytes, klb_image_header& h)
{
    // the fixed part tells the table's length
    const size_t fixed = h.getSizeInBytesFixPortion();
    std::vector<uint8_t> head(fixed);
    if (file_bytes < fixed || !pread_all(fd, head.data(), fixed, 0)) return 2;
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
    if (nb && !pread_all(fd, head.data() + fixed, 8 * nb, fixed)) return 2;
    return h.parseHeader(head.data(), head.size()) ? 2 : 0;
}

bool file_size(int fd, uint64_t* n)
{
    struct stat sb;
    if (::fstat(fd, &sb) != 0) return false;
    *n = (uint64_t)sb.st_size;
    return true;
}
} // namespace

CommittedPrefix committed_prefix(const klb_image_header& ch, int axis, const uint64_t* table, uint64_t nb,
                                 uint64_t payload_bytes, uint64_t from)
{
    CommittedPrefix p;
    uint64_t i = std::min(from, nb), prev = i ? table[i - 1] : 0;
    while (i < nb && table[i] > prev && table[i] <= payload_bytes) prev = table[i++];  // (> prev >= 0: non-zero)
    p.blocks = i;
    // (the float ceil of calculateNumBlocks, so nb is a multiple of it)
    const uint64_t layers_cap = (uint64_t)std::ceil((float)ch.xyzct[axis] / (float)ch.blockSize[axis]);
    p.layer_blocks = layers_cap ? nb / layers_cap : 0;
    p.layers = p.layer_blocks ? p.blocks / p.layer_blocks : 0;
    return p;
}

// ------------------------------------------------------------------ reader --
FileReader::~FileReader()
{
    if (fd_ >= 0) ::close(fd_);
}

// the header and the table its extent asks for into h, as of a closed file
// (2: the file is shorter than that); *closed = its table is a closed file's
int FileReader::load(bool* closed)
{
    if (!file_size(fd_, &file_bytes)) return 2;
    if (int rc = read_header(fd_, file_bytes, h)) return rc;
    const uint64_t head = h.getSizeInBytes();
    bytes_read += head;
    payload_base_ = head;
    axis_ = stream_axis(h);
    live_ = false;
    // not: a table that points past the file's end, or a zero one (the writer never closed it)
    const uint64_t end = h.Nb ? h.blockOffset[h.Nb - 1] : 0;
    *closed = !(head + end > file_bytes || (h.Nb && end == 0));
    return 0;
}

// the committed whole layers of cap_'s table as a header of their own: the
// extent along the axis (0 when no layer is complete) and their entries
void FileReader::make_view()
{
    const uint64_t capacity = cap_.xyzct[axis_];
    const uint64_t payload_bytes = file_bytes > payload_base_ ? file_bytes - payload_base_ : 0;
    const CommittedPrefix p = committed_prefix(cap_, axis_, cap_.blockOffset, cap_.Nb, payload_bytes, known_);
    known_ = p.layers * p.layer_blocks;
    live_ = p.blocks < cap_.Nb;  // a complete table: the writer has closed a stack that reached the capacity
    uint32_t xs[KLB_DATA_DIMS];
    std::memcpy(xs, cap_.xyzct, sizeof(xs));
    xs[axis_] = (uint32_t)std::min<uint64_t>(p.layers * cap_.blockSize[axis_], capacity);
    h.setHeader(xs, cap_.dataType, cap_.pixelSize, cap_.blockSize, cap_.compressionType, cap_.metadata,
                cap_.headerVersion, cap_.Nnum);
    h.resizeBlockOffset(known_);
    if (known_) std::memcpy(h.blockOffset, cap_.blockOffset, known_ * sizeof(uint64_t));
}

int FileReader::open(const char* filename, bool live)
{
    fd_ = ::open(filename, O_RDONLY);
    if (fd_ < 0) {
        std::printf("ERROR: file %s could not be opened\n", filename);
        return 2;
    }
    bool closed = false;
    if (int rc = load(&closed)) return rc;
    if (closed) return 0;
    if (!live) return 2;
    cap_ = h;
    known_ = 0;
    make_view();
    return 0;
}

int FileReader::refresh(uint32_t* extent)
{
    if (fd_ < 0) return 3;
    if (live_) {
        uint8_t fixed[320];
        uint32_t xs[KLB_DATA_DIMS];
        if (!file_size(fd_, &file_bytes) || !pread_all(fd_, fixed, sizeof(fixed), 0)) return 2;
        bytes_read += sizeof(fixed);
        std::memcpy(xs, fixed + 2, sizeof(xs));
        if (xs[axis_] != cap_.xyzct[axis_]) {
            // closed meanwhile with fewer indices than the capacity: a shorter table, the payload moved
            bool closed = false;
            if (int rc = load(&closed)) return rc;
            if (!closed) return 2;
        } else {
            cap_.headerVersion = fixed[0];  // (the request until the first checkpoint)
            const uint64_t rest = cap_.Nb - known_;
            if (rest && !pread_all(fd_, (uint8_t*)(cap_.blockOffset + known_), 8 * rest,
                                   cap_.getSizeInBytesFixPortion() + 8 * known_))
                return 2;
            bytes_read += 8 * rest;
            make_view();
        }
    }
    if (extent) *extent = h.xyzct[axis_];
    return 0;
}

int FileReader::read(const uint32_t lb[5], const uint32_t ub[5], void* out, uint64_t out_bytes, bool dev, int threads,
                     lfm_decode_stats* stats)
{
    if (fd_ < 0 || !lb || !ub || !out) return 3;
    PayloadSource src;
    src.fd = fd_;
    src.base = payload_base_;  // (a live file's payload lies behind the capacity-sized table, not h's)
    src.len = file_bytes > src.base ? file_bytes - src.base : 0;
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

// ---------------------------------------------------------------- recovery --
namespace {

// Stream-level verification of an unclosed file's committed layers, one layer
// at a time: every stream must decode to its block's byte count (bzip2: its
// CRCs hold; ZLIB: it inflates; NONE: the stored size is all there is to
// check).  No inverse predictor runs.  bzip2 streams go through the GPU
// decoder when a device is visible, the ones it hands back (flag 1) and all of
// them without a device through the host library.
class LayerVerifier {
public:
    LayerVerifier(int fd, const klb_image_header& view, uint64_t payload_base, uint64_t layer_blocks, int threads,
                  lfm_recover_stats& s)
        : fd_(fd), h_(view), g_(view), base_(payload_base), lb_(layer_blocks), threads_(threads), s_(s)
    {
        block_bytes_ = h_.getBlockSizeBytes();
        gpu_ = h_.compressionType == BZIP2 && block_bytes_ && gpu_bunzip2_enabled() && lfm_hip_device_count() > 0;
        // the level that sizes a stream's slots, as the pipelined decode derives it (0: single-block entries)
        level_ = bunzip2_multiblock() ? std::min<uint32_t>(9, std::max<uint32_t>(1, (block_bytes_ + 99999) / 100000)) : 0;
    }

    // layer L's streams all pass
    bool layer_ok(uint64_t L)
    {
        const uint64_t b0 = L * lb_;
        const uint64_t* end = h_.blockOffset;
        const uint64_t off0 = b0 ? end[b0 - 1] : 0, bytes = end[b0 + lb_ - 1] - off0;
        pay_.assign(bytes + 64, 0);  // (the GPU bit reader looks ahead past the last stream)
        if (!pread_all(fd_, pay_.data(), bytes, base_ + off0)) return false;
        offs_.resize(lb_ + 1);
        expect_.resize(lb_);
        for (uint64_t i = 0; i < lb_; ++i) {
            uint64_t o[5], sz[5];
            g_.block(b0 + i, o, sz);
            expect_[i] = h_.getBytesPerPixel() * sz[0] * sz[1] * sz[2] * sz[3] * sz[4];
            offs_[i] = (i ? end[b0 + i - 1] : off0) - off0;
            if (end[b0 + i] - off0 - offs_[i] >= ((uint64_t)1 << 32)) return false;  // (no block compresses to 4 GiB)
        }
        offs_[lb_] = bytes;
        s_.verified_streams += lb_;
        host_.clear();
        if (gpu_) {
            const int r = gpu_streams();
            if (r < 0) gpu_ = false;  // a device error says nothing about the file: the host library decides
            else if (r > 0) return false;
        }
        if (!gpu_)
            for (uint64_t i = 0; i < lb_; ++i) host_.push_back(i);
        return host_streams();
    }

private:
    // the layer's streams on the device in batches; flag 1 streams are left to
    // host_.  0, 1 when a stream failed, -1 on a device error
    int gpu_streams()
    {
        const uint64_t kBatch = 4096;  // (about the streams the Huffman kernel holds resident at once)
        const uint64_t nbatch = std::min<uint64_t>(lb_, kBatch);
        const size_t ws = level_ ? lfm_hip_bunzip2_workspace_bytes_multi((uint32_t)nbatch, block_bytes_, level_)
                                 : lfm_hip_bunzip2_workspace_bytes((uint32_t)nbatch, block_bytes_);
        void* d_pay = d_pay_.reserve(pay_.size());
        void* d_ws = d_ws_.reserve(ws);
        void* d_out = d_out_.reserve((size_t)nbatch * block_bytes_);
        if (!ws || !d_pay || !d_ws || !d_out) {
            (void)hipGetLastError();
            return -1;
        }
        if (hipMemcpy(d_pay, pay_.data(), pay_.size(), hipMemcpyHostToDevice) != hipSuccess) return -1;
        lens_.resize(nbatch);
        flags_.resize(nbatch);
        for (uint64_t i0 = 0; i0 < lb_; i0 += nbatch) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(nbatch, lb_ - i0);
            const int rc = level_ ? lfm_hip_bunzip2_blocks_multi(d_pay, offs_.data() + i0, n, d_out, block_bytes_, level_,
                                                                 d_ws, ws, lens_.data(), flags_.data(), nullptr)
                                  : lfm_hip_bunzip2_blocks(d_pay, offs_.data() + i0, n, d_out, block_bytes_, d_ws, ws,
                                                           lens_.data(), flags_.data(), nullptr);
            if (rc != LFM_HIP_OK) return -1;
            for (uint32_t i = 0; i < n; ++i) {
                if (flags_[i] == 1) host_.push_back(i0 + i);
                else if (flags_[i] != 0 || lens_[i] != expect_[i0 + i]) return 1;
            }
        }
        return 0;
    }

    // the streams listed in host_ through the host library
    bool host_streams()
    {
        std::atomic<bool> bad{false};
        std::atomic<uint64_t> decoded{0};
        const int ctype = h_.compressionType;
        parallel_for(host_.size(), threads_, [&](uint64_t j) {
            if (bad.load()) return;
            const uint64_t i = host_[j], n = offs_[i + 1] - offs_[i];
            const uint8_t* in = pay_.data() + offs_[i];
            if (ctype == NONE) {
                if (n != expect_[i]) bad.store(true);
                return;
            }
            // (a stream without bzip2's stream and block magic is no work for the library)
            static const uint8_t magic[6] = {0x31, 0x41, 0x59, 0x26, 0x53, 0x59};
            if (ctype == BZIP2 && (n < 14 || in[0] != 'B' || in[1] != 'Z' || in[2] != 'h' || in[3] < '1' ||
                                   in[3] > '9' || std::memcmp(in + 4, magic, 6) != 0)) {
                bad.store(true);
                return;
            }
            thread_local std::vector<uint8_t> scratch;
            scratch.resize(std::max<uint64_t>(expect_[i], 1));
            ++decoded;
            if (decompress_one(ctype, in, (uint32_t)n, scratch.data(), (uint32_t)expect_[i])) bad.store(true);
        });
        s_.host_streams += decoded.load();
        return !bad.load();
    }

    int fd_;
    const klb_image_header& h_;
    BlockGrid g_;
    uint64_t base_, lb_;
    int threads_;
    lfm_recover_stats& s_;
    uint32_t block_bytes_ = 0, level_ = 0;
    bool gpu_ = false;
    std::vector<uint8_t> pay_;
    std::vector<uint64_t> offs_, expect_, host_;
    std::vector<uint32_t> lens_, flags_;
    DeviceBuffer d_pay_, d_ws_, d_out_;
};

} // namespace

int recover_file(const char* filename, const char* out_filename, bool verify, int threads, lfm_recover_stats* st)
{
    const auto t0 = clk::now();
    lfm_recover_stats s{};
    auto done = [&](int rc) {
        s.total_ms = ms_since(t0);
        if (st) *st = s;
        return rc;
    };
    if (!filename) return done(3);
    if (threads <= 0) threads = default_threads();
    struct Fd {
        int fd = -1;
        ~Fd()
        {
            if (fd >= 0) (void)::close(fd);
        }
    } in, out;
    // (an output that names the input is the in-place case, not an input truncated at open)
    struct stat sa, sb;
    bool in_place = !out_filename;
    if (out_filename && ::stat(filename, &sa) == 0 && ::stat(out_filename, &sb) == 0 && sa.st_dev == sb.st_dev &&
        sa.st_ino == sb.st_ino)
        in_place = true;
    in.fd = ::open(filename, in_place ? O_RDWR : O_RDONLY);
    uint64_t file_bytes = 0;
    klb_image_header cap;
    if (in.fd < 0 || !file_size(in.fd, &file_bytes) || read_header(in.fd, file_bytes, cap)) return done(2);
    const int axis = stream_axis(cap);
    const uint64_t capacity = cap.xyzct[axis], payload_base = cap.getSizeInBytes();
    s.axis = axis;
    s.capacity = capacity;
    s.header_version = cap.headerVersion;
    const CommittedPrefix p = committed_prefix(cap, axis, cap.blockOffset, cap.Nb, file_bytes - payload_base);
    s.committed_blocks = p.blocks;
    if (cap.Nb && p.blocks == cap.Nb) {  // a closed .lfm
        s.already_valid = 1;
        s.kept = capacity;
        return done(0);
    }
    // the header of the committed layers (for the verifier: their blocks' sizes), then of the kept ones
    auto header_of = [&](uint64_t layers) {
        klb_image_header H(cap);
        H.xyzct[axis] = (uint32_t)std::min<uint64_t>(layers * cap.blockSize[axis], capacity);
        return H;
    };
    uint64_t layers = p.layers;
    if (verify && layers) {
        const klb_image_header view = header_of(layers);
        LayerVerifier v(in.fd, view, payload_base, p.layer_blocks, threads, s);
        uint64_t ok = 0;
        while (ok < layers && v.layer_ok(ok)) ++ok;
        layers = ok;
    }
    // what the table names and the result lacks: layers whose entries are there
    // but not plausible (torn), and layers that failed verification
    uint64_t named = 0;
    while (named < cap.Nb && cap.blockOffset[named]) ++named;
    s.dropped_layers = (p.layer_blocks ? named / p.layer_blocks : 0) - layers;
    if (!layers) return done(3);
    klb_image_header H = header_of(layers);
    s.kept = H.xyzct[axis];
    int dst = in.fd;
    if (!in_place) {
        out.fd = ::open(out_filename, O_RDWR | O_CREAT | O_TRUNC, 0666);
        if (out.fd < 0) return done(5);
        dst = out.fd;
    }
    int rc = finalise_file(in.fd, dst, H, cap.blockOffset, layers * p.layer_blocks, payload_base, &s.moved_bytes,
                           &s.bytes_written);
    if (!in_place) {
        if (::close(out.fd) != 0 && !rc) rc = 5;
        out.fd = -1;
        if (rc) (void)::unlink(out_filename);
    }
    return done(rc);
}

} // namespace lfm
