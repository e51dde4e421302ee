// lfm_decode_multi.cpp -- the whole-image reader farmed across the GPUs of one
// node: the reader's mirror of encode_multi.
//
// One .lfm is cut into ranges of whole block layers (decode_shard_plan: the
// writer's split along t, else c, else z).  Such a range is a box of whole
// blocks whose streams are one consecutive run of the payload, so the region
// reader (decode_roi, its `exact` branch) decodes it straight into its slice
// of the destination: no temporary image, no crop, no block decoded twice.
// One host thread per shard sets its device and runs that region decode with
// the existing kernels; no data crosses between GPUs.
//
// The pipelined decode keeps its device buffers, streams and pinned staging
// per host thread (lfm_decode.cpp, lfm_transfer.cpp).  The shard threads are
// therefore kept alive between calls, one per (device, slot on that device):
// a second call on the same device list finds every buffer where the first
// left it.  release_decode_workers() ends the threads, which frees them.
#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "lfm_engine.h"
#include "lfm_hip.h"
#include "lfm_internal.h"

namespace lfm {

namespace {
std::mutex g_dev_mu;
std::vector<int> g_devices;  // lfm_set_decode_devices; empty = env LFM_DECODE_GPUS

// A kept host thread that runs one job at a time.  `use` is held by the
// decode_multi call that has the worker, from before its job is started until
// it has been waited for.
struct Worker {
    std::mutex use;
    void start(std::function<void()> f)
    {
        std::lock_guard<std::mutex> lk(mu);
        job = std::move(f);
        busy = true;
        if (!th.joinable()) th = std::thread([this] { loop(); });
        cv.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !busy; });
    }
    // the thread exits: its thread_local decode state is destroyed
    void stop()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
        quit = false;
    }

private:
    void loop()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return quit || job; });
            if (!job) return;
            std::function<void()> f = std::move(job);
            job = nullptr;
            lk.unlock();
            f();
            lk.lock();
            busy = false;
            cv.notify_all();
        }
    }
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool busy = false, quit = false;
    std::thread th;
};

// Entries are never removed (a stopped worker restarts with its next job), so
// a pointer taken under the lock stays valid; the map itself is never
// destroyed: a worker may still sit in its wait when the process exits.
std::mutex g_pool_mu;
std::map<std::pair<int, int>, Worker*>& pool()
{
    static auto* p = new std::map<std::pair<int, int>, Worker*>;
    return *p;
}
Worker* pooled_worker(int dev, int slot)
{
    std::lock_guard<std::mutex> lk(g_pool_mu);
    Worker*& w = pool()[{dev, slot}];
    if (!w) w = new Worker;
    return w;
}

// does the pipelined GPU decode take this file (decode_payload's and
// gpu_decode's conditions)?  Anything else is not farmed.
bool farmable(const klb_image_header& h, size_t payload_len)
{
    if (h.compressionType != BZIP2 || !gpu_decode_enabled() || !gpu_bunzip2_enabled()) return false;
    const size_t bpp = h.getBytesPerPixel();
    const int k = h.headerVersion & 0x7F;
    if (!bpp || (bpp == 2 && k != 0 && (k > 7 || h.Nnum == 0 || h.Nnum > 31))) return false;
    const BlockGrid g(h);
    if (!g.nblocks || g.nblocks != h.Nb || g.nblocks >= (1ull << 31) || !h.getBlockSizeBytes()) return false;
    uint64_t end = 0;
    for (uint64_t i = 0; i < g.nblocks; ++i) {
        if (i && h.getBlockOffset(i) != end) return false;  // not contiguous
        end = h.getBlockOffset(i) + h.getBlockCompressedSizeBytes(i);
    }
    return end <= payload_len && lfm_hip_device_count() > 0;
}
} // namespace

void set_decode_devices(const std::vector<int>& devs)
{
    std::lock_guard<std::mutex> lk(g_dev_mu);
    g_devices = devs;
}

std::vector<int> default_decode_devices(int n)
{
    const char* e = std::getenv("LFM_DECODE_GPUS");
    return (e && *e) ? parse_device_list(e, n) : std::vector<int>();
}

std::vector<int> decode_devices()
{
    {
        std::lock_guard<std::mutex> lk(g_dev_mu);
        if (!g_devices.empty()) return g_devices;
    }
    const char* e = std::getenv("LFM_DECODE_GPUS");
    if (!e || !*e) return {};  // (the default: no device call at all)
    return parse_device_list(e, lfm_hip_device_count());
}

void release_decode_workers()
{
    std::vector<Worker*> all;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        for (auto& kv : pool()) all.push_back(kv.second);
    }
    for (Worker* w : all) {  // (in the map's (device, slot) order, as decode_multi locks them)
        std::lock_guard<std::mutex> lk(w->use);
        w->stop();
    }
}

ShardPlan decode_shard_plan(const klb_image_header& h, int nworkers)
{
    ShardPlan p;
    const BlockGrid g(h);
    p.axis = h.xyzct[4] > 1 ? 4 : (h.xyzct[3] > 1 ? 3 : 2);
    const uint64_t unit = std::max<uint64_t>(1, g.bs[p.axis]), dim = h.xyzct[p.axis];
    const uint64_t nunits = (dim + unit - 1) / unit;
    const bool predicted = h.getBytesPerPixel() == 2 && (h.headerVersion & 0x7F) != 0;
    const bool video = (h.headerVersion >> 7) & 1;
    // granule: the layers a shard boundary may fall between
    const uint64_t gran = (p.axis == 2 && predicted && video && (unit & 1)) ? 2 : 1;
    const uint64_t ngran = (nunits + gran - 1) / gran;
    const uint64_t n = (uint64_t)std::max(1, nworkers);
    const uint64_t per = std::max<uint64_t>(1, (ngran + n - 1) / n);
    const uint64_t S = std::max<uint64_t>(1, (ngran + per - 1) / per);
    for (uint64_t w = 0; w < S; ++w) {
        const uint64_t first = w * per * gran * unit;
        p.shards.emplace_back((uint32_t)first, (uint32_t)(std::min(dim, (w + 1) * per * gran * unit) - first));
    }
    return p;
}

int decode_multi(const uint8_t* buf, size_t len, const klb_image_header& h, uint8_t* img, void* const* d_out,
                 const uint64_t* out_bytes, int n_out, int threads, const std::vector<int>& devs,
                 lfm_decode_multi_stats* stats, lfm_decode_shard* shards, int shard_cap)
{
    const auto t0 = clk::now();
    const bool to_device = d_out != nullptr;
    if (!buf || (to_device ? (!out_bytes || n_out < 1) : !img)) return 3;
    const size_t hs = h.getSizeInBytes();
    if (hs > len) return 3;
    if (threads <= 0) threads = default_threads();
    const ShardPlan plan = decode_shard_plan(h, to_device ? n_out : (int)devs.size());
    const int axis = plan.axis;
    if (to_device && (int)plan.shards.size() != n_out) return 3;
    const int S = (int)plan.shards.size();
    if (stats) std::memset(stats, 0, sizeof(*stats));
    auto report = [&](int workers, const lfm_decode_shard* sh, int n) {
        if (stats) {
            stats->axis = axis;
            stats->workers = workers;
            for (int w = 0; w < n; ++w) {
                stats->blocks += sh[w].stats.blocks;
                stats->host_blocks += sh[w].stats.host_blocks;
                stats->d2h_bytes += sh[w].stats.d2h_bytes;
            }
            stats->total_ms = ms_since(t0);
        }
        for (int w = 0; shards && w < n && w < shard_cap; ++w) shards[w] = sh[w];
        if (decode_timing())
            std::fprintf(stderr, "decode multi: %d worker(s) along axis %d, total %.2f ms\n", workers, axis,
                         ms_since(t0));
    };

    // one shard, or a file the pipelined decode does not take: today's call
    if (S < 2 || (!to_device && !farmable(h, len - hs))) {
        lfm_decode_shard one{};
        one.first = 0;
        one.count = h.xyzct[axis];
        one.device = -1;
        if (to_device) {
            hipPointerAttribute_t attr;
            if (S == 1 && d_out[0] && hipPointerGetAttributes(&attr, d_out[0]) == hipSuccess) one.device = attr.device;
            else (void)hipGetLastError();
            one.rc = S == 1 ? decode_memory_device(buf, len, nullptr, nullptr, d_out[0], out_bytes[0], threads, &one.stats)
                            : 3;
        } else {
            if (lfm_hip_device_count() > 0 && hipGetDevice(&one.device) != hipSuccess) one.device = -1;
            one.rc = decode_payload(buf + hs, len - hs, h, img, threads, current_family(), nullptr, &one.stats);
            one.stats.total_ms = ms_since(t0);
        }
        report(1, &one, 1);
        return one.rc;
    }

    struct Work {
        int slot = 0;
        Worker* wk = nullptr;
        lfm_decode_shard sh{};
    };
    std::vector<Work> work(S);
    std::map<int, int> slots;
    for (int w = 0; w < S; ++w) {
        lfm_decode_shard& sh = work[w].sh;
        sh.first = plan.shards[w].first;
        sh.count = plan.shards[w].second;
        sh.rc = 3;
        if (to_device) {  // the buffer's device, as decode_memory_device finds it
            hipPointerAttribute_t attr;
            if (!d_out[w] || hipPointerGetAttributes(&attr, d_out[w]) != hipSuccess) {
                (void)hipGetLastError();
                return 3;
            }
            if (attr.type != hipMemoryTypeDevice) return 3;
            sh.device = attr.device;
        } else {
            sh.device = devs[w];
        }
        work[w].slot = slots[sh.device]++;
    }
    // Every worker this call uses is taken here, by the calling thread, in one
    // global (device, slot) order and held until its job is done: two
    // concurrent calls whose device lists differ in order can then never hold
    // one worker each while waiting for the other's.
    std::vector<int> order(S);
    for (int w = 0; w < S; ++w) order[w] = w;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        return std::make_pair(work[a].sh.device, work[a].slot) < std::make_pair(work[b].sh.device, work[b].slot);
    });
    std::vector<std::unique_lock<std::mutex>> held(S);
    for (int w : order) {
        work[w].wk = pooled_worker(work[w].sh.device, work[w].slot);
        held[w] = std::unique_lock<std::mutex>(work[w].wk->use);
    }

    uint64_t stride = h.getBytesPerPixel();  // bytes between consecutive indices along the axis
    for (int d = 0; d < axis; ++d) stride *= h.xyzct[d];
    const int wthreads = std::max(1, threads / S);
    const int family = current_family();
    for (int w = 0; w < S; ++w)
        work[w].wk->start([&, w] {
            lfm_decode_shard& sh = work[w].sh;
            const auto ts = clk::now();
            uint32_t lb[5] = {0, 0, 0, 0, 0}, ub[5];
            for (int d = 0; d < 5; ++d) ub[d] = h.xyzct[d] - 1;
            lb[axis] = sh.first;
            ub[axis] = sh.first + sh.count - 1;
            try {
                if (to_device) {
                    sh.rc = decode_memory_device(buf, len, lb, ub, d_out[w], out_bytes[w], wthreads, &sh.stats);
                } else if (hipSetDevice(sh.device) != hipSuccess) {
                    (void)hipGetLastError();
                    sh.rc = 3;
                } else {
                    sh.rc = decode_roi(buf + hs, len - hs, h, lb, ub, img + (uint64_t)sh.first * stride, wthreads,
                                       family, nullptr, &sh.stats);
                    sh.stats.total_ms = ms_since(ts);
                }
            } catch (...) {  // (out of host memory)
                sh.rc = 3;
            }
        });
    // every worker is waited for before the call returns; the work ran on
    // the workers' threads, so the caller's current device was never changed
    for (int w = 0; w < S; ++w) work[w].wk->wait();
    for (auto& l : held) l.unlock();
    int rc = 0;
    std::vector<lfm_decode_shard> sh(S);
    for (int w = 0; w < S; ++w) {
        sh[w] = work[w].sh;
        if (!rc) rc = sh[w].rc;
    }
    report(S, sh.data(), S);
    return rc;
}

int decode_image(const uint8_t* buf, size_t len, const klb_image_header& h, uint8_t* img, int threads)
{
    const std::vector<int> devs = decode_devices();
    if (devs.size() >= 2) return decode_multi(buf, len, h, img, nullptr, nullptr, 0, threads, devs, nullptr, nullptr, 0);
    const size_t hs = h.getSizeInBytes();
    return decode_payload(buf + hs, len - hs, h, img, threads, current_family());
}

} // namespace lfm
