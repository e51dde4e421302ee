// lfm_transfer.cpp -- host <-> device copies of the engine: the HSA agent,
// the SDMA copies, the pinned staging chunks and the copy pool.
#include "lfm_transfer.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <hsa/hsa_ext_amd.h>

#include "lfm_engine.h"
#include "lfm_internal.h"

namespace lfm {

// ------------------------------------------------------------ SDMA copies --
// Device -> pinned host copies of the compressed payload on a system DMA
// engine (hsa_amd_memory_async_copy).  hipMemcpyAsync does these copies with a
// blit kernel whose PCIe-bound stores hold up the other HIP stream's kernels
// (measured 3x slower while a 140 MB payload copy runs); the SDMA engines
// leave the CUs and their caches to the compute.  Returns false (the caller
// falls back to hipMemcpyAsync) if HSA cannot take the copy; LFM_D2H_SDMA=0
// disables it.  The caller has synchronised the producing stream.
// the HSA CPU agent (SDMA copies are enabled and HSA is up), or null
const hsa_agent_t* hsa_cpu_agent()
{
    struct Cpu {
        bool ok = false;
        hsa_agent_t agent{};
        Cpu()
        {
            if (env_int("LFM_D2H_SDMA", 1) == 0 || hsa_init() != HSA_STATUS_SUCCESS) return;
            hsa_iterate_agents(
                [](hsa_agent_t a, void* d) {
                    hsa_device_type_t t;
                    if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) == HSA_STATUS_SUCCESS &&
                        t == HSA_DEVICE_TYPE_CPU) {
                        *(hsa_agent_t*)d = a;
                        return HSA_STATUS_INFO_BREAK;
                    }
                    return HSA_STATUS_SUCCESS;
                },
                &agent);
            ok = agent.handle != 0;
        }
    };
    static Cpu cpu;
    return cpu.ok ? &cpu.agent : nullptr;
}

bool hsa_owner(const void* p, hsa_agent_t* agent)
{
    hsa_amd_pointer_info_t info;
    std::memset(&info, 0, sizeof(info));
    info.size = sizeof(info);
    if (hsa_amd_pointer_info(p, &info, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS ||
        info.type != HSA_EXT_POINTER_TYPE_HSA)
        return false;
    *agent = info.agentOwner;
    return true;
}

bool SdmaPair::create()
{
    for (int i = 0; i < 2; ++i)
        if (!sig_[i].handle && hsa_signal_create(0, 0, nullptr, &sig_[i]) != HSA_STATUS_SUCCESS) {
            sig_[i].handle = 0;
            destroy();
            return false;
        }
    return true;
}

void SdmaPair::destroy()
{
    for (int i = 0; i < 2; ++i) {
        if (sig_[i].handle) hsa_signal_destroy(sig_[i]);
        sig_[i].handle = 0;
    }
}

bool SdmaPair::issue(int b, void* dst, hsa_agent_t dst_agent, const void* src, hsa_agent_t src_agent, size_t n)
{
    hsa_signal_store_relaxed(sig_[b], 1);
    if (hsa_amd_memory_async_copy(dst, dst_agent, src, src_agent, n, 0, nullptr, sig_[b]) == HSA_STATUS_SUCCESS)
        return true;
    hsa_signal_store_relaxed(sig_[b], 0);
    return false;
}

bool SdmaPair::wait(int b, hsa_wait_state_t state)
{
    return hsa_signal_wait_scacquire(sig_[b], HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, state) == 0;
}

bool sdma_d2h(void* dst, const void* src, size_t n)
{
    const hsa_agent_t* cpu = hsa_cpu_agent();
    if (!cpu || n == 0) return cpu != nullptr;
    hsa_agent_t gpu;
    SdmaPair sig;
    if (!hsa_owner(src, &gpu) || !sig.create()) return false;
    return sig.issue(0, dst, *cpu, src, gpu, n) && sig.wait(0);
}

// ---------------------------------------------------------- pinned staging --
void Staging::release()
{
    for (int i = 0; i < 2; ++i) {
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        if (buf[i]) (void)hipHostFree(buf[i]);
        ev[i] = nullptr;
        buf[i] = nullptr;
        used[i] = false;
    }
    dev = -1;
}

bool Staging::ready()
{
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess) return false;
    if (dev == d && buf[0]) return true;
    for (int i = 0; i < 2; ++i) {
        if (ev[i]) (void)hipEventDestroy(ev[i]);
        ev[i] = nullptr;
        if (!buf[i] && hipHostMalloc(&buf[i], kChunk, hipHostMallocPortable) != hipSuccess) {
            buf[i] = nullptr;
            return false;
        }
        if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return false;
    }
    dev = d;
    return true;
}

Staging& staging()
{
    static thread_local Staging s;  // the pinned chunks stay for the thread's life
    return s;
}

namespace {
// Multi-threaded memcpy on a persistent pool: the staged copies run one
// 32 MiB chunk at a time, and starting and joining 15 threads per chunk
// (parallel_for) cost about as much as the copy.  A copy is split into 1 MiB
// pieces that the caller and up to threads - 1 pool workers take in turn;
// several callers (the decode's upload and download threads) share the pool.
// The pool is never destroyed (its workers may still wait on it at exit).
struct CopyPool {
    struct Job {
        uint8_t* dst;
        const uint8_t* src;
        size_t n, piece;
        uint64_t np;
        int helpers;                      // pool workers still allowed to join
        int active = 0;                   // pool workers inside run() (under mu)
        std::atomic<uint64_t> next{0}, done{0};
    };
    std::mutex mu;
    std::condition_variable cv, done_cv;
    std::vector<Job*> jobs;
    int nthreads = 0;
    static void run(Job& j)
    {
        for (;;) {
            const uint64_t i = j.next.fetch_add(1);
            if (i >= j.np) return;
            const size_t o = i * j.piece;
            std::memcpy(j.dst + o, j.src + o, std::min(j.piece, j.n - o));
            j.done.fetch_add(1);
        }
    }
    void worker()
    {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return !jobs.empty(); });
            Job* j = nullptr;
            for (Job* c : jobs)
                if (c->helpers > 0 && c->next.load() < c->np) {
                    j = c;
                    break;
                }
            if (!j) {  // every queued job is fully handed out: wait for the next one
                cv.wait(lk);
                continue;
            }
            --j->helpers;
            ++j->active;
            lk.unlock();
            run(*j);
            lk.lock();
            --j->active;  // (the last touch of the job: its owner waits for this under mu)
            done_cv.notify_all();
        }
    }
    void copy(void* dst, const void* src, size_t n, int threads)
    {
        Job j;
        j.dst = (uint8_t*)dst;
        j.src = (const uint8_t*)src;
        j.n = n;
        j.piece = 1u << 20;
        j.np = (n + j.piece - 1) / j.piece;
        {
            std::lock_guard<std::mutex> lk(mu);
            while (nthreads < threads - 1) {
                std::thread(&CopyPool::worker, this).detach();
                ++nthreads;
            }
            j.helpers = (int)std::min<uint64_t>((uint64_t)threads - 1, j.np - 1);
            jobs.push_back(&j);
        }
        cv.notify_all();
        run(j);
        std::unique_lock<std::mutex> lk(mu);
        done_cv.wait(lk, [&] { return j.done.load() == j.np && j.active == 0; });
        jobs.erase(std::find(jobs.begin(), jobs.end(), &j));
    }
};

// the wait state of the staged SDMA copies' signal waits (LFM_SDMA_WAIT: 0
// blocked, the default; 1 active)
hsa_wait_state_t sdma_wait_state()
{
    static const int m = env_int("LFM_SDMA_WAIT", 0);
    return m == 1 ? HSA_WAIT_STATE_ACTIVE : HSA_WAIT_STATE_BLOCKED;
}
} // namespace

void par_memcpy(void* dst, const void* src, size_t n, int threads)
{
    const size_t piece = 1u << 20;
    const uint64_t np = (n + piece - 1) / piece;
    if (threads <= 1 || np <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    static CopyPool* pool = new CopyPool;  // (never destroyed, see CopyPool)
    pool->copy(dst, src, n, std::min(threads, 64));
}

// ----------------------------------------------------------- staged copies --
bool staged_h2d(void* d_dst, const void* h_src, size_t n, hipStream_t st, int threads)
{
    Staging& S = staging();
    if (!S.ready()) return hipMemcpyAsync(d_dst, h_src, n, hipMemcpyHostToDevice, st) == hipSuccess;
    double t_wait = 0, t_copy = 0;
    for (size_t off = 0, i = 0; off < n; off += Staging::kChunk, ++i) {
        const int b = (int)(i & 1);
        const size_t len = std::min(Staging::kChunk, n - off);
        auto t0 = clk::now();
        if (S.used[b] && hipEventSynchronize(S.ev[b]) != hipSuccess) return false;
        auto t1 = clk::now();
        par_memcpy(S.buf[b], (const uint8_t*)h_src + off, len, threads);
        auto t2 = clk::now();
        t_wait += ms_between(t0, t1);
        t_copy += ms_between(t1, t2);
        if (decode_timing() && off + len >= n)
            std::fprintf(stderr, "staged h2d: %zu bytes, host copies %.2f ms, waits %.2f ms, %d threads\n", n, t_copy,
                         t_wait, threads);
        if (hipMemcpyAsync((uint8_t*)d_dst + off, S.buf[b], len, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipEventRecord(S.ev[b], st) != hipSuccess)
            return false;
        S.used[b] = true;
    }
    return true;
}

// Host -> device through the pinned chunks with the DMA on an SDMA engine
// (HSA): the host copy of one chunk overlaps the engine's copy of the other.
// The blit-kernel copies of hipMemcpyAsync ran the decode payload upload at
// 5-47 ms depending on the process's state; the engine does not depend on
// the CUs.  Returns false if HSA cannot take the copy (nothing was issued on
// a false return before the first chunk; the caller falls back).  The
// destination stream must be idle (the caller synchronises it).
bool sdma_staged_h2d(void* d_dst, const void* h_src, size_t n, int threads)
{
    const hsa_agent_t* cpu = hsa_cpu_agent();
    Staging& S = staging();
    hsa_agent_t gpu;
    SdmaPair sig;
    if (!cpu || !S.ready() || n == 0 || !hsa_owner(d_dst, &gpu) || !sig.create()) return false;
    bool ok = true;
    double t_wait = 0, t_copy = 0, t_first = 0;
    for (size_t off = 0, i = 0; ok && off < n; off += Staging::kChunk, ++i) {
        const int b = (int)(i & 1);
        const size_t len = std::min(Staging::kChunk, n - off);
        auto t0 = clk::now();
        if (i >= 2) ok = sig.wait(b, sdma_wait_state());
        if (!ok) break;
        auto t1 = clk::now();
        par_memcpy(S.buf[b], (const uint8_t*)h_src + off, len, threads);
        const double w = ms_between(t0, t1);
        t_wait += w;
        if (i == 2) t_first = w;
        t_copy += ms_since(t1);
        ok = sig.issue(b, (uint8_t*)d_dst + off, gpu, S.buf[b], *cpu, len);
    }
    auto t_tail = clk::now();
    for (int b = 0; b < 2; ++b)
        if (!sig.wait(b, sdma_wait_state())) ok = false;
    if (decode_timing())
        std::fprintf(stderr,
                     "sdma h2d: %zu bytes, host copies %.2f ms, waits %.2f ms (first %.2f), last copy %.2f ms, %d threads\n",
                     n, t_copy, t_wait, t_first, ms_since(t_tail), threads);
    S.used[0] = S.used[1] = false;  // the chunks are free (no HIP event pending on them)
    return ok;
}

// Device -> host through the pinned chunks with the DMA on an SDMA engine:
// the engine copies chunk i + 1 while the host threads copy chunk i out (the
// blit kernel of hipMemcpyAsync would run on the CUs beside the next decode
// chunk's kernels).  The source must be complete (the caller synchronised its
// stream).  Returns false if HSA cannot take the copy before anything was
// issued (the caller falls back); a failure after that is reported as false too.
bool sdma_staged_d2h(void* h_dst, const void* d_src, size_t n, int threads, Staging& S)
{
    const hsa_agent_t* cpu = hsa_cpu_agent();
    hsa_agent_t gpu;
    SdmaPair sig;
    if (!cpu || !S.ready() || n == 0 || !hsa_owner(d_src, &gpu) || !sig.create()) return false;
    const size_t nc = (n + Staging::kChunk - 1) / Staging::kChunk;
    auto issue = [&](size_t i) {
        const int b = (int)(i & 1);
        const size_t off = i * Staging::kChunk, len = std::min(Staging::kChunk, n - off);
        return sig.issue(b, S.buf[b], *cpu, (const uint8_t*)d_src + off, gpu, len);
    };
    double t_wait = 0, t_copy = 0;
    bool ok = issue(0);
    for (size_t i = 0; ok && i < nc; ++i) {
        const int b = (int)(i & 1);
        if (i + 1 < nc) ok = issue(i + 1);
        auto t0 = clk::now();
        if (!sig.wait(b, sdma_wait_state())) ok = false;
        if (!ok) break;
        auto t1 = clk::now();
        const size_t off = i * Staging::kChunk, len = std::min(Staging::kChunk, n - off);
        par_memcpy((uint8_t*)h_dst + off, S.buf[b], len, threads);
        t_wait += ms_between(t0, t1);
        t_copy += ms_since(t1);
    }
    for (int b = 0; b < 2; ++b) (void)sig.wait(b, sdma_wait_state());  // nothing still writes a chunk
    if (decode_timing())
        std::fprintf(stderr, "sdma d2h: %zu bytes, host copies %.2f ms, waits %.2f ms, %d threads\n", n, t_copy, t_wait,
                     threads);
    S.used[0] = S.used[1] = false;
    return ok;
}

bool staged_d2h(void* h_dst, const void* d_src, size_t n, hipStream_t st, int threads, Staging& S)
{
    if (!S.ready())
        return hipMemcpyAsync(h_dst, d_src, n, hipMemcpyDeviceToHost, st) == hipSuccess &&
               hipStreamSynchronize(st) == hipSuccess;
    const size_t nc = (n + Staging::kChunk - 1) / Staging::kChunk;
    auto issue = [&](size_t i) {
        const int b = (int)(i & 1);
        const size_t off = i * Staging::kChunk, len = std::min(Staging::kChunk, n - off);
        S.used[b] = true;
        return hipMemcpyAsync(S.buf[b], (const uint8_t*)d_src + off, len, hipMemcpyDeviceToHost, st) == hipSuccess &&
               hipEventRecord(S.ev[b], st) == hipSuccess;
    };
    for (size_t i = 0; i < std::min<size_t>(2, nc); ++i)
        if (!issue(i)) return false;
    for (size_t i = 0; i < nc; ++i) {
        const int b = (int)(i & 1);
        const size_t off = i * Staging::kChunk, len = std::min(Staging::kChunk, n - off);
        if (hipEventSynchronize(S.ev[b]) != hipSuccess) return false;
        par_memcpy((uint8_t*)h_dst + off, S.buf[b], len, threads);
        if (i + 2 < nc && !issue(i + 2)) return false;
    }
    return true;
}

} // namespace lfm
