// lfm_transfer.h -- host <-> device copies of the engine: the HSA agent and
// the SDMA double-buffered copies, the pinned staging chunks, the
// multi-threaded memcpy.  Private to the engine's files.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>

#pragma GCC visibility push(hidden)
namespace lfm {

// the HSA CPU agent (SDMA copies are enabled and HSA is up), or null
const hsa_agent_t* hsa_cpu_agent();
// the agent that owns p: true only for memory HSA allocated (device memory,
// pinned host memory), the only kind an SDMA engine copies
bool hsa_owner(const void* p, hsa_agent_t* agent);

// The two completion signals of a double-buffered SDMA copy: chunk i uses
// signal i & 1.  A signal is 1 while its copy is in flight and 0 otherwise, so
// waiting on one that was never used returns at once.
class SdmaPair {
public:
    SdmaPair() = default;
    SdmaPair(const SdmaPair&) = delete;
    SdmaPair& operator=(const SdmaPair&) = delete;
    ~SdmaPair() { destroy(); }
    // both signals exist afterwards (true), or neither
    bool create();
    void destroy();
    // start an asynchronous copy on signal b; false (signal back at 0) if HSA refuses it
    bool issue(int b, void* dst, hsa_agent_t dst_agent, const void* src, hsa_agent_t src_agent, size_t n);
    // wait until signal b's copy is done
    bool wait(int b, hsa_wait_state_t state = HSA_WAIT_STATE_BLOCKED);

private:
    hsa_signal_t sig_[2] = {{0}, {0}};
};

bool sdma_d2h(void* dst, const void* src, size_t n);

// Host <-> device copies of pageable buffers through two pinned staging
// chunks: the DMA of one chunk overlaps the multi-threaded host copy of the
// other (the runtime's own staging copies with one thread and takes the page
// faults of a fresh destination on that thread).  The pinned chunks and their
// events are kept per host thread and device.
struct Staging {
    static constexpr size_t kChunk = 32u << 20;
    void* buf[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool used[2] = {false, false};
    int dev = -1;
    Staging() = default;
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;
    ~Staging() { release(); }  // a worker thread that exits frees its pinned chunks
    void release();
    bool ready();
};
Staging& staging();  // the calling thread's

bool staged_h2d(void* d_dst, const void* h_src, size_t n, hipStream_t st, int threads);
bool sdma_staged_h2d(void* d_dst, const void* h_src, size_t n, int threads);
bool sdma_staged_d2h(void* h_dst, const void* d_src, size_t n, int threads, Staging& S);
bool staged_d2h(void* h_dst, const void* d_src, size_t n, hipStream_t st, int threads, Staging& S);

} // namespace lfm
#pragma GCC visibility pop
