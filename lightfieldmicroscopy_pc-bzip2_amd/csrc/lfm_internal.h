// lfm_internal.h -- what the host engine's files (lfm_engine.cpp,
// lfm_encode.cpp, lfm_decode.cpp, lfm_decode_multi.cpp, lfm_transfer.cpp, lfm_stream.cpp) share with each other and
// with nobody else.  Nothing here is exported from liblfm.so.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <thread>
#include <vector>
#include "lfm_bz_caps.h"  // per-stream capacities of the GPU bzip2 encoder (bz::out_cap, bz::rle_cap)

#pragma GCC visibility push(hidden)
namespace lfm {

using clk = std::chrono::steady_clock;
inline double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }
inline double ms_between(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

// run-time switches: unset or empty means the default
inline long env_long(const char* name, long dflt)
{
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    return atol(e);
}
inline int env_int(const char* name, int dflt)
{
    const char* e = getenv(name);
    if (!e || !*e) return dflt;
    return atoi(e);
}

// LFM_DECODE_TIMING=1: stage times on stderr
inline bool decode_timing()
{
    static const bool timing = env_int("LFM_DECODE_TIMING", 0) != 0;
    return timing;
}

template <class F>
void parallel_for(uint64_t n, int threads, F&& f)
{
    std::atomic<uint64_t> next{0};
    auto w = [&]() {
        for (;;) {
            uint64_t i = next.fetch_add(1);
            if (i >= n) break;
            f(i);
        }
    };
    threads = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::max(threads, 1), n));
    std::vector<std::thread> pool;
    for (int i = 1; i < threads; ++i) pool.emplace_back(w);
    w();
    for (auto& t : pool) t.join();
}

// one block through the host library of its compression type (lfm_engine.cpp)
int compress_one(int ctype, uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint32_t* out_len,
                 int level);
int decompress_one(int ctype, const uint8_t* in, uint32_t n, uint8_t* out, uint32_t expect);

// every byte of [off, off + n) of an open file read / written, or false (lfm_stream.cpp)
bool pread_all(int fd, uint8_t* dst, uint64_t n, uint64_t off);
bool pwrite_all(int fd, const uint8_t* src, uint64_t n, uint64_t off);

} // namespace lfm
#pragma GCC visibility pop
