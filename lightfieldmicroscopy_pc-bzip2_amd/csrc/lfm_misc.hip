// lfm_misc.hip -- device helpers of the HIP shim: synthetic light-field input
// generator, 5-D region copy, device query, debug switches.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include "lfm_hip.h"

namespace lfm {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ int64_t tri(int64_t a)
{
    int64_t m = a % 2048;
    return m > 1024 ? m - 1024 : 1024 - m;
}

// v = 100 + lens*field/256 + noise  (<= 3235), one thread per 8 pixels (16-byte stores)
__global__ __launch_bounds__(256) void synth_kernel(uint16_t* __restrict__ out, int X, int Y, int Z, int T, int t,
                                                    int z0, uint64_t idx0, uint64_t seed)
{
    const uint64_t total = (uint64_t)X * Y * Z;
    const int64_t half = T / 2;
    const int64_t rm = 2 * half * half + 1;
    for (uint64_t i8 = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) * 8; i8 < total;
         i8 += (uint64_t)gridDim.x * blockDim.x * 8) {
        uint16_t v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint64_t i = i8 + j;
            if (i >= total) { v[j] = 0; continue; }
            const int64_t x = (int64_t)(i % X);
            const int64_t y = (int64_t)((i / X) % Y);
            const int64_t z = z0 + (int64_t)(i / ((uint64_t)X * Y));
            const int64_t du = (x % T) - half, dv = (y % T) - half;
            const int64_t lens = (1024 * (rm - (du * du + dv * dv))) / rm;
            const int64_t field = 256 + tri(3 * x + 40 * z + 97 * t) / 4 + tri(2 * y) / 4;
            const uint64_t idx = idx0 + i;
            const int64_t noise = (int64_t)(splitmix64(seed ^ (idx * 0x9E3779B97F4A7C15ull)) >> 58);
            v[j] = (uint16_t)(100 + (lens * field) / 256 + noise);
        }
        if (i8 + 8 <= total && ((reinterpret_cast<uintptr_t>(out + i8) & 15) == 0)) {
            uint4 w;
            w.x = v[0] | ((uint32_t)v[1] << 16);
            w.y = v[2] | ((uint32_t)v[3] << 16);
            w.z = v[4] | ((uint32_t)v[5] << 16);
            w.w = v[6] | ((uint32_t)v[7] << 16);
            *reinterpret_cast<uint4*>(out + i8) = w;
        } else {
            for (int j = 0; j < 8 && i8 + j < total; ++j) out[i8 + j] = v[j];
        }
    }
}

// ------------------------------------------------------------ region copy --
struct Crop5 {
    uint32_t dims[5], lb[5], n[5], bpp;
};

// bytes [0, len) of sp to dp by `lanes` lanes in units of T: single bytes up to
// dp's first T boundary (sp is on one there too: the caller picks T from the
// two addresses' difference), whole units, single bytes after the last one
template <typename T>
__device__ __forceinline__ void crop_copy(const uint8_t* __restrict__ sp, uint8_t* __restrict__ dp, uint32_t len,
                                          uint32_t lane, uint32_t lanes)
{
    const uint32_t head = min(len, (uint32_t)((0 - reinterpret_cast<uintptr_t>(dp)) & (sizeof(T) - 1)));
    const uint32_t units = (len - head) / (uint32_t)sizeof(T);
    const uint32_t body_end = head + units * (uint32_t)sizeof(T);
    for (uint32_t i = lane; i < head; i += lanes) dp[i] = sp[i];
    const T* s = reinterpret_cast<const T*>(sp + head);
    T* d = reinterpret_cast<T*>(dp + head);
    for (uint32_t u = lane; u < units; u += lanes) d[u] = s[u];
    for (uint32_t i = body_end + lane; i < len; i += lanes) dp[i] = sp[i];
}

// The box lb .. lb + n - 1 of a 5-D image (x fastest) into a dense array of n.
// One work item is a slice of `slice` bytes (a multiple of 16) of one output
// row, copied by a group of `lanes` lanes (a power of two, 4 .. 64: a whole
// wave for rows of 1 KiB and more, so four 16-byte accesses per lane are in
// flight; narrower groups for short rows, so a wave holds several rows).  The
// access width follows from the two row addresses: 16 bytes when they differ
// by a multiple of 16, else 4, 2 or 1 (bpp 1 with an odd lb[0]).  Row and
// item indices are 64-bit: a config-5 stack is larger than 4 GiB.
__global__ __launch_bounds__(256) void crop_region(const uint8_t* __restrict__ src, Crop5 C, uint8_t* __restrict__ dst,
                                                   uint32_t lanes, uint32_t slice, uint64_t spr, uint64_t items)
{
    const uint64_t rb = (uint64_t)C.n[0] * C.bpp;
    const uint32_t lane = threadIdx.x & (lanes - 1);
    const uint64_t gpb = blockDim.x / lanes;
    for (uint64_t it = blockIdx.x * gpb + threadIdx.x / lanes; it < items; it += (uint64_t)gridDim.x * gpb) {
        const uint64_t r = it / spr, o = (it - r * spr) * slice;
        uint64_t q = r;
        const uint64_t y = q % C.n[1]; q /= C.n[1];
        const uint64_t z = q % C.n[2]; q /= C.n[2];
        const uint64_t c = q % C.n[3]; q /= C.n[3];
        const uint64_t e = ((((C.lb[4] + q) * C.dims[3] + (C.lb[3] + c)) * C.dims[2] + (C.lb[2] + z)) * C.dims[1] +
                            (C.lb[1] + y)) * C.dims[0] + C.lb[0];
        const uint8_t* sp = src + e * C.bpp + o;
        uint8_t* dp = dst + r * rb + o;
        const uint32_t len = (uint32_t)min((uint64_t)slice, rb - o);
        const uint32_t rel = (uint32_t)(reinterpret_cast<uintptr_t>(sp) - reinterpret_cast<uintptr_t>(dp));
        if ((rel & 15) == 0) crop_copy<uint4>(sp, dp, len, lane, lanes);
        else if ((rel & 3) == 0) crop_copy<uint32_t>(sp, dp, len, lane, lanes);
        else if ((rel & 1) == 0) crop_copy<uint16_t>(sp, dp, len, lane, lanes);
        else crop_copy<uint8_t>(sp, dp, len, lane, lanes);
    }
}

} // namespace lfm

extern "C" int lfm_hip_synth(uint16_t* d_out, int X, int Y, int Z, int T, int t_index, int z0, uint64_t idx0, uint64_t seed,
                             void* stream)
{
    if (!d_out || X <= 0 || Y <= 0 || Z <= 0 || T <= 0 || z0 < 0) return LFM_HIP_EINVAL;
    const uint64_t total = (uint64_t)X * Y * Z;
    const uint64_t threads = (total + 7) / 8;
    const int grid = (int)(threads < 256ull * 2048 ? (threads + 255) / 256 : 2048);
    hipLaunchKernelGGL(lfm::synth_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_out, X, Y, Z, T, t_index,
                       z0, idx0, seed);
    return hipGetLastError() == hipSuccess ? LFM_HIP_OK : LFM_HIP_ERUNTIME;
}

extern "C" int lfm_hip_crop_region(const void* d_src, const uint32_t src_dims[5], const uint32_t lb[5],
                                   const uint32_t n[5], uint32_t bpp, void* d_dst, void* stream)
{
    if (!d_src || !d_dst || !src_dims || !lb || !n) return LFM_HIP_EINVAL;
    if (bpp != 1 && bpp != 2 && bpp != 4 && bpp != 8) return LFM_HIP_EINVAL;
    lfm::Crop5 C;
    uint64_t nrows = 1;
    for (int d = 0; d < 5; ++d) {
        if (!n[d] || !src_dims[d] || lb[d] >= src_dims[d] || n[d] > src_dims[d] - lb[d]) return LFM_HIP_EINVAL;
        C.dims[d] = src_dims[d];
        C.lb[d] = lb[d];
        C.n[d] = n[d];
        if (d) nrows *= n[d];
    }
    C.bpp = bpp;
    const uint64_t rb = (uint64_t)n[0] * bpp;
    uint32_t lanes = 4;  // 16 bytes per lane cover the row, up to a whole wave
    while (lanes < 64 && (uint64_t)lanes * 16 < rb) lanes *= 2;
    const uint32_t slice = lanes * 64;
    const uint64_t spr = (rb + slice - 1) / slice, items = nrows * spr, gpb = 256 / lanes;
    const uint64_t blocks = (items + gpb - 1) / gpb;
    const int grid = (int)(blocks < 2048 ? blocks : 2048);
    hipLaunchKernelGGL(lfm::crop_region, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)d_src, C,
                       (uint8_t*)d_dst, lanes, slice, spr, items);
    return hipGetLastError() == hipSuccess ? LFM_HIP_OK : LFM_HIP_ERUNTIME;
}

extern "C" int lfm_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int lfm_hip_force_generic(void)
{
    static int v = -1;
    if (v < 0) {
        const char* e = getenv("LFM_FORCE_GENERIC");
        v = (e && e[0] == '1') ? 1 : 0;
    }
    return v;
}
