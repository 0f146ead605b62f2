// What every translation unit of this directory needs around a kernel launch: the block and wavefront sizes, the launch
// status / stream / grid helpers of the C ABI functions, the call index of a counter-based RNG request and a wavefront sum.
// Header-only, like mdx_math.hpp.  (The two edge-chain units keep their own: their machine code is pinned.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"

namespace mdx {

constexpr int kBlock = 256;
constexpr int kWave = 64;      // 64-wide wavefronts are assumed throughout (gfx950)

// the call index of a counter-based RNG request: the device word when the request names one (launches captured into a hipGraph)
__device__ __forceinline__ uint32_t rng_call(const mdx_rng_t& r) { return r.call_dev ? *r.call_dev : r.call; }

// sum over the 64 lanes, xor butterfly in a fixed order: every lane ends with the same bits
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// the key record of a memoised first-layer table (include/mdx_hip.h, mdx_egnn_table_check_keyed): was the table in memory
// built at this sigma?  (nullable key: no record, never current; a NaN sigma is never current)
__device__ __forceinline__ bool table_is_current(const uint32_t* key, const float* sigma)
{
    if (!key) return false;
    const uint32_t bits = __float_as_uint(sigma[0]);
    return key[0] == bits && (bits & 0x7fffffffu) <= 0x7f800000u;
}

inline int launch_status() { return hipGetLastError() == hipSuccess ? MDX_OK : MDX_ERR_HIP; }
inline hipStream_t as_stream(mdx_stream_t s) { return reinterpret_cast<hipStream_t>(s); }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline unsigned flat_grid(int64_t work_items)
{
    int64_t blocks = cdiv(work_items, kBlock);
    if (blocks > 2048) blocks = 2048;   // 256 CUs x 8 resident blocks; the rest is grid-strided
    if (blocks < 1) blocks = 1;
    return (unsigned)blocks;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace mdx
