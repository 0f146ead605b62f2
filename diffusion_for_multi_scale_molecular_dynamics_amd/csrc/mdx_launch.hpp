// What every translation unit of this directory needs around a kernel launch: the block and wavefront sizes, the launch
// status / stream / grid helpers of the C ABI functions, the call index of a counter-based RNG request and the wavefront sums.
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

// the same sum on DPP adds (rows of 16, then lane 15 / 31 of the rows below: the total is lane 63's), handed to every lane
// through a scalar register: no LDS permutes, a fixed order -- another order than wave_sum's, so other bits
__device__ __forceinline__ float wave_total_dpp(float v)
{
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
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

// the grid of a kernel that gives every node a wavefront (blocks of kBlock threads; grid-strided above 16384 blocks)
inline unsigned node_grid(int64_t n_nodes)
{
    int64_t blocks = cdiv(n_nodes * kWave, kBlock);
    if (blocks > 16384) blocks = 16384;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace mdx
