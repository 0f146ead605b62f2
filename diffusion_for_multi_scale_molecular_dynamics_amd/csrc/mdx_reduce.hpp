// The wavefront and workgroup helpers shared by the binary64 units (mdx_analytical.hip, mdx_transport.hip,
// mdx_optimal_translation.hip, mdx_loss.hip, mdx_sw.hip): the validity tests behind the status bits and the fixed-order
// reductions that the bit-for-bit promises of DESIGN.md rest on.  wave_sum(float / double) stays in mdx_launch.hpp.
// Only what leaves every kernel's machine code as it was is here (tools/compare_kernel_code.py): the (value, index) arg-min,
// the __shfl_up lane scan and the lane minimum stay written out at their sites (profiles/r15_shared_helpers.md).
// Header-only with internal linkage: each unit compiles its own copy, no device symbol crosses a unit.
#pragma once
#include <hip/hip_runtime.h>

#include "mdx_launch.hpp"

namespace mdx {

// beside its float / double overloads of mdx_launch.hpp, not in the unnamed namespace below: there it would hide them from
// block_sum, which would then sum its doubles as ints
static __device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

namespace {

// finite and of a magnitude the binary64 arithmetic behind it cannot overflow on: false for NaN and +-inf as well
__device__ __forceinline__ bool finite_(double v) { return __builtin_fabs(v) < 1.0e300; }
__device__ __forceinline__ bool sigma_valid(double s) { return s > 0.0 && finite_(s); }

// maximum over the 64 lanes, xor butterfly in a fixed order: every lane ends with the same bits
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double w = __shfl_xor(v, o, kWave);
        v = w > v ? w : v;
    }
    return v;
}

// the sum of one value per thread over a workgroup of kBlock threads, in a fixed order: lanes by the xor butterfly, wavefronts
// in index order through `scratch` (kBlock / kWave doubles of LDS); every thread ends with the same bits
__device__ double block_sum(double v, double* scratch)
{
    const int tid = threadIdx.x;
    v = wave_sum(v);
    __syncthreads();
    if (tid % kWave == 0) scratch[tid / kWave] = v;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) total += scratch[w];
    return total;
}

}  // namespace
}  // namespace mdx
