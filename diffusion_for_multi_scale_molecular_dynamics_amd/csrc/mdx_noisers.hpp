// The forward noisers' arithmetic, one element at a time: what the stand-alone kernels F1 / F2 / F3 and the repaint kernels of
// mdx_hip.hip and the training-batch kernel of mdx_noising.hip all compute ("MDX arithmetic": binary32, no
// contraction).  Header-only, like mdx_math.hpp.
#pragma once
#include "../../include/mdx_hip.h"
#include "mdx_math.hpp"

namespace mdx {

// F1 (noisers/relative_coordinates_noiser.py:56-66): wrap(x0 + sigma z)
__device__ __forceinline__ float noised_relative_coordinate(float x0, float sigma, float z) { return wrap01(x0 + sigma * z); }

// F3 (noisers/lattice_noiser.py:69-81): sigma_n z + l0
__device__ __forceinline__ float noised_lattice_parameter(float sigma_n, float z, float l0) { return sigma_n * z + l0; }

// F2 (noisers/atom_types_noiser.py:42-60): argmax_c(log Qbar[a0][c] + gumbel_c), the first maximum; a NaN wins over numbers
__device__ __forceinline__ int noised_atom_type(int a0, const float* __restrict__ qbar, int C, const float* gum_u,
                                                bool from_u)
{
    float best = 0.0f;
    int arg = 0;
    for (int c = 0; c < C; ++c) {
        const float lq = logf_(qbar[a0 * C + c]);
        const float gn = from_u ? gumbel_from_u(gum_u[c]) : gum_u[c];
        const float v = lq + gn;
        if (c == 0 || v > best || (v != v && best == best)) { best = v; arg = c; }
    }
    return arg;
}

}  // namespace mdx
