// The cubic interpolation of the first EGNN layer's distance table, shared by the unit that checks the
// table (mdx_egnn_table.hip) and the one that gathers from it (mdx_egnn_node.hip).  Header-only, like mdx_launch.hpp.
#pragma once
#include <hip/hip_runtime.h>

namespace mdx {

// 4-point Lagrange weights on the nodes -1, 0, 1, 2 at t in [0, 1] (t = 1/2: -1/16, 9/16, 9/16, -1/16, all exact)
__device__ __forceinline__ void lagrange_weights(float t, float w[4])
{
    const float tp = t + 1.0f, tm = t - 1.0f, t2 = t - 2.0f;
    w[0] = -(t * tm * t2) / 6.0f;
    w[1] = (tp * tm * t2) / 2.0f;
    w[2] = -(tp * t * t2) / 2.0f;
    w[3] = (tp * t * tm) / 6.0f;
}

__device__ __forceinline__ float interpolate(const float w[4], float v0, float v1, float v2, float v3)
{
    return ((w[0] * v0 + w[1] * v1) + w[2] * v2) + w[3] * v3;
}

}  // namespace mdx
