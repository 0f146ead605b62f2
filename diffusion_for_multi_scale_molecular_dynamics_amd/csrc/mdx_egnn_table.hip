// The first EGNN layer of a sampler forward on a distance grid instead of per edge.
//
// Inside the sampler every structure of the batch has the same sigma, so the first layer's node features h0 take one value per
// class (atom type or MASK) and its whole per-edge output -- the message m_ij and the coordinate head's scalar s_ij -- is a
// function F_ab(rho) of the class pair (a, b) and of rho = |c_i - c_j|.  The caller evaluates F on a uniform grid in rho with
// the edge chain itself (mdx_egnn_edge_chain, MDX_EGNN_MESSAGES_ROWS, one "edge" per (a, b, grid point)); these kernels then
//
//   egnn_table_check_kernel     compare the cubic interpolation of the even grid points at the odd ones (the cell midpoints,
//   egnn_table_verdict_kernel   where the interpolation error peaks) with the chain's own values there, per class pair and
//                               column, relative to the pair's largest |value|; raise MDX_STATUS_EGNN_TABLE above the
//                               tolerance, or when sigma is not uniform over the batch;
//   egnn_table_gather_kernel    per node: interpolate every edge's message and scalar from the table and add them up -- the
//                               output contract of egnn_node_gather_kernel (mdx_egnn_chain.hip).
//
// Grid layout (rows of the chain's output): class pair p = a n_classes + b owns rows [p K, p K + K), K = 2 n_even - 1; row p K + m
// is the even point rho = m h (m < n_even), row p K + n_even + j the midpoint rho = (j + 1/2) h (j < n_even - 1), h = 1 /
// inv_spacing.  F is even in rho (it depends on rho^2 only): the point left of rho = 0 is the point right of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"

using namespace mdx;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

__device__ __forceinline__ f32x4 interpolate4(const float w[4], f32x4 v0, f32x4 v1, f32x4 v2, f32x4 v3)
{
    return ((w[0] * v0 + w[1] * v1) + w[2] * v2) + w[3] * v3;
}

// the edge chain's squared distance: sum over k < D of (c_src[k] - c_dst[k])^2 in component order (mdx_egnn_chain.hip)
__device__ __forceinline__ float squared_distance(const float* ci, const float* __restrict__ cj, int D)
{
    float r2 = 0.0f;
    for (int k = 0; k < D; ++k) {
        const float dlt = ci[k] - cj[k];
        r2 += dlt * dlt;
    }
    return r2;
}

__device__ __forceinline__ float coord_head_value(float s, int flags) { return (flags & MDX_EGNN_COORD_TANH) ? tanhf(s) : s; }
__device__ __forceinline__ float normalize_factor(float r2) { return tanhf(r2) / sqrtf(r2 + 1.0e-16f); }

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// grid (n_pairs, chunks of kCheckRows midpoints); a thread per column (H message columns + the scalar as column H).
// workspace: [n_pairs][H + 1] the bits of the largest |error| per column, then [n_pairs] the bits of the class pair's largest
// |value| over all its columns (non-negative floats order like their bits; a NaN orders above every number and fails the
// verdict).  The error is judged against the PAIR's largest value, not the column's: the chain's own binary32 rounding is set by
// the magnitudes inside its dot products, and a column whose values stay small carries that absolute noise at a large relative
// size (measured: up to 9e-5 of a small column's maximum in exact-f32 mode, with the interpolation itself 5e-9 from the chain).
constexpr int kCheckRows = 32;
__global__ __launch_bounds__(256) void egnn_table_check_kernel(const float* __restrict__ messages, const float* __restrict__ scalar,
                                                               int H, int n_pairs, int n_even, unsigned* __restrict__ workspace,
                                                               const uint32_t* __restrict__ table_key,
                                                               const float* __restrict__ sigma)
{
    if (table_is_current(table_key, sigma)) return;      // nothing was built in this forward: the workspace stays zeroed
    const int p = blockIdx.x, K = 2 * n_even - 1;
    const int j0 = blockIdx.y * kCheckRows, j1 = min(j0 + kCheckRows, n_even - 2);     // midpoints j <= n_even - 3 are used
    float w[4];
    lagrange_weights(0.5f, w);
    for (int c = threadIdx.x; c <= H; c += blockDim.x) {
        auto value = [&](int row) { return c < H ? messages[((int64_t)p * K + row) * H + c] : scalar[(int64_t)p * K + row]; };
        unsigned err = 0, big = 0;
        for (int j = j0; j < j1; ++j) {
            const float v0 = value(j > 0 ? j - 1 : 1), v1 = value(j), v2 = value(j + 1), v3 = value(j + 2);
            const float mid = value(n_even + j);
            err = max(err, abs_bits(interpolate(w, v0, v1, v2, v3) - mid));
            big = max(big, max(max(abs_bits(v1), abs_bits(v2)), max(abs_bits(v3), abs_bits(mid))));
        }
        if (j0 < j1) {
            atomicMax(workspace + (int64_t)p * (H + 1) + c, err);
            atomicMax(workspace + (int64_t)n_pairs * (H + 1) + p, big);
        }
    }
}

// one workgroup: the verdict over the workspace (which it zeroes for the next forward) and the uniform-sigma check.
// With a key record (table_key, nullable): the midpoint verdict only when this forward has built the table -- the kernels of the
// build have then seen the same stale key -- and the key is written HERE, behind everything that reads it in this forward:
// sigma[0]'s bits and one more build when the midpoints passed, "no table" when they failed.  The uniform-sigma check runs in
// every forward (it fails the forward, not the table: the key stays).
__global__ __launch_bounds__(256) void egnn_table_verdict_kernel(unsigned* __restrict__ workspace, int n_pairs, int columns,
                                                                 const float* __restrict__ sigma, int64_t n_sigma, float tolerance,
                                                                 float* __restrict__ worst_out, uint32_t* __restrict__ status,
                                                                 uint32_t* __restrict__ table_key)
{
    __shared__ float worst[256];
    __shared__ int bad[256];
    float mine = 0.0f;
    int fail = 0;
    const bool built = !table_is_current(table_key, sigma);      // (uniform: one word, read before thread 0 writes it below)
    const int64_t n_entries = built ? (int64_t)n_pairs * columns : 0;
    for (int64_t i = threadIdx.x; i < n_entries; i += blockDim.x) {
        const float err = __uint_as_float(workspace[i]), big = __uint_as_float(workspace[n_entries + i / columns]);
        if (!(err <= tolerance * big)) fail = 1;
        if (big > 0.0f) mine = fmaxf(mine, err / big);
        else if (err > 0.0f || err != err) mine = INFINITY;
    }
    __syncthreads();                      // (every thread has read the pair maxima before they are zeroed)
    if (built)
        for (int64_t i = threadIdx.x; i < n_entries + n_pairs; i += blockDim.x) workspace[i] = 0u;
    const int table_fail = fail;
    for (int64_t i = 1 + threadIdx.x; i < n_sigma; i += blockDim.x)
        if (!(sigma[i] == sigma[0])) fail = 1;
    worst[threadIdx.x] = mine;
    bad[threadIdx.x] = fail | (table_fail << 1);
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            worst[threadIdx.x] = fmaxf(worst[threadIdx.x], worst[threadIdx.x + s]);
            bad[threadIdx.x] |= bad[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (worst_out && built) worst_out[0] = worst[0];
        if (bad[0] && status) atomicOr(status, MDX_STATUS_EGNN_TABLE);
        if (table_key && built) {
            if (bad[0] & 2) {
                table_key[0] = MDX_EGNN_TABLE_NO_KEY;
            } else {
                table_key[0] = __float_as_uint(sigma[0]);
                table_key[1] = table_key[1] + 1u;
            }
        }
    }
}

// One wavefront per node.  Lane l first takes the node's edges e0 + l, e0 + l + 64, ...: class pair, rho, the interpolation
// cell and weights, and the coordinate term (dealt and reduced as in egnn_node_gather_kernel); the message sum then walks the
// node's edges in order, every lane reading its four columns of the four table rows, the edge's cell and weights broadcast
// from the lane that computed them.  H <= 256: one quad of columns per lane.
__global__ __launch_bounds__(256) void egnn_table_gather_kernel(const float* __restrict__ table, const float* __restrict__ table_scalar,
                                                                int H, int n_classes, int n_even, float inv_spacing,
                                                                const int64_t* __restrict__ atom_types,
                                                                const int64_t* __restrict__ offsets, const int64_t* __restrict__ degree,
                                                                int64_t n_nodes, int mean_messages, float* __restrict__ out,
                                                                const float* __restrict__ left, const float* __restrict__ coord,
                                                                const int64_t* __restrict__ edges, int D, int mean_coords,
                                                                int flags, float* __restrict__ coord_out, uint32_t* __restrict__ status)
{
    const int lane = threadIdx.x % kWave;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
    const int K = 2 * n_even - 1, quads = H >> 2;
    const bool has_quad = lane < quads;
    bool outside = false;
    for (int64_t node = wave; node < n_nodes; node += n_waves) {
        const int64_t e0 = offsets[node], deg = degree[node], e1 = e0 + deg;
        int64_t a = atom_types[node];
        if (a < 0 || a >= n_classes) { outside = true; a = 0; }
        float part[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ci[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) ci[k] = k < D ? coord[node * D + k] : 0.0f;
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int64_t c0 = e0; c0 < e1; c0 += kWave) {
            const int64_t e = c0 + lane;
            int row = 0, row_left = 0;         // table rows of nodes m and m - 1 (nodes m + 1, m + 2 follow row)
            float w[4] = {0, 0, 0, 0};
            if (e < e1) {
                const int64_t dst = edges[2 * e + 1];
                int64_t b = atom_types[dst];
                if (b < 0 || b >= n_classes) { outside = true; b = 0; }
                const float r2 = squared_distance(ci, coord + dst * D, D);
                const float u = sqrtf(r2) * inv_spacing;
                int m = 0;
                float t = 0.0f;
                if (u <= (float)(n_even - 2)) {
                    m = min((int)u, n_even - 3);
                    t = u - (float)m;
                } else {
                    outside = true;                // beyond the grid (or NaN): the caller recomputes on the per-edge chain
                }
                lagrange_weights(t, w);
                row = (int)(a * n_classes + b) * K + m;
                row_left = m > 0 ? row - 1 : row + 1;
                const float s = coord_head_value(interpolate(w, table_scalar[row_left], table_scalar[row], table_scalar[row + 1],
                                                             table_scalar[row + 2]), flags);
                if (flags & MDX_EGNN_COORD_NORMALIZE) {
                    float diff[8], n2 = 0.0f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        diff[k] = k < D ? ci[k] - coord[dst * D + k] : 0.0f;
                        if (k < D) n2 += diff[k] * diff[k];
                    }
                    const float f = normalize_factor(n2);
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < D) part[k] += (f * diff[k]) * s;
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < D) part[k] += (ci[k] - coord[dst * D + k]) * s;
                }
            }
            const int n = (int)min<int64_t>(kWave, e1 - c0);
            for (int i = 0; i < n; ++i) {
                const int r = __builtin_amdgcn_readlane(row, i), rl = __builtin_amdgcn_readlane(row_left, i);
                float wi[4];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    wi[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w[k]), i));
                if (has_quad) {
                    const f32x4* base = reinterpret_cast<const f32x4*>(table + (int64_t)r * H) + lane;
                    const f32x4 v0 = reinterpret_cast<const f32x4*>(table + (int64_t)rl * H)[lane];
                    acc += interpolate4(wi, v0, base[0], base[quads], base[2 * quads]);
                }
            }
        }
        const float count = (mean_messages && deg > 0) ? (float)deg : 1.0f;      // (a true division: egnn_utils.py:66-68)
        if (has_quad) {
            if (mean_messages) acc = acc / count;
            if (left) {
                reinterpret_cast<f32x4*>(out + node * 2 * H)[lane] = reinterpret_cast<const f32x4*>(left + node * H)[lane];
                reinterpret_cast<f32x4*>(out + node * 2 * H + H)[lane] = acc;
            } else {
                reinterpret_cast<f32x4*>(out + node * H)[lane] = acc;
            }
        }
        // the coordinate sums over the wavefront: the DPP butterfly of egnn_node_gather_kernel (a fixed order)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < D) {
                float v = part[k];
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x111, 0xf, 0xf, false));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x112, 0xf, 0xf, false));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x114, 0xf, 0xf, false));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x118, 0xf, 0xf, false));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));
                v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));
                part[k] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
            }
        }
        if (lane < D) {
            float total = 0.0f, mine = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k == lane) { total = part[k]; mine = ci[k]; }
            }
            if (mean_coords && deg > 0) total = total / (float)deg;
            coord_out[node * D + lane] = mine + total;
        }
    }
    if (outside && status) atomicOr(status, MDX_STATUS_EGNN_TABLE);
}

}  // namespace

extern "C" {

int mdx_egnn_table_check(const float* table, const float* table_scalar, int H, int n_classes, int n_even, const float* sigma,
                         int64_t n_sigma, float tolerance, uint32_t* workspace, float* worst_out, uint32_t* status,
                         mdx_stream_t stream)
{
    return mdx_egnn_table_check_keyed(table, table_scalar, H, n_classes, n_even, sigma, n_sigma, tolerance, workspace, worst_out,
                                      status, nullptr, stream);
}

int mdx_egnn_table_check_keyed(const float* table, const float* table_scalar, int H, int n_classes, int n_even, const float* sigma,
                               int64_t n_sigma, float tolerance, uint32_t* workspace, float* worst_out, uint32_t* status,
                               uint32_t* table_key, mdx_stream_t stream)
{
    if (H < 1 || n_classes < 1 || n_even < 4 || n_sigma < 1 || !(tolerance >= 0.0f)) return MDX_ERR_INVALID_ARG;
    if (!table || !table_scalar || !sigma || !workspace) return MDX_ERR_INVALID_ARG;
    const int n_pairs = n_classes * n_classes;
    const hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(egnn_table_check_kernel, dim3((unsigned)n_pairs, (unsigned)((n_even - 2 + kCheckRows - 1) / kCheckRows)),
                       dim3(256), 0, s, table, table_scalar, H, n_pairs, n_even, reinterpret_cast<unsigned*>(workspace),
                       table_key, sigma);
    hipLaunchKernelGGL(egnn_table_verdict_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<unsigned*>(workspace), n_pairs,
                       H + 1, sigma, n_sigma, tolerance, worst_out, status, table_key);
    return launch_status();
}

int mdx_egnn_table_gather(const float* table, const float* table_scalar, int H, int n_classes, int n_even, float inv_spacing,
                          const int64_t* atom_types, const int64_t* offsets, const int64_t* degree, int64_t n_nodes,
                          int mean_messages, const float* left, float* out, const float* coord, int coord_dimension,
                          const int64_t* edges, int mean_coords, int coord_flags, float* coord_out, uint32_t* status,
                          mdx_stream_t stream)
{
    if (n_nodes < 0 || H < 4 || n_classes < 1 || n_even < 4 || coord_dimension < 1 || !(inv_spacing > 0.0f))
        return MDX_ERR_INVALID_ARG;
    if (coord_flags & ~(MDX_EGNN_COORD_NORMALIZE | MDX_EGNN_COORD_TANH)) return MDX_ERR_INVALID_ARG;
    if ((H & 3) || H > 4 * kWave || coord_dimension > 8) return MDX_ERR_UNSUPPORTED;
    if ((int64_t)n_classes * n_classes * (2 * (int64_t)n_even - 1) * H >= ((int64_t)1 << 31)) return MDX_ERR_UNSUPPORTED;
    if (n_nodes == 0) return MDX_OK;
    if (!table || !table_scalar || !atom_types || !offsets || !degree || !out || !coord || !edges || !coord_out)
        return MDX_ERR_INVALID_ARG;
    int64_t blocks = (n_nodes * kWave + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(egnn_table_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                       table, table_scalar, H, n_classes, n_even, inv_spacing, atom_types, offsets, degree, n_nodes, mean_messages,
                       out, left, coord, edges, coord_dimension, mean_coords, coord_flags, coord_out, status);
    return launch_status();
}

}  // extern "C"
