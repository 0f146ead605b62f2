// The per-node passes behind the EGNN edge chain (DESIGN.md sections 3 and 3b): what turns a graph layer's per-edge output
// into node rows ([h | sum of messages], the input of the node MLP) and new coordinates.  Two forms, one output contract:
//
//   per-edge form        the edge chain (mdx_egnn_chain.hip) has written per-node piece sums of the messages and one scalar per
//                        edge: segment_combine_kernel (messages), egnn_coord_aggregate_kernel (coordinates), and both as one
//                        pass over the nodes, egnn_node_gather_kernel;
//   distance-grid form   the first layer of a sampler forward: egnn_table_gather_kernel interpolates every edge's message and
//                        scalar from the table that mdx_egnn_table.hip has checked.
//
// What the forms share as functions: the head's value and the normalisation, the sum of a node's pieces, and from mdx_launch.hpp
// the wavefront total and the grid.  An edge's coordinate term, the write-back of a node's coordinates and the store of its
// message row are written out in each kernel that has them: as functions they cost a gather instructions, occupancy or time
// (profiles/r23_egnn_node_unit.md) -- a change to one of them is made in each kernel of THIS file that has it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_egnn_table.hpp"
#include "mdx_launch.hpp"

using namespace mdx;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The two per-edge options of E_GCL's coordinate update (models/egnn.py:128-131, 234-264), applied where the head's scalar meets
// the coordinate difference:
//   MDX_EGNN_COORD_TANH       the coordinate MLP ends in nn.Tanh: s_e <- tanh(s_e)
//   MDX_EGNN_COORD_NORMALIZE  coord_diff <- f(r^2) coord_diff, f(r^2) = tanh(r^2) / sqrt(r^2 + epsilon^2), epsilon = 1e-8, r^2 the
//                             squared length of coord_diff summed in component order (normalize_radial_norm)
// trans = (f coord_diff) s, in the reference's order of operations.
__device__ __forceinline__ float coord_head_value(float s, int flags) { return (flags & MDX_EGNN_COORD_TANH) ? tanhf(s) : s; }
__device__ __forceinline__ float normalize_factor(float r2) { return tanhf(r2) / sqrtf(r2 + 1.0e-16f); }

// Quad q of the sum of a node's pieces, in increasing edge order: the boundary rows e / 16 of its edges e = 15 mod 16 and, when
// its last edge is not one of those, its own row (last_row = boundary_rows + node: the compact layout the edge chain writes,
// aggregate_pieces).
__device__ __forceinline__ f32x4 piece_sum(const float* pieces, int64_t e0, int64_t e1, int64_t deg, int64_t last_row, int H, int q)
{
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int64_t e = e0 | 15; e < e1 - 1; e += 16) acc += reinterpret_cast<const f32x4*>(pieces + (e >> 4) * H)[q];
    if (deg > 0) acc += reinterpret_cast<const f32x4*>(pieces + last_row * H)[q];
    return acc;
}

// coord_out[i,:] = coord[i,:] + scale_i sum_{e in segment i} (coord[i,:] - coord[dst_e,:]) * s_e
__global__ __launch_bounds__(256) void egnn_coord_aggregate_kernel(const float* __restrict__ s, const float* __restrict__ coord,
                                                                   const int64_t* __restrict__ edges,
                                                                   const int64_t* __restrict__ offsets,
                                                                   const int64_t* __restrict__ degree, int64_t n_nodes, int D,
                                                                   int mean, int flags, float* __restrict__ out)
{
    const int64_t total = n_nodes * D;
    for (int64_t idx = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t node = idx / D;
        const int k = (int)(idx - node * D);
        const int64_t e0 = offsets[node], deg = degree[node];
        const float ci = coord[idx];
        float acc = 0.0f;
        for (int64_t e = e0; e < e0 + deg; ++e) {
            const int64_t dst = edges[2 * e + 1];
            float diff = ci - coord[dst * D + k];
            if (flags & MDX_EGNN_COORD_NORMALIZE) {
                float r2 = 0.0f;
                for (int j = 0; j < D; ++j) {
                    const float dj = coord[node * D + j] - coord[dst * D + j];
                    r2 += dj * dj;
                }
                diff = normalize_factor(r2) * diff;
            }
            acc += diff * coord_head_value(s[e], flags);
        }
        if (mean && deg > 0) acc = acc / (float)deg;          // (a true division, as unsorted_segment_mean's: egnn_utils.py:66-68)
        out[idx] = ci + acc;
    }
}

// out[i,:] = (1/degree_i if mean) x sum of node i's pieces (piece_sum).  One wavefront per node, 16 bytes per lane.
// `left` (nullable): out rows are [left[i,:] | sum_i] of width 2 H -- the input of the node MLP's first layer (h | agg), written
// in the one pass over the nodes instead of a concatenation afterwards.
__global__ __launch_bounds__(256) void segment_combine_kernel(const float* __restrict__ pieces, const int64_t* __restrict__ offsets,
                                                              const int64_t* __restrict__ degree, int64_t n_nodes, int H,
                                                              int mean, float* __restrict__ out, const float* __restrict__ left,
                                                              int64_t boundary_rows)
{
    const int lane = threadIdx.x % kWave;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
    const int quads = H >> 2;
    for (int64_t node = wave; node < n_nodes; node += n_waves) {
        const int64_t e0 = offsets[node], deg = degree[node], e1 = e0 + deg;
        const float count = (mean && deg > 0) ? (float)deg : 1.0f;      // the mean DIVIDES by the count (egnn_utils.py:66-68)
        // the node's last piece: a boundary row if its last edge is 15 mod 16, else the node's own row
        const int64_t last_row = ((e1 - 1) & 15) == 15 ? ((e1 - 1) >> 4) : boundary_rows + node;
        for (int q = lane; q < quads; q += kWave) {
            f32x4 acc = piece_sum(pieces, e0, e1, deg, last_row, H, q);
            if (mean) acc = acc / count;
            if (left) {
                reinterpret_cast<f32x4*>(out + node * 2 * H)[q] = reinterpret_cast<const f32x4*>(left + node * H)[q];
                reinterpret_cast<f32x4*>(out + node * 2 * H + H)[q] = acc;
            } else {
                reinterpret_cast<f32x4*>(out + node * H)[q] = acc;
            }
        }
    }
}

// segment_combine_kernel and egnn_coord_aggregate_kernel as ONE pass over the nodes (one wavefront per node): the message part
// exactly as segment_combine_kernel; the coordinate part with the node's edges dealt to the lanes (edge offset + lane, + 64, ...),
// D partial sums per lane and a butterfly over the wavefront -- a fixed order, no atomics.  D <= 8.
__global__ __launch_bounds__(256) void egnn_node_gather_kernel(const float* __restrict__ pieces, const int64_t* __restrict__ offsets,
                                                               const int64_t* __restrict__ degree, int64_t n_nodes, int H,
                                                               int mean_messages, float* __restrict__ out,
                                                               const float* __restrict__ left, int64_t boundary_rows,
                                                               const float* __restrict__ s, const float* __restrict__ coord,
                                                               const int64_t* __restrict__ edges, int D, int mean_coords,
                                                               int flags, float* __restrict__ coord_out)
{
    const int lane = threadIdx.x % kWave;
    const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / kWave;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / kWave;
    const int quads = H >> 2;
    for (int64_t node = wave; node < n_nodes; node += n_waves) {
        const int64_t e0 = offsets[node], deg = degree[node], e1 = e0 + deg;
        // coordinates first (their loads are the long-latency ones)
        float part[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ci[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) ci[k] = k < D ? coord[node * D + k] : 0.0f;
        for (int64_t e = e0 + lane; e < e1; e += kWave) {
            const int64_t dst = edges[2 * e + 1];
            const float se = coord_head_value(s[e], flags);
            if (flags & MDX_EGNN_COORD_NORMALIZE) {          // (uniform per launch)
                float diff[8], r2 = 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    diff[k] = k < D ? ci[k] - coord[dst * D + k] : 0.0f;
                    if (k < D) r2 += diff[k] * diff[k];
                }
                const float f = normalize_factor(r2);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < D) part[k] += (f * diff[k]) * se;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < D) part[k] += (ci[k] - coord[dst * D + k]) * se;
            }
        }
        // messages (pieces == null, uniform per launch: the caller reads the coordinates alone -- the last graph layer of a
        // forward whose atom-type logits nobody reads)
        const float count = (mean_messages && deg > 0) ? (float)deg : 1.0f;      // (a true division: egnn_utils.py:66-68)
        const int64_t last_row = ((e1 - 1) & 15) == 15 ? ((e1 - 1) >> 4) : boundary_rows + node;
        for (int q = lane; pieces && q < quads; q += kWave) {
            f32x4 acc = piece_sum(pieces, e0, e1, deg, last_row, H, q);
            if (mean_messages) acc = acc / count;
            if (left) {
                reinterpret_cast<f32x4*>(out + node * 2 * H)[q] = reinterpret_cast<const f32x4*>(left + node * H)[q];
                reinterpret_cast<f32x4*>(out + node * 2 * H + H)[q] = acc;
            } else {
                reinterpret_cast<f32x4*>(out + node * H)[q] = acc;
            }
        }
        // the coordinate sums over the wavefront (a fixed order)
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < D) part[k] = wave_total_dpp(part[k]);
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
}

// ---- the distance-grid form (the table's layout: mdx_egnn_table.hip) -----------------------------------------------------------
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
        // the coordinate sums over the wavefront (a fixed order)
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < D) part[k] = wave_total_dpp(part[k]);
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

int64_t mdx_egnn_piece_rows(int64_t n_edges, int64_t n_nodes)
{
    if (n_edges < 0 || n_nodes < 0) return -1;
    return ((n_edges + 15) >> 4) + n_nodes;
}

int mdx_segment_combine(const float* pieces, int64_t n_edges, const int64_t* offsets, const int64_t* degree, int64_t n_nodes,
                        int H, int mean, const float* left, float* out, mdx_stream_t stream)
{
    if (n_nodes < 0 || H < 4 || n_edges < 0) return MDX_ERR_INVALID_ARG;
    if (H & 3) return MDX_ERR_UNSUPPORTED;
    if (n_nodes == 0) return MDX_OK;
    if (!pieces || !offsets || !degree || !out) return MDX_ERR_INVALID_ARG;
    hipLaunchKernelGGL(segment_combine_kernel, dim3(node_grid(n_nodes)), dim3(kBlock), 0, as_stream(stream),
                       pieces, offsets, degree, n_nodes, H, mean, out, left, (n_edges + 15) >> 4);
    return launch_status();
}

int mdx_egnn_node_gather(const float* pieces, int64_t n_edges, const int64_t* offsets, const int64_t* degree, int64_t n_nodes,
                         int H, int mean_messages, const float* left, float* out, const float* edge_scalar, const float* coord,
                         int coord_dimension, const int64_t* edges, int mean_coords, int coord_flags, float* coord_out,
                         mdx_stream_t stream)
{
    if (n_nodes < 0 || H < 4 || n_edges < 0 || coord_dimension < 1) return MDX_ERR_INVALID_ARG;
    if (coord_flags & ~(MDX_EGNN_COORD_NORMALIZE | MDX_EGNN_COORD_TANH)) return MDX_ERR_INVALID_ARG;
    if ((H & 3) || coord_dimension > 8) return MDX_ERR_UNSUPPORTED;
    if (n_nodes == 0) return MDX_OK;
    if (!offsets || !degree || !edge_scalar || !coord || !edges || !coord_out) return MDX_ERR_INVALID_ARG;
    // pieces == out == left == null: the coordinate half alone (the same bits as with the message half)
    if (pieces ? !out : (out || left)) return MDX_ERR_INVALID_ARG;
    hipLaunchKernelGGL(egnn_node_gather_kernel, dim3(node_grid(n_nodes)), dim3(kBlock), 0, as_stream(stream),
                       pieces, offsets, degree, n_nodes, H, mean_messages, out, left, (n_edges + 15) >> 4, edge_scalar, coord, edges,
                       coord_dimension, mean_coords, coord_flags, coord_out);
    return launch_status();
}

int mdx_egnn_coord_aggregate(const float* edge_scalar, const float* coord, int coord_dimension, const int64_t* edges,
                             const int64_t* offsets, const int64_t* degree, int64_t n_nodes, int mean, int coord_flags,
                             float* coord_out, mdx_stream_t stream)
{
    if (n_nodes < 0 || coord_dimension < 1) return MDX_ERR_INVALID_ARG;
    if (coord_flags & ~(MDX_EGNN_COORD_NORMALIZE | MDX_EGNN_COORD_TANH)) return MDX_ERR_INVALID_ARG;
    if (n_nodes == 0) return MDX_OK;
    if (!edge_scalar || !coord || !edges || !offsets || !degree || !coord_out) return MDX_ERR_INVALID_ARG;
    int64_t blocks = (n_nodes * coord_dimension + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(egnn_coord_aggregate_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                       edge_scalar, coord, edges, offsets, degree, n_nodes, coord_dimension, mean, coord_flags, coord_out);
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
    hipLaunchKernelGGL(egnn_table_gather_kernel, dim3(node_grid(n_nodes)), dim3(kBlock), 0, as_stream(stream),
                       table, table_scalar, H, n_classes, n_even, inv_spacing, atom_types, offsets, degree, n_nodes, mean_messages,
                       out, left, coord, edges, coord_dimension, mean_coords, coord_flags, coord_out, status);
    return launch_status();
}

}  // extern "C"
