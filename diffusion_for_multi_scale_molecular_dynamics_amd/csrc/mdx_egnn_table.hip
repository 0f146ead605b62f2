// The first EGNN layer of a sampler forward on a distance grid instead of per edge.
//
// Inside the sampler every structure of the batch has the same sigma, so the first layer's node features h0 take one value per
// class (atom type or MASK) and its whole per-edge output -- the message m_ij and the coordinate head's scalar s_ij -- is a
// function F_ab(rho) of the class pair (a, b) and of rho = |c_i - c_j|.  The caller evaluates F on a uniform grid in rho with
// the edge chain itself (mdx_egnn_edge_chain, MDX_EGNN_MESSAGES_ROWS, one "edge" per (a, b, grid point)).  This unit decides
// whether that table may be used:
//
//   egnn_table_check_kernel     compare the cubic interpolation of the even grid points at the odd ones (the cell midpoints,
//   egnn_table_verdict_kernel   where the interpolation error peaks) with the chain's own values there, per class pair and
//                               column, relative to the pair's largest |value|; raise MDX_STATUS_EGNN_TABLE above the
//                               tolerance, or when sigma is not uniform over the batch.
//
// The kernel that reads the table per node, egnn_table_gather_kernel, sits with the other per-node passes in mdx_egnn_node.hip;
// the interpolation both use is mdx_egnn_table.hpp.
//
// Grid layout (rows of the chain's output): class pair p = a n_classes + b owns rows [p K, p K + K), K = 2 n_even - 1; row p K + m
// is the even point rho = m h (m < n_even), row p K + n_even + j the midpoint rho = (j + 1/2) h (j < n_even - 1), h = 1 /
// inv_spacing.  F is even in rho (it depends on rho^2 only): the point left of rho = 0 is the point right of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_egnn_table.hpp"
#include "mdx_launch.hpp"

using namespace mdx;

namespace {

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

}  // extern "C"
