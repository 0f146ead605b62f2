// The analytical score network: the exact score of wrapped Gaussians of width sigma_d around equilibrium sites, optionally
// symmetrised over every permutation of the atoms (models/score_networks/analytical_score_network.py:135-298), and the two
// elementwise functions it is made of (score/wrapped_gaussian_score.py:41-92, 131-419).  See include/mdx_hip.h for the contracts.
//
//   wrapped_gaussian_score_kernel   one value per thread: sigma x score by the reference's three formulas (1a, 1b, Ewald form)
//   log_wrapped_gaussians_kernel    one row per thread: sum over the row of logsumexp_k(-(u + k)^2 / 2 sigma^2) - log(sqrt(2 pi) sigma)
//   analytical_score_kernel         one workgroup per structure.  Every term of the reference's [N!, B, N, D] tensors depends
//     only on (atom n, site j, dimension d), so an N x N table replaces them: the per-structure evaluation is
//     mdx_analytical_structure.hpp's, shared with the regression kernel of mdx_loss.hip; this kernel rounds its values once.
//     No float atomics, the same bits on every launch.
// Binary64 throughout, from the binary32 inputs promoted once; the outputs are rounded once to binary32.
// 64-wide wavefronts are assumed (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_analytical_structure.hpp"
#include "mdx_launch.hpp"
#include "mdx_math.hpp"
#include "mdx_reduce.hpp"
#include "mdx_wrapped_score.hpp"

using namespace mdx;

namespace {

constexpr int kMaxAtoms = kAnalyticalMaxAtoms;
constexpr int kMaxDimension = kAnalyticalMaxDimension;
constexpr int kMaxTranslation = kAnalyticalMaxTranslation;

__global__ __launch_bounds__(kBlock) void wrapped_gaussian_score_kernel(const float* __restrict__ u, const float* __restrict__ sigma,
                                                                        int64_t n, int kmax, int coordinates_bounded,
                                                                        float* __restrict__ out, uint32_t* status)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const double ui = (double)u[i], si = (double)sigma[i];
        uint32_t bits = 0;
        if (!sigma_valid(si)) bits |= MDX_STATUS_ANALYTICAL_SIGMA;
        if (coordinates_bounded ? !coordinate_valid(ui) : !finite_(ui)) bits |= MDX_STATUS_ANALYTICAL_COORDINATES;
        if (bits) {
            out[i] = __builtin_nanf("");
            if (status) atomicOr(status, bits);
            continue;
        }
        out[i] = (float)sigma_normalized_score(ui, si, kmax);
    }
}

__global__ __launch_bounds__(kBlock) void log_wrapped_gaussians_kernel(const float* __restrict__ u, const float* __restrict__ sigma,
                                                                       int64_t rows, int row_length, int kmax,
                                                                       float* __restrict__ out, uint32_t* status)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < rows; r += stride) {
        double sum = 0.0;
        uint32_t bits = 0;
        for (int e = 0; e < row_length; ++e) {
            const double ue = (double)u[r * row_length + e], se = (double)sigma[r * row_length + e];
            if (!sigma_valid(se)) bits |= MDX_STATUS_ANALYTICAL_SIGMA;
            if (!finite_(ue)) bits |= MDX_STATUS_ANALYTICAL_COORDINATES;
            if (!bits) sum += log_wrapped_gaussian(ue, se, kmax);
        }
        if (bits) {
            out[r] = __builtin_nanf("");
            if (status) atomicOr(status, bits);
            continue;
        }
        out[r] = (float)sum;
    }
}

__global__ __launch_bounds__(kBlock) void analytical_score_kernel(const float* __restrict__ x, const float* __restrict__ sigma,
                                                                  int sigma_per_element, const float* __restrict__ sites,
                                                                  double sigma_d_square, int kmax, int use_permutations, int N,
                                                                  int D, int permutations, float* __restrict__ score,
                                                                  float* __restrict__ probabilities, uint32_t* status)
{
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x;
    const int ND = N * D;
    float* out = score + b * ND;
    const int bad = analytical_structure(x + b * ND, sigma + (sigma_per_element ? b * ND : b), sigma_per_element, sites,
                                         sigma_d_square, kmax, use_permutations, N, D, permutations,
                                         probabilities ? probabilities + b : nullptr,
                                         [out](int i, double v) { out[i] = (float)v; });
    if (bad != 0) {
        const float nan = __builtin_nanf("");
        for (int i = tid; i < ND; i += kBlock) out[i] = nan;
        if (tid == 0) {
            if (probabilities) probabilities[b] = nan;
            if (status) atomicOr(status, analytical_status_bits(bad));
        }
    }
}

}  // namespace

extern "C" {

int mdx_wrapped_gaussian_sigma_normalized_score(const float* relative_coordinates, const float* sigmas, int64_t n, int kmax,
                                                int coordinates_bounded, float* out, uint32_t* status, mdx_stream_t stream)
{
    if (n < 0 || kmax < 0) return MDX_ERR_INVALID_ARG;
    if (kmax > kMaxTranslation) return MDX_ERR_UNSUPPORTED;
    if (n == 0) return MDX_OK;
    if (!relative_coordinates || !sigmas || !out) return MDX_ERR_INVALID_ARG;
    hipLaunchKernelGGL(wrapped_gaussian_score_kernel, dim3(flat_grid(n)), dim3(kBlock), 0, as_stream(stream), relative_coordinates,
                       sigmas, n, kmax, coordinates_bounded, out, status);
    return launch_status();
}

int mdx_log_wrapped_gaussians(const float* relative_coordinates, const float* sigmas, int64_t rows, int row_length, int kmax,
                              float* out, uint32_t* status, mdx_stream_t stream)
{
    if (rows < 0 || row_length < 1 || kmax < 0) return MDX_ERR_INVALID_ARG;
    if (kmax > kMaxTranslation) return MDX_ERR_UNSUPPORTED;
    if (rows == 0) return MDX_OK;
    if (!relative_coordinates || !sigmas || !out) return MDX_ERR_INVALID_ARG;
    hipLaunchKernelGGL(log_wrapped_gaussians_kernel, dim3(flat_grid(rows)), dim3(kBlock), 0, as_stream(stream), relative_coordinates,
                       sigmas, rows, row_length, kmax, out, status);
    return launch_status();
}

int mdx_analytical_score(const float* relative_coordinates, const float* sigmas, int sigma_per_element,
                         const float* equilibrium_relative_coordinates, double sigma_d_square, int kmax,
                         int use_permutation_invariance, int64_t batch, int number_of_atoms, int spatial_dimension,
                         float* sigma_normalized_scores, float* probabilities, uint32_t* status, mdx_stream_t stream)
{
    const int N = number_of_atoms, D = spatial_dimension;
    if (batch < 0 || N < 1 || D < 1 || kmax < 0 || !(sigma_d_square > 0.0)) return MDX_ERR_INVALID_ARG;
    if (N > kMaxAtoms || D > kMaxDimension || kmax > kMaxTranslation || batch > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (use_permutation_invariance && N > kMaxPermutedAtoms) return MDX_ERR_UNSUPPORTED;
    if (batch == 0) return MDX_OK;
    if (!relative_coordinates || !sigmas || !equilibrium_relative_coordinates || !sigma_normalized_scores) return MDX_ERR_INVALID_ARG;
    hipLaunchKernelGGL(analytical_score_kernel, dim3((unsigned)batch), dim3(kBlock), 0, as_stream(stream), relative_coordinates,
                       sigmas, sigma_per_element ? 1 : 0, equilibrium_relative_coordinates, sigma_d_square, kmax,
                       use_permutation_invariance ? 1 : 0, N, D, analytical_permutations(N, use_permutation_invariance),
                       sigma_normalized_scores, probabilities, status);
    return launch_status();
}

}  // extern "C"
