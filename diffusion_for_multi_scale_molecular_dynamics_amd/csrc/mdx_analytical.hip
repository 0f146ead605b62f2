// The analytical score network: the exact score of wrapped Gaussians of width sigma_d around equilibrium sites, optionally
// symmetrised over every permutation of the atoms (models/score_networks/analytical_score_network.py:135-298), and the two
// elementwise functions it is made of (score/wrapped_gaussian_score.py:41-92, 131-419).  See include/mdx_hip.h for the contracts.
//
//   wrapped_gaussian_score_kernel   one value per thread: sigma x score by the reference's three formulas (1a, 1b, Ewald form)
//   log_wrapped_gaussians_kernel    one row per thread: sum over the row of logsumexp_k(-(u + k)^2 / 2 sigma^2) - log(sqrt(2 pi) sigma)
//   analytical_score_kernel         one workgroup per structure.  Every term of the reference's [N!, B, N, D] tensors depends
//     only on (atom n, site j, dimension d), so an N x N table replaces them:
//       T[n][j]    = sum_d logterm(u_njd, s_nd)         u = wrap(x_n - site_j), s = sqrt(sigma_d^2 + sigma^2)
//       S[n][j][d] = sigma score(u_njd, s_nd) / s_nd
//     without permutations only the diagonal j = n exists (any N <= 1024).  With permutations (N <= 8) the lanes enumerate the
//     N! permutations p by their Lehmer code: log_w[p] = sum_n T[n][p(n)]; a first pass takes the maximum, a second one
//     sum_p exp(log_w - max) and the weighted S.  Reductions are per-lane sums in index order, a fixed xor butterfly over the
//     lanes, then the wavefronts in index order: no float atomics, the same bits on every launch.
// Binary64 throughout, from the binary32 inputs promoted once; the outputs are rounded once to binary32.
// 64-wide wavefronts are assumed (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_math.hpp"
#include "mdx_reduce.hpp"
#include "mdx_wrapped_score.hpp"

using namespace mdx;

namespace {

constexpr int kWaves = kBlock / kWave;
constexpr int kMaxAtoms = 1024;
constexpr int kMaxPermutedAtoms = 8;          // 8! = 40 320 permutations
constexpr int kMaxDimension = 3;
constexpr int kMaxTranslation = 64;           // kmax: the sums run over 2 kmax + 1 translations
constexpr int kTerms = kMaxPermutedAtoms * kMaxDimension;
constexpr int kBadSigma = 1, kBadCoordinate = 2;

__device__ __forceinline__ bool coordinate_valid(double x) { return x >= 0.0 && x < 1.0; }

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

// The permutation with index p in [0, N!) as N nibbles (atom n -> site): p's mixed-radix digits are the Lehmer code c_n in
// [0, N - n), and atom n takes the c_n-th site still free.
__device__ __forceinline__ uint32_t permutation_of(uint32_t p, int N)
{
    uint32_t code = 0;
#pragma unroll
    for (int m = 1; m <= kMaxPermutedAtoms; ++m)
        if (m <= N) {
            code |= (p % (uint32_t)m) << (4 * (N - m));
            p /= (uint32_t)m;
        }
    uint64_t free_sites = 0x76543210ull;
    uint32_t sites = 0;
#pragma unroll
    for (int n = 0; n < kMaxPermutedAtoms; ++n)
        if (n < N) {
            const int shift = 4 * (int)((code >> (4 * n)) & 0xfu);
            sites |= (uint32_t)((free_sites >> shift) & 0xfull) << (4 * n);
            free_sites = (free_sites & ((1ull << shift) - 1ull)) | ((free_sites >> (shift + 4)) << shift);
        }
    return sites;
}

__global__ __launch_bounds__(kBlock) void analytical_score_kernel(const float* __restrict__ x, const float* __restrict__ sigma,
                                                                  int sigma_per_element, const float* __restrict__ sites,
                                                                  double sigma_d_square, int kmax, int use_permutations, int N,
                                                                  int D, int permutations, float* __restrict__ score,
                                                                  float* __restrict__ probabilities, uint32_t* status)
{
    // permutation path only: T [8][8], S [8][8][3] and the log terms [8][8][3] that T is summed from
    __shared__ double table[kMaxPermutedAtoms * kMaxPermutedAtoms * (1 + 2 * kMaxDimension)];
    __shared__ double partial[kWaves * (kTerms + 1)];
    __shared__ int bad;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int ND = N * D;
    const float* xb = x + b * ND;
    const float* sb = sigma + (sigma_per_element ? b * ND : b);
    float* out = score + b * ND;
    if (tid == 0) bad = 0;
    __syncthreads();
    {
        int mine = 0;
        for (int i = tid; i < ND; i += kBlock) {
            if (!coordinate_valid((double)xb[i])) mine |= kBadCoordinate;
            if (!sigma_valid((double)sb[sigma_per_element ? i : 0])) mine |= kBadSigma;
        }
        if (mine) atomicOr(&bad, mine);
    }
    __syncthreads();
    if (bad != 0) {
        const float nan = __builtin_nanf("");
        for (int i = tid; i < ND; i += kBlock) out[i] = nan;
        if (tid == 0) {
            if (probabilities) probabilities[b] = nan;
            if (status)
                atomicOr(status, ((bad & kBadSigma) ? MDX_STATUS_ANALYTICAL_SIGMA : 0u) |
                                     ((bad & kBadCoordinate) ? MDX_STATUS_ANALYTICAL_COORDINATES : 0u));
        }
        return;
    }

    if (!use_permutations) {
        double log_terms = 0.0;
        for (int i = tid; i < ND; i += kBlock) {
            const double s_t = (double)sb[sigma_per_element ? i : 0];
            const double s_eff = sqrt(sigma_d_square + s_t * s_t);
            const double u = wrap01((double)xb[i] - (double)sites[i]);
            out[i] = (float)(s_t * (sigma_normalized_score(u, s_eff, kmax) / s_eff));
            if (probabilities) log_terms += log_wrapped_gaussian(u, s_eff, kmax);
        }
        if (probabilities) {
            const double log_w = block_sum(log_terms, partial);
            if (tid == 0) probabilities[b] = (float)exp(log_w);
        }
        return;
    }

    // ---- stage: the N x N table
    double* T = table;                                                      // [8][8]
    double* S = table + kMaxPermutedAtoms * kMaxPermutedAtoms;              // [8][8][3]
    double* logs = S + kMaxPermutedAtoms * kMaxPermutedAtoms * kMaxDimension;   // [8][8][3]
    for (int e = tid; e < N * N * D; e += kBlock) {
        const int d = e % D, j = (e / D) % N, n = e / (D * N);
        const double s_t = (double)sb[sigma_per_element ? n * D + d : 0];
        const double s_eff = sqrt(sigma_d_square + s_t * s_t);
        const double u = wrap01((double)xb[n * D + d] - (double)sites[j * D + d]);
        const int slot = (n * kMaxPermutedAtoms + j) * kMaxDimension + d;
        S[slot] = s_t * (sigma_normalized_score(u, s_eff, kmax) / s_eff);
        logs[slot] = log_wrapped_gaussian(u, s_eff, kmax);
    }
    __syncthreads();
    for (int e = tid; e < N * N; e += kBlock) {
        const int j = e % N, n = e / N;
        double sum = 0.0;
        for (int d = 0; d < D; ++d) sum += logs[(n * kMaxPermutedAtoms + j) * kMaxDimension + d];
        T[n * kMaxPermutedAtoms + j] = sum;
    }
    __syncthreads();

    // ---- first pass: the largest log weight
    double largest = -__builtin_huge_val();
    for (int p = tid; p < permutations; p += kBlock) {
        const uint32_t perm = permutation_of((uint32_t)p, N);
        double log_w = 0.0;
#pragma unroll
        for (int n = 0; n < kMaxPermutedAtoms; ++n)
            if (n < N) log_w += T[n * kMaxPermutedAtoms + (int)((perm >> (4 * n)) & 0xfu)];
        largest = log_w > largest ? log_w : largest;
    }
    largest = wave_max(largest);
    if (lane == 0) partial[wave] = largest;
    __syncthreads();
    largest = partial[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) largest = partial[w] > largest ? partial[w] : largest;
    __syncthreads();

    // ---- second pass: sum_p exp(log_w - max) and the weighted score terms
    double weight_sum = 0.0;
    double acc[kMaxPermutedAtoms][kMaxDimension];
#pragma unroll
    for (int n = 0; n < kMaxPermutedAtoms; ++n)
#pragma unroll
        for (int d = 0; d < kMaxDimension; ++d) acc[n][d] = 0.0;
    for (int p = tid; p < permutations; p += kBlock) {
        const uint32_t perm = permutation_of((uint32_t)p, N);
        double log_w = 0.0;
#pragma unroll
        for (int n = 0; n < kMaxPermutedAtoms; ++n)
            if (n < N) log_w += T[n * kMaxPermutedAtoms + (int)((perm >> (4 * n)) & 0xfu)];
        const double w = exp(log_w - largest);
        weight_sum += w;
#pragma unroll
        for (int n = 0; n < kMaxPermutedAtoms; ++n)
            if (n < N) {
                const double* row = S + (n * kMaxPermutedAtoms + (int)((perm >> (4 * n)) & 0xfu)) * kMaxDimension;
#pragma unroll
                for (int d = 0; d < kMaxDimension; ++d)
                    if (d < D) acc[n][d] += w * row[d];
            }
    }
    weight_sum = wave_sum(weight_sum);
    if (lane == 0) partial[wave * (kTerms + 1) + kTerms] = weight_sum;
#pragma unroll
    for (int n = 0; n < kMaxPermutedAtoms; ++n)
#pragma unroll
        for (int d = 0; d < kMaxDimension; ++d) {
            if (n < N && d < D) {
                const double v = wave_sum(acc[n][d]);
                if (lane == 0) partial[wave * (kTerms + 1) + n * kMaxDimension + d] = v;
            }
        }
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) total += partial[w * (kTerms + 1) + kTerms];
    if (tid < ND) {
        const int n = tid / D, d = tid % D;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) v += partial[w * (kTerms + 1) + n * kMaxDimension + d];
        out[tid] = (float)(v / total);
    }
    // probabilities = sum_p exp(log_w[p]) / N!   (:242-244)
    if (probabilities && tid == 0) probabilities[b] = (float)exp(largest + log(total / (double)permutations));
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
    int permutations = 1;
    for (int m = 2; m <= N && use_permutation_invariance; ++m) permutations *= m;
    hipLaunchKernelGGL(analytical_score_kernel, dim3((unsigned)batch), dim3(kBlock), 0, as_stream(stream), relative_coordinates,
                       sigmas, sigma_per_element ? 1 : 0, equilibrium_relative_coordinates, sigma_d_square, kmax,
                       use_permutation_invariance ? 1 : 0, N, D, permutations, sigma_normalized_scores, probabilities, status);
    return launch_status();
}

}  // extern "C"
