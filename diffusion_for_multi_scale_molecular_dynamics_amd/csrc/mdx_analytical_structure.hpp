// The analytical score network's evaluation of ONE structure by one workgroup of kBlock threads, shared by the units that need
// its binary64 values (mdx_analytical.hip rounds them to binary32; mdx_loss.hip's regression kernel subtracts them from a
// score first): the validity scan, the plain path, the N x N table and the two passes over the N! permutations
// (models/score_networks/analytical_score_network.py:135-298).
//     T[n][j]    = sum_d logterm(u_njd, s_nd)         u = wrap(x_n - site_j), s = sqrt(sigma_d^2 + sigma^2)
//     S[n][j][d] = sigma score(u_njd, s_nd) / s_nd
// without permutations only the diagonal j = n exists (any N <= 1024).  With permutations (N <= 8) the lanes enumerate the
// N! permutations p by their Lehmer code: log_w[p] = sum_n T[n][p(n)]; a first pass takes the maximum, a second one
// sum_p exp(log_w - max) and the weighted S.  Reductions are per-lane sums in index order, a fixed xor butterfly over the
// lanes, then the wavefronts in index order: no float atomics, the same bits on every launch.
// Header-only with internal linkage, like mdx_wrapped_score.hpp: each unit compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_reduce.hpp"
#include "mdx_wrapped_score.hpp"

namespace mdx {
namespace {

constexpr int kAnalyticalWaves = kBlock / kWave;
constexpr int kAnalyticalMaxAtoms = 1024;
constexpr int kMaxPermutedAtoms = 8;          // 8! = 40 320 permutations
constexpr int kAnalyticalMaxDimension = 3;
constexpr int kAnalyticalMaxTranslation = 64; // kmax: the sums run over 2 kmax + 1 translations
constexpr int kAnalyticalTerms = kMaxPermutedAtoms * kAnalyticalMaxDimension;
constexpr int kBadSigma = 1, kBadCoordinate = 2;

__device__ __forceinline__ bool coordinate_valid(double x) { return x >= 0.0 && x < 1.0; }

// the status bits of what analytical_structure returns
__device__ __forceinline__ uint32_t analytical_status_bits(int bad)
{
    return ((bad & kBadSigma) ? MDX_STATUS_ANALYTICAL_SIGMA : 0u) | ((bad & kBadCoordinate) ? MDX_STATUS_ANALYTICAL_COORDINATES : 0u);
}

// N! for N <= kMaxPermutedAtoms under permutation invariance, else 1 (host side)
inline int analytical_permutations(int N, int use_permutation_invariance)
{
    int permutations = 1;
    for (int m = 2; m <= N && use_permutation_invariance; ++m) permutations *= m;
    return permutations;
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

// One structure: xb f32 [N, D], sb its sigma (one word, or [N, D] with sigma_per_element), sites f32 [N, D].  Every thread of
// the workgroup (kBlock of them) must call it.  emit(i, v) receives the binary64 sigma-normalised score v of element i exactly
// once, from the thread that owns i: i = tid, tid + kBlock, .. in index order on the plain path, i = tid < N D on the
// permutation path.  probability (nullable) receives the structure's probability, rounded once.  Returns 0, or -- the same in
// every thread, with nothing emitted and probability left alone -- kBadSigma | kBadCoordinate for a sigma that is not finite and
// positive or a coordinate outside [0, 1).
template <class Emit>
__device__ __forceinline__ int analytical_structure(const float* __restrict__ xb, const float* __restrict__ sb, int sigma_per_element,
                                                    const float* __restrict__ sites, double sigma_d_square, int kmax,
                                                    int use_permutations, int N, int D, int permutations, float* probability,
                                                    Emit emit)
{
    // permutation path only: T [8][8], S [8][8][3] and the log terms [8][8][3] that T is summed from
    __shared__ double table[kMaxPermutedAtoms * kMaxPermutedAtoms * (1 + 2 * kAnalyticalMaxDimension)];
    __shared__ double partial[kAnalyticalWaves * (kAnalyticalTerms + 1)];
    __shared__ int bad;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int ND = N * D;
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
    if (bad != 0) return bad;

    if (!use_permutations) {
        double log_terms = 0.0;
        for (int i = tid; i < ND; i += kBlock) {
            const double s_t = (double)sb[sigma_per_element ? i : 0];
            const double s_eff = sqrt(sigma_d_square + s_t * s_t);
            const double u = wrap01((double)xb[i] - (double)sites[i]);
            emit(i, s_t * (sigma_normalized_score(u, s_eff, kmax) / s_eff));
            if (probability) log_terms += log_wrapped_gaussian(u, s_eff, kmax);
        }
        if (probability) {
            const double log_w = block_sum(log_terms, partial);
            if (tid == 0) *probability = (float)exp(log_w);
        }
        return 0;
    }

    // ---- stage: the N x N table
    double* T = table;                                                                   // [8][8]
    double* S = table + kMaxPermutedAtoms * kMaxPermutedAtoms;                           // [8][8][3]
    double* logs = S + kMaxPermutedAtoms * kMaxPermutedAtoms * kAnalyticalMaxDimension;  // [8][8][3]
    for (int e = tid; e < N * N * D; e += kBlock) {
        const int d = e % D, j = (e / D) % N, n = e / (D * N);
        const double s_t = (double)sb[sigma_per_element ? n * D + d : 0];
        const double s_eff = sqrt(sigma_d_square + s_t * s_t);
        const double u = wrap01((double)xb[n * D + d] - (double)sites[j * D + d]);
        const int slot = (n * kMaxPermutedAtoms + j) * kAnalyticalMaxDimension + d;
        S[slot] = s_t * (sigma_normalized_score(u, s_eff, kmax) / s_eff);
        logs[slot] = log_wrapped_gaussian(u, s_eff, kmax);
    }
    __syncthreads();
    for (int e = tid; e < N * N; e += kBlock) {
        const int j = e % N, n = e / N;
        double sum = 0.0;
        for (int d = 0; d < D; ++d) sum += logs[(n * kMaxPermutedAtoms + j) * kAnalyticalMaxDimension + d];
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
    for (int w = 1; w < kAnalyticalWaves; ++w) largest = partial[w] > largest ? partial[w] : largest;
    __syncthreads();

    // ---- second pass: sum_p exp(log_w - max) and the weighted score terms
    double weight_sum = 0.0;
    double acc[kMaxPermutedAtoms][kAnalyticalMaxDimension];
#pragma unroll
    for (int n = 0; n < kMaxPermutedAtoms; ++n)
#pragma unroll
        for (int d = 0; d < kAnalyticalMaxDimension; ++d) acc[n][d] = 0.0;
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
                const double* row = S + (n * kMaxPermutedAtoms + (int)((perm >> (4 * n)) & 0xfu)) * kAnalyticalMaxDimension;
#pragma unroll
                for (int d = 0; d < kAnalyticalMaxDimension; ++d)
                    if (d < D) acc[n][d] += w * row[d];
            }
    }
    weight_sum = wave_sum(weight_sum);
    if (lane == 0) partial[wave * (kAnalyticalTerms + 1) + kAnalyticalTerms] = weight_sum;
#pragma unroll
    for (int n = 0; n < kMaxPermutedAtoms; ++n)
#pragma unroll
        for (int d = 0; d < kAnalyticalMaxDimension; ++d) {
            if (n < N && d < D) {
                const double v = wave_sum(acc[n][d]);
                if (lane == 0) partial[wave * (kAnalyticalTerms + 1) + n * kAnalyticalMaxDimension + d] = v;
            }
        }
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < kAnalyticalWaves; ++w) total += partial[w * (kAnalyticalTerms + 1) + kAnalyticalTerms];
    if (tid < ND) {
        const int n = tid / D, d = tid % D;
        double v = 0.0;
#pragma unroll
        for (int w = 0; w < kAnalyticalWaves; ++w) v += partial[w * (kAnalyticalTerms + 1) + n * kAnalyticalMaxDimension + d];
        emit(tid, v / total);
    }
    // probabilities = sum_p exp(log_w[p]) / N!   (:242-244)
    if (probability && tid == 0) *probability = (float)exp(largest + log(total / (double)permutations));
    return 0;
}

}  // namespace
}  // namespace mdx
