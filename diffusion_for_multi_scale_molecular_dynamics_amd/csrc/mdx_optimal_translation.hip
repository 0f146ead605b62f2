// The global translation that minimises the squared geodesic distance between two configurations on the torus: the reference's
// transport/optimal_translation.py (find_squared_geodesic_distance_minimizing_translation), which tabulates the solutions of
//     tau = (sum_i l_i(tau)) / N - (sum_i (y_i - x_i)) / N,      l_i(tau) = Round(y_i - x_i + tau),     -1/2 <= tau < 1/2
// per structure and dimension and keeps the one of least distance.  See include/mdx_hip.h.
//
//   optimal_translation_kernel    one workgroup per (structure, dimension), one thread per atom (64 .. 256 threads)
//       stage     delta_i = y_i - x_i, l0_i = floor(delta_i - 1/2 + 1/2), crossing c_i = -(delta_i - l0_i - 1/2) into LDS
//       rank      one loop over the atoms: the rank of the thread's own crossing (#{c_j < c_i} + #{j < i : c_j = c_i}: a
//                 permutation also with equal crossings), sorted[rank_i] = c_i; one wavefront of the workgroup also makes
//                 sum delta and sum l0 in atom order and #{c_j < 1/2} in that loop
//       plateaus  thread k: left_k, right_k from the sorted crossings, L_k = sum l0 + min(k, #{c_j < 1/2}) (the crossings are
//                 sorted, so the reference's cumulative count is that minimum), rhs_k = L_k / N - (sum delta) / N and the strict
//                 test left_k < rhs_k < right_k
//       costs     the candidates dealt round-robin to the wavefronts (every wavefront ballots the same flags): sum_i g_i^2,
//                 g = d - rint d, d = (y_i + rhs_k) - x_i; lane l adds atoms l, l + 64, .. in that order, then the fixed xor
//                 butterfly
//       choose    the first minimum in plateau order (torch.argmin's rule on the reference's candidate order), by one wavefront
// Binary64 throughout, from the binary32 inputs promoted once; tau is rounded once.  No atomics in the arithmetic, every sum in
// a fixed order and every loop bounded by N + 1 whatever the data: a launch or a hipGraph replay always gives the same bits.
// The status word alone is OR-ed atomically, as everywhere in this library.  64-wide wavefronts are assumed (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_reduce.hpp"

using namespace mdx;

namespace {

constexpr int kMaxAtoms = 256;                // the transport unit's limits
constexpr int kMaxDimension = 3;
constexpr double kTauMin = -0.5, kTauMax = 0.5;      // TAU_RANGE_MIN, TAU_RANGE_MAX
constexpr int kNoPlateau = 0x7fffffff;

__global__ __launch_bounds__(kMaxAtoms) void optimal_translation_kernel(const float* __restrict__ x, int64_t x_stride,
                                                                        const float* __restrict__ y, int N, int D,
                                                                        float* __restrict__ tau, double* __restrict__ squared_distance,
                                                                        int32_t* __restrict__ number_of_candidates, uint32_t* status)
{
    __shared__ double xs[kMaxAtoms], ys[kMaxAtoms], delta[kMaxAtoms], ell0[kMaxAtoms], crossing[kMaxAtoms], sorted[kMaxAtoms];
    __shared__ double rhs[kMaxAtoms + 1], cost[kMaxAtoms + 1];      // cost: +inf where plateau k is no candidate
    __shared__ double sums[2];
    __shared__ int below;
    __shared__ uint8_t candidate[kMaxAtoms + 1];
    const int tid = threadIdx.x, threads = blockDim.x, waves = threads / kWave, wave = tid / kWave, lane = tid % kWave;
    const int64_t b = blockIdx.x / D;
    const int d = blockIdx.x % D;
    const int ND = N * D;
    const float* xb = x + b * x_stride;
    const float* yb = y + b * ND;
    const int64_t out = b * D + d;

    // ---- stage: a coordinate of the structure that is not finite (in any dimension) voids the whole structure
    int mine = 0;
    for (int e = tid; e < ND; e += threads)
        if (!finite_((double)xb[e]) || !finite_((double)yb[e])) mine = 1;
    if (tid < N) {
        const double xi = (double)xb[tid * D + d], yi = (double)yb[tid * D + d];
        const double dl = yi - xi;
        const double l0 = floor((dl + kTauMin) + 0.5);
        xs[tid] = xi;
        ys[tid] = yi;
        delta[tid] = dl;
        ell0[tid] = l0;
        crossing[tid] = -((dl - l0) + kTauMin);
    }
    if (__syncthreads_or(mine)) {
        if (tid == 0) {
            tau[out] = __builtin_nanf("");
            if (squared_distance) squared_distance[out] = __builtin_nan("");
            if (number_of_candidates) number_of_candidates[out] = -1;
            if (status) atomicOr(status, MDX_STATUS_ANALYTICAL_COORDINATES);
        }
        return;
    }

    // ---- rank: one wavefront of the workgroup (its number turns with the workgroup, so that these do not gather on one SIMD)
    // also makes the sums, in atom order; the loads of eight steps are issued together (the loops are bound by LDS latency)
    int rank = 0;
    const double ci = tid < N ? crossing[tid] : 0.0;
    if (wave == (int)(blockIdx.x % waves)) {                    // wave-uniform
        double sum_delta = 0.0, sum_ell0 = 0.0;
        int below_max = 0;
#pragma unroll 8
        for (int j = 0; j < N; ++j) {
            const double cj = crossing[j];
            sum_delta += delta[j];
            sum_ell0 += ell0[j];
            below_max += cj < kTauMax ? 1 : 0;
            rank += (cj < ci || (cj == ci && j < tid)) ? 1 : 0;
        }
        if (lane == 0) {
            sums[0] = sum_delta;
            sums[1] = sum_ell0;
            below = below_max;
        }
    } else {
#pragma unroll 8
        for (int j = 0; j < N; ++j) {
            const double cj = crossing[j];
            rank += (cj < ci || (cj == ci && j < tid)) ? 1 : 0;
        }
    }
    if (tid < N && rank < N) sorted[rank] = ci;
    __syncthreads();

    // ---- plateaus
    const double sum_ell0 = sums[1];
    const double mean_delta = sums[0] / (double)N;
    const int below_max = below;
    for (int k = tid; k <= N; k += threads) {
        const double left = k == 0 ? kTauMin : sorted[k - 1];
        const double right = k == N ? kTauMax : sorted[k];
        const double ell = sum_ell0 + (double)(k < below_max ? k : below_max);
        const double r = ell / (double)N - mean_delta;
        rhs[k] = r;
        cost[k] = __builtin_huge_val();
        candidate[k] = (left < r && r < right) ? 1 : 0;
    }
    __syncthreads();

    // ---- costs: every wavefront reads the same candidate flags, 64 plateaus a round, and takes every waves-th candidate
    int ordinal = 0;
    for (int base = 0; base <= N; base += kWave) {
        const int mine_k = base + lane;
        unsigned long long found = __ballot(mine_k <= N && candidate[mine_k] != 0);
        while (found) {                                         // wave-uniform, at most 64 rounds
            const int k = base + __builtin_ctzll(found);
            found &= found - 1;
            if (ordinal % waves == wave) {
                const double t = rhs[k];
                double part = 0.0;
                for (int i = lane; i < N; i += kWave) {
                    const double dl = (ys[i] + t) - xs[i];
                    const double g = dl - rint(dl);
                    part += g * g;
                }
                const double total = wave_sum(part);
                if (lane == 0) cost[k] = total;
            }
            ++ordinal;
        }
    }
    __syncthreads();

    // ---- choose: the first minimum in plateau order
    if (wave != 0) return;
    double best = __builtin_huge_val();
    int best_k = kNoPlateau, count = 0;
    for (int k = lane; k <= N; k += kWave) {
        const double c = cost[k];
        count += c < __builtin_huge_val() ? 1 : 0;
        if (c < best) {
            best = c;
            best_k = k;
        }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        const double other = __shfl_xor(best, o, kWave);
        const int other_k = __shfl_xor(best_k, o, kWave);
        const bool take = other < best || (other == best && other_k < best_k);
        best = take ? other : best;
        best_k = take ? other_k : best_k;
    }
    count = wave_sum(count);
    if (lane == 0) {
        const bool found = best_k <= N;
        tau[out] = found ? (float)rhs[best_k] : __builtin_huge_valf();
        if (squared_distance) squared_distance[out] = best;      // +inf when no plateau holds its own solution
        if (number_of_candidates) number_of_candidates[out] = count;
        if (!found && status) atomicOr(status, MDX_STATUS_TRANSLATION_NO_CANDIDATE);
    }
}

}  // namespace

extern "C" {

int mdx_optimal_translation(const float* x, int64_t x_batch_stride, const float* y, int64_t batch, int number_of_atoms,
                            int spatial_dimension, float* tau, double* squared_distance, int32_t* number_of_candidates,
                            uint32_t* status, mdx_stream_t stream)
{
    const int N = number_of_atoms, D = spatial_dimension;
    if (batch < 0 || N < 1 || D < 1) return MDX_ERR_INVALID_ARG;
    if (N > kMaxAtoms || D > kMaxDimension || batch > 0x7fffffffLL / kMaxDimension) return MDX_ERR_UNSUPPORTED;
    if (x_batch_stride != 0 && x_batch_stride != (int64_t)N * D) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return MDX_OK;
    if (!x || !y || !tau) return MDX_ERR_INVALID_ARG;
    const dim3 grid((unsigned)(batch * D)), block((unsigned)(cdiv(N, kWave) * kWave));
    hipLaunchKernelGGL(optimal_translation_kernel, grid, block, 0, as_stream(stream), x, x_batch_stride, y, N, D, tau,
                       squared_distance, number_of_candidates, status);
    return launch_status();
}

}  // extern "C"
