// Linear assignment on the device, and what the reference's transport/ and equivariant analytical score network build on it
// (transport/transporter.py:13-196, models/score_networks/equivariant_analytical_score_network.py).  See include/mdx_hip.h.
//
//   lap_solve                     one wavefront per assignment problem: the shortest-augmenting-path Hungarian algorithm with row
//     duals u, column duals v, minv and a way chain.  N augmentations of at most N steps; a step relaxes the free columns against
//     the current row and takes ONE wavefront arg-min.  Lane l owns columns l, l + 64, .. (1, 2 or 4 of them: N <= 256): v, minv,
//     way, the used flag and the column's row stay in its registers; u lives in the wavefront's LDS, where u[row of column] +=
//     delta is a conflict-free scatter (the rows of distinct columns are distinct).  The arg-min is a fixed xor butterfly over
//     (value, column), lexicographic: equal values go to the lower column.  No atomics: a launch always gives the same bits.
//     Every loop is bounded by N whatever the rounding does, and every index it dereferences is checked against N.
//     The cost is a functor: a matrix row in memory, or recomputed from coordinates (the N x N matrix then never exists).
//   linear_assignment_kernel      the raw solver: four wavefronts (problems) per workgroup, costs f32 or f64 in memory
//   transport_align_kernel        one workgroup per structure: Transporter.get_optimal_transport, optionally with the wrapped-
//     Gaussian score of the aligned image fused in (the equivariant analytical network's forward).
//       stage   atan2 centres of x and mu (sums in atom order), x~ = wrap(x - c_x), mu~ = wrap(mu - c_mu) into LDS
//       solve   the point-group operations dealt round-robin to the wavefronts; a lane keeps R_o mu~_j of its columns in
//               registers, cost(i, j) = sum_d (delta - rint delta)^2, delta = (R_o mu~)_j - x~_i; (cost_o, col_idx_o) to LDS
//       choose  the first minimum of cost_o in operation order (torch.argmin's rule)
//       write   row n = wrap(R_best mu~[col_idx[n]]), or the score of wrap(x~ - that)
// Binary64 throughout, from the binary32 inputs promoted once; binary32 outputs are rounded once.
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

constexpr int kMaxAtoms = 256;                // 4 columns per lane
constexpr int kMaxDimension = 3;
constexpr int kMaxOperations = 48;            // the cubic point group in three dimensions
constexpr int kMaxAlignWaves = 8;
constexpr int kMaxTranslation = 64;
constexpr int kRawWaves = kBlock / kWave;
constexpr int kNoColumn = 0x7fffffff;
constexpr int kBadSigma = 1, kBadCoordinate = 2;
constexpr double kTwoPi = 2.0 * kPi;

// LDS written by some lanes of this wavefront is read by others after this point
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a[j / 64] of lane j % 64, for a wave-uniform column j in [0, 64 CPL)
template <int CPL>
__device__ __forceinline__ int owned(const int (&a)[CPL], int j)
{
    int mine = a[0];
#pragma unroll
    for (int k = 1; k < CPL; ++k) mine = ((j >> 6) == k) ? a[k] : mine;
    return __shfl(mine, j & (kWave - 1), kWave);
}

// Solves min sum_i cost(i, col(i)) over the permutations of N columns.  `u` is N doubles of this wavefront's LDS.  On return
// row[k] is the row assigned to column lane + 64 k.  False (wave-uniform) when no finite step was found: the costs were not finite.
template <int CPL, class Cost>
__device__ bool lap_solve(int N, int lane, const Cost& cost, double* u, int (&row)[CPL])
{
    double v[CPL], minv[CPL];
    int way[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        v[k] = 0.0;
        row[k] = -1;
    }
    for (int i = lane; i < N; i += kWave) u[i] = 0.0;
    wave_sync();
    for (int i = 0; i < N; ++i) {
        unsigned used = 0;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            minv[k] = __builtin_huge_val();
            way[k] = -1;
        }
        int j0 = -1, i0 = i;        // column -1 is the virtual column that holds the new row i
        bool found = false;
        for (int step = 0; step < N; ++step) {
            const double ui0 = u[i0];
            double best = __builtin_huge_val();
            int best_j = kNoColumn;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int c = lane + kWave * k;
                if (c < N && !(used & (1u << k))) {
                    const double cur = cost(i0, k, c) - ui0 - v[k];
                    if (cur < minv[k]) {
                        minv[k] = cur;
                        way[k] = j0;
                    }
                    if (best_j == kNoColumn || minv[k] < best) {
                        best = minv[k];
                        best_j = c;
                    }
                }
            }
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) {
                const double other = __shfl_xor(best, o, kWave);
                const int other_j = __shfl_xor(best_j, o, kWave);
                const bool take = other < best || (other == best && other_j < best_j);
                best = take ? other : best;
                best_j = take ? other_j : best_j;
            }
            if (best_j >= N || !finite_(best)) return false;
#pragma unroll
            for (int k = 0; k < CPL; ++k) {
                const int c = lane + kWave * k;
                if (c < N) {
                    if (used & (1u << k)) {
                        if (row[k] >= 0 && row[k] < N) u[row[k]] += best;
                        v[k] -= best;
                    } else {
                        minv[k] -= best;
                    }
                    if (c == best_j) used |= 1u << k;
                }
            }
            if (lane == 0) u[i] += best;
            wave_sync();
            j0 = best_j;
            i0 = owned<CPL>(row, j0);
            if (i0 < 0) {
                found = true;
                break;
            }
        }
        if (!found) return false;
        // augment along the way chain: every column on it takes the row of its predecessor, the first one the new row
        for (int s = 0; s < N && j0 >= 0; ++s) {
            const int w = owned<CPL>(way, j0);
            const int r_w = owned<CPL>(row, w < 0 ? 0 : w);
            const int r = w < 0 ? i : r_w;
#pragma unroll
            for (int k = 0; k < CPL; ++k)
                if (lane + kWave * k == j0) row[k] = r;
            j0 = w;
        }
    }
    return true;
}

// After a solve: the row -> column map into LDS, each row's cost into u (no longer needed), and the total summed in row order.
template <int CPL, class Cost>
__device__ double lap_finish(int N, int lane, const Cost& cost, bool solved, const int (&row)[CPL], double* u, int* row_to_col)
{
    for (int r = lane; r < N; r += kWave) {
        row_to_col[r] = solved ? 0 : -1;
        u[r] = 0.0;
    }
    wave_sync();
    if (!solved) return __builtin_nan("");
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int c = lane + kWave * k;
        if (c < N && row[k] >= 0 && row[k] < N) {
            row_to_col[row[k]] = c;
            u[row[k]] = cost(row[k], k, c);
        }
    }
    wave_sync();
    double total = 0.0;
    for (int r = 0; r < N; ++r) total += u[r];
    return total;
}

template <class T>
struct MatrixCost {
    const T* matrix;
    int N;
    __device__ __forceinline__ double operator()(int i, int, int c) const { return (double)matrix[(int64_t)i * N + c]; }
};

template <int CPL>
struct GeodesicCost {
    const double* x;                          // x~ [N][D] in LDS
    double image[CPL][kMaxDimension];         // R mu~ of this lane's columns
    int D;
    __device__ __forceinline__ double operator()(int i, int k, int) const
    {
        double sum = 0.0;
#pragma unroll
        for (int d = 0; d < kMaxDimension; ++d)
            if (d < D) {
                const double delta = image[k][d] - x[i * D + d];
                const double g = delta - rint(delta);
                sum += g * g;
            }
        return sum;
    }
};

template <int CPL, class T>
__global__ __launch_bounds__(kBlock) void linear_assignment_kernel(const T* __restrict__ matrices, int64_t problems, int N,
                                                                   int32_t* __restrict__ col_idx, double* __restrict__ costs,
                                                                   uint32_t* status)
{
    __shared__ double u_all[kRawWaves * kMaxAtoms];
    __shared__ int row_to_col_all[kRawWaves * kMaxAtoms];
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int64_t m = (int64_t)blockIdx.x * kRawWaves + wave;
    if (m >= problems) return;                                   // no workgroup barrier below: a whole wavefront leaves
    double* u = u_all + wave * kMaxAtoms;
    int* row_to_col = row_to_col_all + wave * kMaxAtoms;
    const MatrixCost<T> cost{matrices + m * N * N, N};
    bool all_finite = true;
    for (int e = lane; e < N * N; e += kWave) all_finite = all_finite && finite_((double)cost.matrix[e]);
    int row[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) row[k] = -1;
    bool solved = !__any(!all_finite);
    if (solved) solved = lap_solve<CPL>(N, lane, cost, u, row);
    const double total = lap_finish<CPL>(N, lane, cost, solved, row, u, row_to_col);
    for (int r = lane; r < N; r += kWave) col_idx[m * N + r] = row_to_col[r];
    if (lane == 0) {
        costs[m] = total;
        if (!solved && status) atomicOr(status, MDX_STATUS_LAP_COST);
    }
}

template <int CPL>
__global__ __launch_bounds__(kMaxAlignWaves* kWave) void transport_align_kernel(
    const float* __restrict__ x, const float* __restrict__ mu, int64_t mu_stride, const float* __restrict__ operations, int O, int N,
    int D, const float* __restrict__ sigma, double sigma_d_square, int kmax, float* __restrict__ out,
    int32_t* __restrict__ operation_idx, int32_t* __restrict__ col_idx, double* __restrict__ costs, uint32_t* status)
{
    extern __shared__ double lds[];
    __shared__ int bad;
    const int tid = threadIdx.x, threads = blockDim.x, waves = threads / kWave, wave = tid / kWave, lane = tid % kWave;
    const int ND = N * D;
    const int64_t b = blockIdx.x;
    double* xt = lds;                                   // x~  [N][D]   (sines while the centres are made)
    double* mt = xt + ND;                               // mu~ [N][D]
    double* cosines = mt + ND;                          // [2][N][D], staging only
    double* centre = cosines + 2 * ND;                  // [2][D] in 8 slots
    double* cost_o = centre + 8;                        // [O] in 48 slots
    double* u_all = cost_o + kMaxOperations;            // [waves][N]
    int* row_to_col_all = (int*)(u_all + waves * N);    // [waves][N]
    uint8_t* cols = (uint8_t*)(row_to_col_all + waves * N);     // [O][N]: a column index fits a byte (N <= 256)
    const float* xb = x + b * ND;
    const float* mb = mu + b * mu_stride;
    float* ob = out + b * ND;

    // ---- stage
    if (tid == 0) bad = 0;
    __syncthreads();
    {
        int mine = 0;
        for (int e = tid; e < ND; e += threads) {
            const double xv = (double)xb[e], mv = (double)mb[e];
            if (!finite_(xv) || !finite_(mv)) mine |= kBadCoordinate;
            xt[e] = sin(kTwoPi * xv);
            cosines[e] = cos(kTwoPi * xv);
            mt[e] = sin(kTwoPi * mv);
            cosines[ND + e] = cos(kTwoPi * mv);
        }
        if (sigma && tid == 0 && !sigma_valid((double)sigma[b])) mine |= kBadSigma;
        if (mine) atomicOr(&bad, mine);
    }
    __syncthreads();
    if (bad != 0) {
        const float nan = __builtin_nanf("");
        for (int e = tid; e < ND; e += threads) ob[e] = nan;
        if (col_idx)
            for (int n = tid; n < N; n += threads) col_idx[b * N + n] = -1;
        if (costs)
            for (int o = tid; o < O; o += threads) costs[b * O + o] = __builtin_nan("");
        if (tid == 0) {
            if (operation_idx) operation_idx[b] = -1;
            if (status)
                atomicOr(status, ((bad & kBadSigma) ? MDX_STATUS_ANALYTICAL_SIGMA : 0u) |
                                     ((bad & kBadCoordinate) ? MDX_STATUS_ANALYTICAL_COORDINATES : 0u));
        }
        return;
    }
    if (tid < 2 * D) {
        // the atan2 centre of one dimension of x (tid < D) or mu: mean sine and cosine, summed in atom order
        const int d = tid % D;
        const double* sines = tid < D ? xt : mt;
        const double* coses = tid < D ? cosines : cosines + ND;
        double sine_sum = 0.0, cosine_sum = 0.0;
        for (int n = 0; n < N; ++n) {
            sine_sum += sines[n * D + d];
            cosine_sum += coses[n * D + d];
        }
        centre[tid] = atan2(sine_sum / (double)N, cosine_sum / (double)N) / kTwoPi;
    }
    __syncthreads();
    for (int e = tid; e < ND; e += threads) {
        const int d = e % D;
        xt[e] = wrap01((double)xb[e] - centre[d]);
        mt[e] = wrap01((double)mb[e] - centre[D + d]);
    }
    __syncthreads();

    // ---- solve
    double* u = u_all + wave * N;
    int* row_to_col = row_to_col_all + wave * N;
    for (int o = wave; o < O; o += waves) {
        GeodesicCost<CPL> cost;
        cost.x = xt;
        cost.D = D;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            const int c = lane + kWave * k;
#pragma unroll
            for (int d1 = 0; d1 < kMaxDimension; ++d1) {
                double sum = 0.0;
                if (c < N && d1 < D)
                    for (int d2 = 0; d2 < D; ++d2) sum += (double)operations[(o * D + d1) * D + d2] * mt[c * D + d2];
                cost.image[k][d1] = sum;
            }
        }
        int row[CPL];
        const bool solved = lap_solve<CPL>(N, lane, cost, u, row);
        const double total = lap_finish<CPL>(N, lane, cost, solved, row, u, row_to_col);
        if (lane == 0) cost_o[o] = total;
        for (int r = lane; r < N; r += kWave) cols[o * N + r] = (uint8_t)(solved ? row_to_col[r] : 0);
        wave_sync();
    }
    __syncthreads();

    // ---- choose: the first minimum in operation order
    int chosen = 0;
    double lowest = cost_o[0];
    for (int o = 1; o < O; ++o)
        if (cost_o[o] < lowest) {
            lowest = cost_o[o];
            chosen = o;
        }

    // ---- write
    const double s_t = sigma ? (double)sigma[b] : 0.0;
    const double s_eff = sqrt(sigma_d_square + s_t * s_t);
    for (int e = tid; e < ND; e += threads) {
        const int n = e / D, d = e % D;
        const int j = cols[chosen * N + n];
        double rotated = 0.0;
        for (int d2 = 0; d2 < D; ++d2) rotated += (double)operations[(chosen * D + d) * D + d2] * mt[j * D + d2];
        const double image = wrap01(rotated);
        if (sigma) {
            const double residual = wrap01(xt[e] - image);
            ob[e] = (float)((s_t * sigma_normalized_score(residual, s_eff, kmax)) / s_eff);
        } else {
            const float rounded = (float)image;
            ob[e] = rounded >= 1.0f ? 0.0f : rounded;       // a fraction that rounds to 1 becomes 0, as in the wrap
        }
    }
    if (col_idx)
        for (int n = tid; n < N; n += threads) col_idx[b * N + n] = cols[chosen * N + n];
    if (costs)
        for (int o = tid; o < O; o += threads) costs[b * O + o] = cost_o[o];
    if (operation_idx && tid == 0) operation_idx[b] = chosen;
}

template <class T>
void launch_linear_assignment(const T* matrices, int64_t problems, int N, int32_t* col_idx, double* costs, uint32_t* status,
                              hipStream_t stream)
{
    const dim3 grid((unsigned)cdiv(problems, kRawWaves)), block(kBlock);
    if (N <= kWave)
        hipLaunchKernelGGL((linear_assignment_kernel<1, T>), grid, block, 0, stream, matrices, problems, N, col_idx, costs, status);
    else if (N <= 2 * kWave)
        hipLaunchKernelGGL((linear_assignment_kernel<2, T>), grid, block, 0, stream, matrices, problems, N, col_idx, costs, status);
    else
        hipLaunchKernelGGL((linear_assignment_kernel<4, T>), grid, block, 0, stream, matrices, problems, N, col_idx, costs, status);
}

int launch_align(const float* x, const float* mu, int64_t mu_stride, const float* operations, int O, int64_t batch, int N, int D,
                 const float* sigma, double sigma_d_square, int kmax, float* out, int32_t* operation_idx, int32_t* col_idx,
                 double* costs, uint32_t* status, mdx_stream_t stream)
{
    if (batch < 0 || N < 1 || D < 1 || O < 1 || kmax < 0 || (mu_stride != 0 && mu_stride != (int64_t)N * D)) return MDX_ERR_INVALID_ARG;
    if (N > kMaxAtoms || D > kMaxDimension || O > kMaxOperations || kmax > kMaxTranslation || batch > 0x7fffffffLL)
        return MDX_ERR_UNSUPPORTED;
    if (batch == 0) return MDX_OK;
    if (!x || !mu || !operations || !out) return MDX_ERR_INVALID_ARG;
    const int waves = O < kMaxAlignWaves ? O : kMaxAlignWaves;
    const int ND = N * D;
    const size_t doubles = (size_t)4 * ND + 8 + kMaxOperations + (size_t)waves * N;
    const size_t bytes = doubles * sizeof(double) + (size_t)waves * N * sizeof(int) + (size_t)O * N;
    const dim3 grid((unsigned)batch), block(waves * kWave);
    const hipStream_t s = as_stream(stream);
    if (N <= kWave)
        hipLaunchKernelGGL(transport_align_kernel<1>, grid, block, bytes, s, x, mu, mu_stride, operations, O, N, D, sigma,
                           sigma_d_square, kmax, out, operation_idx, col_idx, costs, status);
    else if (N <= 2 * kWave)
        hipLaunchKernelGGL(transport_align_kernel<2>, grid, block, bytes, s, x, mu, mu_stride, operations, O, N, D, sigma,
                           sigma_d_square, kmax, out, operation_idx, col_idx, costs, status);
    else
        hipLaunchKernelGGL(transport_align_kernel<4>, grid, block, bytes, s, x, mu, mu_stride, operations, O, N, D, sigma,
                           sigma_d_square, kmax, out, operation_idx, col_idx, costs, status);
    return launch_status();
}

}  // namespace

extern "C" {

int mdx_linear_assignment(const void* cost_matrices, int costs_are_f64, int64_t problems, int n, int32_t* col_idx, double* costs,
                          uint32_t* status, mdx_stream_t stream)
{
    if (problems < 0 || n < 1) return MDX_ERR_INVALID_ARG;
    if (n > kMaxAtoms || problems > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (problems == 0) return MDX_OK;
    if (!cost_matrices || !col_idx || !costs) return MDX_ERR_INVALID_ARG;
    if (costs_are_f64)
        launch_linear_assignment((const double*)cost_matrices, problems, n, col_idx, costs, status, as_stream(stream));
    else
        launch_linear_assignment((const float*)cost_matrices, problems, n, col_idx, costs, status, as_stream(stream));
    return launch_status();
}

int mdx_transport_align(const float* x, const float* mu, int64_t mu_batch_stride, const float* point_group_operations,
                        int number_of_operations, int64_t batch, int number_of_atoms, int spatial_dimension, float* aligned_mu,
                        int32_t* operation_idx, int32_t* col_idx, double* costs, uint32_t* status, mdx_stream_t stream)
{
    return launch_align(x, mu, mu_batch_stride, point_group_operations, number_of_operations, batch, number_of_atoms,
                        spatial_dimension, nullptr, 0.0, 0, aligned_mu, operation_idx, col_idx, costs, status, stream);
}

int mdx_equivariant_analytical_score(const float* relative_coordinates, const float* sigmas,
                                     const float* equilibrium_relative_coordinates, const float* point_group_operations,
                                     int number_of_operations, double sigma_d_square, int kmax, int64_t batch, int number_of_atoms,
                                     int spatial_dimension, float* sigma_normalized_scores, uint32_t* status, mdx_stream_t stream)
{
    if (!sigmas || !(sigma_d_square > 0.0)) return MDX_ERR_INVALID_ARG;
    return launch_align(relative_coordinates, equilibrium_relative_coordinates, 0, point_group_operations, number_of_operations,
                        batch, number_of_atoms, spatial_dimension, sigmas, sigma_d_square, kmax, sigma_normalized_scores, nullptr,
                        nullptr, nullptr, status, stream);
}

}  // extern "C"
