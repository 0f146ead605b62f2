// HIP kernel (gfx950 / CDNA4) + C ABI of the training side's batch noising: the gather of a batch's dataset rows, the draw of a time
// index per structure, the schedule rows there and the three forward noisers (F1, F2, F3 of mdx_noisers.hpp) in ONE launch.
// See include/mdx_hip.h for the contract.
//
// Kernel inventory
//   noise_training_batch_kernel    one lane per (structure, atom) and one more per structure for what a structure has once
//                                  (time, sigma, the three [C, C] rows, the lattice parameters); flat and grid-strided
// The production shapes are tiny (512 x 8 x 3): the launch and the dependent reads row -> time index -> table row are what it
// costs, so every lane resolves its own row and index (a few cached words) and nothing is exchanged between lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_math.hpp"
#include "mdx_noisers.hpp"

using namespace mdx;

namespace {

struct NoiseBatchArgs {
    int T, C;
    const float *time, *sigma, *q, *qbar, *qbar_tm1;
    const float* x0;
    const int64_t* a0;
    const float* l0;
    int64_t M;
    const int64_t* rows;
    int64_t n_positions, row_offset;
    const int32_t* d_cursor;
    const int64_t* time_indices_in;
    const float *z, *u, *z_lat;
    mdx_rng_t rng;
    int64_t B;
    int N, d, nl;
    float root;
    int fixed_lattice;
    float* x0_out;
    int64_t* a0_out;
    float* l0_out;
    int64_t* time_indices_out;
    float *time_out, *sigma_out, *xt_out;
    int64_t* at_out;
    float *lt_out, *q_out, *qbar_out, *qbar_tm1_out;
    uint32_t* status;
};

__global__ __launch_bounds__(kBlock) void noise_training_batch_kernel(NoiseBatchArgs p)
{
    const int N = p.N, d = p.d, C = p.C, nl = p.nl;
    const uint32_t k0 = (uint32_t)p.rng.seed, k1 = (uint32_t)(p.rng.seed >> 32);
    const uint32_t call8 = rng_call(p.rng) << 8;
    const uint32_t draw = p.rng.draw_offset;
    const int64_t first = p.row_offset + (int64_t)(p.d_cursor ? *p.d_cursor : 0) * p.B;
    const int64_t total = p.B * (N + 1);
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / (N + 1);
        const int n = (int)(t - b * (N + 1));
        bool bad = false;
        // the dataset row: position -> (rows) -> r, each clamped into its range so that nothing is read out of bounds
        int64_t position = first + b;
        if (position < 0 || position >= p.n_positions) { bad = true; position = position < 0 ? 0 : p.n_positions - 1; }
        int64_t r = p.rows ? p.rows[position] : position;
        if (r < 0 || r >= p.M) { bad = true; r = r < 0 ? 0 : p.M - 1; }
        // the time index: as given, or the high word of (one Philox word x T)
        int64_t index;
        if (p.time_indices_in) {
            index = p.time_indices_in[b];
            if (index < 0 || index >= p.T) { bad = true; index = index < 0 ? 0 : p.T - 1; }
        } else {
            const uint32_t w = philox4x32_10((uint32_t)r, call8, draw, MDX_TAG_TRAIN_TIME_INDEX, k0, k1).v[0];
            index = (int64_t)(((uint64_t)w * (uint64_t)p.T) >> 32);
        }
        const float sigma = p.sigma[index];
        if (n < N) {                                   // one atom: F1 and F2
            const int64_t in = r * N + n, out = b * N + n;
            float zz[4];
            if (!p.z) {
                const u32x4 g = philox4x32_10((uint32_t)in, call8, draw, MDX_TAG_TRAIN_Z, k0, k1);
                box_muller(g.v[0], g.v[1], zz[0], zz[1]);
                if (d > 2) box_muller(g.v[2], g.v[3], zz[2], zz[3]);
            }
            for (int c = 0; c < d; ++c) {
                const float x0 = p.x0[in * d + c];
                if (p.x0_out) p.x0_out[out * d + c] = x0;
                if (p.xt_out) p.xt_out[out * d + c] = noised_relative_coordinate(x0, sigma, p.z ? p.z[out * d + c] : zz[c]);
            }
            const int64_t a0 = p.a0[in];
            if (p.a0_out) p.a0_out[out] = a0;
            if (a0 < 0 || a0 >= C - 1) bad = true;
            if (p.at_out) {
                float uu[MDX_MAX_CLASSES];
                if (p.u) {
                    for (int c = 0; c < C; ++c) uu[c] = p.u[out * C + c];
                } else {
                    for (int sub = 0; sub * 4 < C; ++sub) {
                        const u32x4 g = philox4x32_10((uint32_t)in, call8 | (uint32_t)sub, draw, MDX_TAG_TRAIN_U, k0, k1);
                        for (int l = 0; l < 4 && sub * 4 + l < C; ++l) uu[sub * 4 + l] = u01(g.v[l]);
                    }
                }
                const int row = a0 < 0 ? 0 : a0 > C - 1 ? C - 1 : (int)a0;
                p.at_out[out] = noised_atom_type(row, p.qbar + index * C * C, C, uu, true);
            }
        } else {                                       // once per structure: the schedule rows and F3
            if (p.time_indices_out) p.time_indices_out[b] = index;
            if (p.time_out) p.time_out[b] = p.time[index];
            if (p.sigma_out) p.sigma_out[b] = sigma;
            for (int e = 0; e < C * C; ++e) {
                if (p.q_out) p.q_out[b * C * C + e] = p.q[index * C * C + e];
                if (p.qbar_out) p.qbar_out[b * C * C + e] = p.qbar[index * C * C + e];
                if (p.qbar_tm1_out) p.qbar_tm1_out[b * C * C + e] = p.qbar_tm1[index * C * C + e];
            }
            const float sigma_n = sigma / p.root;
            const bool noised = p.lt_out && !p.fixed_lattice;
            float zl[8];                               // nl <= 6: two Philox calls at the most, every index a constant
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                if (!noised || p.z_lat || sub * 4 >= nl) continue;
                const u32x4 g = philox4x32_10((uint32_t)r, call8 | (uint32_t)sub, draw, MDX_TAG_TRAIN_LATTICE, k0, k1);
                box_muller(g.v[0], g.v[1], zl[sub * 4], zl[sub * 4 + 1]);
                box_muller(g.v[2], g.v[3], zl[sub * 4 + 2], zl[sub * 4 + 3]);
            }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                if (k >= nl) continue;
                const float l0 = p.l0[r * nl + k];
                if (p.l0_out) p.l0_out[b * nl + k] = l0;
                if (!p.lt_out) continue;
                if (p.fixed_lattice) { p.lt_out[b * nl + k] = l0; continue; }
                p.lt_out[b * nl + k] = noised_lattice_parameter(sigma_n, p.z_lat ? p.z_lat[b * nl + k] : zl[k], l0);
            }
        }
        if (bad && p.status) atomicOr(p.status, MDX_STATUS_NOISING_INDEX);
    }
}

}  // namespace

int mdx_noise_training_batch(const mdx_schedule_t* sched_host, const float* x0, const int64_t* a0, const float* l0,
                             int64_t dataset_size, const int64_t* rows, int64_t rows_count, int64_t row_offset,
                             const int32_t* d_cursor, const int64_t* time_indices_in, const float* z, const float* u,
                             const float* z_lattice, mdx_rng_t rng, int64_t batch, int number_of_atoms, int spatial_dimension,
                             float root, int use_fixed_lattice_parameters, float* x0_out, int64_t* a0_out, float* l0_out,
                             int64_t* time_indices_out, float* time_out, float* sigma_out, float* xt_out, int64_t* at_out,
                             float* lt_out, float* q_out, float* q_bar_out, float* q_bar_tm1_out, uint32_t* status,
                             mdx_stream_t stream)
{
    if (!sched_host || batch < 0 || dataset_size < 1 || number_of_atoms < 1 || spatial_dimension < 1) return MDX_ERR_INVALID_ARG;
    if (spatial_dimension > 3) return MDX_ERR_UNSUPPORTED;
    const int T = sched_host->total_time_steps, C = sched_host->num_classes;
    if (T < 1 || C < 2 || !(root > 0.0f)) return MDX_ERR_INVALID_ARG;
    if (C > MDX_MAX_CLASSES) return MDX_ERR_UNSUPPORTED;
    if (dataset_size > 0xffffffffLL / number_of_atoms) return MDX_ERR_INVALID_ARG;   // M N >= 2^32: the 32-bit Philox item
    if (batch > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (rows && rows_count < 1) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return MDX_OK;
    if (!x0 || !a0 || !l0 || !sched_host->time || !sched_host->sigma || !sched_host->q_matrix || !sched_host->q_bar_matrix ||
        !sched_host->q_bar_tm1_matrix)
        return MDX_ERR_INVALID_ARG;
    NoiseBatchArgs p;
    p.T = T; p.C = C;
    p.time = sched_host->time; p.sigma = sched_host->sigma;
    p.q = sched_host->q_matrix; p.qbar = sched_host->q_bar_matrix; p.qbar_tm1 = sched_host->q_bar_tm1_matrix;
    p.x0 = x0; p.a0 = a0; p.l0 = l0;
    p.M = dataset_size;
    p.rows = rows;
    p.n_positions = rows ? rows_count : dataset_size;
    p.row_offset = row_offset;
    p.d_cursor = d_cursor;
    p.time_indices_in = time_indices_in;
    p.z = z; p.u = u; p.z_lat = z_lattice;
    p.rng = rng;
    p.B = batch;
    p.N = number_of_atoms; p.d = spatial_dimension; p.nl = spatial_dimension * (spatial_dimension + 1) / 2;
    p.root = root;
    p.fixed_lattice = use_fixed_lattice_parameters;
    p.x0_out = x0_out; p.a0_out = a0_out; p.l0_out = l0_out;
    p.time_indices_out = time_indices_out; p.time_out = time_out; p.sigma_out = sigma_out;
    p.xt_out = xt_out; p.at_out = at_out; p.lt_out = lt_out;
    p.q_out = q_out; p.qbar_out = q_bar_out; p.qbar_tm1_out = q_bar_tm1_out;
    p.status = status;
    hipLaunchKernelGGL(noise_training_batch_kernel, dim3(flat_grid(batch * (number_of_atoms + 1))), dim3(kBlock), 0,
                       as_stream(stream), p);
    return launch_status();
}
