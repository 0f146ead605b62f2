// The optimizer step: torch's single-tensor Adam / AdamW (amsgrad off, maximize off), which is what the reference's
// load_optimizer (models/optimizer.py:60-82) constructs, for every tensor of a parameter group in ONE launch; and the global
// 2-norm of the group's gradients that Lightning's gradient_clip_algorithm="norm" (torch's clip_grad_norm_) clips by.
// See include/mdx_hip.h.
//
//   adam_step_kernel         one workgroup of kBlock threads per chunk of MDX_ADAM_CHUNK_ELEMENTS elements of one tensor.  The
//       tables (device memory, written once by the host) name, per tensor, the addresses of p, g, exp_avg, exp_avg_sq and the
//       element count, and per workgroup the tensor it serves and its element offset in it: no launch per tensor, no
//       concatenated copy, no host read.  Thread 0 reads the hyper-parameters (binary64, device memory: a captured launch follows
//       a scheduler's learning rate), the tensor's step counter and -- with clipping -- the norm, and forms the workgroup's
//       coefficients, beta^t by pow in binary64; the chunk's loads are issued before that barrier.
//       Per element: the four operands widened to binary64, the closed form of include/mdx_hip.h with -ffp-contract=off, each
//       of p', m', v' rounded to binary32 once.  16-byte accesses where the four addresses are 16-byte aligned, dwords
//       otherwise -- the same element-to-thread map, so the same bits.
//   step counters            int32, t_old = the steps taken; ONE ENTRY PER CHUNK, at counter_slots[tensor] + offset / CHUNK, and
//       every chunk of a tensor holds the same value (a call serves all chunks of a tensor or none: a tensor without a
//       gradient is left out of a call's tables and its counters stay behind).  The rule: a workgroup reads t_old, uses
//       t = t_old + 1 and stores t: it is the only reader and the only writer of its entry, so every workgroup of a tensor
//       sees the same pre-increment value and nothing is published to another workgroup inside the launch -- no second
//       array whose parity the host would flip per call (a captured launch would freeze it), no atomic, no fence.  (One entry
//       per tensor needs its last-arriving workgroup to publish the new value behind an agent-scope release; at the
//       production-size EGNN that form ran 98 us, this one 31.5 us: profiles/r21_optimizer_step.md.)  A tensor's step is its
//       first chunk's entry.
//   gradient_squares_kernel  the same grid and element-to-thread map: per-thread sums of g^2 in element order (a binary32
//       square is exact in binary64), then block_sum's fixed tree; the chunk's partial goes to the workspace
//   norm_total_kernel        one workgroup: thread t adds the partials t, t + kBlock, .. in that order, then block_sum's fixed
//       tree (the total kernel of mdx_loss.hip with its serial sum spread over the threads); writes the norm and its square
// Every sum in a fixed order: a launch or a hipGraph replay always gives the same bits.  64-wide wavefronts (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_reduce.hpp"

using namespace mdx;

namespace {

constexpr int kChunk = MDX_ADAM_CHUNK_ELEMENTS;
constexpr int kGroups = kChunk / (4 * kBlock);      // groups of 4 consecutive elements per thread
static_assert(kChunk % (4 * kBlock) == 0, "a chunk is a whole number of 4-element groups per thread");

struct Tables {
    const uint64_t* addresses;      // [tensors, 4]: p, g, exp_avg, exp_avg_sq
    const int64_t* counts;          // [tensors]
    const int32_t* block_tensor;    // [blocks]
    const int64_t* block_offset;    // [blocks]: a multiple of kChunk
};

// what a workgroup needs to find its chunk: false when the tables name nothing for it
struct ChunkView {
    int tensor;
    int64_t offset, count;
    int n;              // elements of this chunk, 1 .. kChunk
};

__device__ __forceinline__ bool chunk_view(const Tables& t, ChunkView& c)
{
    c.tensor = t.block_tensor[blockIdx.x];
    c.offset = t.block_offset[blockIdx.x];
    c.count = t.counts[c.tensor];
    if (c.offset < 0 || c.offset >= c.count) return false;
    const int64_t left = c.count - c.offset;
    c.n = left < kChunk ? (int)left : kChunk;
    return true;
}

__device__ __forceinline__ float* tensor_pointer(const Tables& t, int tensor, int which, int64_t offset)
{
    return reinterpret_cast<float*>(t.addresses[4 * (int64_t)tensor + which]) + offset;
}

__device__ __forceinline__ bool aligned16_device(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// group j of thread tid holds the chunk's elements base .. base + 3, base = (j kBlock + tid) 4: consecutive lanes, consecutive
// 16 bytes.  Elements at or beyond n are not touched (they read as 0).
__device__ __forceinline__ void load_group(const float* src, int base, int n, bool vector, float (&out)[4])
{
    if (vector && base + 4 <= n) {
        const float4 w = *reinterpret_cast<const float4*>(src + base);
        out[0] = w.x, out[1] = w.y, out[2] = w.z, out[3] = w.w;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) out[c] = base + c < n ? src[base + c] : 0.0f;
    }
}

__device__ __forceinline__ void store_group(float* dst, int base, int n, bool vector, const float (&in)[4])
{
    if (vector && base + 4 <= n) {
        *reinterpret_cast<float4*>(dst + base) = make_float4(in[0], in[1], in[2], in[3]);
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (base + c < n) dst[base + c] = in[c];
    }
}

// the workgroup's coefficients, formed once by thread 0
struct Coefficients {
    double gradient_factor;     // gradient_scale x clip
    double weight_decay;
    double keep;                // AdamW: 1 - lr weight_decay
    double one_minus_beta1, beta2, one_minus_beta2;
    double step_size;           // lr / (1 - beta1^t)
    double root_correction2;    // sqrt(1 - beta2^t)
    double eps;
};

struct AdamArgs {
    Tables tables;
    const int32_t* slots;           // [tensors]: the entry of `steps` of each tensor's first chunk
    int32_t* steps;
    const double* hyper;
    const double* norm;
    int decoupled, zero_gradients;
    uint32_t* status;
};

__global__ __launch_bounds__(kBlock) void adam_step_kernel(const AdamArgs a)
{
    __shared__ Coefficients shared;
    ChunkView chunk;
    if (!chunk_view(a.tables, chunk)) return;
    const int tid = threadIdx.x, n = chunk.n;
    float* p = tensor_pointer(a.tables, chunk.tensor, 0, chunk.offset);
    float* g = tensor_pointer(a.tables, chunk.tensor, 1, chunk.offset);
    float* m = tensor_pointer(a.tables, chunk.tensor, 2, chunk.offset);
    float* v = tensor_pointer(a.tables, chunk.tensor, 3, chunk.offset);
    const bool vector = aligned16_device(p) && aligned16_device(g) && aligned16_device(m) && aligned16_device(v);

    float pw[kGroups][4], gw[kGroups][4], mw[kGroups][4], vw[kGroups][4];
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const int base = (j * kBlock + tid) * 4;
        load_group(p, base, n, vector, pw[j]);
        load_group(g, base, n, vector, gw[j]);
        load_group(m, base, n, vector, mw[j]);
        load_group(v, base, n, vector, vw[j]);
    }

    if (tid == 0) {
        const double lr = a.hyper[MDX_ADAM_HYPER_LR], beta1 = a.hyper[MDX_ADAM_HYPER_BETA1], beta2 = a.hyper[MDX_ADAM_HYPER_BETA2];
        const double weight_decay = a.hyper[MDX_ADAM_HYPER_WEIGHT_DECAY];
        // this chunk's own counter: no other workgroup reads or writes it
        int32_t* counter = a.steps + a.slots[chunk.tensor] + (int32_t)(chunk.offset / kChunk);
        const int32_t t_old = *counter;
        *counter = t_old + 1;
        const double t = (double)t_old + 1.0;
        double clip = 1.0;
        if (a.norm) {           // torch's clip_grad_norm_: max_norm / (norm + 1e-6), clamped at 1
            const double ratio = a.hyper[MDX_ADAM_HYPER_MAX_NORM] / (a.norm[0] + 1.0e-6);
            clip = ratio > 1.0 ? 1.0 : ratio;       // a NaN ratio stays NaN, as torch.clamp keeps it
        }
        shared.gradient_factor = a.hyper[MDX_ADAM_HYPER_GRADIENT_SCALE] * clip;
        shared.weight_decay = weight_decay;
        shared.keep = 1.0 - lr * weight_decay;
        shared.one_minus_beta1 = 1.0 - beta1;
        shared.beta2 = beta2;
        shared.one_minus_beta2 = 1.0 - beta2;
        shared.step_size = lr / (1.0 - pow(beta1, t));
        shared.root_correction2 = sqrt(1.0 - pow(beta2, t));
        shared.eps = a.hyper[MDX_ADAM_HYPER_EPS];
    }
    __syncthreads();
    const Coefficients c = shared;

    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double p0 = (double)pw[j][e], m0 = (double)mw[j][e], v0 = (double)vw[j][e];
            double gradient = c.gradient_factor * (double)gw[j][e];
            if (!(__builtin_fabs(gradient) < __builtin_huge_val())) bits |= MDX_STATUS_OPTIMIZER_NONFINITE;
            double q;
            if (a.decoupled) {
                q = p0 * c.keep;
            } else {
                gradient = gradient + c.weight_decay * p0;
                q = p0;
            }
            const double m1 = m0 + (gradient - m0) * c.one_minus_beta1;
            const double v1 = c.beta2 * v0 + c.one_minus_beta2 * gradient * gradient;
            const double denominator = sqrt(v1) / c.root_correction2 + c.eps;
            const double p1 = q - c.step_size * m1 / denominator;
            pw[j][e] = (float)p1;
            mw[j][e] = (float)m1;
            vw[j][e] = (float)v1;
            gw[j][e] = 0.0f;
        }
    }
    // (the elements beyond n were computed on zeros and are not stored; their gradient 0 sets no bit)
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const int base = (j * kBlock + tid) * 4;
        store_group(p, base, n, vector, pw[j]);
        store_group(m, base, n, vector, mw[j]);
        store_group(v, base, n, vector, vw[j]);
        if (a.zero_gradients) store_group(g, base, n, vector, gw[j]);
    }
    if (bits && a.status) atomicOr(a.status, bits);
}

__global__ __launch_bounds__(kBlock) void gradient_squares_kernel(const Tables tables, double* partials)
{
    __shared__ double scratch[kBlock / kWave];
    ChunkView chunk;
    const bool served = chunk_view(tables, chunk);       // uniform over the workgroup
    double sum = 0.0;
    if (served) {
        const float* g = tensor_pointer(tables, chunk.tensor, 1, chunk.offset);
        const bool vector = aligned16_device(g);
#pragma unroll
        for (int j = 0; j < kGroups; ++j) {
            float w[4];
            load_group(g, (j * kBlock + (int)threadIdx.x) * 4, chunk.n, vector, w);
#pragma unroll
            for (int e = 0; e < 4; ++e) sum += (double)w[e] * (double)w[e];
        }
    }
    const double total = block_sum(sum, scratch);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// one workgroup: thread t adds the partials t, t + kBlock, .. in that order, then the fixed tree of block_sum
__global__ __launch_bounds__(kBlock) void norm_total_kernel(const double* partials, int64_t blocks, double* norm)
{
    __shared__ double scratch[kBlock / kWave];
    double sum = 0.0;
    for (int64_t k = threadIdx.x; k < blocks; k += kBlock) sum += partials[k];
    const double total = block_sum(sum, scratch);
    if (threadIdx.x == 0) {
        norm[0] = sqrt(total);
        norm[1] = total;
    }
}

struct HyperValues {
    double v[MDX_ADAM_HYPER_COUNT];
};

__global__ void hyper_fill_kernel(const HyperValues values, double* hyper)
{
    if (threadIdx.x < MDX_ADAM_HYPER_COUNT) hyper[threadIdx.x] = values.v[threadIdx.x];
}

bool tables_given(const uint64_t* addresses, const int64_t* counts, const int32_t* block_tensor, const int64_t* block_offset)
{
    return addresses && counts && block_tensor && block_offset;
}

}  // namespace

extern "C" {

int mdx_adam_hyper_fill(double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                        double gradient_scale, double* hyper, mdx_stream_t stream)
{
    if (!hyper) return MDX_ERR_INVALID_ARG;
    HyperValues values = {};
    values.v[MDX_ADAM_HYPER_LR] = lr, values.v[MDX_ADAM_HYPER_BETA1] = beta1, values.v[MDX_ADAM_HYPER_BETA2] = beta2;
    values.v[MDX_ADAM_HYPER_EPS] = eps, values.v[MDX_ADAM_HYPER_WEIGHT_DECAY] = weight_decay;
    values.v[MDX_ADAM_HYPER_MAX_NORM] = max_norm, values.v[MDX_ADAM_HYPER_GRADIENT_SCALE] = gradient_scale;
    hipLaunchKernelGGL(hyper_fill_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), values, hyper);
    return launch_status();
}

int mdx_gradient_norm(const uint64_t* addresses, const int64_t* counts, const int32_t* block_tensor, const int64_t* block_offset,
                      int64_t number_of_blocks, double* partials, double* norm, mdx_stream_t stream)
{
    if (number_of_blocks < 0 || !norm) return MDX_ERR_INVALID_ARG;
    if (number_of_blocks > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (number_of_blocks > 0 && (!tables_given(addresses, counts, block_tensor, block_offset) || !partials)) return MDX_ERR_INVALID_ARG;
    const Tables tables = {addresses, counts, block_tensor, block_offset};
    if (number_of_blocks > 0)
        hipLaunchKernelGGL(gradient_squares_kernel, dim3((unsigned)number_of_blocks), dim3(kBlock), 0, as_stream(stream), tables,
                           partials);
    hipLaunchKernelGGL(norm_total_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), partials, number_of_blocks, norm);
    return launch_status();
}

int mdx_adam_step(const uint64_t* addresses, const int64_t* counts, const int32_t* counter_slots, const int32_t* block_tensor,
                  const int64_t* block_offset, int64_t number_of_blocks, int32_t* steps, const double* hyper, const double* norm,
                  int decoupled_weight_decay, int zero_gradients, uint32_t* status, mdx_stream_t stream)
{
    if (number_of_blocks < 0) return MDX_ERR_INVALID_ARG;
    if (number_of_blocks > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (number_of_blocks == 0) return MDX_OK;
    if (!tables_given(addresses, counts, block_tensor, block_offset) || !counter_slots || !steps || !hyper)
        return MDX_ERR_INVALID_ARG;
    AdamArgs a;
    a.tables = {addresses, counts, block_tensor, block_offset};
    a.slots = counter_slots, a.steps = steps, a.hyper = hyper, a.norm = norm;
    a.decoupled = decoupled_weight_decay ? 1 : 0, a.zero_gradients = zero_gradients ? 1 : 0;
    a.status = status;
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)number_of_blocks), dim3(kBlock), 0, as_stream(stream), a);
    return launch_status();
}

}  // extern "C"
