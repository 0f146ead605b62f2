// Training the MLP score network: the forward that keeps what a backward needs, and the gradient of every parameter.
// See include/mdx_hip.h (mdx_mlp_train_forward, mdx_mlp_train_backward) for the record's layout and the contract.
//
// The parameters are the module's own tensors in nn.Linear layout ([out, in], float32), read through a device table of
// addresses (weight, bias per layer; the order of the header).  Nothing is packed: an optimizer step changes the values in place
// and the next launch reads the new ones.
//
//   mlp_train_forward_kernel   four wavefronts per workgroup, one structure each, activations in the wavefront's two LDS vectors.
//       A layer's weights are staged by the whole workgroup TRANSPOSED into LDS, Wt[i][o] with an odd row length: the global
//       read runs along a row of W (coalesced), the LDS store of 64 consecutive i lands in 64 different banks, and the layer
//       loop's read Wt[k][lane] is consecutive.  A row's sum is mdx_mlp_forward's: fused multiply-adds into four partial sums
//       by k mod 4, ((s0 + s1) + (s2 + s3)) + bias; SiLU is the same hardware form.  Every value fed to a Linear, and the
//       pre-activation of every layer that goes through SiLU, is stored to the record as it is computed.
//   mlp_train_chain_kernel     one workgroup per slab of MDX_MLP_TRAIN_STRUCTURES_PER_SLAB consecutive structures.  First each
//       wavefront runs the per-structure chain of its structures in binary64, lanes over the INPUT index i of
//       delta_in[i] = sum_o W[o, i] delta[o] (a row of W per o: coalesced), o in index order, and leaves every layer's delta in
//       LDS.  After one barrier every thread owns gradient elements e = tid, tid + 256, ... of each tensor and adds
//       delta_b[o] a_b[i] over the slab's structures in index order (for the atom-type embedding: structures, then atoms), a
//       read from the binary32 record widened to binary64; the sum goes to the workgroup's slab of the workspace.
//   mlp_train_reduce_kernel    one thread per gradient element: the slabs in slab order, x scale, + the old value when
//       accumulating, all in binary64, ONE rounding to binary32.
// No atomics, no ticket: the same bits on every launch and under graph replay.  64-wide wavefronts (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_math.hpp"

using namespace mdx;

namespace {

constexpr int kWaves = 4;                                   // wavefronts (= structures) per workgroup of the forward
constexpr int kSlab = MDX_MLP_TRAIN_STRUCTURES_PER_SLAB;
constexpr int kMaxLinears = 5 + MDX_MLP_MAX_HIDDEN + 3;
constexpr size_t kLdsDefault = 64 * 1024;                   // default dynamic-LDS limit per workgroup
constexpr size_t kLdsLimit = 128 * 1024;                    // what mdx_mlp_forward allows itself

// linear layers in table order: the table holds (weight, bias) of layer k at entries 2 k, 2 k + 1
enum { kCoordinates = 0, kNoise = 1, kTime = 2, kAtomType = 3, kLattice = 4, kHidden0 = 5 };

struct Shape {
    int N, d, C, H, NH, ec, en, et, ea, el;
    int nd, nl, F0, NO, NC;
    // the record, in floats from a structure's start
    int r_circle, r_sigma, r_time, r_classes, r_lattice, r_features, r_hidden, r_z, R;
    int linears;
    __host__ __device__ int heads() const { return kHidden0 + NH; }
};

// the shape words checked, the derived sizes and the record's layout; every product below stays far inside an int
int checked_shape(const int32_t* v, Shape& s)
{
    if (!v) return MDX_ERR_INVALID_ARG;
    for (int k = 0; k < MDX_MLP_TRAIN_SHAPE_COUNT; ++k)
        if (v[k] < 1) return MDX_ERR_INVALID_ARG;
    s.N = v[0], s.d = v[1], s.C = v[2], s.H = v[3], s.NH = v[4];
    s.ec = v[5], s.en = v[6], s.et = v[7], s.ea = v[8], s.el = v[9];
    if (s.d > 3 || s.NH > MDX_MLP_MAX_HIDDEN || s.C > MDX_MAX_CLASSES) return MDX_ERR_UNSUPPORTED;
    for (int k = 0; k < MDX_MLP_TRAIN_SHAPE_COUNT; ++k)
        if (v[k] > 4096) return MDX_ERR_UNSUPPORTED;
    s.nd = s.N * s.d, s.nl = s.d * (s.d + 1) / 2, s.NC = s.N * s.C;
    s.F0 = s.ec + s.en + s.et + s.N * s.ea + s.el, s.NO = s.NC + s.nd + s.nl;
    int t = 0;
    s.r_circle = t, t += 2 * s.nd;
    s.r_sigma = t, t += 1;
    s.r_time = t, t += 1;
    s.r_classes = t, t += s.N;
    s.r_lattice = t, t += s.nl;
    s.r_features = t, t += s.F0;
    s.r_hidden = t, t += s.NH * s.H;     // input of hidden layer k at r_hidden + (k - 1) H, k = 1 .. NH - 1; of the heads at k = NH
    s.r_z = t, t += (s.NH - 1) * s.H;    // z_k at r_z + k H, k = 0 .. NH - 2
    s.R = t;
    s.linears = kHidden0 + s.NH + 3;
    return MDX_OK;
}

// per layer: rows, columns, where its delta sits in a structure's LDS vector, where its input sits in the record, and where its
// weight and bias gradients sit in the flat buffer
struct Layers {
    int out[kMaxLinears], in[kMaxLinears], delta[kMaxLinears], input[kMaxLinears];
    int64_t weight[kMaxLinears], bias[kMaxLinears];
    int stride;                          // doubles of LDS per structure: [heads NO | hidden NH H | features F0]
    int64_t P;
};

Layers make_layers(const Shape& s)
{
    Layers y = {};
    const int d_hidden = s.NO, d_features = s.NO + s.NH * s.H;
    y.stride = d_features + s.F0;
    auto set = [&y](int k, int out, int in, int delta, int input) { y.out[k] = out, y.in[k] = in, y.delta[k] = delta, y.input[k] = input; };
    set(kCoordinates, s.ec, 2 * s.nd, d_features, s.r_circle);
    set(kNoise, s.en, 1, d_features + s.ec, s.r_sigma);
    set(kTime, s.et, 1, d_features + s.ec + s.en, s.r_time);
    set(kAtomType, s.ea, s.C, d_features + s.ec + s.en + s.et, s.r_classes);
    set(kLattice, s.el, s.nl, d_features + s.ec + s.en + s.et + s.N * s.ea, s.r_lattice);
    for (int k = 0; k < s.NH; ++k)
        set(kHidden0 + k, s.H, k ? s.H : s.F0, d_hidden + k * s.H, k ? s.r_hidden + (k - 1) * s.H : s.r_features);
    const int last = s.r_hidden + (s.NH - 1) * s.H;
    set(s.heads() + 0, s.NC, s.H, 0, last);
    set(s.heads() + 1, s.nd, s.H, s.NC, last);
    set(s.heads() + 2, s.nl, s.H, s.NC + s.nd, last);
    int64_t t = 0;
    for (int k = 0; k < s.linears; ++k) {
        y.weight[k] = t, t += (int64_t)y.out[k] * y.in[k];
        y.bias[k] = t, t += y.out[k];
    }
    y.P = t;
    return y;
}

__device__ __forceinline__ const float* tensor(const uint64_t* table, int entry)
{
    return reinterpret_cast<const float*>(table[entry]);
}

__device__ __forceinline__ float silu_(float a) { return __fdividef(a, 1.0f + __expf(-a)); }

// W [out, in] of global memory into Wt[i * ldw + col0 + o], by the whole workgroup
__device__ __forceinline__ void stage_transposed(float* wt, int ldw, int col0, const float* W, int out, int in)
{
    const int n = out * in;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        const int o = e / in, i = e - o * in;
        wt[i * ldw + col0 + o] = W[e];
    }
}

// sum_k Wt[k][j] v[k] as mdx_mlp_forward adds it: four partial sums by k mod 4, fused multiply-adds, ((s0 + s1) + (s2 + s3))
__device__ __forceinline__ float row_sum(const float* wt, int ldw, int j, const float* v, int n)
{
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    const float* w = wt + j;
    int k = 0;
#pragma unroll 4
    for (; k + 4 <= n; k += 4) {
        s0 = __builtin_fmaf(w[(k + 0) * ldw], v[k + 0], s0);
        s1 = __builtin_fmaf(w[(k + 1) * ldw], v[k + 1], s1);
        s2 = __builtin_fmaf(w[(k + 2) * ldw], v[k + 2], s2);
        s3 = __builtin_fmaf(w[(k + 3) * ldw], v[k + 3], s3);
    }
    if (k < n) s0 = __builtin_fmaf(w[k * ldw], v[k], s0);
    if (k + 1 < n) s1 = __builtin_fmaf(w[(k + 1) * ldw], v[k + 1], s1);
    if (k + 2 < n) s2 = __builtin_fmaf(w[(k + 2) * ldw], v[k + 2], s2);
    return (s0 + s1) + (s2 + s3);
}

struct ForwardArgs {
    Shape s;
    const uint64_t* table;
    const int64_t* a;
    const float *x, *l, *time, *sigma;
    int64_t B;
    float *logits, *score_x, *score_l, *record;
    int weight_floats, vector_floats;
};

__global__ __launch_bounds__(kWaves* kWave) void mlp_train_forward_kernel(const ForwardArgs p)
{
    extern __shared__ float lds[];
    const Shape& s = p.s;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    float* wt = lds;
    float* buf_a = lds + p.weight_floats + wave * 2 * p.vector_floats;
    float* buf_b = buf_a + p.vector_floats;
    const int64_t b = (int64_t)blockIdx.x * kWaves + wave;
    const bool live = b < p.B;                       // a wavefront beyond the batch stages and waits, and touches no structure
    float* rec = p.record + (live ? b : 0) * s.R;

    // (cos 2 pi x | sin 2 pi x), all cosines first; the scalars, the classes and the lattice as the layers read them
    int ldw = s.ec | 1;
    stage_transposed(wt, ldw, 0, tensor(p.table, 2 * kCoordinates), s.ec, 2 * s.nd);
    float sigma = 0.0f, time = 0.0f;
    if (live) {
        const float* x = p.x + b * s.nd;
        for (int e = lane; e < s.nd; e += kWave) {
            float sn, cs;
            sincospif_(2.0f * x[e], sn, cs);
            buf_a[e] = cs, buf_a[s.nd + e] = sn;
            rec[s.r_circle + e] = cs, rec[s.r_circle + s.nd + e] = sn;
        }
        sigma = p.sigma[b], time = p.time[b];
        if (lane == 0) rec[s.r_sigma] = sigma, rec[s.r_time] = time;
        for (int n = lane; n < s.N; n += kWave) {
            const int64_t given = p.a[b * s.N + n];
            rec[s.r_classes + n] = (float)(given < 0 ? 0 : (given >= s.C ? s.C - 1 : given));      // never an index outside W
        }
        for (int k = lane; k < s.nl; k += kWave) rec[s.r_lattice + k] = p.l[b * s.nl + k];
    }
    __syncthreads();
    if (live) {
        int o = 0;
        const float* bc = tensor(p.table, 2 * kCoordinates + 1);
        for (int j = lane; j < s.ec; j += kWave) buf_b[j] = row_sum(wt, ldw, j, buf_a, 2 * s.nd) + bc[j];
        o += s.ec;
        const float *wn = tensor(p.table, 2 * kNoise), *bn = tensor(p.table, 2 * kNoise + 1);
        for (int j = lane; j < s.en; j += kWave) buf_b[o + j] = __builtin_fmaf(wn[j], sigma, bn[j]);
        o += s.en;
        const float *wtm = tensor(p.table, 2 * kTime), *btm = tensor(p.table, 2 * kTime + 1);
        for (int j = lane; j < s.et; j += kWave) buf_b[o + j] = __builtin_fmaf(wtm[j], time, btm[j]);
        o += s.et;
        const float *wa = tensor(p.table, 2 * kAtomType), *ba = tensor(p.table, 2 * kAtomType + 1);
        for (int t = lane; t < s.N * s.ea; t += kWave) {             // Linear(one_hot(a)) = W[:, a] + b
            const int n = t / s.ea, e = t - n * s.ea;
            const int64_t given = p.a[b * s.N + n];
            const int cls = (int)(given < 0 ? 0 : (given >= s.C ? s.C - 1 : given));
            buf_b[o + t] = wa[e * s.C + cls] + ba[e];
        }
        o += s.N * s.ea;
        const float *wl = tensor(p.table, 2 * kLattice), *bl = tensor(p.table, 2 * kLattice + 1);
        const float* l = p.l + b * s.nl;
        for (int j = lane; j < s.el; j += kWave) {
            float acc = bl[j];
            for (int k = 0; k < s.nl; ++k) acc = __builtin_fmaf(wl[j * s.nl + k], l[k], acc);
            buf_b[o + j] = acc;
        }
    }
    __syncthreads();
    if (live)
        for (int i = lane; i < s.F0; i += kWave) rec[s.r_features + i] = buf_b[i];

    // hidden stack: SiLU between layers, none after the last
    float* in = buf_b;
    float* out = buf_a;
    int in_dim = s.F0;
    ldw = s.H | 1;
    for (int k = 0; k < s.NH; ++k) {
        stage_transposed(wt, ldw, 0, tensor(p.table, 2 * (kHidden0 + k)), s.H, in_dim);
        __syncthreads();
        if (live) {
            const float* bias = tensor(p.table, 2 * (kHidden0 + k) + 1);
            for (int j = lane; j < s.H; j += kWave) {
                float z = row_sum(wt, ldw, j, in, in_dim) + bias[j];
                if (k + 1 < s.NH) {
                    rec[s.r_z + k * s.H + j] = z;
                    z = silu_(z);
                }
                out[j] = z;
                rec[s.r_hidden + k * s.H + j] = z;                  // the input of layer k + 1, or of the heads
            }
        }
        __syncthreads();
        float* t = in; in = out; out = t;
        in_dim = s.H;
    }

    // the three heads as one staged matrix: columns logits | score_x | score_l; raw outputs (no -inf on MASK)
    ldw = s.NO | 1;
    const int h0 = s.heads();
    stage_transposed(wt, ldw, 0, tensor(p.table, 2 * h0), s.NC, s.H);
    stage_transposed(wt, ldw, s.NC, tensor(p.table, 2 * (h0 + 1)), s.nd, s.H);
    stage_transposed(wt, ldw, s.NC + s.nd, tensor(p.table, 2 * (h0 + 2)), s.nl, s.H);
    __syncthreads();
    if (live) {
        const float *ba = tensor(p.table, 2 * h0 + 1), *bx = tensor(p.table, 2 * (h0 + 1) + 1), *bl = tensor(p.table, 2 * (h0 + 2) + 1);
        for (int j = lane; j < s.NO; j += kWave) {
            const float acc = row_sum(wt, ldw, j, in, s.H);
            if (j < s.NC) p.logits[b * s.NC + j] = acc + ba[j];
            else if (j < s.NC + s.nd) p.score_x[b * s.nd + (j - s.NC)] = acc + bx[j - s.NC];
            else p.score_l[b * s.nl + (j - s.NC - s.nd)] = acc + bl[j - s.NC - s.nd];
        }
    }
}

// LDS exchanges between the lanes of ONE wavefront need no s_barrier (a wave's LDS operations execute in issue order); this
// only stops the compiler from moving memory operations across the hand-off.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct BackwardArgs {
    Shape s;
    Layers y;
    const uint64_t* table;
    const float *record, *grad_logits, *grad_x, *grad_l;
    int64_t B;
    double* slabs;
};

// delta_in[i] = sum_o W[o, i] delta[o], o in index order, for this lane's i
__device__ __forceinline__ double transposed_row(const float* W, int out, int in, int i, const double* delta)
{
    double acc = 0.0;
    for (int o = 0; o < out; ++o) acc += (double)W[(int64_t)o * in + i] * delta[o];
    return acc;
}

__global__ __launch_bounds__(kBlock) void mlp_train_chain_kernel(const BackwardArgs p)
{
    extern __shared__ double deltas[];
    const Shape& s = p.s;
    const Layers& y = p.y;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    const int64_t first = (int64_t)blockIdx.x * kSlab;
    if (first >= p.B) return;                                       // (uniform; the grid is ceil(B / kSlab))
    const int count = p.B - first < kSlab ? (int)(p.B - first) : kSlab;
    const int h0 = s.heads();

    for (int q = wave; q < count; q += kBlock / kWave) {
        const int64_t b = first + q;
        double* D = deltas + q * y.stride;
        const float* rec = p.record + b * s.R;
        for (int j = lane; j < s.NO; j += kWave) {
            float g = 0.0f;
            if (j < s.NC) { if (p.grad_logits) g = p.grad_logits[b * s.NC + j]; }
            else if (j < s.NC + s.nd) { if (p.grad_x) g = p.grad_x[b * s.nd + (j - s.NC)]; }
            else if (p.grad_l) g = p.grad_l[b * s.nl + (j - s.NC - s.nd)];
            D[j] = (double)g;
        }
        wave_sync();
        // through the heads: no activation follows the last hidden layer, so this is the delta of its output
        double* Dk = D + y.delta[kHidden0 + s.NH - 1];
        for (int i = lane; i < s.H; i += kWave) {
            double acc = 0.0;
            for (int h = 0; h < 3; ++h) {
                const float* W = tensor(p.table, 2 * (h0 + h));
                const double* Dh = D + y.delta[h0 + h];
                for (int o = 0; o < y.out[h0 + h]; ++o) acc += (double)W[(int64_t)o * s.H + i] * Dh[o];
            }
            Dk[i] = acc;
        }
        wave_sync();
        for (int k = s.NH - 1; k >= 1; --k) {
            const float* W = tensor(p.table, 2 * (kHidden0 + k));
            const float* z = rec + s.r_z + (k - 1) * s.H;
            const double* Dout = D + y.delta[kHidden0 + k];
            double* Din = D + y.delta[kHidden0 + k - 1];
            for (int i = lane; i < s.H; i += kWave) {
                const double acc = transposed_row(W, s.H, s.H, i, Dout);
                const double zz = (double)z[i];
                const double sg = 1.0 / (1.0 + exp(-zz));
                Din[i] = acc * (sg * (1.0 + zz * (1.0 - sg)));      // silu'(z)
            }
            wave_sync();
        }
        {   // through hidden layer 0 into the concatenated features: the deltas of the five embedding layers' outputs
            const float* W = tensor(p.table, 2 * kHidden0);
            const double* Dout = D + y.delta[kHidden0];
            double* Din = D + y.delta[kCoordinates];
            for (int i = lane; i < s.F0; i += kWave) Din[i] = transposed_row(W, s.H, s.F0, i, Dout);
        }
    }
    __syncthreads();

    // the batch contraction of this slab: every element owned by one thread, structures in index order
    double* slab = p.slabs + (int64_t)blockIdx.x * y.P;
    const float* record = p.record + first * s.R;
    for (int k = 0; k < s.linears; ++k) {
        const int out = y.out[k], in = y.in[k], delta = y.delta[k], input = y.input[k];
        if (k == kAtomType) {
            // one weight over the N atoms: dW[e, c] = sum_b sum_n delta_b[n ea + e] one_hot(a_b[n])[c], db[e] = sum_b sum_n delta
            for (int e = tid; e < out * in; e += kBlock) {
                const int q = e / in, c = e - q * in;
                double acc = 0.0;
                for (int b = 0; b < count; ++b)
                    for (int n = 0; n < s.N; ++n)
                        acc += deltas[b * y.stride + delta + n * s.ea + q] * (record[(int64_t)b * s.R + input + n] == (float)c ? 1.0 : 0.0);
                slab[y.weight[k] + e] = acc;
            }
            for (int q = tid; q < out; q += kBlock) {
                double acc = 0.0;
                for (int b = 0; b < count; ++b)
                    for (int n = 0; n < s.N; ++n) acc += deltas[b * y.stride + delta + n * s.ea + q];
                slab[y.bias[k] + q] = acc;
            }
            continue;
        }
        for (int e = tid; e < out * in; e += kBlock) {
            const int o = e / in, i = e - o * in;
            double acc = 0.0;
            for (int b = 0; b < count; ++b) acc += deltas[b * y.stride + delta + o] * (double)record[(int64_t)b * s.R + input + i];
            slab[y.weight[k] + e] = acc;
        }
        for (int o = tid; o < out; o += kBlock) {
            double acc = 0.0;
            for (int b = 0; b < count; ++b) acc += deltas[b * y.stride + delta + o];
            slab[y.bias[k] + o] = acc;
        }
    }
}

__global__ __launch_bounds__(kBlock) void mlp_train_reduce_kernel(const double* slabs, int64_t number_of_slabs, int64_t P,
                                                                  double scale, int accumulate, float* gradients)
{
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < P; e += (int64_t)gridDim.x * kBlock) {
        double sum = 0.0;
        for (int64_t q = 0; q < number_of_slabs; ++q) sum += slabs[q * P + e];
        double value = sum * scale;
        if (accumulate) value += (double)gradients[e];
        gradients[e] = (float)value;
    }
}

}  // namespace

extern "C" {

int64_t mdx_mlp_train_record_floats(const int32_t* shape_host)
{
    Shape s;
    return checked_shape(shape_host, s) == MDX_OK ? s.R : -1;
}

int64_t mdx_mlp_train_parameter_count(const int32_t* shape_host)
{
    Shape s;
    return checked_shape(shape_host, s) == MDX_OK ? make_layers(s).P : -1;
}

int64_t mdx_mlp_train_workspace_doubles(const int32_t* shape_host, int64_t batch)
{
    Shape s;
    if (checked_shape(shape_host, s) != MDX_OK || batch < 0) return -1;
    return cdiv(batch, kSlab) * make_layers(s).P;
}

int mdx_mlp_train_forward(const int32_t* shape_host, const uint64_t* addresses, const int64_t* atom_types, const float* x,
                          const float* l, const float* time, const float* sigma, int64_t batch, float* logits_out,
                          float* score_x_out, float* score_l_out, float* record_out, mdx_stream_t stream)
{
    ForwardArgs p;
    const int ok = checked_shape(shape_host, p.s);
    if (ok != MDX_OK) return ok;
    if (batch < 0) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return MDX_OK;
    if (!addresses || !atom_types || !x || !l || !time || !sigma || !logits_out || !score_x_out || !score_l_out || !record_out)
        return MDX_ERR_INVALID_ARG;
    const Shape& s = p.s;
    auto staged = [](int64_t in, int64_t out) { return in * (out | 1); };
    int64_t weights = staged(2 * s.nd, s.ec);
    if (staged(s.F0, s.H) > weights) weights = staged(s.F0, s.H);
    if (staged(s.H, s.H) > weights) weights = staged(s.H, s.H);
    if (staged(s.H, s.NO) > weights) weights = staged(s.H, s.NO);
    int64_t widest = 2 * s.nd;
    if (s.F0 > widest) widest = s.F0;
    if (s.H > widest) widest = s.H;
    if (s.NO > widest) widest = s.NO;
    weights = (weights + 3) & ~(int64_t)3, widest = (widest + 3) & ~(int64_t)3;
    const int64_t bytes = 4 * (weights + 2 * kWaves * widest);
    if (bytes > (int64_t)kLdsLimit) return MDX_ERR_UNSUPPORTED;
    const int64_t blocks = cdiv(batch, kWaves);
    if (blocks > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (bytes > (int64_t)kLdsDefault &&
        hipFuncSetAttribute((const void*)mlp_train_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return MDX_ERR_HIP;
    p.table = addresses, p.a = atom_types, p.x = x, p.l = l, p.time = time, p.sigma = sigma, p.B = batch;
    p.logits = logits_out, p.score_x = score_x_out, p.score_l = score_l_out, p.record = record_out;
    p.weight_floats = (int)weights, p.vector_floats = (int)widest;
    hipLaunchKernelGGL(mlp_train_forward_kernel, dim3((unsigned)blocks), dim3(kWaves * kWave), (size_t)bytes, as_stream(stream), p);
    return launch_status();
}

int mdx_mlp_train_backward(const int32_t* shape_host, const uint64_t* addresses, const float* record, const float* grad_logits,
                           const float* grad_x, const float* grad_l, int64_t batch, double* workspace, int accumulate,
                           double scale, float* gradients_inout, mdx_stream_t stream)
{
    BackwardArgs p;
    const int ok = checked_shape(shape_host, p.s);
    if (ok != MDX_OK) return ok;
    if (batch < 0 || !gradients_inout) return MDX_ERR_INVALID_ARG;
    if (batch > 0 && (!addresses || !record || !workspace)) return MDX_ERR_INVALID_ARG;
    p.y = make_layers(p.s);
    const int64_t slabs = cdiv(batch, kSlab);
    if (slabs > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    const int64_t bytes = 8 * (int64_t)kSlab * p.y.stride;
    if (bytes > (int64_t)kLdsLimit) return MDX_ERR_UNSUPPORTED;
    if (slabs > 0) {
        if (bytes > (int64_t)kLdsDefault &&
            hipFuncSetAttribute((const void*)mlp_train_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
            return MDX_ERR_HIP;
        p.table = addresses, p.record = record, p.grad_logits = grad_logits, p.grad_x = grad_x, p.grad_l = grad_l;
        p.B = batch, p.slabs = workspace;
        hipLaunchKernelGGL(mlp_train_chain_kernel, dim3((unsigned)slabs), dim3(kBlock), (size_t)bytes, as_stream(stream), p);
    }
    hipLaunchKernelGGL(mlp_train_reduce_kernel, dim3(flat_grid(p.y.P)), dim3(kBlock), 0, as_stream(stream), workspace, slabs, p.y.P,
                       scale, accumulate ? 1 : 0, gradients_inout);
    return launch_status();
}

}  // extern "C"
