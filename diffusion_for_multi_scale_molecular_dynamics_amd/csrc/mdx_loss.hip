// The denoising loss of a score network on a noised batch: the reference's AXLDiffusionLightningModel._generic_step
// (models/axl_diffusion_lightning_model.py:243-346) after the network's forward, with its three calculators
// (loss/coordinates_loss_calculator.py, loss/atom_type_loss_calculator.py on utils/d3pm_utils.py) and its two targets
// (score/wrapped_gaussian_score.py through mdx_wrapped_score.hpp, score/gaussian_score.py).  See include/mdx_hip.h.
//
//   denoising_loss_kernel    one workgroup per structure (64 .. 256 threads)
//       tables    the structure's three transition matrices, rows of the [T, C, C] tables at its time index (or of [B, C, C]
//                 tables at its own number), promoted into LDS: no [B, N, C, C] broadcast exists anywhere
//       X         element e = tid, tid + threads, ..: target = sigma x score of wrap(xt - x0), loss = (predicted - target)^2
//                 (x (exp(exponent (sigma - sigma0)) + 1) for weighted_mse)
//       A         atom n = tid, tid + threads, ..: softmax, clipped probabilities, the cross-entropy term, the two posteriors,
//                 the KL term (the NLL term at time index 0), all in registers (C <= 8)
//       L         thread p < P: target = -(lt - l0) / sigma_n, loss as for X
//       means     per-thread sums in the order above, the fixed xor butterfly per wavefront, the wavefronts in order by thread 0
// Binary64 throughout, from the binary32 inputs promoted once; every output value is rounded once.  No atomics in the
// arithmetic, every sum in a fixed order: a launch or a hipGraph replay always gives the same bits.  The status word alone is
// OR-ed atomically, as everywhere in this library.  64-wide wavefronts are assumed (gfx950).
//
// The consistency regularizer's target and loss (mdx_consistency_loss) are the second member of the family, further down; the
// regression regularizer's target and error (mdx_regression_loss) the third.  The fourth, mdx_denoising_loss_gradient, is
// denoising_loss_kernel<true>: the same body, which also writes d loss / d predicted_x, d loss / d logits and
// d loss / d predicted_l (the closed form is in include/mdx_hip.h) and the structures' binary64 aggregates, which
// structure_total_kernel adds in structure order for the batch's loss.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_analytical_structure.hpp"
#include "mdx_launch.hpp"
#include "mdx_reduce.hpp"
#include "mdx_wrapped_score.hpp"

using namespace mdx;

namespace {

constexpr int kMaxAtoms = MDX_LOSS_MAX_ATOMS;
constexpr int kMaxDimension = 3;
constexpr int kMaxClasses = MDX_MAX_CLASSES;
constexpr int kMaxLattice = MDX_LOSS_MAX_LATTICE_PARAMETERS;
constexpr int kMaxTranslation = 64;           // the analytical unit's limit on kmax
constexpr int kMaxWaves = kBlock / kWave;
// torch.testing.assert_close's absolute tolerance for binary32 (utils/d3pm_utils.py:144-145): in binary64 the clipped softmax
// sums to one within 1e-15 unless a logit is NaN or +inf, or every logit is -inf
constexpr double kProbabilitySumTolerance = 1.0e-5;

struct LossArgs {
    const float *x0, *xt, *target_x_in, *predicted_x, *sigma;
    int sigma_per_element;
    const int64_t *a0, *at;
    const float* logits;
    const int64_t* time_indices;
    const float *q, *q_bar, *q_bar_tm1;
    int T;
    const float *l0, *lt, *predicted_l, *sigma_n;
    float sigma_n_divisor;
    int N, D, C, P, kmax;
    int x_algorithm, l_algorithm;
    double x_sigma0, x_exponent, l_sigma0, l_exponent, ce_weight, eps, lambda_a, lambda_x, lambda_l;
    float *target_x, *target_l, *loss_x, *loss_a, *loss_l, *per_structure, *q_atm1, *p_atm1, *vb_term, *ce_term;
    uint32_t* status;
};

// what mdx_denoising_loss_gradient makes beside the forward's outputs: d loss / d prediction of
// loss = sum_b (lambda_x mean_x[b] + lambda_l mean_l[b] + lambda_a mean_a[b]) / batch_divisor, and the structures' aggregates
struct GradientOutputs {
    double batch_divisor;
    float *gradient_x, *gradient_a, *gradient_l;
    double* structure_sums;
};

// the kernel's argument: the forward instantiation takes LossArgs alone, as before
template <bool kGradient>
struct KernelArgs : LossArgs {};
template <>
struct KernelArgs<true> : LossArgs, GradientOutputs {};

// torch.clip(min=floor): a NaN stays a NaN
__device__ __forceinline__ double clip_min(double v, double floor_value) { return v < floor_value ? floor_value : v; }

// torch.xlogy(t, t): 0 at t = 0, NaN at NaN
__device__ __forceinline__ double xlogx(double t) { return t == 0.0 ? 0.0 : t * log(t); }

// (predicted - target)^2, times exp(exponent (sigma - sigma0)) + 1 for weighted_mse (loss/coordinates_loss_calculator.py:84-120)
__device__ __forceinline__ double squared_error(double predicted, double target, int algorithm, double sigma, double sigma0,
                                                double exponent)
{
    const double r = predicted - target;
    const double mse = r * r;
    return algorithm == MDX_LOSS_WEIGHTED_MSE ? mse * (exp(exponent * (sigma - sigma0)) + 1.0) : mse;
}

// d squared_error / d predicted
__device__ __forceinline__ double squared_error_gradient(double predicted, double target, int algorithm, double sigma,
                                                         double sigma0, double exponent)
{
    const double slope = 2.0 * (predicted - target);
    return algorithm == MDX_LOSS_WEIGHTED_MSE ? slope * (exp(exponent * (sigma - sigma0)) + 1.0) : slope;
}

__device__ __forceinline__ void store(float* out, int64_t i, double v)
{
    if (out) out[i] = (float)v;
}

// kGradient: the same body also writes the derivative of the batch's loss with respect to the three predictions
// (mdx_denoising_loss_gradient); every line of it stands under `if constexpr`, so the forward instantiation is the code it was
template <bool kGradient>
__global__ __launch_bounds__(kBlock) void denoising_loss_kernel(const KernelArgs<kGradient> a)
{
    __shared__ double tables[3][kMaxClasses * kMaxClasses];      // Q_t, Qbar_t, Qbar_{t-1} of this structure
    __shared__ double partial[2][kMaxWaves];
    __shared__ double lattice[kMaxLattice];
    const int tid = threadIdx.x, threads = blockDim.x, waves = threads / kWave, wave = tid / kWave, lane = tid % kWave;
    const int64_t b = blockIdx.x;
    const int N = a.N, D = a.D, C = a.C, P = a.P, ND = N * D;
    const double nan = __builtin_nan("");
    uint32_t bits = 0;

    // ---- tables: the structure's rows, once
    const bool with_tables = a.q != nullptr;
    const int64_t time_index = a.time_indices ? a.time_indices[b] : 0;
    const bool row_valid = a.T > 0 ? (time_index >= 0 && time_index < a.T) : time_index >= 0;
    if (a.a0 && with_tables) {
        if (row_valid) {
            const int64_t row = (a.T > 0 ? time_index : b) * C * C;
            for (int k = tid; k < 3 * C * C; k += threads) {
                const int which = k / (C * C), entry = k % (C * C);
                const float* table = which == 0 ? a.q : which == 1 ? a.q_bar : a.q_bar_tm1;
                tables[which][entry] = (double)table[row + entry];
            }
        } else {
            bits |= MDX_STATUS_LOSS_INDEX;
        }
    }
    __syncthreads();

    // ---- X
    double sum_x = 0.0;
    if (a.predicted_x) {
        for (int e = tid; e < ND; e += threads) {
            const int64_t i = b * ND + e;
            const double s = a.sigma ? (double)a.sigma[a.sigma_per_element ? i : b] : 0.0;
            double target;
            if (a.target_x_in) {
                target = (double)a.target_x_in[i];
            } else {
                const double x0 = (double)a.x0[i], xt = (double)a.xt[i];
                if (!sigma_valid(s)) {
                    bits |= MDX_STATUS_ANALYTICAL_SIGMA;
                    target = nan;
                } else if (!finite_(x0) || !finite_(xt)) {
                    bits |= MDX_STATUS_ANALYTICAL_COORDINATES;
                    target = nan;
                } else {
                    target = sigma_normalized_score(wrap01(xt - x0), s, a.kmax);
                }
            }
            const double loss = squared_error((double)a.predicted_x[i], target, a.x_algorithm, s, a.x_sigma0, a.x_exponent);
            store(a.target_x, i, target);
            store(a.loss_x, i, loss);
            sum_x += loss;
            if constexpr (kGradient) {
                const double scale = a.lambda_x / (a.batch_divisor * (double)ND);
                store(a.gradient_x, i,
                      scale * squared_error_gradient((double)a.predicted_x[i], target, a.x_algorithm, s, a.x_sigma0, a.x_exponent));
            }
        }
    }

    // ---- A
    double sum_a = 0.0;
    if (a.a0) {
        const double* Q = tables[0];
        const double* Qbar = tables[1];
        const double* Qbar_tm1 = tables[2];
        for (int n = tid; n < N; n += threads) {
            const int64_t atom = b * N + n, out = atom * C;
            const int64_t c0 = a.a0[atom], ct = a.at ? a.at[atom] : 0;
            const bool classes_valid = c0 >= 0 && c0 < C && ct >= 0 && ct < C;
            if (!classes_valid || (with_tables && !row_valid)) {
                bits |= MDX_STATUS_LOSS_INDEX;
                for (int c = 0; c < C; ++c) {
                    store(a.q_atm1, out + c, nan);
                    store(a.p_atm1, out + c, nan);
                    store(a.vb_term, out + c, nan);
                    store(a.ce_term, out + c, nan);
                    store(a.loss_a, out + c, nan);
                    if constexpr (kGradient) store(a.gradient_a, out + c, nan);
                }
                sum_a += nan;
                continue;
            }
            double probability[kMaxClasses], cross_entropy[kMaxClasses], variational[kMaxClasses];
#pragma unroll
            for (int c = 0; c < kMaxClasses; ++c) probability[c] = cross_entropy[c] = variational[c] = 0.0;
            // the gradient's own registers: the softmax before the clip, and d vb / d p_j (then d vb / d softmax_k)
            double softmax[kGradient ? kMaxClasses : 1], slope[kGradient ? kMaxClasses : 1], clipped_total = 1.0;
            if constexpr (kGradient) {
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) softmax[c] = slope[c] = 0.0;
            }
            if (a.logits) {
                // softmax and log_softmax with the largest logit taken out; probabilities clipped at eps and renormalised
                // (utils/d3pm_utils.py:127-150); -log_softmax with the MASK column forced to 0, kept at a_0 (:41-46 of the calculator)
                double logit[kMaxClasses], largest = -__builtin_huge_val(), total = 0.0;
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) {
                    if (c < C) {
                        logit[c] = (double)a.logits[out + c];
                        largest = logit[c] > largest ? logit[c] : largest;
                    }
                }
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) {
                    if (c < C) {
                        probability[c] = exp(logit[c] - largest);
                        total += probability[c];
                    }
                }
                const double log_total = log(total);
                double raw_sum = 0.0, clipped_sum = 0.0;
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) {
                    if (c < C) {
                        const double raw = probability[c] / total;
                        raw_sum += raw;
                        if constexpr (kGradient) softmax[c] = raw;
                        probability[c] = clip_min(raw, a.eps);
                        clipped_sum += probability[c];
                        const double nll = c == C - 1 ? 0.0 : -((logit[c] - largest) - log_total);
                        cross_entropy[c] = (c == c0 ? 1.0 : 0.0) * nll;
                    }
                }
                if (!(__builtin_fabs(raw_sum - 1.0) <= kProbabilitySumTolerance)) bits |= MDX_STATUS_LOSS_LOGITS;
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c)
                    if (c < C) probability[c] = probability[c] / clipped_sum;
                if constexpr (kGradient) clipped_total = clipped_sum;
            }
            double p_denominator_of_atom = 1.0;
            if (with_tables) {
                // P(a_{t-1} = i | a_t, gamma) = (gamma Qbar_{t-1})_i (Q_t)_{i, a_t} / (gamma Qbar_t)_{a_t}  (utils/d3pm_utils.py:105-124)
                // for gamma = the one-hot a_0 (a one-hot row times a matrix is that row: every other term is an exact zero) and for
                // gamma = the clipped probabilities
                const double q_denominator = Qbar[c0 * C + ct];
                double p_denominator = 0.0;
                if (a.logits) {
#pragma unroll
                    for (int j = 0; j < kMaxClasses; ++j)
                        if (j < C) p_denominator += probability[j] * Qbar[j * C + ct];
                    if constexpr (kGradient) p_denominator_of_atom = p_denominator;
                }
#pragma unroll
                for (int i = 0; i < kMaxClasses; ++i) {
                    if (i < C) {
                        const double step = Q[i * C + ct];
                        const double q_posterior = Qbar_tm1[c0 * C + i] * step / q_denominator;
                        store(a.q_atm1, out + i, q_posterior);
                        if (a.logits) {
                            double reached = 0.0;
#pragma unroll
                            for (int j = 0; j < kMaxClasses; ++j)
                                if (j < C) reached += probability[j] * Qbar_tm1[j * C + i];
                            const double p_posterior = reached * step / p_denominator;
                            store(a.p_atm1, out + i, p_posterior);
                            // kl_div(log p, q) = xlogy(q, q) - q log p, a target of 0 gives 0; at time index 0 the NLL of a_0
                            // (loss/atom_type_loss_calculator.py:113-124)
                            const double log_p = log(clip_min(p_posterior, a.eps));
                            variational[i] = time_index == 0 ? -log_p * (i == c0 ? 1.0 : 0.0) : xlogx(q_posterior) - q_posterior * log_p;
                            if constexpr (kGradient) {
                                // d vb / d pi_i = -q_i / pi_i, at time index 0 -delta(i, a_0) / pi_i; torch's clamp passes the
                                // gradient where pi_i >= eps and gives 0 elsewhere (a select: no 0 x inf).  Then through
                                // pi_i = step_i (sum_j p_j Qbar_tm1[j, i]) / Dn and Dn = sum_j p_j Qbar[j, a_t] to p_j, x Dn
                                const double kept = time_index == 0 ? (i == c0 ? 1.0 : 0.0) : q_posterior;
                                const double to_posterior = p_posterior >= a.eps ? -kept / p_posterior : 0.0;
#pragma unroll
                                for (int j = 0; j < kMaxClasses; ++j)
                                    if (j < C) slope[j] += to_posterior * (step * Qbar_tm1[j * C + i] - p_posterior * Qbar[j * C + ct]);
                            }
                        }
                    }
                }
            }
            if (a.logits) {
                double atom_sum = 0.0;
#pragma unroll
                for (int c = 0; c < kMaxClasses; ++c) {
                    if (c < C) {
                        const double loss = variational[c] + a.ce_weight * cross_entropy[c];
                        store(a.ce_term, out + c, cross_entropy[c]);
                        if (with_tables) {
                            store(a.vb_term, out + c, variational[c]);
                            store(a.loss_a, out + c, loss);
                            atom_sum += loss;
                        }
                    }
                }
                sum_a += atom_sum;
                if constexpr (kGradient) {
                    if (with_tables && a.gradient_a) {
                        // p = u / sum(u), u = max(softmax, eps) (the clip passes where softmax_k >= eps), then the softmax
                        double through_sum = 0.0, through_softmax = 0.0;
#pragma unroll
                        for (int j = 0; j < kMaxClasses; ++j) {
                            if (j < C) {
                                slope[j] = slope[j] / p_denominator_of_atom;
                                through_sum += slope[j] * probability[j];
                            }
                        }
#pragma unroll
                        for (int k = 0; k < kMaxClasses; ++k) {
                            if (k < C) {
                                const double to_clipped = (slope[k] - through_sum) / clipped_total;
                                slope[k] = softmax[k] >= a.eps ? to_clipped : 0.0;
                                through_softmax += softmax[k] * slope[k];
                            }
                        }
                        // the cross-entropy: ce_weight (softmax_c - delta(c, a_0)) unless a_0 is MASK, whose term is forced to 0
                        const double scale = a.lambda_a / (a.batch_divisor * (double)(N * C));
                        const double ce_weight = c0 == C - 1 ? 0.0 : a.ce_weight;
#pragma unroll
                        for (int c = 0; c < kMaxClasses; ++c) {
                            if (c < C) {
                                const double to_logit = softmax[c] * (slope[c] - through_softmax);
                                a.gradient_a[out + c] = (float)(scale * (to_logit + ce_weight * (softmax[c] - (c == c0 ? 1.0 : 0.0))));
                            }
                        }
                    }
                }
            }
        }
    }

    // ---- L
    if (a.predicted_l && tid < P) {
        const int64_t i = b * P + tid;
        const float sigma_b = a.sigma ? a.sigma[a.sigma_per_element ? b * ND : b] : 0.0f;
        const double s = (double)sigma_b;
        // without sigma_n: sigma / divisor as the reference's binary32 tensors give it (utils/noise_utils.py:29)
        const float sigma_n = a.sigma_n ? a.sigma_n[b] : sigma_b / a.sigma_n_divisor;
        const double target = -((double)a.lt[i] - (double)a.l0[i]) / (double)sigma_n;
        const double loss = squared_error((double)a.predicted_l[i], target, a.l_algorithm, s, a.l_sigma0, a.l_exponent);
        store(a.target_l, i, target);
        store(a.loss_l, i, loss);
        lattice[tid] = loss;
        if constexpr (kGradient) {
            const double scale = a.lambda_l / (a.batch_divisor * (double)P);
            store(a.gradient_l, i,
                  scale * squared_error_gradient((double)a.predicted_l[i], target, a.l_algorithm, s, a.l_sigma0, a.l_exponent));
        }
    }

    // ---- means: lanes by the butterfly, wavefronts and lattice parameters in order
    sum_x = wave_sum(sum_x);
    sum_a = wave_sum(sum_a);
    if (lane == 0) {
        partial[0][wave] = sum_x;
        partial[1][wave] = sum_a;
    }
    __syncthreads();
    bool with_means = tid == 0 && a.per_structure;
    if constexpr (kGradient) with_means = tid == 0 && (a.per_structure || a.structure_sums);
    if (with_means) {
        double total_x = 0.0, total_a = 0.0, total_l = 0.0;
        for (int w = 0; w < waves; ++w) {
            total_x += partial[0][w];
            total_a += partial[1][w];
        }
        if (a.predicted_l)
            for (int p = 0; p < P; ++p) total_l += lattice[p];
        const double mean_x = a.predicted_x ? total_x / (double)ND : 0.0;
        const double mean_a = (a.a0 && a.logits && with_tables) ? total_a / (double)(N * C) : 0.0;
        const double mean_l = a.predicted_l ? total_l / (double)P : 0.0;
        // the reference's order (models/axl_diffusion_lightning_model.py:325-338): X, then L, then A
        const double aggregate = (a.lambda_x * mean_x + a.lambda_l * mean_l) + a.lambda_a * mean_a;
        if (a.per_structure) {
            float* row = a.per_structure + b * 4;
            row[0] = (float)mean_a;
            row[1] = (float)mean_x;
            row[2] = (float)mean_l;
            row[3] = (float)aggregate;
        }
        if constexpr (kGradient) {
            if (a.structure_sums) a.structure_sums[b] = aggregate;
        }
    }
    if (bits && a.status) atomicOr(a.status, bits);
}

// ---- the consistency regularizer's target and loss (regularizers/consistency_regularizer.py:190-308; see include/mdx_hip.h)
//
//   consistency_loss_kernel     one workgroup per structure (64 .. 256 threads), element e = tid, tid + threads, ..
//       u = wrap(x_start - x_end), sigma_eff = sqrt(sigma_start^2 - sigma_end^2),
//       target = (sigma_start / sigma_eff) x [sigma_eff x score of the wrapped Gaussian at u], term = s (s - 2 target),
//       gradient = 2 (s - target) / batch; the structure's sum of terms as denoising_loss_kernel forms its means
//   structure_total_kernel      one workgroup: the binary64 sums of the structures, added in structure order by thread 0, divided
//                               by `divisor` (the batch here; the number of elements for the regression loss)
struct ConsistencyArgs {
    const float *x_start, *x_end, *score, *sigma_start, *sigma_end;
    int sigma_stride, ND, kmax;
    double batch;
    float *target, *gradient, *per_structure;
    double* structure_sums;
    uint32_t* status;
};

__global__ __launch_bounds__(kBlock) void consistency_loss_kernel(const ConsistencyArgs a)
{
    __shared__ double partial[kMaxWaves];
    const int tid = threadIdx.x, threads = blockDim.x, waves = threads / kWave, wave = tid / kWave, lane = tid % kWave;
    const int64_t b = blockIdx.x;
    const int ND = a.ND;
    const double nan = __builtin_nan("");
    uint32_t bits = 0;

    // sigma_end = 0 is the end of a trajectory that reaches time index 0: valid
    const double sigma_start = (double)a.sigma_start[b * a.sigma_stride], sigma_end = (double)a.sigma_end[b * a.sigma_stride];
    const bool sigmas_valid = sigma_valid(sigma_start) && sigma_end >= 0.0 && finite_(sigma_end) && sigma_start > sigma_end;
    const double sigma_effective = sigmas_valid ? sqrt(sigma_start * sigma_start - sigma_end * sigma_end) : nan;
    const double ratio = sigma_start / sigma_effective;
    if (!sigmas_valid) bits |= MDX_STATUS_ANALYTICAL_SIGMA;

    double sum = 0.0;
    for (int e = tid; e < ND; e += threads) {
        const int64_t i = b * ND + e;
        const double x_start = (double)a.x_start[i], x_end = (double)a.x_end[i];
        double target;
        if (!sigmas_valid) {
            target = nan;
        } else if (!finite_(x_start) || !finite_(x_end)) {
            bits |= MDX_STATUS_ANALYTICAL_COORDINATES;
            target = nan;
        } else {
            target = ratio * sigma_normalized_score(wrap01(x_start - x_end), sigma_effective, a.kmax);
        }
        store(a.target, i, target);
        if (a.score) {
            const double s = (double)a.score[i];
            store(a.gradient, i, 2.0 * (s - target) / a.batch);
            sum += s * (s - 2.0 * target);
        }
    }

    if (a.score && (a.per_structure || a.structure_sums)) {
        sum = wave_sum(sum);
        if (lane == 0) partial[wave] = sum;
        __syncthreads();
        if (tid == 0) {
            double total = 0.0;
            for (int w = 0; w < waves; ++w) total += partial[w];
            store(a.per_structure, b, total);
            if (a.structure_sums) a.structure_sums[b] = total;
        }
    }
    if (bits && a.status) atomicOr(a.status, bits);
}

// one workgroup of kBlock threads: the sums come through LDS kBlock at a time (one coalesced read, not one round trip to memory
// per structure), thread 0 adds them in structure order
__global__ __launch_bounds__(kBlock) void structure_total_kernel(const double* structure_sums, int64_t batch, double divisor,
                                                                 float* loss)
{
    __shared__ double chunk[kBlock];
    const int tid = threadIdx.x;
    double total = 0.0;
    for (int64_t base = 0; base < batch; base += kBlock) {
        if (base + tid < batch) chunk[tid] = structure_sums[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int count = batch - base < kBlock ? (int)(batch - base) : kBlock;
            for (int k = 0; k < count; ++k) total += chunk[k];
        }
        __syncthreads();
    }
    if (tid == 0) loss[0] = (float)(total / divisor);
}

// ---- the regression regularizer's target and error (regularizers/regression_regularizer.py:35-68; see include/mdx_hip.h)
//
//   regression_loss_kernel      one workgroup per structure, kBlock threads.  The target t is the analytical score network's
//       binary64 value (mdx_analytical_structure.hpp: the evaluation mdx_analytical_score rounds), or given_target promoted;
//       e = s - t with t NOT rounded first, target = (float)t, gradient = 2 e / M, the structure's sum of e^2: per-thread sums
//       in index order, then block_sum
//   structure_total_kernel      the sums in structure order, divided by M = the number of elements of the batch
struct RegressionArgs {
    const float *x, *sigma, *score, *given_target, *sites;
    double sigma_d_square, elements;
    int kmax, use_permutations, N, D, permutations;
    float *target, *gradient, *per_structure;
    double* structure_sums;
    uint32_t* status;
};

__global__ __launch_bounds__(kBlock) void regression_loss_kernel(const RegressionArgs a)
{
    __shared__ double partial[kMaxWaves];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int ND = a.N * a.D;
    const float* score = a.score ? a.score + b * ND : nullptr;
    float* target = a.target ? a.target + b * ND : nullptr;
    float* gradient = a.gradient ? a.gradient + b * ND : nullptr;
    const double elements = a.elements;
    double sum = 0.0;
    const auto element = [&](int64_t i, double t) {
        store(target, i, t);
        if (score) {
            const double e = (double)score[i] - t;
            store(gradient, i, 2.0 * e / elements);
            sum += e * e;
        }
    };
    if (a.given_target) {
        const float* given = a.given_target + b * ND;
        for (int64_t i = tid; i < ND; i += kBlock) element(i, (double)given[i]);
    } else {
        const int bad = analytical_structure(a.x + b * ND, a.sigma + b, 0, a.sites, a.sigma_d_square, a.kmax, a.use_permutations,
                                             a.N, a.D, a.permutations, nullptr, element);
        if (bad != 0) {
            const double nan = __builtin_nan("");
            for (int64_t i = tid; i < ND; i += kBlock) {
                store(target, i, nan);
                if (score) store(gradient, i, nan);
            }
            sum = nan;
            if (tid == 0 && a.status) atomicOr(a.status, analytical_status_bits(bad));
        }
    }
    if (score && (a.per_structure || a.structure_sums)) {
        const double total = block_sum(sum, partial);
        if (tid == 0) {
            store(a.per_structure, b, total);
            if (a.structure_sums) a.structure_sums[b] = total;
        }
    }
}

// mdx_denoising_loss (gradient == nullptr: the forward instantiation) and mdx_denoising_loss_gradient (gradient given, `loss`
// nullable): the checks of both, then the one launch, then the family's one-workgroup total for `loss`
int denoising_loss_entry(const float* x0, const float* xt, const float* target_x_in, const float* predicted_x, const float* sigma,
                         int sigma_per_element, const int64_t* a0, const int64_t* at, const float* logits,
                         const int64_t* time_indices, const float* q_matrices, const float* q_bar_matrices,
                         const float* q_bar_tm1_matrices, int total_time_steps, const float* l0, const float* lt,
                         const float* predicted_l, const float* sigma_n, float sigma_n_divisor, int64_t batch, int number_of_atoms,
                         int spatial_dimension, int num_classes, int number_of_lattice_parameters, int kmax, int x_algorithm,
                         double x_sigma0, double x_exponent, int l_algorithm, double l_sigma0, double l_exponent, double ce_weight,
                         double eps, double lambda_a, double lambda_x, double lambda_l, float* target_x, float* target_l,
                         float* loss_x, float* loss_a, float* loss_l, float* per_structure, float* q_atm1, float* p_atm1,
                         float* vb_term, float* ce_term, uint32_t* status, mdx_stream_t stream, const GradientOutputs* gradient,
                         float* loss)
{
    const int N = number_of_atoms, D = spatial_dimension, C = num_classes, P = number_of_lattice_parameters;
    const bool with_x = predicted_x != nullptr, with_a = a0 != nullptr, with_l = predicted_l != nullptr;
    if (batch < 0 || N < 1 || D < 1 || C < 0 || P < 0 || kmax < 0 || total_time_steps < 0) return MDX_ERR_INVALID_ARG;
    if (N > kMaxAtoms || D > kMaxDimension || C > kMaxClasses || P > kMaxLattice || kmax > kMaxTranslation ||
        batch > 0x7fffffffLL)
        return MDX_ERR_UNSUPPORTED;
    const auto algorithm_known = [](int algorithm) { return algorithm == MDX_LOSS_MSE || algorithm == MDX_LOSS_WEIGHTED_MSE; };
    if (!algorithm_known(x_algorithm) || !algorithm_known(l_algorithm)) return MDX_ERR_INVALID_ARG;
    if (!with_x && !with_a && !with_l) return MDX_ERR_INVALID_ARG;
    if (with_x) {
        if (!target_x_in && (!x0 || !xt || !sigma)) return MDX_ERR_INVALID_ARG;
        if (x_algorithm == MDX_LOSS_WEIGHTED_MSE && !sigma) return MDX_ERR_INVALID_ARG;
    } else if (target_x || loss_x) {
        return MDX_ERR_INVALID_ARG;
    }
    const bool any_table = q_matrices || q_bar_matrices || q_bar_tm1_matrices;
    if (with_a) {
        if (C < 1) return MDX_ERR_INVALID_ARG;
        if (any_table && (!q_matrices || !q_bar_matrices || !q_bar_tm1_matrices || !at || !time_indices)) return MDX_ERR_INVALID_ARG;
        if (!any_table && (!logits || q_atm1 || p_atm1 || vb_term || loss_a)) return MDX_ERR_INVALID_ARG;
        if (!logits && (p_atm1 || vb_term || ce_term || loss_a)) return MDX_ERR_INVALID_ARG;
    } else if (logits || any_table || q_atm1 || p_atm1 || vb_term || ce_term || loss_a) {
        return MDX_ERR_INVALID_ARG;
    }
    if (with_l) {
        if (P < 1 || !l0 || !lt || (!sigma_n && !(sigma && sigma_n_divisor > 0.0f))) return MDX_ERR_INVALID_ARG;
        if (l_algorithm == MDX_LOSS_WEIGHTED_MSE && !sigma) return MDX_ERR_INVALID_ARG;
    } else if (target_l || loss_l) {
        return MDX_ERR_INVALID_ARG;
    }
    if (gradient) {
        // a part that is absent has no gradient; the atom types' needs the whole chain, logits and tables
        if (!(gradient->batch_divisor > 0.0)) return MDX_ERR_INVALID_ARG;
        if (gradient->gradient_x && !with_x) return MDX_ERR_INVALID_ARG;
        if (gradient->gradient_a && !(with_a && logits && any_table)) return MDX_ERR_INVALID_ARG;
        if (gradient->gradient_l && !with_l) return MDX_ERR_INVALID_ARG;
        if (loss && !gradient->structure_sums) return MDX_ERR_INVALID_ARG;
    }
    if (batch == 0) return MDX_OK;
    KernelArgs<true> a;
    a.x0 = x0, a.xt = xt, a.target_x_in = target_x_in, a.predicted_x = predicted_x, a.sigma = sigma;
    a.sigma_per_element = sigma_per_element ? 1 : 0;
    a.a0 = a0, a.at = at, a.logits = logits, a.time_indices = time_indices;
    a.q = q_matrices, a.q_bar = q_bar_matrices, a.q_bar_tm1 = q_bar_tm1_matrices, a.T = total_time_steps;
    a.l0 = l0, a.lt = lt, a.predicted_l = predicted_l, a.sigma_n = sigma_n, a.sigma_n_divisor = sigma_n_divisor;
    a.N = N, a.D = D, a.C = C, a.P = P, a.kmax = kmax;
    a.x_algorithm = x_algorithm, a.l_algorithm = l_algorithm;
    a.x_sigma0 = x_sigma0, a.x_exponent = x_exponent, a.l_sigma0 = l_sigma0, a.l_exponent = l_exponent;
    a.ce_weight = ce_weight, a.eps = eps, a.lambda_a = lambda_a, a.lambda_x = lambda_x, a.lambda_l = lambda_l;
    a.target_x = target_x, a.target_l = target_l, a.loss_x = loss_x, a.loss_a = loss_a, a.loss_l = loss_l;
    a.per_structure = per_structure, a.q_atm1 = q_atm1, a.p_atm1 = p_atm1, a.vb_term = vb_term, a.ce_term = ce_term;
    a.status = status;
    int64_t threads = cdiv((int64_t)N * D, kWave) * kWave;
    threads = threads > kBlock ? kBlock : threads;
    if (gradient) {
        static_cast<GradientOutputs&>(a) = *gradient;
        hipLaunchKernelGGL(denoising_loss_kernel<true>, dim3((unsigned)batch), dim3((unsigned)threads), 0, as_stream(stream), a);
        if (loss)
            hipLaunchKernelGGL(structure_total_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), gradient->structure_sums,
                               batch, gradient->batch_divisor, loss);
    } else {
        KernelArgs<false> forward;
        static_cast<LossArgs&>(forward) = a;
        hipLaunchKernelGGL(denoising_loss_kernel<false>, dim3((unsigned)batch), dim3((unsigned)threads), 0, as_stream(stream),
                           forward);
    }
    return launch_status();
}

}  // namespace

extern "C" {

int mdx_denoising_loss(const float* x0, const float* xt, const float* target_x_in, const float* predicted_x, const float* sigma,
                       int sigma_per_element, const int64_t* a0, const int64_t* at, const float* logits,
                       const int64_t* time_indices, const float* q_matrices, const float* q_bar_matrices,
                       const float* q_bar_tm1_matrices, int total_time_steps, const float* l0, const float* lt,
                       const float* predicted_l, const float* sigma_n, float sigma_n_divisor, int64_t batch, int number_of_atoms,
                       int spatial_dimension,
                       int num_classes, int number_of_lattice_parameters, int kmax, int x_algorithm, double x_sigma0,
                       double x_exponent, int l_algorithm, double l_sigma0, double l_exponent, double ce_weight, double eps,
                       double lambda_a, double lambda_x, double lambda_l, float* target_x, float* target_l, float* loss_x,
                       float* loss_a, float* loss_l, float* per_structure, float* q_atm1, float* p_atm1, float* vb_term,
                       float* ce_term, uint32_t* status, mdx_stream_t stream)
{
    return denoising_loss_entry(x0, xt, target_x_in, predicted_x, sigma, sigma_per_element, a0, at, logits, time_indices, q_matrices,
                                q_bar_matrices, q_bar_tm1_matrices, total_time_steps, l0, lt, predicted_l, sigma_n, sigma_n_divisor,
                                batch, number_of_atoms, spatial_dimension, num_classes, number_of_lattice_parameters, kmax,
                                x_algorithm, x_sigma0, x_exponent, l_algorithm, l_sigma0, l_exponent, ce_weight, eps, lambda_a,
                                lambda_x, lambda_l, target_x, target_l, loss_x, loss_a, loss_l, per_structure, q_atm1, p_atm1,
                                vb_term, ce_term, status, stream, nullptr, nullptr);
}

int mdx_denoising_loss_gradient(const float* x0, const float* xt, const float* target_x_in, const float* predicted_x,
                                const float* sigma, int sigma_per_element, const int64_t* a0, const int64_t* at,
                                const float* logits, const int64_t* time_indices, const float* q_matrices,
                                const float* q_bar_matrices, const float* q_bar_tm1_matrices, int total_time_steps,
                                const float* l0, const float* lt, const float* predicted_l, const float* sigma_n,
                                float sigma_n_divisor, int64_t batch, int number_of_atoms, int spatial_dimension, int num_classes,
                                int number_of_lattice_parameters, int kmax, int x_algorithm, double x_sigma0, double x_exponent,
                                int l_algorithm, double l_sigma0, double l_exponent, double ce_weight, double eps, double lambda_a,
                                double lambda_x, double lambda_l, float* target_x, float* target_l, float* loss_x, float* loss_a,
                                float* loss_l, float* per_structure, float* q_atm1, float* p_atm1, float* vb_term, float* ce_term,
                                double batch_divisor, float* gradient_x, float* gradient_a, float* gradient_l,
                                double* structure_sums, float* loss, uint32_t* status, mdx_stream_t stream)
{
    const GradientOutputs gradient = {batch_divisor, gradient_x, gradient_a, gradient_l, structure_sums};
    return denoising_loss_entry(x0, xt, target_x_in, predicted_x, sigma, sigma_per_element, a0, at, logits, time_indices, q_matrices,
                                q_bar_matrices, q_bar_tm1_matrices, total_time_steps, l0, lt, predicted_l, sigma_n, sigma_n_divisor,
                                batch, number_of_atoms, spatial_dimension, num_classes, number_of_lattice_parameters, kmax,
                                x_algorithm, x_sigma0, x_exponent, l_algorithm, l_sigma0, l_exponent, ce_weight, eps, lambda_a,
                                lambda_x, lambda_l, target_x, target_l, loss_x, loss_a, loss_l, per_structure, q_atm1, p_atm1,
                                vb_term, ce_term, status, stream, &gradient, loss);
}

int mdx_consistency_loss(const float* x_start, const float* x_end, const float* score, const float* sigma_start,
                         const float* sigma_end, int sigma_stride, int64_t batch, int number_of_atoms, int spatial_dimension,
                         int kmax, float* target, float* gradient, float* per_structure, double* structure_sums, float* loss,
                         uint32_t* status, mdx_stream_t stream)
{
    const int N = number_of_atoms, D = spatial_dimension;
    if (batch < 0 || N < 1 || D < 1 || kmax < 0 || (sigma_stride != 0 && sigma_stride != 1)) return MDX_ERR_INVALID_ARG;
    if (N > kMaxAtoms || D > kMaxDimension || kmax > kMaxTranslation || batch > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (!x_start || !x_end || !sigma_start || !sigma_end) return MDX_ERR_INVALID_ARG;
    if (!score && (gradient || per_structure || structure_sums || loss)) return MDX_ERR_INVALID_ARG;
    if (!score && !target) return MDX_ERR_INVALID_ARG;
    if (loss && !structure_sums) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return MDX_OK;
    ConsistencyArgs a;
    a.x_start = x_start, a.x_end = x_end, a.score = score, a.sigma_start = sigma_start, a.sigma_end = sigma_end;
    a.sigma_stride = sigma_stride, a.ND = N * D, a.kmax = kmax;
    a.batch = (double)batch;
    a.target = target, a.gradient = gradient, a.per_structure = per_structure, a.structure_sums = structure_sums;
    a.status = status;
    int64_t threads = cdiv((int64_t)N * D, kWave) * kWave;
    threads = threads > kBlock ? kBlock : threads;
    hipLaunchKernelGGL(consistency_loss_kernel, dim3((unsigned)batch), dim3((unsigned)threads), 0, as_stream(stream), a);
    if (loss)
        hipLaunchKernelGGL(structure_total_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), structure_sums, batch,
                           (double)batch, loss);
    return launch_status();
}

int mdx_regression_loss(const float* relative_coordinates, const float* sigmas, const float* score, const float* given_target,
                        const float* equilibrium_relative_coordinates, double sigma_d_square, int kmax,
                        int use_permutation_invariance, int64_t batch, int number_of_atoms, int spatial_dimension, float* target,
                        float* gradient, float* per_structure, double* sums, float* loss, uint32_t* status, mdx_stream_t stream)
{
    const int N = number_of_atoms, D = spatial_dimension;
    const bool analytical = given_target == nullptr;
    if (batch < 0 || N < 1 || D < 1) return MDX_ERR_INVALID_ARG;
    if (batch > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (analytical) {
        if (kmax < 0 || !(sigma_d_square > 0.0)) return MDX_ERR_INVALID_ARG;
        if (N > kAnalyticalMaxAtoms || D > kAnalyticalMaxDimension || kmax > kAnalyticalMaxTranslation) return MDX_ERR_UNSUPPORTED;
        if (use_permutation_invariance && N > kMaxPermutedAtoms) return MDX_ERR_UNSUPPORTED;
        if (!relative_coordinates || !sigmas || !equilibrium_relative_coordinates) return MDX_ERR_INVALID_ARG;
    } else {
        if ((int64_t)N * D > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
        if (!score) return MDX_ERR_INVALID_ARG;
    }
    if (!score && (gradient || per_structure || sums || loss)) return MDX_ERR_INVALID_ARG;
    if (!score && !target) return MDX_ERR_INVALID_ARG;
    if (loss && !sums) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return MDX_OK;
    RegressionArgs a;
    a.x = relative_coordinates, a.sigma = sigmas, a.score = score, a.given_target = given_target;
    a.sites = equilibrium_relative_coordinates;
    a.sigma_d_square = sigma_d_square, a.elements = (double)batch * (double)N * (double)D;
    a.kmax = kmax, a.use_permutations = (analytical && use_permutation_invariance) ? 1 : 0, a.N = N, a.D = D;
    a.permutations = analytical ? analytical_permutations(N, use_permutation_invariance) : 1;
    a.target = target, a.gradient = gradient, a.per_structure = per_structure, a.structure_sums = sums;
    a.status = status;
    hipLaunchKernelGGL(regression_loss_kernel, dim3((unsigned)batch), dim3(kBlock), 0, as_stream(stream), a);
    if (loss) hipLaunchKernelGGL(structure_total_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), sums, batch, a.elements, loss);
    return launch_status();
}

}  // extern "C"
