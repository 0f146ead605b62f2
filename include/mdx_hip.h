/*
 * mdx_hip.h -- C ABI of the MI355X (gfx950) sampling hot path.
 *
 * Drop-in boundary for the per-step work of the reference's predictor-corrector sampler
 * (mila-iqia/diffusion_for_multi_scale_molecular_dynamics).  The reference is pure PyTorch and has no FFI of
 * its own; every entry point below names the reference function (file:line, relative to
 * src/diffusion_for_multi_scale_molecular_dynamics/) whose arithmetic it replaces, and INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add at that call site.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless its name ends in _host.
 *   - the caller (PyTorch) owns every buffer; the library never allocates, frees or retains a pointer.
 *   - stateless, re-entrant, stream-ordered: work is enqueued on `stream` (a hipStream_t passed as void*),
 *     no hidden synchronisation, no globals.  Safe to capture into a hipGraph.
 *   - return value: MDX_OK or a negative status; no exceptions or aborts cross the ABI.  Conditions the
 *     reference checks with device-side asserts (cutoff too large, MASK left at the last step) are reported
 *     through an optional device status word (`status`, OR-ed bits below) that the host reads when it chooses.
 *   - layouts: A int64 [B,N]; X float32 [B,N,d]; L float32 [B,d(d+1)/2]; logits float32 [B,N,C];
 *     C = num_atom_types + 1, class C-1 is MASK.  All arrays C-contiguous.
 *   - arithmetic: IEEE binary32 in the exact operation order documented in DESIGN.md ("MDX arithmetic");
 *     integer outputs are bit-identical to oracle/mdx_oracle.c on identical inputs.
 */
#ifndef MDX_HIP_H
#define MDX_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDX_ABI_VERSION 14

/* status codes */
#define MDX_OK 0
#define MDX_ERR_INVALID_ARG (-1)
#define MDX_ERR_UNSUPPORTED (-2)
#define MDX_ERR_HIP (-3)

/* bits of the optional device status word */
#define MDX_STATUS_CUTOFF_TOO_LARGE 1u   /* utils/neighbors.py:107-113 assert               */
#define MDX_STATUS_MASK_AT_LAST_STEP 2u  /* generators/langevin_generator.py:616-620 assert */
#define MDX_STATUS_EGNN_F16_RANGE 4u     /* mdx_egnn_edge_chain, split-f16 mode: an activation left the f16 range     */
#define MDX_STATUS_GRAPH_CAPACITY 8u     /* mdx_radius_graph_fill_capped: more edges than the caller's capacity      */
#define MDX_STATUS_EGNN_TABLE 16u        /* mdx_egnn_table_check / _gather: the first layer's distance table does not
                                            stand in for the per-edge chain (interpolation error, sigma not uniform,
                                            a distance or class outside the table) -- recompute on the per-edge chain */
#define MDX_STATUS_SW_NEIGHBOURS 32u     /* mdx_stillinger_weber_energy_forces: an atom has more neighbours than the
                                            caller's neighbour capacity (its structure's results are NaN, not truncated) */
#define MDX_STATUS_SW_ATOM_TYPE 64u      /* mdx_stillinger_weber_energy_forces: an atom type outside the parameter table
                                            (MASK included); its structure's results are NaN                           */
#define MDX_STATUS_ANALYTICAL_SIGMA 128u /* mdx_analytical_score and the wrapped-Gaussian functions: a sigma that is not a
                                            finite positive number (score/wrapped_gaussian_score.py:155 assert); the
                                            structure's (element's) results are NaN                                     */
#define MDX_STATUS_ANALYTICAL_COORDINATES 256u /* the same functions: a relative coordinate outside [0, 1) or not finite
                                            (score/wrapped_gaussian_score.py:156-159 assert); results NaN likewise      */

#define MDX_STATUS_EXCISE_CAPACITY 512u  /* mdx_excise_environments: an environment holds more atoms than the caller's capacity
                                            (its count is the true one; the first `capacity` slots are written)        */
#define MDX_STATUS_EXCISE_OUTSIDE_BOX 1024u /* the same function: an embedded atom lies outside (0, L_new)
                                            (active_learning_loop/sample_maker/base_sample_maker.py:278-283 assert)    */
#define MDX_STATUS_EXCISE_CENTRAL_INDEX 2048u /* the same function: a central atom index outside [0, number_of_atoms);
                                            that environment comes out empty                                           */
#define MDX_STATUS_RANDOM_FILL_COUNT 4096u /* mdx_random_fill_environments: an environment holds more constrained atoms than
                                            the sample has atoms (active_learning_loop/sample_maker/
                                            excise_and_random_sample_maker.py:305-308 assert); its samples come out zero     */
#define MDX_STATUS_RANDOM_FILL_ENVIRONMENT 8192u /* the same function: a sample names an environment outside [0, E), or the
                                            environment's active atom is not one of its constrained atoms; zero likewise  */
#define MDX_STATUS_LAP_COST 16384u       /* mdx_linear_assignment: a cost that is not finite (|c| >= 1e300 included); that
                                            problem's col_idx is -1 and its cost NaN                                        */
#define MDX_STATUS_TRANSLATION_NO_CANDIDATE 32768u /* mdx_optimal_translation: no plateau holds its own solution (the minimum sits
                                            on the boundary tau = +-1/2); that entry's tau and squared distance are +inf   */

#define MDX_STATUS_LOSS_LOGITS 65536u     /* mdx_denoising_loss: the softmax of an atom's logits does not sum to one (a NaN or
                                            +inf logit, or every logit -inf: utils/d3pm_utils.py:144-145 assert); that atom's
                                            atom-type results are NaN                                                       */
#define MDX_STATUS_LOSS_INDEX 131072u    /* the same function: a time index outside [0, T) or an atom type outside [0, C); the
                                            structure's (atom's) atom-type results are NaN and no table entry is read       */
#define MDX_STATUS_KS_NAN 262144u        /* mdx_sort_keys: a NaN among the values (scipy's nan_policy='propagate': the
                                            Kolmogorov-Smirnov distance of such a sample is NaN); the output is unspecified  */
#define MDX_STATUS_OPTIMIZER_NONFINITE 524288u /* mdx_adam_step: a scaled, clipped gradient that is not finite; the arithmetic
                                            goes on as torch's does (the NaN propagates into the parameter and its state)    */
#define MDX_STATUS_NOISING_INDEX 1048576u /* mdx_noise_training_batch: a batch position or a dataset row outside its range, a given
                                            time index outside [0, T), or an atom type outside [0, C - 1) (MASK included); the
                                            index is clamped into its range before it is used, so nothing is read out of bounds */

#define MDX_MAX_CLASSES 8      /* C supported by the fused atom-type kernels */
#define MDX_PREDICTOR 0
#define MDX_CORRECTOR 1

/* tags of the device-RNG specification ("Device RNG") */
#define MDX_TAG_COORD 0
#define MDX_TAG_GUMBEL 1
#define MDX_TAG_LATTICE 2
#define MDX_TAG_INIT 3
#define MDX_TAG_REPAINT_X0 4
#define MDX_TAG_BINARY 5
#define MDX_TAG_REPAINT_Z 6
#define MDX_TAG_REPAINT_U 7
#define MDX_TAG_INIT_LATTICE 8
#define MDX_TAG_RESAMPLE_Z 9
#define MDX_TAG_RESAMPLE_U 10
#define MDX_TAG_FILL_UNIFORM 11
#define MDX_TAG_FILL_TYPE 12
#define MDX_TAG_FILL_VOXEL 13
#define MDX_TAG_TRAIN_TIME_INDEX 14
#define MDX_TAG_TRAIN_Z 15
#define MDX_TAG_TRAIN_U 16
#define MDX_TAG_TRAIN_LATTICE 17

#if defined(__GNUC__)
#define MDX_API __attribute__((visibility("default")))
#else
#define MDX_API
#endif

typedef void* mdx_stream_t;

/* Device-resident schedule tables (S1), uploaded/built once per generator.
 * Mirrors the Noise / LangevinDynamics namedtuples of noise_schedulers/noise_scheduler.py:348-378. */
typedef struct mdx_schedule {
    int32_t total_time_steps;       /* T */
    int32_t num_classes;            /* C */
    double sigma_min;               /* NoiseParameters.sigma_min as the Python double it is */
    const float* time;              /* [T] */
    const float* sigma;             /* [T] */
    const float* g;                 /* [T] */
    const float* g_squared;         /* [T] */
    const float* epsilon;           /* [T] */
    const float* q_matrix;          /* [T,C,C] */
    const float* q_bar_matrix;      /* [T,C,C] */
    const float* q_bar_tm1_matrix;  /* [T,C,C] */
} mdx_schedule_t;

/* Counter-based RNG request: used only where the corresponding pre-drawn noise pointer is NULL.
 * value(item, k) comes from Philox4x32-10 with key = seed and
 * counter = (item, (call << 8) | k/4, draw, tag); draw = index * draw_stride + draw_offset.
 * item and k: per-atom draws (MDX_TAG_COORD, _GUMBEL, _BINARY) take item = b N + atom and k = the dimension / class; the lattice
 * draw (MDX_TAG_LATTICE) takes item = the structure b and k = the lattice parameter, i.e. z_lattice [B, nl] is what
 * mdx_rng_fill(kind 1, seed, call, draw, MDX_TAG_LATTICE, B, nl) writes.  index is the step's time index: a predictor from
 * index i draws with draw = i * draw_stride, its corrector m with (i - 1) * draw_stride + 1 + m. */
typedef struct mdx_rng {
    uint64_t seed;
    uint32_t call;          /* index of the sample() call (sub-batch) */
    uint32_t draw_stride;   /* number_of_corrector_steps + 1 */
    uint32_t draw_offset;   /* 0 predictor, 1+m for corrector m */
    uint32_t reserved;      /* 0 */
    const uint32_t* call_dev;   /* nullable: device word that holds the call index instead of `call` -- a launch captured into a
                                   hipGraph then serves every later sample() call of the same shape (the word is rewritten
                                   between replays, like the step index) */
} mdx_rng_t;

/* Per-step flags of PredictorCorrectorSamplingParameters (generators/predictor_corrector_axl_generator.py:22-30). */
typedef struct mdx_pc_flags {
    int32_t atom_type_greedy_sampling;
    int32_t one_atom_type_transition_per_step;
    int32_t use_fixed_lattice_parameters;
    int32_t update_atom_types;      /* predictor: 1; corrector: atom_type_transition_in_corrector */
    float small_epsilon;
} mdx_pc_flags_t;

MDX_API int mdx_abi_version(void);
MDX_API const char* mdx_status_string(int status);

/* S1 -- NoiseScheduler.__init__ (noise_schedulers/noise_scheduler.py:112-267; sigma_calculator.py:72-74,102-104).
 * schedule_type 0 = exponential, 1 = linear.  Outputs: 9 vectors [T] and 3 tensors [T,C,C]. */
MDX_API int mdx_noise_schedule_build(int total_time_steps, int schedule_type, double time_delta, double sigma_min,
                             double sigma_max, double corrector_step_epsilon, int num_classes, float* time,
                             float* sigma, float* sigma_squared, float* g, float* g_squared, float* epsilon,
                             float* sqrt_2_epsilon, float* beta, float* alpha_bar, float* q_matrix,
                             float* q_bar_matrix, float* q_bar_tm1_matrix, mdx_stream_t stream);

/* Step index kept on the device so that one captured graph serves every iteration. */
MDX_API int mdx_index_set(int32_t* d_index, int32_t value, mdx_stream_t stream);
MDX_API int mdx_index_add(int32_t* d_index, int32_t delta, mdx_stream_t stream);

/* Score-network inputs TIME / NOISE as [B,1] tensors -- LangevinGenerator._get_model_predictions
 * (generators/langevin_generator.py:140-143) with the scalars of predictor_step (:559-563) or
 * corrector_step (:719-729).  index = d_index ? *d_index + index_i : index_i. */
MDX_API int mdx_fill_time_sigma(const mdx_schedule_t* sched_host, int mode, int index_i, const int32_t* d_index,
                        float* time_out, float* sigma_out, int64_t batch, mdx_stream_t stream);

/* P1 -- LangevinGenerator._relative_coordinates_update (generators/langevin_generator.py:155-201) +
 * map_relative_coordinates_to_unit_cell (utils/basis_transformations.py:95-119):
 * out = wrap((x + (score_weight*s)/sigma) + noise_weight*z), elementwise over `count` floats. */
MDX_API int mdx_relative_coordinates_update(const float* x, const float* sigma_normalized_scores, const float* z,
                                    float score_weight, float gaussian_noise_weight, float sigma, int64_t count,
                                    float* out, mdx_stream_t stream);

/* P3 -- LangevinGenerator._lattice_parameters_update (generators/langevin_generator.py:485-490). */
MDX_API int mdx_lattice_parameters_update(const float* l, const float* sigma_normalized_scores, const float* z,
                                  float score_weight, float gaussian_noise_weight, float sigma_n, int64_t count,
                                  float* out, mdx_stream_t stream);

/* P1 / P3 with the three scalars read on the device: weights = {score_weight, gaussian_noise_weight, sigma (sigma_n)}.
 * AdaptiveCorrectorGenerator (generators/adaptive_corrector.py:97-148): its step size eps_i is a batch statistic of the
 * scores and the noise -- computed on the device and never read by the host. */
MDX_API int mdx_relative_coordinates_update_dev(const float* x, const float* sigma_normalized_scores, const float* z,
                                        const float* weights, int64_t count, float* out, mdx_stream_t stream);
MDX_API int mdx_lattice_parameters_update_dev(const float* l, const float* sigma_normalized_scores, const float* z,
                                      const float* weights, int64_t count, float* out, mdx_stream_t stream);

/* P2 -- LangevinGenerator._atom_types_update (generators/langevin_generator.py:247-439) with
 * get_probability_at_previous_time_step / get_probability_from_logits (utils/d3pm_utils.py:64-150).
 * q, q_bar, q_bar_tm1: [C,C] of the current step.  gumbel [B,N,C]; u [B,N] (read only if greedy).
 * probabilities_out (nullable) [B,N,C]: the transition probabilities after the greedy adjustment. */
MDX_API int mdx_atom_types_update(const float* logits, const int64_t* atom_types, const float* q, const float* q_bar,
                          const float* q_bar_tm1, const float* gumbel, const float* u, int64_t batch,
                          int number_of_atoms, int num_classes, float small_epsilon, int greedy,
                          int one_transition, int64_t* atom_types_out, float* probabilities_out,
                          mdx_stream_t stream);

/* Fused per-step update: P2 + P1 + P3 of LangevinGenerator.predictor_step (:536-645) or P1 + P3 (+P2) of
 * corrector_step (:693-805) in ONE launch, scalars taken from the device-resident tables.
 * Pre-drawn noise (reference-RNG parity mode): z_coordinates [B,N,d], gumbel [B,N,C], u [B,N], z_lattice [B,nl];
 * any NULL pointer switches that draw to the device RNG (rng).  Outputs may alias inputs.
 * status (nullable): MDX_STATUS_MASK_AT_LAST_STEP is OR-ed in when index 1 leaves a MASK.
 * logits == NULL with ONE atom type (num_classes == 2): every atom's logits are (0, -inf) -- what the update makes of any
 * (finite, -inf), the only logits a score network can return there (the MASK logit is forced to -inf, and the clipped softmax
 * of (l0, -inf) does not depend on a finite l0).  With more classes: MDX_ERR_INVALID_ARG. */
MDX_API int mdx_pc_step_update(const mdx_schedule_t* sched_host, int mode, int index_i, const int32_t* d_index,
                       const mdx_pc_flags_t* flags_host, const int64_t* atom_types, const float* x, const float* l,
                       const float* logits, const float* score_x, const float* score_l, const float* z_coordinates,
                       const float* gumbel, const float* u, const float* z_lattice, mdx_rng_t rng, int64_t batch,
                       int number_of_atoms, int spatial_dimension, int64_t* atom_types_out, float* x_out,
                       float* l_out, uint32_t* status, mdx_stream_t stream);

/* AdaptiveCorrectorGenerator (generators/adaptive_corrector.py:41-63,97-148) in three stream-ordered stages with no host read;
 * index = d_index ? *d_index + index_i : index_i as everywhere, the corrector's index rules (sigma_min at index 0).
 *
 * Stage 1, batch statistics of ONE corrector step (:125-136).  Per structure, on mdx_pc_step_update's lane mapping and with a
 * fixed-order cross-lane sum: |s_X[b]| over atoms x space, sum over atoms of |z_X[b, atom]| (torch.linalg.norm(z, dim=-1)) and,
 * with a free lattice, |s_L[b]| and |z_L[b]| -- binary32, correctly rounded sqrt -- stored to workspace [batch, 4] (floats).
 * z_coordinates [B,N,d] / z_lattice_for_step_size [B,nl]: pre-drawn noise; NULL regenerates mdx_pc_step_update's draw of the
 * same rng request in registers (same bits as mdx_rng_fill).  A second launch of ONE workgroup then sums the workspace in
 * binary64 in a fixed order (no atomics: two calls on the same inputs give the same bits) into
 *   totals[8] (doubles) = {sum|s_X|, B, sum|z_X|, B N, sum|s_L|, B, sum|z_L|, B}
 * -- sums and counts, so ONE SUM all-reduce of `totals` over the ranks of a sharded batch reproduces the un-sharded means.
 * weights (nullable, [6] floats): stage 2 runs as the tail of that launch (statistics not synchronised across ranks).
 * sched_host, corrector_r, small_epsilon are read for that tail only. */
MDX_API int mdx_adaptive_corrector_statistics(const mdx_schedule_t* sched_host, int index_i, const int32_t* d_index,
                                      const float* score_x, const float* score_l, const float* z_coordinates,
                                      const float* z_lattice_for_step_size, mdx_rng_t rng, int64_t batch,
                                      int number_of_atoms, int spatial_dimension, int use_fixed_lattice_parameters,
                                      float corrector_r, float small_epsilon, float* workspace, double* totals,
                                      float* weights, mdx_stream_t stream);
/* Stage 2, the step size (:137-146): each mean = (float)(sum / count), then in binary32
 *   score_norm = mean_s / sigma;  ratio = (r mean_z) / max(score_norm, small_epsilon);  eps = (2 ratio) ratio
 * weights[6] = {eps, sqrt(2 eps), sigma, eps_L, sqrt(2 eps_L), sigma_n}, sigma_n = sigma / N^(1/d); eps_L = 0 with a fixed
 * lattice. */
MDX_API int mdx_adaptive_corrector_step_size(const mdx_schedule_t* sched_host, int index_i, const int32_t* d_index,
                                     const double* totals, int number_of_atoms, int spatial_dimension,
                                     int use_fixed_lattice_parameters, float corrector_r, float small_epsilon,
                                     float* weights, mdx_stream_t stream);
/* Stage 3, the update, on mdx_pc_step_update's body (same operands, same in-register draws, outputs may alias inputs).
 * mode MDX_CORRECTOR (:97-148): the score weight, noise weight and sigma of X and of L are read from `weights` and not from the
 * tables.  z_lattice is the draw the UPDATE uses: the reference computes the lattice step size from one lattice draw and
 * updates with the next, so stage 1 and stage 3 take their lattice noise separately.
 * mode MDX_PREDICTOR (:41-63): atom types only -- x, l, the scores, x_out and l_out are neither read nor written; weights may be
 * NULL; MDX_STATUS_MASK_AT_LAST_STEP is reported as by mdx_pc_step_update. */
MDX_API int mdx_adaptive_corrector_update(const mdx_schedule_t* sched_host, int mode, int index_i, const int32_t* d_index,
                                  const mdx_pc_flags_t* flags_host, const int64_t* atom_types, const float* x,
                                  const float* l, const float* logits, const float* score_x, const float* score_l,
                                  const float* z_coordinates, const float* gumbel, const float* u, const float* z_lattice,
                                  const float* weights, mdx_rng_t rng, int64_t batch, int number_of_atoms,
                                  int spatial_dimension, int64_t* atom_types_out, float* x_out, float* l_out,
                                  uint32_t* status, mdx_stream_t stream);

/* F1 -- RelativeCoordinatesNoiser.get_noisy_relative_coordinates_sample
 * (noisers/relative_coordinates_noiser.py:33-67): out = wrap(x0 + sigma*z). */
MDX_API int mdx_noise_relative_coordinates(const float* x0, const float* z, float sigma, int64_t count, float* out,
                                   mdx_stream_t stream);

/* F2 -- AtomTypesNoiser.get_noisy_atom_types_sample (noisers/atom_types_noiser.py:30-60) with
 * compute_q_at_given_a0 (utils/d3pm_utils.py:23-39): a_t = argmax_c(log(Qbar[a0][c]) - log(-log u_c)). */
MDX_API int mdx_noise_atom_types(const int64_t* a0, const float* q_bar, const float* u, int64_t n_atoms, int num_classes,
                         int64_t* out, mdx_stream_t stream);

/* F1 / F2 / F3 with the reference's own operands -- one sigma per ELEMENT, one cumulative transition matrix per ATOM (the training
 * transform hands the noisers tensors broadcast from per-structure values, data/diffusion/noising_transform.py:140-195):
 *   mdx_noise_relative_coordinates_sigmas   out = wrap(x0 + sigmas * z)           (relative_coordinates_noiser.py:56-66)
 *   mdx_noise_atom_types_per_atom           q_bar [n_atoms, C, C]; a one-hot a0 times q_bar is the row pick a0 -> q_bar[a0,:]
 *                                           (every other term an exact zero)      (atom_types_noiser.py:42-60)
 *   mdx_noise_lattice_parameters            out = sigmas_n * z + l0               (lattice_noiser.py:69-81) */
MDX_API int mdx_noise_relative_coordinates_sigmas(const float* x0, const float* z, const float* sigmas, int64_t count,
                                                  float* out, mdx_stream_t stream);
MDX_API int mdx_noise_atom_types_per_atom(const int64_t* a0, const float* q_bar, const float* u, int64_t n_atoms,
                                          int num_classes, int64_t* out, mdx_stream_t stream);
MDX_API int mdx_noise_lattice_parameters(const float* l0, const float* z, const float* sigmas_n, int64_t count, float* out,
                                         mdx_stream_t stream);

/* The training side's batch: NoisingTransform.transform (data/diffusion/noising_transform.py:82-200) of `batch` rows of a
 * device-resident dataset in ONE launch -- the gather of the rows, a time index per structure, the schedule's rows there, F1, F2
 * and F3 (the same device functions as the stand-alone entries above: the same bits).
 * Dataset: x0 f32 [M,N,d], a0 int64 [M,N], l0 f32 [M,nl], nl = d(d+1)/2, M = dataset_size.  Structure b of the batch is row
 *   r = rows ? rows[p] : p,   p = row_offset + cursor * batch + b,   cursor = d_cursor ? *d_cursor : 0
 * rows (nullable) int64 [rows_count], e.g. an epoch's permutation; d_cursor (nullable) a device word, so that a launch captured
 * into a hipGraph walks the permutation as the word is incremented; row_offset addresses a tail batch (batch = what is left).
 * Time index: time_indices_in[b] (int64 [B]) or, NULL, from the device RNG: (w T) >> 32 of one 32-bit Philox word w, in 64-bit
 * integer arithmetic -- in [0, T) by construction.  The rows of sched_host's time, sigma, q_matrix, q_bar_matrix and
 * q_bar_tm1_matrix at that index are the structure's.
 *   xt = wrap(x0[r] + sigma z)                                   (F1)
 *   at = argmax_c(log Qbar[a0[r]][c] - log(-log u_c))            (F2, the first maximum)
 *   lt = (sigma / root) z_l + l0[r]                              (F3; root = N^(1/d) as the caller's binary32 number)
 *        use_fixed_lattice_parameters != 0: lt = l0[r], and no lattice draw is made
 * Noise: z [B,N,d], u [B,N,C], z_lattice [B,nl] pre-drawn and indexed by the position in the BATCH; a NULL pointer switches that
 * draw to the device RNG, keyed by the DATASET ROW: counter = (item, (call << 8) | k/4, rng.draw_offset, tag) with
 *   MDX_TAG_TRAIN_TIME_INDEX  item = r, word 0           MDX_TAG_TRAIN_Z        item = r N + atom, k = the dimension
 *   MDX_TAG_TRAIN_LATTICE     item = r, k = parameter    MDX_TAG_TRAIN_U        item = r N + atom, k = the class
 * (what mdx_rng_fill writes at those items: kind 1 for z and z_lattice, kind 0 for u) and call = rng.call_dev ? *rng.call_dev :
 * rng.call.  A row's noise therefore does not depend on the batch it sits in, its size or its order, and a fixed call
 * reproduces a dataset noised once without storing it.  rng.draw_stride is not read.
 * Outputs, every pointer nullable: x0_out [B,N,d], a0_out [B,N], l0_out [B,nl] (the gathered clean rows); time_indices_out int64
 * [B], time_out [B], sigma_out [B]; xt_out, at_out, lt_out; q_out, q_bar_out, q_bar_tm1_out [B,C,C] (one row per structure).
 * status (nullable): MDX_STATUS_NOISING_INDEX.  M N >= 2^32 (the 32-bit Philox item): MDX_ERR_INVALID_ARG.  d <= 3 and
 * C <= MDX_MAX_CLASSES, else MDX_ERR_UNSUPPORTED. */
MDX_API int mdx_noise_training_batch(const mdx_schedule_t* sched_host, const float* x0, const int64_t* a0, const float* l0,
                                     int64_t dataset_size, const int64_t* rows, int64_t rows_count, int64_t row_offset,
                                     const int32_t* d_cursor, const int64_t* time_indices_in, const float* z, const float* u,
                                     const float* z_lattice, mdx_rng_t rng, int64_t batch, int number_of_atoms,
                                     int spatial_dimension, float root, int use_fixed_lattice_parameters, float* x0_out,
                                     int64_t* a0_out, float* l0_out, int64_t* time_indices_out, float* time_out, float* sigma_out,
                                     float* xt_out, int64_t* at_out, float* lt_out, float* q_out, float* q_bar_out,
                                     float* q_bar_tm1_out, uint32_t* status, mdx_stream_t stream);

/* R1 -- ConstrainedLangevinGenerator._repaint_composition (generators/constrained_langevin_generator.py:136-163):
 * for each sample and each constrained row k: forward-noise the known (x_k, a_k) to time index `index_i`
 * (NoisingTransform.transform_given_time_index, data/diffusion/noising_transform.py:98-200; identity when
 * index_i == 0) and overwrite row constrained_indices[k] of X and A in place.
 * z [B,N,d] and u [B,N,C] are the FULL-size draws the reference makes (only constrained rows are read);
 * NULL switches to the device RNG. */
MDX_API int mdx_repaint_constrained_rows(const mdx_schedule_t* sched_host, int index_i, const int32_t* d_index,
                                 const float* constrained_x, const int64_t* constrained_a,
                                 const int64_t* constrained_indices, int number_of_constraints, const float* z,
                                 const float* u, mdx_rng_t rng, int64_t batch, int number_of_atoms,
                                 int spatial_dimension, float* x_inout, int64_t* a_inout, mdx_stream_t stream);

/* R1 with one constraint table per ENVIRONMENT of the batch (no reference counterpart: the reference's excise-and-repaint
 * sample maker, active_learning_loop/sample_maker/excise_and_repaint_sample_maker.py:162-174, builds one generator per
 * environment and runs them one after another).  Sample b belongs to environment e = sample_environment[b] (int32 [B]) and
 * takes rows 0 .. counts[e]-1 of constrained_x [E,K,d], constrained_a [E,K] and constrained_indices [E,K], K = capacity;
 * the rows past counts[e] are padding and are skipped, as is a row whose index lies outside [0, N) or whose atom type lies
 * outside [0, C).  Arithmetic, noise arguments and the Philox counter (item = b N + row, the same tags and draw ids) are those
 * of mdx_repaint_constrained_rows: with equal environments the two entries write the same bits.  The tables are read at
 * execution time: a captured launch sees what they hold when the graph is replayed. */
MDX_API int mdx_repaint_rows_per_sample(const mdx_schedule_t* sched_host, int index_i, const int32_t* d_index,
                                        const float* constrained_x, const int64_t* constrained_a,
                                        const int64_t* constrained_indices, const int32_t* counts,
                                        int number_of_environments, int capacity, const int32_t* sample_environment,
                                        const float* z, const float* u, mdx_rng_t rng, int64_t batch, int number_of_atoms,
                                        int spatial_dimension, float* x_inout, int64_t* a_inout, mdx_stream_t stream);

/* Environment excision -- SphericalExcision / NearestNeighborsExcision._excise_one_environment
 * (active_learning_loop/excisor/spherical_excisor.py:45-68, nearest_neighbors_excisor.py:48-67), center_structure
 * (excisor/base_excisor.py:65-74) and embed_structure_in_new_box (sample_maker/base_sample_maker.py:247-291) for every
 * central atom in ONE launch, one workgroup per central atom.  relative_coordinates [N,d] and box_sides [d] are binary64 (an
 * orthogonal box, like the reference); everything is computed in binary64 in the reference's order:
 *   distance   (x_j L - x_c L), per dimension min(D^2, (D - L)^2, (D + L)^2), sqrt of the sum   (utils.py:113-135)
 *   members    mode MDX_EXCISE_RADIUS: distance < radial_cutoff; MDX_EXCISE_NEIGHBOURS: the number_of_neighbors + 1 nearest
 *   slot       the rank by (distance, atom index): ties go to the LOWER atom index (numpy's argsort leaves them unspecified)
 *   centring   center_atoms != 0: mod(x + (0.5 - x_slot0), 1), numpy's mod
 *   embedding  new_box_sides != NULL: ((x - 0.5) L + 0.5 L_new) (1 / L_new); outside (0, L_new): MDX_STATUS_EXCISE_OUTSIDE_BOX
 * Outputs, zero-padded to `capacity` slots per environment: source_indices int64 [E,capacity], constrained_x float32
 * [E,capacity,d] (ONE rounding of the binary64 value, as torch.FloatTensor(...) in excise_and_repaint_sample_maker.py:105),
 * counts int32 [E] (the true member count, also when it exceeds capacity: MDX_STATUS_EXCISE_CAPACITY).  `status` nullable.
 * number_of_atoms and capacity <= MDX_EXCISE_MAX_ATOMS (MDX_ERR_UNSUPPORTED above); d <= 3. */
#define MDX_EXCISE_RADIUS 0
#define MDX_EXCISE_NEIGHBOURS 1
#define MDX_EXCISE_MAX_ATOMS 4096
MDX_API int mdx_excise_environments(const double* relative_coordinates, const double* box_sides, int number_of_atoms,
                                    int spatial_dimension, const int64_t* central_atoms, int number_of_environments, int mode,
                                    double radial_cutoff, int number_of_neighbors, int center_atoms, const double* new_box_sides,
                                    int capacity, int64_t* source_indices, float* constrained_x, int32_t* counts,
                                    uint32_t* status, mdx_stream_t stream);

/* The sample edit -- ExciseAndRepaintSampleMaker.edit_generated_structure (excise_and_repaint_sample_maker.py:224-236) for a
 * batch: keep[b,n] = n < counts[e] or distance(atom n, atom active_atoms[e]) > radius, e = sample_environment[b], with the
 * distance of mdx_excise_environments in binary64 on the widened float32 relative_coordinates [B,N,d] and the sample's own box
 * lattice_parameters[b, :d] (row stride lattice_stride).  active_atoms and counts int32 [number_of_environments]; a sample whose
 * environment or active atom is out of range keeps every atom.  keep uint8 [B,N]; the caller compacts the ragged result. */
MDX_API int mdx_edit_keep_mask(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride,
                               const int32_t* sample_environment, const int32_t* active_atoms, const int32_t* counts,
                               int number_of_environments, double radius, int64_t batch, int number_of_atoms, int spatial_dimension, uint8_t* keep,
                               mdx_stream_t stream);

/* The excise-and-random sample maker (active_learning_loop/sample_maker/excise_and_random_sample_maker.py:169-328) for every
 * sample of a frame at once.  Two functions: the proposals of all max_attempts attempts, then placement, retry and acceptance.
 *
 * mdx_random_fill_proposals -- the device draws.  For sample b < batch and attempt m < max_attempts:
 *   uniforms f64 [B,M,N,d] in [0, 1), types int32 [B,M,N] in [0, num_atom_types), and, with number_of_voxels > 0, voxels
 *   int32 [B,M,N] by select_occupied_voxels' rule (active_learning_loop/utils.py:203-212): atom n < (N / V) V takes voxel
 *   n mod V (all voxels once per full round); the N mod V atoms left take distinct voxels, the one after the other the voxels
 *   of rank 0, 1, ... by (key, voxel index) of one 32-bit Philox key per voxel: a uniformly random ordered subset.
 * Philox4x32-10 with key = seed and counter = (item, (call << 8) | sub, first_sample + b, (m << 8) | tag): a sample's numbers
 * depend on (seed, call, its index, the attempt) and not on the batch it sits in.
 *   MDX_TAG_FILL_UNIFORM  item = atom, sub = axis: words w0, w1 give ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53, a multiple of 2^-53
 *                         in [0, 1) -- 27 high and 26 low bits, every binary64 of that grid equally likely
 *   MDX_TAG_FILL_TYPE     item = atom, sub = 0: the high word of w0 * num_atom_types (the bias is below num_atom_types 2^-32)
 *   MDX_TAG_FILL_VOXEL    item = voxel, sub = 0: the key w0
 * voxels NULL with number_of_voxels = 0.  N <= MDX_RANDOM_FILL_MAX_ATOMS, V <= MDX_RANDOM_FILL_MAX_VOXELS, d <= 3,
 * call and max_attempts < 2^24, first_sample + batch <= 2^32.
 *
 * mdx_random_fill_environments -- one workgroup per sample; nothing is read back between attempts.  Sample b belongs to
 * environment e = sample_environment[b]: its first counts[e] atoms are the rows of constrained_x f64 [E,K,d] / constrained_a
 * int64 [E,K], untouched (binary64 copies), in the box box_sides f64 [E,d] (orthogonal).  For attempt m = 0, 1, ... until one
 * is accepted:
 *   sites      uniforms[b,m]; with partition != NULL (a HOST pointer to d ints, the voxels per axis; voxel v = (i0 p1 + i1) p2
 *              + i2) site = i_a (1 / p_a) + u / p_a, in binary64 in that order (numpy's linspace corner, divide, add)
 *   placement  constrained atom k = 0 .. count-1 in order takes the nearest site not yet taken, by the periodic distance of
 *              mdx_excise_environments (utils.py:113-135); equal distances go to the LOWER site index
 *   structure  the constrained atoms in their own order with their own coordinates and types, then the sites not taken in
 *              ascending site index with types[b,m,site]
 *   distance   the least periodic distance over all pairs i != j: the least sum of squares, one sqrt
 *   accepted   distance > minimal_interatomic_distance
 * The last attempt is returned when none is accepted.  Outputs: x f64 [B,N,d], a int64 [B,N], active_out int32 [B] (=
 * active[e], the active atom's index in the constrained order), attempts int32 [B] (1-based: the attempt returned), accepted
 * uint8 [B], min_distance f64 [B].  `status` (nullable): MDX_STATUS_RANDOM_FILL_COUNT / _ENVIRONMENT; such a sample comes
 * out zero with attempts = 0.  Limits (the workgroup's LDS holds the sites and the structure): 2 <= N <=
 * MDX_RANDOM_FILL_MAX_ATOMS, K <= MDX_RANDOM_FILL_MAX_ATOMS (MDX_ERR_UNSUPPORTED above), d <= 3, max_attempts >= 1. */
#define MDX_RANDOM_FILL_MAX_ATOMS 1024
#define MDX_RANDOM_FILL_MAX_VOXELS 4096
MDX_API int mdx_random_fill_proposals(uint64_t seed, uint32_t call, int64_t first_sample, int64_t batch, int max_attempts,
                                      int number_of_atoms, int spatial_dimension, int num_atom_types, int number_of_voxels,
                                      double* uniforms, int32_t* types, int32_t* voxels, mdx_stream_t stream);
MDX_API int mdx_random_fill_environments(const double* uniforms, const int32_t* types, const int32_t* voxels,
                                         const int32_t* partition, const double* constrained_x, const int64_t* constrained_a,
                                         const int32_t* counts, const int32_t* active, int number_of_environments,
                                         int constrained_capacity, const int32_t* sample_environment, const double* box_sides,
                                         int max_attempts, double minimal_interatomic_distance, int64_t batch,
                                         int number_of_atoms, int spatial_dimension, double* x, int64_t* a, int32_t* active_out,
                                         int32_t* attempts, uint8_t* accepted, double* min_distance, uint32_t* status,
                                         mdx_stream_t stream);

/* RePaint resampling ("2000 steps with resampling", BASELINE configs[4]) -- no reference counterpart: the reference's
 * ConstrainedLangevinGenerator (generators/constrained_langevin_generator.py:94-163) has no resampling loop, so this
 * entry is the build-only option `repaint_resampling_steps` of SURVEY section 8(d); with 0 resampling steps it is never
 * called and the reference's behaviour is unchanged.  One step of the FORWARD process from time index i to i+1
 * (i = *d_index + index_i, 1 <= i < T), in place, for every atom of every structure, with the table row idx = i that
 * the predictor step i+1 -> i reads:  X <- wrap(X + g[idx] * z)        (variance-exploding kernel, F1 arithmetic)
 *                                     A <- argmax_c(log Q[idx][A][c] - log(-log u_c))   (one-step D3PM kernel, F2)
 * z [B,N,d] / u [B,N,C] pre-drawn, or NULL for the device RNG (tags MDX_TAG_RESAMPLE_Z / _U). */
MDX_API int mdx_forward_diffusion_step(const mdx_schedule_t* sched_host, int index_i, const int32_t* d_index,
                                       const float* z, const float* u, mdx_rng_t rng, int64_t batch,
                                       int number_of_atoms, int spatial_dimension, float* x_inout, int64_t* a_inout,
                                       mdx_stream_t stream);

/* N1 -- get_periodic_adjacency_information (utils/neighbors.py:36-224) and the EGNN consumer
 * get_edges_with_radial_cutoff (models/egnn_utils.py:107-144).  Two-call protocol:
 *   1. mdx_radius_graph_count  -> counts[B*N] (edges per source atom)
 *   2. caller: offsets = exclusive_scan(counts), E = sum(counts); allocates outputs
 *   3. mdx_radius_graph_fill   -> edges, ordered by (structure, source, destination[, image])
 * unique = 1: one edge per (src,dst) pair whatever the image (torch.unique(dim=1) of the reference), edges
 *             [E,2] int64 with batch-global node indices (b*N + i); image_out unused.
 * unique = 0: one edge per (src,dst,image); edges [E,2] with per-structure indices, image_out[E] in 0..26
 *             (itertools.product(-1,0,1) order, utils/lattice_utils.py:10-29), shifts_out [E,3] (nullable).
 * Positions [B,N,3] and cells [B,3,3].  The reference takes spatial_dimension 1, 2 or 3: a caller with fewer dimensions
 * embeds its problem -- zero coordinates and orthogonal cell vectors of 4 x cutoff in the missing dimensions: no periodic
 * image along them is within the cutoff, the cutoff-too-large status is decided by the real vectors -- and keeps the first
 * d components of the shifts (what the Python host side does: utils/neighbors.py::embed_in_three_dimensions). */
MDX_API int mdx_radius_graph_count(const float* cartesian_positions, const float* basis_vectors, float radial_cutoff,
                           int64_t batch, int number_of_atoms, int unique, int64_t* counts, uint32_t* status,
                           mdx_stream_t stream);
MDX_API int mdx_radius_graph_fill(const float* cartesian_positions, const float* basis_vectors, float radial_cutoff,
                          int64_t batch, int number_of_atoms, int unique, const int64_t* offsets,
                          int64_t* edges_out, int32_t* image_out, float* shifts_out, mdx_stream_t stream);
/* The same with a caller-sized edge list ("capacity + overflow flag"): step 2 happens on the device --
 * offsets = exclusive scan of counts, E = its last element + last count, both left in device memory -- and the outputs
 * hold `capacity` rows, so no host read sits between count and fill (the step can be captured into a hipGraph).  Edges
 * beyond `capacity` are not written and MDX_STATUS_GRAPH_CAPACITY is OR-ed into `status` (nullable).  capacity =
 * batch * N * (N - 1) can never overflow in unique mode. */
MDX_API int mdx_radius_graph_fill_capped(const float* cartesian_positions, const float* basis_vectors, float radial_cutoff,
                                         int64_t batch, int number_of_atoms, int unique, const int64_t* offsets,
                                         int64_t capacity, int64_t* edges_out, int32_t* image_out, float* shifts_out,
                                         uint32_t* status, mdx_stream_t stream);

/* The graph EGNNScoreNetwork builds per forward (models/score_networks/egnn_score_network.py:236-247): the unique-pair radius
 * graph of RELATIVE coordinates [batch, N, 3] in the orthogonal cell diag(max(lattice_parameters[b, 0..2], clip_min)) (the
 * reference clips the cell lengths to 2.2 x cutoff and zeroes the angles); no host read, nothing but the caller's buffers
 * (counts, offsets [batch*N]; n_edges [1]; edges_out [capacity, 2]).  Cartesian positions are formed in the kernels as
 * relative x length, the bits of the reference's matmul with the diagonal cell.  lattice_stride = row length of
 * lattice_parameters (>= 3).  Status bits as mdx_radius_graph_count / _fill_capped.
 * With a `workspace` of mdx_egnn_radius_graph_workspace_words(batch, N) 64-bit words (caller-owned, need not be initialised, not
 * read after the call) the build is TWO launches and every pair is tested once: the first keeps each source row's hits as 64-bit
 * words in the workspace, the second sums the totals of the structures in front, scans the row counts and writes the pairs.
 * The helper returns 0 where that form does not apply (N > 1024 or batch > 2048); then, or with workspace = NULL, the build is
 * count -> device-side exclusive scan -> fill (three launches).  Same outputs, bit for bit, either way. */
MDX_API int64_t mdx_egnn_radius_graph_workspace_words(int64_t batch, int number_of_atoms);
MDX_API int mdx_egnn_radius_graph(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride,
                                  float clip_min, float radial_cutoff, int64_t batch, int number_of_atoms, int64_t capacity,
                                  int64_t* counts, int64_t* offsets, int64_t* n_edges, int64_t* edges_out, uint32_t* status,
                                  uint64_t* workspace, int64_t workspace_words, mdx_stream_t stream);

/* The pseudo-force of ForceFieldAugmentedScoreNetwork (models/score_networks/force_field_augmented_score_network.py:86-236,
 * with utils/neighbors.py:36-224 and utils/basis_transformations.py:230-256): phi(r) = s (r - rc)^2 over every (i, j, image)
 * pair of the full radius graph of RELATIVE coordinates [batch, N, 3] in the cell diag(max(lattice_parameters[b, 0..2],
 * clip_min)) (the reference's min_box_size; lattice_stride as mdx_egnn_radius_graph), returned in relative coordinates:
 *   out[b, i] = (sum_{j, l} two_strength (r - rc) / (r + 1e-8) disp) x (1 / L),  disp = (p_j - p_i) + shift_l,  r = |disp|
 * two_strength = (float)(2.0 * strength), formed in double as the reference's Python does.  The pairs are the ones
 * mdx_radius_graph_count / _fill list (0 < d^2 <= rc^2, 27 images), tested in place: no edge list, no atomics, no workspace,
 * no host read.  A row's sum is a fixed-order reduction: it does not depend on the rest of the batch or on the run.
 * score_in (nullable, [batch, N, 3]): out = score_in + pseudo-force (the reference's raw.X + forces, same bits).
 * status (nullable): MDX_STATUS_CUTOFF_TOO_LARGE is OR-ed in where rc reaches the cell's crossing distance (the reference's
 * assert, neighbors.py:107-113).  Spatial dimension 3 only (the reference's :131-135); N <= 5000 (LDS), else
 * MDX_ERR_UNSUPPORTED. */
MDX_API int mdx_force_field_pseudo_force(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride,
                                         float clip_min, float radial_cutoff, float two_strength, int64_t batch,
                                         int number_of_atoms, const float* score_in, float* out, uint32_t* status,
                                         mdx_stream_t stream);

/* Stillinger-Weber energies and forces (LAMMPS `pair_style sw`, metal units): what the reference's energy oracle obtains from
 * LAMMPS for every sample (oracle/lammps_energy_oracle.py:56-158, called through oracle/energy_oracle.py:44-131), evaluated
 * from the closed formula over all periodic images of an ORTHOGONAL box:
 *   E    = sum_i sum_{j>i} phi2(r_ij) + sum_i sum_{j != i} sum_{k>j} phi3(r_ij, r_ik, theta_jik)
 *   phi2 = A eps [B (sigma/r)^p - (sigma/r)^q] exp(sigma / (r - a sigma))                 r < a sigma, entry (ti, tj, tj)
 *   phi3 = lambda eps (cos theta - cos theta0)^2 exp(g_ij s_ij / (r_ij - a_ij s_ij)) exp(g_ik s_ik / (r_ik - a_ik s_ik))
 *          lambda, eps, cos theta0 of entry (ti, tj, tk); sigma, a, gamma of the ij leg of (ti, tj, tj), of the ik leg of
 *          (ti, tk, tk); each leg inside its own cutoff
 * relative_coordinates f32 [batch, N, 3], expected in [0, 1) as the sampler leaves them (the sweep covers the images -1, 0, +1 of
 * the coordinates as given: it does not wrap them); lattice_parameters f32 [batch, lattice_stride], the first three the box sides (the
 * rest is not read); atom_types int64 [batch, N]; parameter_table: DEVICE double [n_types^3][10], entry (ti, tj, tk) =
 * {eps, sigma, a, lambda, gamma, cos theta0, A, B, p, q}.  energies: double [batch] (eV); forces (nullable): double
 * [batch, N, 3], Cartesian (eV / Angstrom).  Binary64 throughout, from the binary32 inputs promoted once (position =
 * (double)relative * (double)side).  No float atomics: every force is gathered and every sum has a fixed order, so the bits
 * do not depend on the launch or on the rest of the batch.  One launch, no host read.
 * The +-1 image sweep is complete only while every side >= the largest a sigma of the table: a structure with a shorter (or
 * NaN) side gets NaN energy and forces and MDX_STATUS_CUTOFF_TOO_LARGE.  An atom type outside [0, n_types) gives NaNs and
 * MDX_STATUS_SW_ATOM_TYPE; an atom with more than neighbour_capacity neighbours NaNs and MDX_STATUS_SW_NEIGHBOURS (never a
 * truncated sum).  Non-finite coordinates give NaNs.  status is nullable.
 * workspace: caller-owned, at least mdx_stillinger_weber_workspace_doubles(batch, N, neighbour_capacity) doubles (the neighbour
 * lists: 4 doubles per slot); workspace_doubles is its size.  N <= 1024 and n_types <= 8, else MDX_ERR_UNSUPPORTED. */
MDX_API int64_t mdx_stillinger_weber_workspace_doubles(int64_t batch, int number_of_atoms, int neighbour_capacity);
MDX_API int mdx_stillinger_weber_energy_forces(const float* relative_coordinates, const float* lattice_parameters,
                                               int lattice_stride, const int64_t* atom_types, const double* parameter_table,
                                               int n_types, int64_t batch, int number_of_atoms, int neighbour_capacity,
                                               double* workspace, int64_t workspace_doubles, double* energies, double* forces,
                                               uint32_t* status, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Analytical score network (csrc/mdx_analytical.hip): wrapped Gaussians of width sigma_d around equilibrium sites.
 * Common to the three functions: binary32 inputs are promoted once, everything inside is binary64, every output is rounded
 * once to binary32; kmax in [0, 64] (the sums run over k in [-kmax, kmax], the reference's truncation), else
 * MDX_ERR_UNSUPPORTED; status (nullable) receives MDX_STATUS_ANALYTICAL_SIGMA / _COORDINATES and the affected outputs are NaN --
 * invalid input is reported, never a fault; no float atomics, so a launch (or a hipGraph replay) always gives the same bits. */

/* sigma x score of the wrapped Gaussian, elementwise over n values (score/wrapped_gaussian_score.py:131-419,
 * get_coordinates_sigma_normalized_score): the reference's three formulas with its truncation -- 1a for sigma <= thr and
 * u < 0.5, 1b for sigma <= thr and u >= 0.5, the Ewald form for sigma > thr, thr the BINARY32 constant 1 / sqrt(2 pi) the
 * reference compares with.  (They are different truncations: at small kmax not one converged lattice sum.)
 * coordinates_bounded != 0: a u outside [0, 1) is reported; 0: only a non-finite one. */
MDX_API int mdx_wrapped_gaussian_sigma_normalized_score(const float* relative_coordinates, const float* sigmas, int64_t n,
                                                        int kmax, int coordinates_bounded, float* out, uint32_t* status,
                                                        mdx_stream_t stream);

/* log of the wrapped Gaussians, summed over rows (score/wrapped_gaussian_score.py:41-92, get_log_wrapped_gaussians):
 * out[r] = sum over the row_length trailing elements of logsumexp_k(-(u + k)^2 / (2 sigma^2)) - log(sqrt(2 pi) sigma), with
 * sqrt(2 pi) the binary32 value the reference multiplies by. */
MDX_API int mdx_log_wrapped_gaussians(const float* relative_coordinates, const float* sigmas, int64_t rows, int row_length,
                                      int kmax, float* out, uint32_t* status, mdx_stream_t stream);

/* The analytical score network's forward (models/score_networks/analytical_score_network.py:135-298,
 * get_probabilities_and_normalized_scores): relative_coordinates f32 [batch, N, D]; sigmas f32 [batch] (sigma_per_element 0) or
 * [batch, N, D] (1); equilibrium_relative_coordinates f32 [N, D]; sigma_normalized_scores f32 [batch, N, D]; probabilities
 * (nullable) f32 [batch].  With u = wrap(x_n - site_j) (binary64 difference; a fraction that rounds to 1 becomes 0) and
 * s = sqrt(sigma_d_square + sigma^2), a structure's result is the softmax-weighted sum over the equilibrium arrangements p of
 * sigma score(u, s) / s with weights log_w[p] = sum_{n, d} log wrapped Gaussian(u, s): ONE arrangement (site n for atom n)
 * without use_permutation_invariance, all N! assignments of sites to atoms with it -- evaluated from an N x N table of terms,
 * never from N! copies.  probabilities = sum_p exp(log_w[p]) / (number of arrangements) (0 or inf where binary32 under- or
 * overflows).  One workgroup per structure, one launch, no host read.
 * N <= 1024 and D <= 3; with use_permutation_invariance N <= 8; else MDX_ERR_UNSUPPORTED.  A structure holding a sigma that is
 * not finite and positive, or a coordinate outside [0, 1), gets NaN outputs and its bit in status; the others are unaffected. */
MDX_API int mdx_analytical_score(const float* relative_coordinates, const float* sigmas, int sigma_per_element,
                                 const float* equilibrium_relative_coordinates, double sigma_d_square, int kmax,
                                 int use_permutation_invariance, int64_t batch, int number_of_atoms, int spatial_dimension,
                                 float* sigma_normalized_scores, float* probabilities, uint32_t* status, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Linear assignment and optimal transport (csrc/mdx_transport.hip): the reference's transport/transporter.py and its
 * equivariant analytical score network, which solve their assignment problems one by one on the host
 * (scipy.optimize.linear_sum_assignment), here in one launch with no host read.  The solver is the shortest-augmenting-path
 * Hungarian algorithm in binary64, one wavefront per problem, for n <= 256 (else MDX_ERR_UNSUPPORTED).  Among equal values its
 * arg-min takes the lower column, and it uses no atomics: a launch (or a hipGraph replay) always gives the same bits.  Its loop
 * counts are bounded by n whatever the data, and invalid input is reported, never a fault. */

/* min over permutations of sum_i cost[i][col_idx[i]] for `problems` matrices [n][n], row-major, f32 (costs_are_f64 0: promoted
 * once) or f64.  col_idx int32 [problems][n]: the column of each row; costs f64 [problems]: the optimum, summed in row order.
 * A matrix with an entry that is not finite gives col_idx -1, cost NaN and MDX_STATUS_LAP_COST in status (nullable). */
MDX_API int mdx_linear_assignment(const void* cost_matrices, int costs_are_f64, int64_t problems, int n, int32_t* col_idx,
                                  double* costs, uint32_t* status, mdx_stream_t stream);

/* Transporter.get_optimal_transport (transport/transporter.py:148-196), one workgroup per structure.  x f32 [batch, N, D];
 * mu f32 [N, D] shared by the batch (mu_batch_stride 0) or [batch, N, D] (mu_batch_stride N D; anything else is
 * MDX_ERR_INVALID_ARG); point_group_operations f32 [O, D, D].  N <= 256, D <= 3, O <= 48, else MDX_ERR_UNSUPPORTED.
 *   centre   c = atan2(mean_n sin 2 pi x, mean_n cos 2 pi x) / 2 pi per dimension (sums in atom order); x~ = wrap(x - c_x),
 *            mu~ = wrap(mu - c_mu); wrap(y) = y - floor(y), a fraction that rounds to 1 becomes 0
 *   solve    per operation o: cost(i, j) = sum_d g^2, g = delta - rint(delta), delta = (R_o mu~)_j - x~_i (the square of the
 *            reference's atan2(sin, cos) / 2 pi, up to rounding), solved as above
 *   choose   the first minimum of the O optimal costs, in operation order
 *   write    aligned_mu [batch, N, D] row n = wrap(R_chosen mu~[col_idx[n]]), rounded once to f32
 * Optional outputs (NULL: not written): operation_idx int32 [batch], col_idx int32 [batch, N] (of the chosen operation),
 * costs f64 [batch, O].  A structure with a coordinate that is not finite gets NaN (-1 in the integer outputs) and
 * MDX_STATUS_ANALYTICAL_COORDINATES in status (nullable); any finite coordinate is accepted. */
MDX_API int mdx_transport_align(const float* x, const float* mu, int64_t mu_batch_stride, const float* point_group_operations,
                                int number_of_operations, int64_t batch, int number_of_atoms, int spatial_dimension,
                                float* aligned_mu, int32_t* operation_idx, int32_t* col_idx, double* costs, uint32_t* status,
                                mdx_stream_t stream);

/* find_squared_geodesic_distance_minimizing_translation (transport/optimal_translation.py:188-251; csrc/
 * mdx_optimal_translation.hip): per structure and dimension the translation tau in [-1/2, 1/2) that minimises the squared
 * geodesic distance D^2(x, y + tau), one workgroup per (structure, dimension), one launch, no host read.  x f32 [N, D] shared by
 * the batch (x_batch_stride 0) or [batch, N, D] (x_batch_stride N D; anything else is MDX_ERR_INVALID_ARG); y f32 [batch, N, D].
 * N <= 256 and D <= 3, else MDX_ERR_UNSUPPORTED.  Any finite coordinate is accepted.  Binary64 from the promoted inputs:
 *   delta_i = y_i - x_i; l0_i = floor((delta_i - 1/2) + 1/2); crossing c_i = -((delta_i - l0_i) - 1/2), sorted ascending
 *   plateau k = 0 .. N: left_k = -1/2 or c_(k), right_k = c_(k+1) or 1/2, L_k = sum_i l0_i + #{j <= k : c_(j) < 1/2},
 *   rhs_k = L_k / N - (sum_i delta_i) / N (sums in atom order); a candidate when left_k < rhs_k < right_k, both strict
 *   cost_k = sum_i g_i^2, g = d - rint(d), d = (y_i + rhs_k) - x_i
 * tau f32 [batch, D]: rhs_k of the first minimum of the costs in plateau order, rounded once.  Optional outputs (NULL: not
 * written): squared_distance f64 [batch, D], that minimum; number_of_candidates int32 [batch, D].  An entry without a candidate
 * gets tau = squared_distance = +inf, the count 0 and MDX_STATUS_TRANSLATION_NO_CANDIDATE in status (nullable), where the
 * reference has +inf too.  A structure with a coordinate that is not finite gets NaN, the count -1 and
 * MDX_STATUS_ANALYTICAL_COORDINATES.  No atomics in the arithmetic, every sum in a fixed order, every loop bounded by N + 1
 * whatever the data: the same bits on every launch and hipGraph replay. */
MDX_API int mdx_optimal_translation(const float* x, int64_t x_batch_stride, const float* y, int64_t batch, int number_of_atoms,
                                    int spatial_dimension, float* tau, double* squared_distance, int32_t* number_of_candidates,
                                    uint32_t* status, mdx_stream_t stream);

/* The equivariant analytical score network's forward (models/score_networks/equivariant_analytical_score_network.py,
 * get_normalized_scores): the alignment above of the shared equilibrium sites [N, D] onto each structure, then per element
 * u = wrap(x~ - aligned image), s = sqrt(sigma_d_square + sigma^2) and sigma_normalized_scores = sigma score(u, s) / s with the
 * wrapped-Gaussian score of mdx_wrapped_gaussian_sigma_normalized_score (kmax in [0, 64]), rounded once to f32.
 * sigmas f32 [batch], one per structure.  A sigma that is not finite and positive, or a coordinate that is not finite, gives
 * that structure NaNs and MDX_STATUS_ANALYTICAL_SIGMA / _COORDINATES in status (nullable). */
MDX_API int mdx_equivariant_analytical_score(const float* relative_coordinates, const float* sigmas,
                                             const float* equilibrium_relative_coordinates, const float* point_group_operations,
                                             int number_of_operations, double sigma_d_square, int kmax, int64_t batch,
                                             int number_of_atoms, int spatial_dimension, float* sigma_normalized_scores,
                                             uint32_t* status, mdx_stream_t stream);

/* The denoising loss of a score network on a noised batch in one launch (csrc/mdx_loss.hip): what
 * AXLDiffusionLightningModel._generic_step (models/axl_diffusion_lightning_model.py:243-346) computes after the network's
 * forward -- the two targets, the three unreduced losses of loss/coordinates_loss_calculator.py and
 * loss/atom_type_loss_calculator.py (on utils/d3pm_utils.py), their per-structure means and the weighted aggregate.  One
 * workgroup per structure; N <= MDX_LOSS_MAX_ATOMS, D <= 3, C <= MDX_MAX_CLASSES, P <= MDX_LOSS_MAX_LATTICE_PARAMETERS and
 * kmax <= 64, else MDX_ERR_UNSUPPORTED (before anything is launched).  Binary64 from the binary32 inputs promoted once, every
 * output value rounded once; no atomics in the arithmetic and every sum in a fixed order: the same bits on every launch and
 * hipGraph replay.  No host read.  The three parts are independent; a part whose prediction pointer is NULL is left out (its
 * outputs must be NULL, its mean is 0 and it adds nothing to the aggregate):
 *   X  predicted_x f32 [batch, N, D]; sigma f32 [batch] (sigma_per_element 0) or [batch, N, D] (1).  The target is
 *      target_x_in f32 [batch, N, D] when given, else sigma x score of the wrapped Gaussian at u = wrap(xt - x0) with the
 *      reference's formulas and truncation kmax (mdx_wrapped_gaussian_sigma_normalized_score), from x0, xt f32 [batch, N, D];
 *      loss = (predicted - target)^2, times exp(x_exponent (sigma - x_sigma0)) + 1 when x_algorithm is MDX_LOSS_WEIGHTED_MSE.
 *      The reference keeps sigma0 and exponent as BINARY32 buffers: pass the binary32-rounded values.  A sigma that is not
 *      finite and positive or a coordinate that is not finite gives NaN and MDX_STATUS_ANALYTICAL_SIGMA / _COORDINATES.
 *   A  a0 int64 [batch, N] (a_0), at int64 [batch, N] (a_t), logits f32 [batch, N, C] (class C - 1 is MASK), time_indices int64
 *      [batch]; the three transition tables f32 [T, C, C] with T = total_time_steps, read at the structure's time index, or with
 *      total_time_steps 0 f32 [batch, C, C], read at the structure's own number.  p = the softmax of the logits clipped at eps
 *      and renormalised; ce = -log_softmax with the MASK column forced to 0, kept at a_0; q(a_{t-1} | a_t, a_0) and
 *      p(a_{t-1} | a_t) by (gamma Qbar_{t-1})_i (Q_t)_{i, a_t} / (gamma Qbar_t)_{a_t} with gamma = one-hot a_0 and gamma = p;
 *      vb = xlogy(q, q) - q log(max(p(a_{t-1} | a_t), eps)) (a target of 0 gives 0), and at time index 0 -log(..) kept at a_0;
 *      loss = vb + ce_weight ce.  Without tables only ce_term is made, without logits only q_atm1; at is needed with tables.
 *   L  l0, lt, predicted_l f32 [batch, P]; sigma_n f32 [batch], or NULL: then sigma_n = sigma / sigma_n_divisor, one binary32
 *      division (utils/noise_utils.py:29 on binary32 tensors; the divisor is n^(1/d)).  target = -(lt - l0) / sigma_n; the loss as
 *      for X with l_algorithm, l_sigma0, l_exponent and the structure's sigma (NOT sigma_n:
 *      models/axl_diffusion_lightning_model.py:319-323).
 * Outputs, f32, each nullable: target_x, loss_x [batch, N, D]; loss_a, q_atm1, p_atm1, vb_term, ce_term [batch, N, C]; target_l,
 * loss_l [batch, P]; per_structure [batch, 4] = the means of loss_a, loss_x, loss_l over the structure (taken in binary64) and
 * lambda_x mean_x + lambda_l mean_l + lambda_a mean_a.  status (nullable) receives the bits named above. */
#define MDX_LOSS_MSE 0
#define MDX_LOSS_WEIGHTED_MSE 1
#define MDX_LOSS_MAX_ATOMS 1024
#define MDX_LOSS_MAX_LATTICE_PARAMETERS 6
MDX_API int mdx_denoising_loss(const float* x0, const float* xt, const float* target_x_in, const float* predicted_x,
                               const float* sigma, int sigma_per_element, const int64_t* a0, const int64_t* at,
                               const float* logits, const int64_t* time_indices, const float* q_matrices,
                               const float* q_bar_matrices, const float* q_bar_tm1_matrices, int total_time_steps,
                               const float* l0, const float* lt, const float* predicted_l, const float* sigma_n, float sigma_n_divisor,
                               int64_t batch, int number_of_atoms, int spatial_dimension, int num_classes, int number_of_lattice_parameters,
                               int kmax, int x_algorithm, double x_sigma0, double x_exponent, int l_algorithm, double l_sigma0,
                               double l_exponent, double ce_weight, double eps, double lambda_a, double lambda_x,
                               double lambda_l, float* target_x, float* target_l, float* loss_x, float* loss_a, float* loss_l,
                               float* per_structure, float* q_atm1, float* p_atm1, float* vb_term, float* ce_term,
                               uint32_t* status, mdx_stream_t stream);

/* The denoising loss with its gradient (csrc/mdx_loss.hip; the same kernel body as mdx_denoising_loss, instantiated with the
 * derivative switched on): every argument of mdx_denoising_loss up to ce_term in the same order and meaning, six more, then
 * status and stream last as everywhere in this library.  It makes everything mdx_denoising_loss makes (the same bits), and in
 * the same launch, one workgroup per structure, the derivative of
 *   loss = (1 / batch_divisor) sum_b (lambda_x mean_x[b] + lambda_l mean_l[b] + lambda_a mean_a[b])
 * with respect to predicted_x, logits and predicted_l; batch_divisor > 0 (the batch size for the mean over the batch).
 *   gradient_x f32 [batch, N, D] = lambda_x 2 (s - t) w / (batch_divisor N D), w = 1 for MDX_LOSS_MSE and
 *      exp(x_exponent (sigma - x_sigma0)) + 1 for MDX_LOSS_WEIGHTED_MSE; t is the binary64 target, not its rounded output
 *   gradient_l f32 [batch, P]: the same with P for N D, l_algorithm, l_sigma0, l_exponent and the structure's sigma (not sigma_n)
 *   gradient_a f32 [batch, N, C]: per atom, with r the softmax, u = max(r, eps), S = sum(u), p = u / S, step_i = Q[i, a_t],
 *      Dn = sum_j p_j Qbar[j, a_t], pi_i = step_i sum_j p_j Qbar_tm1[j, i] / Dn (the forward's p(a_{t-1} | a_t)):
 *        g_i = -q_i / pi_i, at time index 0 -delta(i, a_0) / pi_i, and 0 where pi_i < eps
 *        h_j = sum_i g_i (step_i Qbar_tm1[j, i] - pi_i Qbar[j, a_t]) / Dn
 *        v_k = (h_k - sum_j h_j p_j) / S where r_k >= eps, else 0
 *        d / d z_c = r_c (v_c - sum_k r_k v_k) + ce_weight (r_c - delta(c, a_0))   (the second term 0 when a_0 is MASK)
 *      times lambda_a / (batch_divisor N C).  The two clips pass the gradient where their argument is >= eps, equality
 *      included, as torch.clamp does; they are selects, so a logit of -inf (r = 0) has an exact 0 and no 0 x inf arises.
 *      xlogy(q, q) has no gradient.  gradient_a needs logits and the tables.
 *   structure_sums f64 [batch]: the unrounded aggregates per_structure[:, 3] rounds; the caller's scratch, needed with loss
 *   loss f32 [1] = (sum_b structure_sums[b]) / batch_divisor, added in structure order by the family's one-workgroup launch
 * Each of the five outputs is nullable on its own; a gradient whose part is absent (its prediction NULL; for gradient_a also
 * without tables) must be NULL, else MDX_ERR_INVALID_ARG.  Where the forward's rules give NaN -- an invalid sigma or
 * coordinate, a time index or atom type outside its range, a softmax that does not sum to one -- the gradient's elements are
 * NaN too and the same status bits are raised; the other structures keep their bits.  Binary64 from the promoted binary32
 * inputs, every value rounded once, no atomics in the arithmetic, every sum in a fixed order, no host read: the same bits on
 * every launch and hipGraph replay. */
MDX_API int mdx_denoising_loss_gradient(const float* x0, const float* xt, const float* target_x_in, const float* predicted_x,
                                        const float* sigma, int sigma_per_element, const int64_t* a0, const int64_t* at,
                                        const float* logits, const int64_t* time_indices, const float* q_matrices,
                                        const float* q_bar_matrices, const float* q_bar_tm1_matrices, int total_time_steps,
                                        const float* l0, const float* lt, const float* predicted_l, const float* sigma_n,
                                        float sigma_n_divisor, int64_t batch, int number_of_atoms, int spatial_dimension,
                                        int num_classes, int number_of_lattice_parameters, int kmax, int x_algorithm,
                                        double x_sigma0, double x_exponent, int l_algorithm, double l_sigma0, double l_exponent,
                                        double ce_weight, double eps, double lambda_a, double lambda_x, double lambda_l,
                                        float* target_x, float* target_l, float* loss_x, float* loss_a, float* loss_l,
                                        float* per_structure, float* q_atm1, float* p_atm1, float* vb_term, float* ce_term,
                                        double batch_divisor, float* gradient_x, float* gradient_a, float* gradient_l,
                                        double* structure_sums, float* loss, uint32_t* status, mdx_stream_t stream);

/* The consistency regularizer's target and loss (regularizers/consistency_regularizer.py:190-308, after Daras et al.;
 * csrc/mdx_loss.hip): for a batch of structures x_start f32 [batch, N, D] at noise sigma_start that the sampler carried to
 * x_end f32 [batch, N, D] at noise sigma_end < sigma_start, and the network's sigma-normalised score s f32 [batch, N, D] at the
 * start,
 *   u = wrap(x_start - x_end), sigma_eff = sqrt(sigma_start^2 - sigma_end^2),
 *   target = (sigma_start / sigma_eff) x [sigma_eff x score of the wrapped Gaussian of width sigma_eff at u]
 *            (mdx_wrapped_gaussian_sigma_normalized_score's formulas and truncation kmax in [0, 64]),
 *   per_structure[b] = sum over the structure of s (s - 2 target), gradient = 2 (s - target) / batch = d loss / d s,
 *   loss = (sum_b per_structure[b]) / batch, summed in structure order.
 * sigma_start, sigma_end are DEVICE words (nothing is read on the host: the call can be captured): one f32 for the batch
 * (sigma_stride 0) or f32 [batch] (sigma_stride 1); sigma_end = 0 is valid.  One workgroup per structure, then -- when loss is
 * asked for -- one tiny launch for the batch total; N <= MDX_LOSS_MAX_ATOMS, D <= 3 and kmax <= 64, else MDX_ERR_UNSUPPORTED
 * (before anything is launched).  Binary64 from the binary32 inputs promoted once, every output value rounded once; no atomics
 * in the arithmetic, every sum in a fixed order: the same bits on every launch and hipGraph replay.  A structure whose
 * sigma_start is not finite and positive, or not above a finite sigma_end >= 0, holds NaNs (MDX_STATUS_ANALYTICAL_SIGMA); an
 * element with a coordinate that is not finite is NaN, and so is its structure's sum (MDX_STATUS_ANALYTICAL_COORDINATES).
 * Outputs, each nullable: target, gradient f32 [batch, N, D]; per_structure f32 [batch]; loss f32 [1]; structure_sums
 * f64 [batch], the unrounded sums that the second launch adds up: the caller's scratch, needed with loss.  With score == NULL
 * only target is written (the other outputs must be NULL). */
MDX_API int mdx_consistency_loss(const float* x_start, const float* x_end, const float* score, const float* sigma_start,
                                 const float* sigma_end, int sigma_stride, int64_t batch, int number_of_atoms,
                                 int spatial_dimension, int kmax, float* target, float* gradient, float* per_structure,
                                 double* structure_sums, float* loss, uint32_t* status, mdx_stream_t stream);

/* The regression regularizer's target and error (regularizers/regression_regularizer.py:35-68; csrc/mdx_loss.hip): how far a
 * network's sigma-normalised score s f32 [batch, N, D] is from a known target t, with M = batch N D,
 *   e = s - t (binary64, t NOT rounded first), target = t rounded once, gradient = 2 e / M = d loss / d s,
 *   sums[b] = sum over the structure of e^2, per_structure[b] = sums[b] rounded once,
 *   loss = (sum_b sums[b]) / M, summed in structure order: the reference's mean((s - t)^2).
 * Two modes.  given_target == NULL: t is the analytical score network's score at relative_coordinates f32 [batch, N, D] with
 * sigmas f32 [batch] (one per structure) and equilibrium_relative_coordinates f32 [N, D] -- exactly mdx_analytical_score's
 * evaluation (the same code: the plain path, and the N! permutations with use_permutation_invariance), kept in binary64;
 * target then holds the bits mdx_analytical_score gives.  Its limits hold: N <= 1024, D <= 3, kmax in [0, 64], N <= 8 with
 * permutations, else MDX_ERR_UNSUPPORTED; sigma_d_square > 0.  A structure holding a sigma that is not finite and positive or a
 * coordinate outside [0, 1) gets NaNs in target, gradient and per_structure, loss is NaN, and its MDX_STATUS_ANALYTICAL_SIGMA /
 * _COORDINATES bit goes to status (nullable); the other structures are unaffected.  given_target != NULL: t is that tensor,
 * f32 [batch, N, D], promoted; relative_coordinates, sigmas and the sites are not read (they may be NULL), sigma_d_square,
 * kmax and use_permutation_invariance are ignored, score is required, and any N D that fits an int is served.
 * One workgroup per structure, then -- when loss is asked for -- one tiny launch for the batch total; no host read.  Binary64
 * from the binary32 inputs promoted once, every output value rounded once; no atomics in the arithmetic, every sum in a fixed
 * order: the same bits on every launch and hipGraph replay.  Outputs, each nullable: target, gradient f32 [batch, N, D];
 * per_structure f32 [batch]; loss f32 [1]; sums f64 [batch], the unrounded sums that the second launch adds up: the caller's
 * scratch, needed with loss.  With score == NULL (analytical mode only) only target is written (the other outputs must be
 * NULL). */
MDX_API int mdx_regression_loss(const float* relative_coordinates, const float* sigmas, const float* score,
                                const float* given_target, const float* equilibrium_relative_coordinates, double sigma_d_square,
                                int kmax, int use_permutation_invariance, int64_t batch, int number_of_atoms,
                                int spatial_dimension, float* target, float* gradient, float* per_structure, double* sums,
                                float* loss, uint32_t* status, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Sampling metrics (csrc/mdx_metrics.hip): the two-sample Kolmogorov-Smirnov distance the reference takes between the samples'
 * and the dataset's interatomic distances, energies and lattice parameters (metrics/kolmogorov_smirnov_metrics.py:42-75 --
 * scipy.stats.ks_2samp on host copies), on the device the samples are on: a sort, then a rank kernel.
 *
 * mdx_sort_keys: sorted_out f64 [n] = the ascending sort of values, n binary32 (values_are_f64 0) or binary64 (1) numbers,
 * widened exactly; values is not modified.  +-inf are ordinary keys; -0.0 and +0.0 are one key and come out as +0.0; a NaN
 * anywhere sets MDX_STATUS_KS_NAN in status (nullable) and leaves the output unspecified.  A hand-written least-significant-
 * digit radix sort on 8-bit digits of an orderable image of each value in the input's own width (4 passes for binary32, 8 for
 * binary64; histogram, scan and stable scatter per pass over tiles of MDX_KS_SORT_TILE keys): no vendor sort, no allocation, no
 * host read, stream-ordered and capturable; a stable keys-only sort has one correct output, so every launch and hipGraph
 * replay gives the same bits.  workspace: mdx_sort_keys_workspace_bytes(n, values_are_f64) bytes, 16-byte aligned (0 for an n
 * that is not supported).  1 <= n <= MDX_KS_MAX_SAMPLES, else MDX_ERR_UNSUPPORTED before anything is launched.
 *
 * mdx_ks_two_sample_sorted: for ascending a_sorted f64 [n1] and b_sorted f64 [n2] (no NaN), g = gcd(n1, n2) and c_s(x) = the
 * number of elements of sample s that are <= x, numerator_out int64 [1] =
 *   h = max over x in a U b of | c_a(x) (n2 / g) - c_b(x) (n1 / g) |,
 * so that the Kolmogorov-Smirnov distance is d = h / lcm(n1, n2), ONE correctly rounded division left to the caller: scipy's
 * two-sided statistic (searchsorted(..., side='right') on the concatenation, both signs), and the integer its exact branch
 * rounds to.  Every product stays below 2^48 (MDX_KS_MAX_SAMPLES = 2^24).  One thread per element, two binary searches for the
 * upper bound; integer block maxima and one small final workgroup: independent of the reduction order, no float atomics.
 * workspace: mdx_ks_two_sample_workspace_bytes(n1, n2) bytes, 8-byte aligned.  1 <= n1, n2 <= MDX_KS_MAX_SAMPLES, else
 * MDX_ERR_UNSUPPORTED before anything is launched. */
#define MDX_KS_MAX_SAMPLES 16777216
#define MDX_KS_SORT_TILE 2048
MDX_API int64_t mdx_sort_keys_workspace_bytes(int64_t n, int values_are_f64);
MDX_API int mdx_sort_keys(const void* values, int64_t n, int values_are_f64, double* sorted_out, void* workspace,
                          uint32_t* status, mdx_stream_t stream);
MDX_API int64_t mdx_ks_two_sample_workspace_bytes(int64_t n1, int64_t n2);
MDX_API int mdx_ks_two_sample_sorted(const double* a_sorted, int64_t n1, const double* b_sorted, int64_t n2, void* workspace,
                                     int64_t* numerator_out, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * The optimizer step (csrc/mdx_optimizer.hip): torch's single-tensor Adam and AdamW (amsgrad off, maximize off) -- what the
 * reference's load_optimizer constructs (models/optimizer.py:60-82) -- on every tensor of a parameter group in one launch, and
 * the global 2-norm of the group's gradients that torch's clip_grad_norm_ (Lightning's gradient_clip_algorithm="norm") clips by.
 *
 * The tables describe the group; the host writes them once, they are device memory:
 *   addresses uint64 [tensors, 4]   the addresses of p, g, exp_avg, exp_avg_sq: binary32, contiguous, 4-byte aligned
 *   counts int64 [tensors]          the elements of each (> 0: a tensor without elements is left out)
 *   counter_slots int32 [tensors]   (mdx_adam_step) the entry of `steps` of each tensor's first chunk: the counters outlive a table
 *   block_tensor int32 [blocks], block_offset int64 [blocks]   per workgroup: the tensor it serves and its element offset in it;
 *                                   a tensor of n elements is served by ceil(n / MDX_ADAM_CHUNK_ELEMENTS) workgroups at offsets
 *                                   0, MDX_ADAM_CHUNK_ELEMENTS, ... in table order.  An offset outside [0, n) does nothing.
 * A tensor without a gradient in some call is left out of that call's tables.
 *
 * mdx_adam_step, with t = the tensor's counter after this step and hyper f64 [MDX_ADAM_HYPER_COUNT] in device memory (a
 * captured launch follows a scheduler's learning rate; mdx_adam_hyper_fill writes it from its arguments, a launch and no copy):
 *   g  = (gradient_scale clip) grad          clip = 1 with norm == NULL, else min(1, max_norm / (norm[0] + 1e-6))
 *   decoupled_weight_decay 0 (Adam):   g = g + weight_decay p;  q = p
 *   decoupled_weight_decay 1 (AdamW):  q = p (1 - lr weight_decay)
 *   m' = m + (g - m) (1 - beta1)
 *   v' = beta2 v + (1 - beta2) g g
 *   p' = q - (lr / (1 - beta1^t)) m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)
 * The four operands of an element are widened to binary64, the form above is evaluated in binary64 in this order without
 * contraction, and each of p', m', v' is rounded to binary32 once.  steps int32 holds the steps taken, ONE ENTRY
 * PER CHUNK: the workgroup at element offset o of tensor k owns entry counter_slots[k] + o / MDX_ADAM_CHUNK_ELEMENTS, reads it,
 * uses t = entry + 1 and stores t.  All chunks of a tensor hold the same value (a call serves all of them or none), so every
 * workgroup of a tensor uses the same t and none reads what another writes; a tensor's step is its first chunk's entry.
 * With zero_gradients every consumed gradient is overwritten by +0.0.  16-byte accesses where a tensor's four addresses are 16-byte aligned, dwords otherwise: the same bits.
 * A g that is not finite sets MDX_STATUS_OPTIMIZER_NONFINITE in status (nullable); the arithmetic goes on.
 *
 * mdx_gradient_norm: norm f64 [2] = the 2-norm of all gradients in the tables and its square.  Squares and sums in binary64, a
 * fixed tree per chunk into partials f64 [blocks] (the caller's scratch), then one small launch adds them in a fixed tree.
 * Two launches; with it and clipping a step is three.  No atomics in the arithmetic: the same bits on every launch and replay. */
#define MDX_ADAM_CHUNK_ELEMENTS 2048
#define MDX_ADAM_HYPER_LR 0
#define MDX_ADAM_HYPER_BETA1 1
#define MDX_ADAM_HYPER_BETA2 2
#define MDX_ADAM_HYPER_EPS 3
#define MDX_ADAM_HYPER_WEIGHT_DECAY 4
#define MDX_ADAM_HYPER_MAX_NORM 5
#define MDX_ADAM_HYPER_GRADIENT_SCALE 6
#define MDX_ADAM_HYPER_COUNT 8
MDX_API int mdx_adam_hyper_fill(double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                                double gradient_scale, double* hyper, mdx_stream_t stream);
MDX_API int mdx_gradient_norm(const uint64_t* addresses, const int64_t* counts, const int32_t* block_tensor,
                              const int64_t* block_offset, int64_t number_of_blocks, double* partials, double* norm,
                              mdx_stream_t stream);
MDX_API int mdx_adam_step(const uint64_t* addresses, const int64_t* counts, const int32_t* counter_slots,
                          const int32_t* block_tensor, const int64_t* block_offset, int64_t number_of_blocks, int32_t* steps,
                          const double* hyper, const double* norm, int decoupled_weight_decay, int zero_gradients,
                          uint32_t* status, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused score network: the reference's MLPScoreNetwork (models/score_networks/mlp_score_network.py:54-370,
 * unconditional forward, no permutation symmetrisation, no time prefactor) evaluated inside the kernels.
 * All pointers are float32 device memory; every w_*_t is the TRANSPOSE of the nn.Linear weight, i.e. [in, out]
 * row-major, so that consecutive lanes (output neurons) read consecutive addresses. */
#define MDX_MLP_MAX_HIDDEN 8
typedef struct mdx_mlp {
    int32_t number_of_atoms, spatial_dimension, num_classes;
    int32_t hidden_size, n_hidden;                       /* hidden_dimensions_size, n_hidden_dimensions */
    int32_t e_coordinates, e_noise, e_time, e_atom_type, e_lattice;   /* embedding sizes */
    const float *w_coordinates_t, *b_coordinates;        /* [2*N*d, e_coordinates] */
    const float *w_noise_t, *b_noise;                    /* [1, e_noise] */
    const float *w_time_t, *b_time;                      /* [1, e_time] */
    const float *w_atom_type_t, *b_atom_type;            /* [C, e_atom_type] */
    const float *w_lattice_t, *b_lattice;                /* [d(d+1)/2, e_lattice] */
    const float* w_hidden_t[MDX_MLP_MAX_HIDDEN];         /* [in_k, hidden_size] */
    const float* b_hidden[MDX_MLP_MAX_HIDDEN];
    const float *w_out_a_t, *b_out_a;                    /* [hidden_size, N*C] */
    const float *w_out_x_t, *b_out_x;                    /* [hidden_size, N*d] */
    const float *w_out_l_t, *b_out_l;                    /* [hidden_size, d(d+1)/2] */
    const float* packed_image;                           /* optional (NULL allowed): all of the above re-laid out by
                                                            mdx_mlp_pack_image; lets a kernel stage the weights into
                                                            LDS with one coalesced copy */
    const float* folded_input;                           /* optional (NULL allowed): the five embedding layers folded
                                                            into hidden layer 0 (no activation lies between them), for the
                                                            input vector [cos 2 pi x (N d) | sin 2 pi x (N d) | sigma | t |
                                                            atom-type embeddings (N e_atom_type) | lattice embedding
                                                            (e_lattice)] of length F: ceil(F/4) x hidden_size weight
                                                            quads [q][neuron][4] (zero-padded), then the folded bias
                                                            [hidden_size].  Used by mdx_mlp_pc_sample for the template
                                                            network; same function, last-bit different rounding */
    const float* folded_output;                          /* optional, used together with folded_input: the last hidden
                                                            layer (no activation follows it) folded into the three heads:
                                                            ceil(hidden_size/4) x (N C + N d + d(d+1)/2) weight quads
                                                            [q][output][4] (outputs: logits | score_x | score_l), then the
                                                            folded bias */
    const float* folded_padded;                          /* optional (ABI v12): the folded layers zero-padded to fixed sizes,
                                                            for the register-resident family of mdx_mlp_pc_sample (hidden_size
                                                            <= 64, N <= 8, <= 64 outputs, F <= 192 folded inputs, 2 .. 4 hidden
                                                            layers): [FQ][64][4] + bias [64] with FQ = 16 ceil(F / 64) quads of
                                                            the folded first layer (neurons >= hidden_size and inputs >= F
                                                            zero) | per middle hidden layer [16][64][4] + bias [64] |
                                                            [16][64][4] + bias [64] of the folded output layer (outputs >= N C
                                                            + N d + d(d+1)/2 zero) */
} mdx_mlp_t;

/* Size (in floats) and construction of the packed weight image referenced by mdx_mlp_t.packed_image. */
MDX_API int64_t mdx_mlp_image_floats(const mdx_mlp_t* mlp_host);
MDX_API int mdx_mlp_pack_image(const mdx_mlp_t* mlp_host, float* image_out, mdx_stream_t stream);

/* ScoreNetwork.forward of the MLP (mlp_score_network.py:281-370 + score_network.py:183-185: MASK logit = -inf):
 * one wavefront per structure, activations in LDS.  time, sigma: [B,1].  The weights are staged into LDS -- one copy of the
 * packed image, or the same re-layout done in the kernel when packed_image is NULL (the same bits) -- when the image of
 * mdx_mlp_image_floats floats and the four wavefronts' regions fit 128 KiB of LDS together; a larger network is read from the
 * caller's tensors in global memory (the same function; a row's sum is rounded differently in its last, partial quad).
 * mdx_mlp_pc_sample applies the same limit. */
MDX_API int mdx_mlp_forward(const mdx_mlp_t* mlp_host, const int64_t* atom_types, const float* x, const float* l,
                            const float* time, const float* sigma, int64_t batch, float* logits_out,
                            float* score_x_out, float* score_l_out, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training the MLP score network (csrc/mdx_mlp_train.hip): the same cover as mdx_mlp_forward (MLPScoreNetwork._single,
 * unconditional, no permutation symmetrisation, no time prefactor; n_hidden <= MDX_MLP_MAX_HIDDEN, C <= MDX_MAX_CLASSES), on the
 * module's OWN parameters: nn.Linear layout, weight [out, in] and bias [out], float32, contiguous.  Nothing is copied or packed,
 * so an optimizer step between two calls is seen by the next one.
 *   shape_host int32 [MDX_MLP_TRAIN_SHAPE_COUNT], host memory: number_of_atoms N, spatial_dimension d, num_classes C,
 *       hidden_size H, n_hidden, then the embedding sizes e_coordinates, e_noise, e_time, e_atom_type, e_lattice.
 *       Below nd = N d, nl = d (d + 1) / 2, F0 = e_coordinates + e_noise + e_time + N e_atom_type + e_lattice.
 *   addresses uint64 [2 (5 + n_hidden + 3)], device memory: (weight, bias) of the layers in the order coordinates, noise, time,
 *       atom type, lattice embedding, hidden 0 .. n_hidden - 1, output A, X, L: the order named_parameters() gives the
 *       parameters the unconditional forward reads.  The flat gradient buffer holds them in this order, each tensor row-major:
 *       mdx_mlp_train_parameter_count floats.
 *
 * mdx_mlp_train_forward: one wavefront per structure, activations in LDS, a layer's weights staged transposed into LDS (odd row
 * length: no bank conflict in the store or in the layer loop), binary32 without contraction, the row sums and the SiLU of
 * mdx_mlp_forward.  time, sigma: [B, 1].  Writes the RAW head outputs -- logits [B, N, C] WITHOUT the -inf of the MASK class,
 * score_x [B, N, d], score_l [B, nl] -- and the activation record [B, mdx_mlp_train_record_floats], per structure, float32, the
 * value the forward fed to every Linear:
 *   cos 2 pi x [nd] | sin 2 pi x [nd] | sigma | time | atom classes [N] (as floats; clamped to [0, C)) | lattice [nl] |
 *   the concatenated features [F0] (input of hidden 0) | the input of hidden k [H], k = 1 .. n_hidden - 1 | the input of the
 *   heads [H] | the pre-activation z_k [H] of every hidden layer that goes through SiLU, k = 0 .. n_hidden - 2.
 * MDX_ERR_UNSUPPORTED when the largest staged layer and the wavefronts' vectors exceed 128 KiB of LDS.
 *
 * mdx_mlp_train_backward: the gradient of every parameter from the record and the three output cotangents (each nullable: a
 * part that is absent contributes nothing); no input gradient.  Two launches, no atomics, no ticket.
 *   1. One workgroup per slab of MDX_MLP_TRAIN_STRUCTURES_PER_SLAB consecutive structures.  Per structure, one wavefront, in
 *      binary64: delta_in[i] = sum_o W[o, i] delta[o] with o in index order, through the heads (A, X, L in that order), then per
 *      hidden layer times silu'(z) = s (1 + z (1 - s)), s = 1 / (1 + exp(-z)), from the saved binary32 z, down to the features.
 *      Then every gradient element, owned by one thread: dW[o, i] = sum_b delta_b[o] a_b[i], db[o] = sum_b delta_b[o] over the
 *      slab's structures in index order (the atom-type embedding: structures in order, each one's atoms in order, the one-hot
 *      input as 1.0 / 0.0), a_b the record's binary32 value widened -- delta is never rounded to binary32 -- into the slab's
 *      part of workspace f64 [mdx_mlp_train_workspace_doubles] = [ceil(B / slab), parameter count].
 *   2. Per element: the slabs in slab order, times scale, plus the buffer's old value when accumulate != 0, all in binary64,
 *      rounded to binary32 ONCE into gradients_inout.  Every element is written, every workspace entry is written first.
 * The same bits on every launch and under graph replay.  Non-finite values propagate; there is no status bit. */
#define MDX_MLP_TRAIN_SHAPE_COUNT 10
#define MDX_MLP_TRAIN_STRUCTURES_PER_SLAB 8
MDX_API int64_t mdx_mlp_train_record_floats(const int32_t* shape_host);
MDX_API int64_t mdx_mlp_train_parameter_count(const int32_t* shape_host);
MDX_API int64_t mdx_mlp_train_workspace_doubles(const int32_t* shape_host, int64_t batch);
MDX_API int mdx_mlp_train_forward(const int32_t* shape_host, const uint64_t* addresses, const int64_t* atom_types,
                                  const float* x, const float* l, const float* time, const float* sigma, int64_t batch,
                                  float* logits_out, float* score_x_out, float* score_l_out, float* record_out,
                                  mdx_stream_t stream);
MDX_API int mdx_mlp_train_backward(const int32_t* shape_host, const uint64_t* addresses, const float* record,
                                   const float* grad_logits, const float* grad_x, const float* grad_l, int64_t batch,
                                   double* workspace, int accumulate, double scale, float* gradients_inout,
                                   mdx_stream_t stream);

/* The whole sampling loop of LangevinGenerator.sample_from_noisy_composition
 * (generators/predictor_corrector_axl_generator.py:145-160 with langevin_generator.py:536-805) in ONE launch for an
 * MLP score network: every wavefront owns one structure, keeps its composition in LDS, and runs
 * `n_iterations` x (predictor + M correctors) -- network forward and fused update -- without returning to the host.
 * Device RNG only (the Philox specification makes it equal, draw for draw, to the per-step kernels).
 * The first iteration's predictor has time index `start_index`; the composition is updated in place.
 * noise_workspace (nullable, device, caller-owned, `workspace_floats` floats): when given, the draws of the segment
 * are generated ahead of the loop by a chip-filling pre-pass kernel into this buffer (same Philox counters, same
 * arithmetic => the same bits) and the persistent kernel only reads them; a workspace smaller than
 * mdx_mlp_pc_sample_workspace_floats(...) splits the segment into several launches.  NULL: every wavefront draws
 * in-kernel.
 * options: OR of the MDX_MLP_SAMPLE_* bits below (0 = the product path).  There are no environment variables: every
 * switch of this entry point is an explicit argument that the caller can print.
 * Record layout of the workspace (what MDX_MLP_SAMPLE_CALLER_NOISE expects the caller to have written), float32:
 *   [iteration it = 0 .. n_iterations-1][structure b][ predictor record rec0 | M corrector records rec1 ]
 *   rec0 = [ z N*d | gumbel N*C | u N | table 8 ]  (table[7] = 0: "no per-step posterior table", always valid)
 *   rec1 = rec0 if atom_type_transition_in_corrector else [ z N*d ]. */
#define MDX_MLP_SAMPLE_GENERIC_KERNEL 1u    /* never select a dimension-specialised instantiation                       */
#define MDX_MLP_SAMPLE_UNFOLDED 2u          /* layer-by-layer forward even when folded_input / folded_output are given
                                             * (the generic kernel too uses them, for any dimensions, when the folded first
                                             * layer is smaller than the two it replaces and the matrices fit in LDS)   */
#define MDX_MLP_SAMPLE_CALLER_NOISE 4u      /* noise_workspace already holds the records (parity tests replay the
                                               reference's recorded draws): the pre-pass is skipped; the whole segment
                                               must fit the workspace                                                    */
#define MDX_MLP_SAMPLE_NO_FIXED_SOFTMAX 8u  /* evaluate the clipped softmax per atom (bit-identical; tests)              */
#define MDX_MLP_SAMPLE_NO_P2_TABLE 16u      /* ignore the per-step posterior table of the records (bit-identical; tests) */
#define MDX_MLP_SAMPLE_PADDED_FAMILY 128u   /* prefer the padded register-resident family (any dimensions within its limits)
                                               to the exact-dimension one where both apply (A/B runs, tests)             */
#define MDX_MLP_SAMPLE_DIAG_NO_FORWARD 256u /* timing diagnostics, honoured only by a -DMDX_DIAGNOSTICS build of the     */
#define MDX_MLP_SAMPLE_DIAG_NO_UPDATE 512u  /* library; the release build returns MDX_ERR_UNSUPPORTED for them           */
MDX_API int64_t mdx_mlp_pc_sample_workspace_floats(const mdx_mlp_t* mlp_host, int number_of_corrector_steps,
                                                   int atom_type_transition_in_corrector, int n_iterations,
                                                   int64_t batch);
/* Which instantiation mdx_mlp_pc_sample runs for this network and these options: 0 = generic (any shape), 1 = the
 * reference template's dimensions as literals (layer by layer), 100 + 10 C + NH = the register-resident family with folded
 * input / output layers: N = 8, d = 3, hidden 64, embeddings 32/16/16/1/1, C in {2,3} classes, NH in {2,3,4} hidden layers
 * (needs folded_input and folded_output); 200 + 10 ceil(F / 64) + NH = the PADDED register-resident family (needs
 * folded_padded: hidden_size <= 64, N <= 8, <= 64 outputs, F <= 192 folded inputs, NH in {2,3,4}): every MLP configuration
 * of the reference's templates and experiments.  -1: invalid descriptor. */
MDX_API int mdx_mlp_pc_sample_variant(const mdx_mlp_t* mlp_host, uint32_t options);
MDX_API int mdx_mlp_pc_sample(const mdx_schedule_t* sched_host, const mdx_mlp_t* mlp_host,
                              const mdx_pc_flags_t* flags_host, int number_of_corrector_steps,
                              int atom_type_transition_in_corrector, int start_index, int n_iterations, mdx_rng_t rng,
                              int64_t batch, int64_t* atom_types, float* x, float* l, float* noise_workspace,
                              int64_t workspace_floats, uint32_t options, uint32_t* status, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * EGNN score network helpers (the forward stays a PyTorch module; these remove passes PyTorch cannot fuse).
 * (No vendor GEMM library behind this ABI: every matrix product of the library is a hand-written MFMA kernel; shapes the
 * edge chain does not cover stay plain PyTorch modules on the caller's side.) */

/* First layer of E_GCL.message_model (models/egnn.py:136-160) on an edge list [E,2] of node indices:
 * out[e,:] = act(node_proj[src_e, :H] + node_proj[dst_e, H:] + bias + radial[e] * w_radial), node_proj [n_nodes, 2H] being
 * the per-node projections h W_src^T | h W_dst^T of the layer's weight.  H % 4 == 0. */
MDX_API int mdx_egnn_message_input(const float* node_proj, const int64_t* edges, const float* radial, const float* bias,
                                   const float* w_radial, int64_t n_edges, int H, int silu, float* out,
                                   mdx_stream_t stream);

/* Segment operations on the radius graph's SORTED edge list: the edges of node i are rows
 * [offsets[i], offsets[i] + degree[i]) (what mdx_radius_graph_fill produces).  One wavefront per node, no atomics,
 * fixed summation order.  H % 4 == 0.
 * mdx_egnn_coord_head: trans[i,:] = (1/degree_i if mean) * sum_e coord_diff[e,:] * (hidden[e,:] . w_out) -- the last
 *   layer of E_GCL.coord_model (nn.Linear(H, 1, bias=False), models/egnn.py:162-200), the product with coord_diff and
 *   unsorted_segment_sum / _mean (models/egnn_utils.py:11-70) in one pass over hidden [E,H]; coord_diff [E,d] with
 *   d <= 64 (the EGNN works on uplifted coordinates, d = 6 for three spatial dimensions).
 * mdx_segment_rows: out[i,:] = (1/degree_i if mean) * sum_e data[e,:] -- the message aggregation of E_GCL.node_model
 *   (models/egnn.py:202-230). */
MDX_API int mdx_egnn_coord_head(const float* hidden, const float* w_out, const float* coord_diff, const int64_t* offsets,
                                const int64_t* degree, int64_t n_nodes, int H, int spatial_dimension, int mean,
                                float* trans, mdx_stream_t stream);
MDX_API int mdx_segment_rows(const float* data, const int64_t* offsets, const int64_t* degree, int64_t n_nodes, int H,
                             int mean, float* out, mdx_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused EGNN edge chain on the matrix cores (hand-written MFMA kernel, csrc/mdx_egnn_chain.hip; the per-node passes behind
 * it -- mdx_segment_combine, mdx_egnn_node_gather, mdx_egnn_coord_aggregate, mdx_egnn_table_gather -- are
 * csrc/mdx_egnn_node.hip): for every edge of the
 * SORTED edge list, the whole per-edge part of E_GCL.forward (models/egnn.py:136-200, 232-289) in one launch --
 *   x0  = SiLU(node_proj[src,:H] + node_proj[dst,H:] + bias_in + |coord_src - coord_dst|^2 w_radial)   (first message layer)
 *   x   = SiLU(x W_l^T + b_l), l = 0 .. n_message_layers-1                  -> messages_out [E,H]
 *   y   = SiLU(y W_l^T + b_l), l = n_message_layers .. +n_coord_layers-1    (coordinate MLP, all its H -> H layers)
 *   edge_scalar_out[e] = y . w_out                                          (its last layer, Linear(H, 1, bias=False))
 * The [E,H] activations stay in registers between layers (accumulator tile == next layer's MFMA operand).
 * hidden in {32, 64, 128, 256}; message and coordinate MLPs of equal width (a caller with narrower or unequal widths passes
 * zero-padded matrices, biases and vectors: a padded neuron computes SiLU(0) = 0 and feeds zeros on -- what the Python host
 * side does for the reference's default widths 16 / 32); SiLU activations.  E_GCL's options
 * (models/egnn.py:128-135, 148-160, 234-264):
 *   attention  attention_weight [H] / attention_bias [1] (device, both or neither): the messages are gated,
 *              m_e <- m_e sigmoid(m_e . attention_weight + attention_bias), between the message and the coordinate layers --
 *              messages_out and the coordinate MLP see the gated messages; instantiated for message_mode =
 *              MDX_EGNN_MESSAGES_PIECE_SUMS (MDX_ERR_UNSUPPORTED with MDX_EGNN_MESSAGES_ROWS);
 *   tanh, normalize  act where edge_scalar_out meets the coordinate difference: the coord_flags of mdx_egnn_node_gather /
 *              mdx_egnn_coord_aggregate (edge_scalar_out itself is the head's raw value).
 * precision 0: v_mfma_f32_32x32x2_f32, exact binary32 (== fmaf chains in a fixed order).
 * precision 1: split-f16, three v_mfma_f32_32x32x16_f16 per product (hi.hi + hi.lo + lo.hi), binary32 accumulation:
 *              ~2^-22 relative per product.  Both operands are held scaled by exact powers of two so that the f16 halves
 *              keep their 22 bits at small magnitudes: the image of layer l is 2^a_l W_l with the layer's largest |W| in
 *              [2^13, 2^14) (a_l chosen by mdx_egnn_chain_pack and written to weight_exponents), the activations carried
 *              between layers are 2^MDX_EGNN_F16_ACTIVATION_EXPONENT times their value; the kernel undoes both (exact).
 *              Sets MDX_STATUS_EGNN_F16_RANGE when an activation leaves the f16 range: |SiLU output| > ~709.
 * weight_image: the n_message_layers + n_coord_layers matrices [H,H] (nn.Linear layout; weights_host = host array of
 * device pointers) and the head's weight w_out [H], re-laid out by mdx_egnn_chain_pack for the chosen precision
 * (mdx_egnn_chain_image_bytes bytes, caller-owned, 16-byte aligned); the head rides the same pipeline as one more
 * 32-row chunk whose row 0 is w_out.
 * n_edges: number of edge rows to process = capacity of the outputs; n_edges_dev (nullable): device word with the actual
 * count (<= n_edges), for callers that size the edge list without reading it back. */
#define MDX_EGNN_CHAIN_MAX_LAYERS 16
#define MDX_EGNN_MESSAGES_ROWS 0        /* messages_out [E,H] = the messages                                            */
#define MDX_EGNN_MESSAGES_PIECE_SUMS 1  /* messages_out [mdx_egnn_piece_rows(E, n_nodes), H] = per-node piece sums      */
#define MDX_EGNN_F16_ACTIVATION_EXPONENT 6
typedef struct mdx_egnn_chain {
    int32_t hidden, n_message_layers, n_coord_layers, precision;
    int32_t message_mode, reserved;     /* MDX_EGNN_MESSAGES_*; reserved = 0 */
    const void* weight_image;
    const float* biases;       /* [n_message_layers + n_coord_layers, H] */
    const float* bias_in;      /* [H]  bias of the first message layer                       */
    const float* w_radial;     /* [H]  its weight column for the squared distance            */
    const int32_t* weight_exponents;   /* device, [packed layers + 1]: as written by mdx_egnn_chain_pack; required for
                                          precision 1, ignored (may be NULL) for precision 0 */
    /* Split-f16 precisions, nullable (NULL: MDX_EGNN_F16_ACTIVATION_EXPONENT everywhere): one power of two per POSITION of the
     * chain, device, [n_layers + 2], n_layers = n_message_layers + n_coord_layers.  Position q <= n_layers = the operand
     * entering layer q (0: the first layer's output / the rows handed in; n_layers: what leaves the last layer), position
     * n_layers + 1 = the rows read back in front of the projection layers of mdx_node_mlp_rows.  The activations carried at
     * position q are 2^e_q times their value; the f16 range is left at |value| > 65504 / 2^e_q (MDX_STATUS_EGNN_F16_RANGE).
     * mdx_node_mlp_rows treats positions 0 and 1 as one (position 0's exponent).  Read by the kernel at every launch: a
     * launch captured into a hipGraph follows later changes of the array. */
    const int32_t* activation_exponents;
    /* Precision 0, nullable: device, uint32 [n_layers + 2], the float bits of the largest |carried value| seen at each
     * position so far (atomic maxima; the caller zero-fills it) -- the input of mdx_egnn_chain_adapt_activation_exponents. */
    uint32_t* activation_maxima;
    /* E_GCL.att_mlp = Linear(H, 1) + Sigmoid, nullable (both or neither; mdx_egnn_edge_chain only): device, [H] and [1]. */
    const float* attention_weight;
    const float* attention_bias;
} mdx_egnn_chain_t;
#define MDX_EGNN_COORD_NORMALIZE 1   /* coord_diff <- tanh(r^2) / sqrt(r^2 + 1e-16) coord_diff   (E_GCL normalize=True)   */
#define MDX_EGNN_COORD_TANH 2        /* edge_scalar <- tanh(edge_scalar)                          (E_GCL tanh=True)        */
/* exponents_inout[q] = min(exponents_inout[q], e) with 2^e maxima[q] in [2^12, 2^13) (e clamped to [-14,
 * MDX_EGNN_F16_ACTIVATION_EXPONENT]) for every position with a recorded maximum; the maxima are zeroed.  Device-side, no host
 * synchronisation: what a caller runs after an exact-f32 pass that followed an MDX_STATUS_EGNN_F16_RANGE report, so that the
 * split-f16 kernels carry the hot positions with more headroom from then on. */
MDX_API int mdx_egnn_chain_adapt_activation_exponents(uint32_t* maxima_inout, int count, int32_t* exponents_inout,
                                                      mdx_stream_t stream);
MDX_API int64_t mdx_egnn_chain_image_bytes(int hidden, int n_layers);
/* tied_layers: bit l set = layer l uses the same power of two as layer l - 1 (the two H x H halves of a Linear(2H, H), whose
 * accumulators continue one another: mdx_node_mlp_rows).  exponents_out: device, [n_layers + 1] (last: the head row's);
 * required for precision 1; with precision 0 it is zero-filled when given.  No host synchronisation. */
MDX_API int mdx_egnn_chain_pack(const float* const* weights_host, int n_layers, const float* w_out, int hidden,
                                int precision, uint32_t tied_layers, void* image_out, int32_t* exponents_out,
                                mdx_stream_t stream);
MDX_API int mdx_egnn_edge_chain(const mdx_egnn_chain_t* chain_host, const float* node_proj, const float* coord,
                                int coord_dimension, const int64_t* edges, int64_t n_edges, const int64_t* n_edges_dev,
                                float* messages_out, float* edge_scalar_out, uint32_t* status, mdx_stream_t stream);
/* Message aggregation without the [E,H] round trip (the per-node side: csrc/mdx_egnn_node.hip): with message_mode = MDX_EGNN_MESSAGES_PIECE_SUMS the edge chain adds
 * the messages of a node's edges up INSIDE the kernel, per group of 16 consecutive edge rows (the list is sorted by source),
 * and writes only those sums, into a COMPACT buffer of mdx_egnn_piece_rows(n_edges, n_nodes) = ceil(n_edges / 16) + n_nodes
 * rows (n_edges = the capacity passed to mdx_egnn_edge_chain): the sum over the edges of node i inside group
 * [16 k, 16 k + 16) lands in row k when the group's last edge belongs to node i, otherwise -- the node's last edge is then
 * inside the group -- in the node's own row ceil(n_edges / 16) + i; every other row is left untouched.  No [E,H] buffer
 * exists in this mode (C3: 165 MB instead of 2.1 GB; C5 at 256 structures per GPU: 0.8 GB instead of 12.2 GB).
 * mdx_segment_combine (same n_edges) then gives out[i,:] = (1/degree_i if mean) sum of node i's pieces, read in edge order --
 * unsorted_segment_sum / _mean of the messages (models/egnn_utils.py:11-70) with a fixed summation order and no atomics; it
 * replaces mdx_segment_rows, reads ~2 rows per node instead of degree_i, and the messages themselves never reach memory.
 * Node indices must be < 2^31.
 * left (nullable, [n_nodes,H]): out is [n_nodes, 2H] = [left | sums] -- torch.cat([h, agg], dim=1), the input of the node
 * MLP (models/egnn.py:202-230), written in the same pass. */
MDX_API int64_t mdx_egnn_piece_rows(int64_t n_edges, int64_t n_nodes);
MDX_API int mdx_segment_combine(const float* pieces, int64_t n_edges, const int64_t* offsets, const int64_t* degree,
                                int64_t n_nodes, int H, int mean, const float* left, float* out, mdx_stream_t stream);
/* mdx_segment_combine and mdx_egnn_coord_aggregate (below) as ONE pass over the nodes -- everything E_GCL.forward does per node
 * between the per-edge chain and the node MLP (models/egnn.py:162-230: both unsorted_segment_sum / _mean calls, the product
 * with coord_diff, the coordinate residual, torch.cat([h, agg])): out = [left | message sums] (or the sums alone),
 * coord_out[i,:] = coord[i,:] + (1/degree_i if mean_coords) sum_e (coord[i,:] - coord[dst_e,:]) edge_scalar[e].  The node's
 * edges are dealt to the lanes of one wavefront and reduced by a butterfly: fixed order, no atomics.  coord_dimension <= 8.
 * coord_flags: MDX_EGNN_COORD_* bits (0 for the plain layer).
 * pieces = left = out = NULL: the coordinate half alone -- coord_out with the same bits, nothing else read or written (the
 * last graph layer of a forward whose atom-type logits nobody reads: its node features feed the classification head only). */
MDX_API int mdx_egnn_node_gather(const float* pieces, int64_t n_edges, const int64_t* offsets, const int64_t* degree,
                                 int64_t n_nodes, int H, int mean_messages, const float* left, float* out,
                                 const float* edge_scalar, const float* coord, int coord_dimension, const int64_t* edges,
                                 int mean_coords, int coord_flags, float* coord_out, mdx_stream_t stream);

/* The first graph layer of a sampler forward on a distance grid (the check: csrc/mdx_egnn_table.hip; the gather:
 * csrc/mdx_egnn_node.hip).  With one
 * sigma per batch the layer's per-edge output (messages [H] and the coordinate head's raw scalar) is a function F_ab(rho) of the
 * class pair (a, b) -- atom type, MASK = n_classes - 1 -- and of rho = sqrt(|c_i - c_j|^2).  `table` [n_classes^2 K, H] and
 * `table_scalar` [n_classes^2 K] are mdx_egnn_edge_chain's MDX_EGNN_MESSAGES_ROWS outputs on the grid problem: class pair
 * p = a n_classes + b owns rows [p K, p K + K), K = 2 n_even - 1; row p K + m is rho = m h (m < n_even), row p K + n_even + j the
 * cell midpoint rho = (j + 1/2) h (j < n_even - 1), h = 1 / inv_spacing.
 * mdx_egnn_table_check: the 4-point Lagrange interpolation of the even points at the midpoints j <= n_even - 3 against the
 *   chain's values there, per class pair and column (the scalar is column H), relative to the class pair's largest |value| over
 *   all its columns; ORs MDX_STATUS_EGNN_TABLE into status when an error exceeds `tolerance` or sigma[0 .. n_sigma) is not
 *   uniform.  workspace: device, uint32 [n_classes^2 (H + 2)], zero-filled once by the caller (the call leaves it zeroed);
 *   worst_out (nullable): device float [1], the largest relative error.  Two launches, no host synchronisation.
 * mdx_egnn_table_gather: the output contract of mdx_egnn_node_gather with the messages and scalars interpolated per edge from
 *   the table (even symmetry at rho = 0): out = [left | message sums] (or the sums), coord_out; atom_types [n_nodes] in
 *   [0, n_classes).  A distance beyond the grid or a class outside it ORs MDX_STATUS_EGNN_TABLE into status (nullable).
 *   H % 4 == 0, H <= 256, coord_dimension <= 8. */
MDX_API int mdx_egnn_table_check(const float* table, const float* table_scalar, int H, int n_classes, int n_even,
                                 const float* sigma, int64_t n_sigma, float tolerance, uint32_t* workspace, float* worst_out,
                                 uint32_t* status, mdx_stream_t stream);
/* The table memoised on the device.  It depends on sigma, the weights and the activation exponents only, and a sampler runs
 * three consecutive forwards at one sigma, so the caller keeps `table`, `table_scalar` and the grid's node_proj in buffers of
 * its own beside a KEY RECORD `table_key`: device, uint32 [2] = { the bits of the sigma the table in memory was built at
 * (MDX_EGNN_TABLE_NO_KEY: none), the number of builds so far (it only goes up) }.  Each kernel of a build first compares
 * table_key[0] with the bits of this forward's sigma[0] and returns at once when they agree (a NaN sigma never agrees): the
 * launches stay where they are -- in a captured graph too -- and only their work goes.
 *   mdx_egnn_node_inputs_keyed / mdx_egnn_edge_chain_keyed: the unkeyed calls with that early return (table_key nullable: the
 *     unkeyed call; the chain: MDX_EGNN_MESSAGES_ROWS without attention only).
 *   mdx_egnn_table_check_keyed: the midpoint check only when a build has happened, the uniform-sigma check ALWAYS; writes the key
 *     last -- the bits of sigma[0] and the counter + 1 when the build passed, MDX_EGNN_TABLE_NO_KEY when it failed (the next
 *     forward then builds and reports again).
 * The caller resets table_key[0] to MDX_EGNN_TABLE_NO_KEY (a fill on the stream) whenever something else the table depends on
 * changes. */
#define MDX_EGNN_TABLE_NO_KEY 0x7fc00000u
MDX_API int mdx_egnn_node_inputs_keyed(const float* x, const float* k_vectors, int n_k, const float* sigma,
                                       int atoms_per_structure, const int64_t* atom_types, const float* emb_weight,
                                       const float* emb_bias, int n_features, int H, int64_t n_nodes, float* z_out, float* h_out,
                                       const float* second_weight, const float* second_bias, int second_width, float* second_out,
                                       const uint32_t* table_key, mdx_stream_t stream);
MDX_API int mdx_egnn_edge_chain_keyed(const mdx_egnn_chain_t* chain_host, const float* node_proj, const float* coord,
                                      int coord_dimension, const int64_t* edges, int64_t n_edges, const int64_t* n_edges_dev,
                                      float* messages_out, float* edge_scalar_out, uint32_t* status, const uint32_t* table_key,
                                      const float* sigma, mdx_stream_t stream);
MDX_API int mdx_egnn_table_check_keyed(const float* table, const float* table_scalar, int H, int n_classes, int n_even,
                                       const float* sigma, int64_t n_sigma, float tolerance, uint32_t* workspace,
                                       float* worst_out, uint32_t* status, uint32_t* table_key, mdx_stream_t stream);
MDX_API int mdx_egnn_table_gather(const float* table, const float* table_scalar, int H, int n_classes, int n_even,
                                  float inv_spacing, const int64_t* atom_types, const int64_t* offsets, const int64_t* degree,
                                  int64_t n_nodes, int mean_messages, const float* left, float* out, const float* coord,
                                  int coord_dimension, const int64_t* edges, int mean_coords, int coord_flags, float* coord_out,
                                  uint32_t* status, mdx_stream_t stream);

/* EGNNScoreNetwork's per-node inputs and outputs around the EGNN (models/score_networks/egnn_score_network.py:253-290), one
 * launch each instead of a dozen elementwise passes (spatial dimension 3):
 *   mdx_egnn_node_inputs   z [n_nodes, 2 n_k] = (cos, sin)(2 pi x . K_k) interleaved -- the torus uplift of the relative
 *                          coordinates x [n_nodes,3] with the Bloch wave vectors K [n_k,3] -- and h [n_nodes,H] =
 *                          EGNN.embedding_in([sigma | one_hot(atom type)]) = b + sigma W[:,0] + W[:,1 + a]
 *                          (emb_weight [H, n_features] row-major, n_features = 2 + number of atom types; sigma [B] per
 *                          structure, atoms_per_structure nodes each; the same binary32 operations as the reference's).
 *                          An atom type outside [0, n_features - 2] contributes no column: h = b + sigma W[:,0];
 *                          h_out nullable (a caller that keeps one row of h per class): z, and second_out when given,
 *                          are written alone, with the same bits;
 *                          second_out (nullable, [n_nodes, second_width]): a second linear map of the same input,
 *                          b2 + sigma W2[:,0] + W2[:,1 + a] -- with W2 = P W, b2 = P b (formed by the caller) the first
 *                          graph layer's per-node projections P h without an [n_nodes,H] x [H,2H] product;
 *   mdx_egnn_scores        S^alpha = z . Gamma^alpha . x_hat, Gamma^alpha = blockdiag_k(K_k[alpha] [[0,-1],[1,0]]):
 *                          scores [n_nodes,3] from the EGNN's coordinate output x_hat [n_nodes, 2 n_k]. */
MDX_API int mdx_egnn_node_inputs(const float* x, const float* k_vectors, int n_k, const float* sigma, int atoms_per_structure,
                                 const int64_t* atom_types, const float* emb_weight, const float* emb_bias, int n_features,
                                 int H, int64_t n_nodes, float* z_out, float* h_out, const float* second_weight,
                                 const float* second_bias, int second_width, float* second_out, mdx_stream_t stream);
MDX_API int mdx_egnn_scores(const float* z, const float* x_hat, const float* k_vectors, int n_k, int64_t n_nodes,
                            float* scores_out, mdx_stream_t stream);

/* Everything behind the last graph layer in one launch: logits [n_nodes, num_classes] = EGNN.node_classification_layer(h)
 * (models/egnn.py:362-385; class_weight [num_classes, H] row-major, num_classes <= 8) with the logit of class `mask_class` set to
 * -inf (score_network.py:183-185; -1: none), the scores of mdx_egnn_scores, and n_zero zeros into zero_out (nullable with
 * n_zero = 0): the network's all-zero lattice output. */
MDX_API int mdx_egnn_outputs(const float* z, const float* x_hat, const float* k_vectors, int n_k, const float* h,
                             const float* class_weight, const float* class_bias, int H, int num_classes, int mask_class,
                             int64_t n_nodes, float* scores_out, float* logits_out, float* zero_out, int64_t n_zero,
                             mdx_stream_t stream);

/* The same pipeline over the ROWS of a matrix (the per-node MLP of an EGNN layer, models/egnn.py:202-230, after its first
 * layer): out[r,:] = residual[r,:] + W_L (SiLU(W_{L-1} ... SiLU(W_1 x[r,:] + b_1) ...)) + b_L -- L = chain->n_message_layers
 * layers of H x H (chain->n_coord_layers must be 0; bias_in / w_radial unused; image packed with w_out = NULL), every layer
 * but the last followed by SiLU; residual nullable; x, residual, out [n_rows, H] row-major; n_rows_dev nullable as above. */
MDX_API int mdx_mlp_chain_rows(const mdx_egnn_chain_t* chain_host, const float* x, const float* residual, int64_t n_rows,
                               const int64_t* n_rows_dev, float* out, uint32_t* status, mdx_stream_t stream);
/* The WHOLE per-node MLP of an EGNN layer (models/egnn.py:202-230) in one launch: node_in [n_rows, 2H] = [h | agg] (what
 * mdx_segment_combine writes with `left`), first layer Linear(2H, H) + SiLU, then H -> H layers as above, last one linear;
 * out[r,:] = (node_in[r,:H] if add_residual) + MLP(node_in[r,:]).  The chain holds the first layer's weight [H, 2H] as TWO
 * H x H layers -- W[:, :H] then W[:, H:] -- so n_message_layers = 1 + number of Linear modules (>= 3); biases [n, H]: row 0
 * the first layer's bias, row 1 unused.  The first half is multiplied with h, its raw accumulators wait in registers, the
 * second half with agg continues from them.
 * proj_out (nullable, [n_rows, 2H]): the image holds TWO MORE H x H layers behind the n_message_layers of the MLP -- the
 * source and destination halves of the NEXT graph layer's first message layer (models/egnn.py:136-160) -- and
 * proj_out[r,:] = [out[r,:] W_src^T | out[r,:] W_dst^T]: the node_proj input of that layer's mdx_egnn_edge_chain. */
MDX_API int mdx_node_mlp_rows(const mdx_egnn_chain_t* chain_host, const float* node_in, int add_residual, int64_t n_rows,
                              const int64_t* n_rows_dev, float* out, float* proj_out, uint32_t* status, mdx_stream_t stream);
/* The same with the two halves of the row as separate matrices, h [n_rows, H] and agg [n_rows, H] (what mdx_egnn_node_gather
 * writes with left = NULL): the concatenated [h | agg] never exists -- 134 MB less through HBM per layer at C3. */
MDX_API int mdx_node_mlp_rows_split(const mdx_egnn_chain_t* chain_host, const float* h, const float* agg, int add_residual,
                                    int64_t n_rows, const int64_t* n_rows_dev, float* out, float* proj_out, uint32_t* status,
                                    mdx_stream_t stream);
/* mdx_node_mlp_rows_split for an h with ONE value per class (the first graph layer inside a sampler: sigma is uniform over the
 * batch, so embedding_in([sigma | one_hot(a)]) has n_classes distinct rows): class_rows [n_classes, H], row_class int64
 * [n_rows]; row r's operand and residual are class_rows[row_class[r]] -- the [n_rows, H] matrix is neither written nor read.
 * The same arithmetic, tile order and epilogue: out and proj_out have the bits of the split call on h = class_rows[row_class].
 * A row_class outside [0, n_classes) reads row 0 and ORs MDX_STATUS_EGNN_TABLE into status (nullable); the call returns MDX_OK. */
MDX_API int mdx_node_mlp_rows_indexed(const mdx_egnn_chain_t* chain_host, const float* class_rows, int n_classes,
                                      const int64_t* row_class, const float* agg, int add_residual, int64_t n_rows,
                                      const int64_t* n_rows_dev, float* out, float* proj_out, uint32_t* status,
                                      mdx_stream_t stream);
/* coord_out[i,:] = coord[i,:] + (1/degree_i if mean) sum_{e in segment i} (coord[i,:] - coord[dst_e,:]) edge_scalar[e]
 * -- E_GCL.coord_model's trans = coord_diff * coord_mlp(m), unsorted_segment_sum / _mean and the residual add
 * (models/egnn.py:162-200), on the sorted segments; no atomics, fixed summation order. */
MDX_API int mdx_egnn_coord_aggregate(const float* edge_scalar, const float* coord, int coord_dimension, const int64_t* edges,
                                     const int64_t* offsets, const int64_t* degree, int64_t n_nodes, int mean,
                                     int coord_flags, float* coord_out, mdx_stream_t stream);

/* Device-RNG draws as stand-alone fills (trajectory initialisation, tests of the RNG specification).
 * kind 0 = uniform (0,1), 1 = standard normal, 2 = Gumbel(0,1).  out [n_items, width]. */
MDX_API int mdx_rng_fill(int kind, uint64_t seed, uint32_t call, uint32_t draw, uint32_t tag, int64_t n_items, int width,
                 float* out, mdx_stream_t stream);

/* MDX arithmetic probes (tests only): y = f(x) elementwise; fn 0 logf, 1 expf, 2 sinpi, 3 cospi (the software sequences of the
 * arithmetic contract); 4 cos(2 pi x), 5 sin(2 pi x) as the hardware instructions v_cos_f32 / v_sin_f32 give them, x in
 * revolutions -- what the folded forwards of mdx_mlp_pc_sample evaluate (not part of the bit-exact contract). */
MDX_API int mdx_math_probe(int fn, const float* x, int64_t count, float* y, mdx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MDX_HIP_H */
