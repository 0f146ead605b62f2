// Periodic pair kernels (gfx950 / CDNA4) and their C ABI: the 27-image radius graph, the force-field pseudo-force on the same
// structure tile and pair test, and the EGNN graph built in two passes.  See include/mdx_hip.h for the contract.
//
// Kernel inventory
//   radius_graph_kernel    N1  27-image radius graph, structure tile staged in LDS, one wavefront per source
//                              row, ballot/scan ranked writes => edges come out sorted, no atomics
//   force_field_kernel         the force-field wrapper's pseudo-force on N1's tile and pair test, no edge list:
//                              per-lane sums + a fixed cross-lane reduction, optional fused add to the score
//   offsets_scan_kernel        exclusive scan of the per-row edge counts (one workgroup) + the edge total
//   egnn_graph_mask_kernel     EGNN graph, pass 1: one workgroup per structure, per-row neighbour bit masks and counts
//   egnn_graph_emit_kernel     pass 2: offsets from the counts and the sorted edge list from the masks
//   excise_environments_kernel the active-learning excisors: one workgroup per central atom, binary64 image distances in LDS,
//                              slots by counting rank (distance, atom index), centring and embedding in the new box
//   edit_keep_mask_kernel      the sample edit: which generated atoms lie outside the radius around the active atom
//   random_fill_proposals_kernel    the excise-and-random maker's draws: binary64 uniforms, types and voxel occupancies of every
//                              attempt of every sample, Philox keyed by (seed, call, sample, attempt)
//   random_fill_environments_kernel one workgroup per sample: nearest-free-site placement of the constrained atoms, the
//                              structure, its least pair distance, retry until accepted -- all attempts in one launch
// 64-wide wavefronts are assumed throughout (gfx950).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_math.hpp"

using namespace mdx;

namespace {

// ---------------------------------------------------------------------------------------------------------------
// N1: radius graph
// ---------------------------------------------------------------------------------------------------------------
constexpr int kRowsPerBlock = 16;

__device__ __forceinline__ float crossing_distance(const float* cell)
{
    const float* a1 = cell; const float* a2 = cell + 3; const float* a3 = cell + 6;
    const float c12x = a1[1] * a2[2] - a1[2] * a2[1], c12y = a1[2] * a2[0] - a1[0] * a2[2], c12z = a1[0] * a2[1] - a1[1] * a2[0];
    const float c13x = a1[1] * a3[2] - a1[2] * a3[1], c13y = a1[2] * a3[0] - a1[0] * a3[2], c13z = a1[0] * a3[1] - a1[1] * a3[0];
    const float c23x = a2[1] * a3[2] - a2[2] * a3[1], c23y = a2[2] * a3[0] - a2[0] * a3[2], c23z = a2[0] * a3[1] - a2[1] * a3[0];
    const float vol = __builtin_fabsf((c12x * a3[0] + c12y * a3[1]) + c12z * a3[2]);
    const float n12 = __builtin_sqrtf((c12x * c12x + c12y * c12y) + c12z * c12z);
    const float n13 = __builtin_sqrtf((c13x * c13x + c13y * c13y) + c13z * c13z);
    const float n23 = __builtin_sqrtf((c23x * c23x + c23y * c23y) + c23z * c23z);
    float dmin = vol / n12;
    const float d2 = vol / n13;
    if (d2 < dmin) dmin = d2;
    const float d3 = vol / n23;
    if (d3 < dmin) dmin = d3;
    return dmin;
}

// Bit l of the result: image l (itertools.product(-1, 0, 1) order) of atom j lies within the cutoff of atom i, 0 < d^2 <= rc^2
// (neighbors.py:192-194 excludes coincident atoms as well as the atom itself).  `ortho`: the cell is diagonal with
// rc <= L_min / 2.2, so only the nearest image can qualify and ONE is evaluated, with the expression of the sweep: same bits.
__device__ __forceinline__ uint32_t images_within_cutoff(bool ortho, float pix, float piy, float piz, float pjx, float pjy, float pjz,
                                                         float inv_lx, float inv_ly, float inv_lz, float lx, float ly, float lz,
                                                         const float* lv, float rc2)
{
    uint32_t mask = 0;
    if (ortho) {
        const int nx = max(-1, min(1, (int)__builtin_rintf((pix - pjx) * inv_lx)));
        const int ny = max(-1, min(1, (int)__builtin_rintf((piy - pjy) * inv_ly)));
        const int nz = max(-1, min(1, (int)__builtin_rintf((piz - pjz) * inv_lz)));
        // image vector of a diagonal cell: n_k * L_k, exact, identical to the fma chain that fills lv[]
        const float sx = pjx + (float)nx * lx, sy = pjy + (float)ny * ly, sz = pjz + (float)nz * lz;
        const float dx = pix - sx, dy = piy - sy, dz = piz - sz;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (0.0f < d2 && d2 <= rc2) mask = (1u << ((nx + 1) * 9 + (ny + 1) * 3 + (nz + 1)));
    } else {
        // not unrolled: a full unroll hoists the 81 image-vector components into registers (113 VGPRs, half the
        // occupancy) for the benefit of the rare triclinic path
#pragma nounroll
        for (int l = 0; l < 27; ++l) {
            const float sx = pjx + lv[3 * l], sy = pjy + lv[3 * l + 1], sz = pjz + lv[3 * l + 2];
            const float dx = pix - sx, dy = piy - sy, dz = piz - sz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (0.0f < d2 && d2 <= rc2) mask |= (1u << l);
        }
    }
    return mask;
}

// images_within_cutoff(...) != 0 for a caller that does not need to know WHICH image: the image number stays a float (rint, then
// clamped to -1 .. 1 by a median) instead of going through an integer -- the same n, the same n * L, pj + n * L, pi - (...) and d^2,
// ten instructions fewer per pair.  (A NaN difference gives n = 0 there and an unspecified n here; d^2 is NaN either way: no hit.)
__device__ __forceinline__ bool any_image_within_cutoff(bool ortho, float pix, float piy, float piz, float pjx, float pjy, float pjz,
                                                        float inv_lx, float inv_ly, float inv_lz, float lx, float ly, float lz,
                                                        const float* lv, float rc2)
{
    if (!ortho) return images_within_cutoff(false, pix, piy, piz, pjx, pjy, pjz, inv_lx, inv_ly, inv_lz, lx, ly, lz, lv, rc2) != 0;
    const float nx = __builtin_amdgcn_fmed3f(__builtin_rintf((pix - pjx) * inv_lx), -1.0f, 1.0f);
    const float ny = __builtin_amdgcn_fmed3f(__builtin_rintf((piy - pjy) * inv_ly), -1.0f, 1.0f);
    const float nz = __builtin_amdgcn_fmed3f(__builtin_rintf((piz - pjz) * inv_lz), -1.0f, 1.0f);
    const float sx = pjx + nx * lx, sy = pjy + ny * ly, sz = pjz + nz * lz;
    const float dx = pix - sx, dy = piy - sy, dz = piz - sz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return 0.0f < d2 && d2 <= rc2;
}

// One workgroup = one (structure, chunk of kRowsPerBlock source rows).  The structure's positions and its 27
// image vectors are staged in LDS once; each wavefront then owns source rows and sweeps the destinations 64 at
// a time.  Lane ranks from ballot/scan make the writes dense and ordered by (src, dst, image).
template <bool FILL>
__global__ __launch_bounds__(kBlock) void radius_graph_kernel(const float* __restrict__ cart, const float* __restrict__ cell,
                                                              float rc, int64_t B, int N, int unique, int chunks,
                                                              int64_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                              int64_t* __restrict__ edges, int32_t* __restrict__ image_out,
                                                              float* __restrict__ shifts_out, uint32_t* status,
                                                              int64_t capacity, const float* __restrict__ lattice,
                                                              int lattice_stride, float clip_min)
{
    extern __shared__ float lds[];
    float* pos = lds;            // [N][3]
    float* lv = lds + 3 * N;     // [27][3]
    const int64_t b = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const float* P = cart + b * N * 3;
    // lattice != nullptr (the EGNN score network's graph, egnn_score_network.py:236-247): `cart` holds RELATIVE coordinates and
    // the cell is diag(max(lattice[b, k], clip_min)); relative x diagonal cell is one product per component -- the bits
    // torch.matmul(relative, diag_embed(lengths)) gives (its other terms are exact zeros)
    float cl[9];
    if (lattice) {
#pragma unroll
        for (int k = 0; k < 9; ++k) cl[k] = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = lattice[b * lattice_stride + k];
            cl[4 * k] = v < clip_min ? clip_min : v;          // torch.clip(min=): a NaN stays a NaN
        }
        for (int i = threadIdx.x; i < 3 * N; i += blockDim.x) {
            const int c = i % 3;
            pos[i] = P[i] * (c == 0 ? cl[0] : c == 1 ? cl[4] : cl[8]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) cl[k] = cell[b * 9 + k];
        for (int i = threadIdx.x; i < 3 * N; i += blockDim.x) pos[i] = P[i];
    }
    if (threadIdx.x < 81) {
        const int l = threadIdx.x / 3, c = threadIdx.x % 3;
        const float rel[3] = {(float)(l / 9 - 1), (float)((l / 3) % 3 - 1), (float)(l % 3 - 1)};
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = __builtin_fmaf(rel[k], c == 0 ? cl[k * 3] : c == 1 ? cl[k * 3 + 1] : cl[k * 3 + 2], acc);
        lv[threadIdx.x] = acc;
    }
    if (!FILL && chunk == 0 && threadIdx.x == 96 && status) {
        if (!(crossing_distance(cl) > rc)) atomicOr(status, MDX_STATUS_CUTOFF_TOO_LARGE);
    }
    // Orthorhombic cell with rc <= L_min / 2.2 (always true on the EGNN path, which clips the cell to 2.2 rc):
    // an image within rc has every component |delta_k| <= rc <= 0.4546 L_k, so it is THE nearest image and the
    // other 26 cannot qualify.  One image is then evaluated -- with the same expression, hence the same bits.
    const bool ortho = cl[1] == 0.0f && cl[2] == 0.0f && cl[3] == 0.0f && cl[5] == 0.0f && cl[6] == 0.0f &&
                       cl[7] == 0.0f && cl[0] > 0.0f && cl[4] > 0.0f && cl[8] > 0.0f &&
                       rc * 2.2f <= fminf(cl[0], fminf(cl[4], cl[8]));
    const float inv_lx = ortho ? 1.0f / cl[0] : 0.0f, inv_ly = ortho ? 1.0f / cl[4] : 0.0f,
                inv_lz = ortho ? 1.0f / cl[8] : 0.0f;
    __syncthreads();
    const float rc2 = rc * rc;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int row_end = min(N, (chunk + 1) * kRowsPerBlock);
    for (int i = chunk * kRowsPerBlock + wave; i < row_end; i += kBlock / kWave) {
        const float pix = pos[3 * i], piy = pos[3 * i + 1], piz = pos[3 * i + 2];
        const int64_t row = b * N + i;
        const int64_t base = FILL ? offsets[row] : 0;
        int64_t running = 0;
        for (int j0 = 0; j0 < N; j0 += kWave) {
            const int j = j0 + lane;
            uint32_t mask = 0;
            if (j < N)
                mask = images_within_cutoff(ortho, pix, piy, piz, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], inv_lx, inv_ly,
                                            inv_lz, cl[0], cl[4], cl[8], lv, rc2);
            int cnt, rank, total;
            if (unique) {
                cnt = (mask != 0);
                const unsigned long long hits = __ballot(cnt);
                rank = __popcll(hits & ((1ull << lane) - 1ull));
                total = __popcll(hits);
            } else {
                cnt = __popc(mask);
                int incl = cnt;                      // inclusive prefix over the lanes
#pragma unroll
                for (int o = 1; o < kWave; o <<= 1) {
                    const int v = __shfl_up(incl, o, kWave);
                    if (lane >= o) incl += v;
                }
                total = __shfl(incl, kWave - 1, kWave);
                rank = incl - cnt;
            }
            if (FILL && cnt) {
                int64_t e = base + running + rank;
                if (unique) {
                    longlong2 pair;
                    pair.x = row;
                    pair.y = row - i + j;
                    if (e < capacity) reinterpret_cast<longlong2*>(edges)[e] = pair;      // one 16-B store per edge
                } else {
                    uint32_t m = mask;
                    while (m && e < capacity) {
                        const int l = __ffs(m) - 1;
                        m &= m - 1;
                        longlong2 pair;
                        pair.x = i;
                        pair.y = j;
                        reinterpret_cast<longlong2*>(edges)[e] = pair;
                        image_out[e] = l;
                        if (shifts_out) {
                            shifts_out[3 * e] = lv[3 * l];
                            shifts_out[3 * e + 1] = lv[3 * l + 1];
                            shifts_out[3 * e + 2] = lv[3 * l + 2];
                        }
                        ++e;
                    }
                }
            }
            running += total;
        }
        if (!FILL && lane == 0) counts[row] = running;
        // a caller-sized edge list that is too small: nothing is written beyond it, and the caller is told
        if (FILL && lane == 0 && status && base + running > capacity) atomicOr(status, MDX_STATUS_GRAPH_CAPACITY);
    }
}

// The force-field wrapper's pseudo-force (force_field_augmented_score_network.py:86-236) straight from the coordinates: the
// staging, the image set and the hit predicate of radius_graph_kernel in its lattice mode (so the edges are the ones the full
// radius graph lists), and the reference's arithmetic per hit (i, j, image l):
//   disp = (p_j - p_i) + shift_l,  r = |disp|,  c = two_s (r - rc) / (r + 1e-8) disp
// Each lane sums its own hits; a fixed xor-butterfly over the 64 lanes then gives the row's sum, so a row depends on nothing but
// its structure.  F_rel = F_cart x (1 / L) (the reference's matmul with inverse(diag(L)): its off-diagonal terms are exact zeros)
// is rounded before the optional add of score_in -- the bits of raw.X + forces.  No edge list, no atomics, no workspace.
__global__ __launch_bounds__(kBlock) void force_field_kernel(const float* __restrict__ relative, const float* __restrict__ lattice,
                                                             int lattice_stride, float clip_min, float rc, float two_s, int N,
                                                             int chunks, const float* __restrict__ score_in,
                                                             float* __restrict__ out, uint32_t* status)
{
    extern __shared__ float lds[];
    float* pos = lds;            // [N][3]
    float* lv = lds + 3 * N;     // [27][3]
    const int64_t b = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks;
    const float* P = relative + b * N * 3;
    float cl[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) cl[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = lattice[b * lattice_stride + k];
        cl[4 * k] = v < clip_min ? clip_min : v;              // torch.clip(min=): a NaN stays a NaN
    }
    for (int i = threadIdx.x; i < 3 * N; i += blockDim.x) {
        const int c = i % 3;
        pos[i] = P[i] * (c == 0 ? cl[0] : c == 1 ? cl[4] : cl[8]);
    }
    if (threadIdx.x < 81) {
        const int l = threadIdx.x / 3, c = threadIdx.x % 3;
        const float rel[3] = {(float)(l / 9 - 1), (float)((l / 3) % 3 - 1), (float)(l % 3 - 1)};
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = __builtin_fmaf(rel[k], c == 0 ? cl[k * 3] : c == 1 ? cl[k * 3 + 1] : cl[k * 3 + 2], acc);
        lv[threadIdx.x] = acc;
    }
    if (chunk == 0 && threadIdx.x == 96 && status) {
        if (!(crossing_distance(cl) > rc)) atomicOr(status, MDX_STATUS_CUTOFF_TOO_LARGE);
    }
    const bool ortho = cl[0] > 0.0f && cl[4] > 0.0f && cl[8] > 0.0f && rc * 2.2f <= fminf(cl[0], fminf(cl[4], cl[8]));
    const float inv_lx = ortho ? 1.0f / cl[0] : 0.0f, inv_ly = ortho ? 1.0f / cl[4] : 0.0f,
                inv_lz = ortho ? 1.0f / cl[8] : 0.0f;
    // relative = cartesian x inverse(diag(L)): the reciprocal of the clipped length, then one product per component
    const float rx = 1.0f / cl[0], ry = 1.0f / cl[4], rz = 1.0f / cl[8];
    __syncthreads();
    const float rc2 = rc * rc;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int row_end = min(N, (chunk + 1) * kRowsPerBlock);
    for (int i = chunk * kRowsPerBlock + wave; i < row_end; i += kBlock / kWave) {
        const float pix = pos[3 * i], piy = pos[3 * i + 1], piz = pos[3 * i + 2];
        float fx = 0.0f, fy = 0.0f, fz = 0.0f;
        for (int j0 = 0; j0 < N; j0 += kWave) {
            const int j = j0 + lane;
            if (j >= N) continue;
            const float pjx = pos[3 * j], pjy = pos[3 * j + 1], pjz = pos[3 * j + 2];
            uint32_t m = images_within_cutoff(ortho, pix, piy, piz, pjx, pjy, pjz, inv_lx, inv_ly, inv_lz, cl[0], cl[4], cl[8],
                                              lv, rc2);
            while (m) {
                const int l = __ffs(m) - 1;
                m &= m - 1;
                const float dx = (pjx - pix) + lv[3 * l], dy = (pjy - piy) + lv[3 * l + 1], dz = (pjz - piz) + lv[3 * l + 2];
                const float r = __builtin_sqrtf((dx * dx + dy * dy) + dz * dz);
                const float c = two_s * (r - rc) / (r + 1.0e-8f);
                fx += c * dx;
                fy += c * dy;
                fz += c * dz;
            }
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {
            fx += __shfl_xor(fx, o, kWave);
            fy += __shfl_xor(fy, o, kWave);
            fz += __shfl_xor(fz, o, kWave);
        }
        if (lane == 0) {
            const int64_t row = (b * N + i) * 3;
            const float gx = fx * rx, gy = fy * ry, gz = fz * rz;
            out[row] = score_in ? score_in[row] + gx : gx;
            out[row + 1] = score_in ? score_in[row + 1] + gy : gy;
            out[row + 2] = score_in ? score_in[row + 2] + gz : gz;
        }
    }
}

// offsets[i] = counts[0] + ... + counts[i-1], *total = the sum: ONE workgroup walks the list in tiles of 16 384 entries (the list is
// the per-atom edge count of a batch -- 32 768 entries, two tiles, at C3; a launch of its own between the two radius-graph passes
// costs less than the three library launches of cumsum + subtraction it replaces).  A tile is kScanRows rows of 2 x kScanBlock
// entries; thread t owns entries 2t, 2t + 1 of every row, so each of its loads and stores is one coalesced 16-byte lane access
// (a thread owning 16 CONSECUTIVE entries made every wavefront-wide access touch 64 cache lines: 18 us instead of 6).  The sums
// inside a tile are 32-bit (an entry is the edge count of ONE atom: < 2^13 at the largest structure the radius graph takes,
// 16 384 of them < 2^27), the carry between tiles 64-bit.
constexpr int kScanBlock = 1024, kScanRows = 8, kScanWaves = kScanBlock / kWave;

// inclusive prefix sum over the 64 lanes with DPP adds (no LDS): within rows of 16 lanes, then lane 15 of rows 0 / 2 into rows
// 1 / 3, then lane 31 into the upper half
__device__ __forceinline__ int wave_inclusive_scan(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);      // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);      // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);      // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);      // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return x;
}

__global__ __launch_bounds__(kScanBlock) void offsets_scan_kernel(const int64_t* __restrict__ counts, int64_t n,
                                                                  int64_t* __restrict__ offsets, int64_t* __restrict__ total)
{
    // per (row, wavefront) sums of a tile, then their exclusive prefix in row-major order; [parity of the tile] so that a
    // wavefront one barrier ahead does not write what a slower one still reads
    __shared__ int sums[2][kScanRows * kScanWaves + 1];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    int64_t carry = 0;
    int parity = 0;
    for (int64_t base = 0; base < n; base += (int64_t)kScanRows * 2 * kScanBlock, parity ^= 1) {
        int* tile_sums = sums[parity];
        int v0[kScanRows], v1[kScanRows], incl[kScanRows];
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) {
            const int64_t i = base + ((int64_t)r * kScanBlock + threadIdx.x) * 2;
            if (i + 1 < n) {
                const longlong2 pair = *reinterpret_cast<const longlong2*>(counts + i);
                v0[r] = (int)pair.x;
                v1[r] = (int)pair.y;
            } else {
                v0[r] = i < n ? (int)counts[i] : 0;
                v1[r] = 0;
            }
        }
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) {
            incl[r] = wave_inclusive_scan(v0[r] + v1[r]);
            if (lane == kWave - 1) tile_sums[r * kScanWaves + wave] = incl[r];
        }
        __syncthreads();
        if (wave == 0) {
            // 128 sums, two per lane, in row-major order -> what lies before each of them in the tile; the tile's total behind
            static_assert(kScanRows * kScanWaves == 2 * kWave, "one wavefront scans the tile's sums two per lane");
            const int a = tile_sums[2 * lane], b = tile_sums[2 * lane + 1];
            const int through = wave_inclusive_scan(a + b);
            tile_sums[2 * lane] = through - a - b;
            tile_sums[2 * lane + 1] = through - b;
            if (lane == kWave - 1) tile_sums[kScanRows * kScanWaves] = through;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kScanRows; ++r) {
            const int64_t i = base + ((int64_t)r * kScanBlock + threadIdx.x) * 2;
            const int64_t first = carry + (tile_sums[r * kScanWaves + wave] + (incl[r] - v0[r] - v1[r]));
            if (i + 1 < n) {
                longlong2 pair;
                pair.x = first;
                pair.y = first + v0[r];
                *reinterpret_cast<longlong2*>(offsets + i) = pair;
            } else if (i < n) {
                offsets[i] = first;
            }
        }
        carry += tile_sums[kScanRows * kScanWaves];
    }
    if (threadIdx.x == 0) *total = carry;
}

// ---------------------------------------------------------------------------------------------------------------
// N1 as the EGNN score network builds it, in TWO launches: hit masks, then emission
// ---------------------------------------------------------------------------------------------------------------
// count -> scan -> fill evaluates every pair twice and puts a one-workgroup scan of B*N counts between two chip-wide launches.  Here
// the adjacency of a structure is kept as what the ballot already is -- one 64-bit word per (source row, 64 destinations) -- in a
// caller's workspace (N = 64: 512 bytes per structure); the second launch needs no positions and no arithmetic: it sums the totals
// of the structures before its own (B words), scans its N row counts, and turns the words into ordered 16-byte pairs.
// One workgroup per structure in both; a wavefront owns a CONTIGUOUS run of source rows, so its edges are one contiguous run of the
// list and the write position is a running sum.  Same pair test as radius_graph_kernel (images_within_cutoff): same edges, same order.
constexpr int kGraphMaxAtoms = 1024, kGraphMaxBatch = 2048;

template <int THREADS>
__global__ __launch_bounds__(THREADS) void egnn_graph_mask_kernel(const float* __restrict__ relative, const float* __restrict__ lattice,
                                                                   int lattice_stride, float clip_min, float rc, int N,
                                                                   int64_t* __restrict__ counts, unsigned long long* __restrict__ masks,
                                                                   int64_t* __restrict__ totals, uint32_t* status)
{
    extern __shared__ float lds[];
    float* pos = lds;                                    // [N][3]
    float* lv = lds + 3 * N;                             // [27][3]
    int* wave_total = reinterpret_cast<int*>(lv + 81);   // [THREADS / kWave]
    const int64_t b = blockIdx.x;
    const float* P = relative + b * N * 3;
    float cl[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) cl[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = lattice[b * lattice_stride + k];
        cl[4 * k] = v < clip_min ? clip_min : v;             // torch.clip(min=): a NaN stays a NaN
    }
    for (int i = threadIdx.x; i < 3 * N; i += THREADS) {
        const int c = i % 3;
        pos[i] = P[i] * (c == 0 ? cl[0] : c == 1 ? cl[4] : cl[8]);
    }
    if (threadIdx.x < 81) {
        const int l = threadIdx.x / 3, c = threadIdx.x % 3;
        const float rel[3] = {(float)(l / 9 - 1), (float)((l / 3) % 3 - 1), (float)(l % 3 - 1)};
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc = __builtin_fmaf(rel[k], c == 0 ? cl[k * 3] : c == 1 ? cl[k * 3 + 1] : cl[k * 3 + 2], acc);
        lv[threadIdx.x] = acc;
    }
    if (threadIdx.x == 96 && status) {
        if (!(crossing_distance(cl) > rc)) atomicOr(status, MDX_STATUS_CUTOFF_TOO_LARGE);
    }
    const bool ortho = cl[0] > 0.0f && cl[4] > 0.0f && cl[8] > 0.0f && rc * 2.2f <= fminf(cl[0], fminf(cl[4], cl[8]));
    const float inv_lx = ortho ? 1.0f / cl[0] : 0.0f, inv_ly = ortho ? 1.0f / cl[4] : 0.0f, inv_lz = ortho ? 1.0f / cl[8] : 0.0f;
    __syncthreads();
    const float rc2 = rc * rc;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int words = (N + kWave - 1) / kWave;                           // per source row
    const int rows = (N + THREADS / kWave - 1) / (THREADS / kWave);      // per wavefront, contiguous
    const int first = wave * rows, last = min(N, first + rows);
    int total = 0;
    if (N <= kWave) {
        // one word per row: the lane's destination atom stays in registers over the wavefront's rows
        const int j = lane < N ? lane : 0;
        const float pjx = pos[3 * j], pjy = pos[3 * j + 1], pjz = pos[3 * j + 2];
        for (int i = first; i < last; ++i) {
            const bool hit = any_image_within_cutoff(ortho, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2], pjx, pjy, pjz, inv_lx, inv_ly,
                                                     inv_lz, cl[0], cl[4], cl[8], lv, rc2);
            const unsigned long long hits = __ballot(lane < N && hit);
            const int count = __popcll(hits);
            if (lane == 0) {
                masks[b * N + i] = hits;
                counts[b * N + i] = count;
            }
            total += count;
        }
    } else
    for (int i = first; i < last; ++i) {
        const float pix = pos[3 * i], piy = pos[3 * i + 1], piz = pos[3 * i + 2];
        unsigned long long* row_words = masks + (b * N + i) * words;
        int count = 0;
        for (int w = 0; w < words; ++w) {
            const int j = w * kWave + lane;
            bool hit = false;
            if (j < N)
                hit = any_image_within_cutoff(ortho, pix, piy, piz, pos[3 * j], pos[3 * j + 1], pos[3 * j + 2], inv_lx, inv_ly,
                                              inv_lz, cl[0], cl[4], cl[8], lv, rc2);
            const unsigned long long hits = __ballot(hit);
            if (lane == 0) row_words[w] = hits;
            count += __popcll(hits);
        }
        if (lane == 0) counts[b * N + i] = count;
        total += count;
    }
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t sum = 0;
        for (int w = 0; w < THREADS / kWave; ++w) sum += wave_total[w];
        totals[b] = sum;
    }
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void egnn_graph_emit_kernel(int N, int64_t B, const int64_t* __restrict__ counts,
                                                                   const unsigned long long* __restrict__ masks,
                                                                   const int64_t* __restrict__ totals, int64_t* __restrict__ offsets,
                                                                   int64_t* __restrict__ n_edges, int64_t* __restrict__ edges,
                                                                   int64_t capacity, uint32_t* status)
{
    extern __shared__ int row_offset[];                  // [N + 1]: exclusive scan of the structure's row counts, the total behind
    __shared__ int64_t partial[THREADS / kWave];
    const int64_t b = blockIdx.x;
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
    const int words = (N + kWave - 1) / kWave;
    const int rows = (N + THREADS / kWave - 1) / (THREADS / kWave);
    const int first = min(N, wave * rows), last = min(N, first + rows);
    const int n_words = (last - first) * words;          // this wavefront's hit words: one contiguous run
    const unsigned long long* my_words = masks + (b * N + first) * words;
    unsigned long long held = lane < n_words ? my_words[lane] : 0ull;        // requested before anything waits
    // edges of the structures before this one
    int64_t before = 0;
    for (int64_t k = threadIdx.x; k < b; k += THREADS) before += totals[k];
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) before += __shfl_xor(before, o, kWave);
    if (lane == 0) partial[wave] = before;
    if (wave == 0) {
        int carry = 0;
        for (int c0 = 0; c0 < N; c0 += kWave) {
            const int i = c0 + lane;
            const int v = i < N ? (int)counts[b * N + i] : 0;
            const int incl = wave_inclusive_scan(v);
            if (i < N) row_offset[i] = carry + incl - v;
            carry += __shfl(incl, kWave - 1, kWave);
        }
        if (lane == 0) row_offset[N] = carry;
    }
    __syncthreads();
    int64_t base = 0;
#pragma unroll
    for (int w = 0; w < THREADS / kWave; ++w) base += partial[w];
    for (int i = threadIdx.x; i < N; i += THREADS) offsets[b * N + i] = base + row_offset[i];
    const int total = row_offset[N];
    if (threadIdx.x == 0) {
        if (b == B - 1) *n_edges = base + total;
        // a caller-sized edge list that is too small: nothing is written beyond it, and the caller is told
        if (status && base + total > capacity) atomicOr(status, MDX_STATUS_GRAPH_CAPACITY);
    }
    if (n_words == 0) return;
    int64_t e = base + row_offset[first];
    int64_t src = b * N + first;
    int w_in_row = 0;
    for (int c0 = 0; c0 < n_words; c0 += kWave) {
        if (c0) held = c0 + lane < n_words ? my_words[c0 + lane] : 0ull;
        const int limit = min(kWave, n_words - c0);
        for (int k = 0; k < limit; ++k) {
            const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)held, k), hi = __builtin_amdgcn_readlane((uint32_t)(held >> 32), k);
            const unsigned long long hits = ((unsigned long long)hi << 32) | lo;
            if ((hits >> lane) & 1ull) {
                const int64_t at = e + __popcll(hits & ((1ull << lane) - 1ull));
                longlong2 pair;
                pair.x = src;
                pair.y = b * N + w_in_row * kWave + lane;
                if (at < capacity) reinterpret_cast<longlong2*>(edges)[at] = pair;        // one 16-B store per edge
            }
            e += __popcll(hits);
            if (++w_in_row == words) { w_in_row = 0; ++src; }
        }
    }
}

template <int THREADS>
static void launch_graph_two_pass(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride, float clip_min,
                                  float rc, int64_t batch, int N, int64_t capacity, int64_t* counts, int64_t* offsets,
                                  int64_t* n_edges, int64_t* edges_out, uint32_t* status, uint64_t* workspace, hipStream_t stream)
{
    unsigned long long* masks = reinterpret_cast<unsigned long long*>(workspace);
    int64_t* totals = reinterpret_cast<int64_t*>(workspace) + batch * N * (int64_t)cdiv(N, kWave);
    const size_t lds = sizeof(float) * (3 * (size_t)N + 81) + sizeof(int) * (THREADS / kWave);
    hipLaunchKernelGGL(egnn_graph_mask_kernel<THREADS>, dim3((unsigned)batch), dim3(THREADS), lds, stream, relative_coordinates,
                       lattice_parameters, lattice_stride, clip_min, rc, N, counts, masks, totals, status);
    hipLaunchKernelGGL(egnn_graph_emit_kernel<THREADS>, dim3((unsigned)batch), dim3(THREADS), sizeof(int) * ((size_t)N + 1), stream,
                       N, batch, (const int64_t*)counts, (const unsigned long long*)masks, (const int64_t*)totals, offsets, n_edges,
                       edges_out, capacity, status);
}

// ---------------------------------------------------------------------------------------------------------------
// Environment excision and the sample edit (active_learning_loop/excisor/*.py, utils.py:98-135,
// sample_maker/base_sample_maker.py:221-299, excise_and_repaint_sample_maker.py:204-242): binary64, the reference's order
// ---------------------------------------------------------------------------------------------------------------
// get_distances_from_reference_point (utils.py:113-135) for one atom: Cartesian difference, per dimension the least of the three
// squared image differences, the sum in dimension order, the square root
__device__ __forceinline__ double image_distance_squared(const double* cart, const double* reference_cart, const double* side, int d)
{
    double sum = 0.0;
    for (int a = 0; a < d; ++a) {
        const double delta = cart[a] - reference_cart[a];
        double least = delta * delta;
        const double below = delta - side[a], above = delta + side[a];
        least = fmin(least, below * below);
        least = fmin(least, above * above);
        sum = a == 0 ? least : sum + least;
    }
    return sum;
}

__device__ __forceinline__ double image_distance(const double* cart, const double* reference_cart, const double* side, int d)
{
    return sqrt(image_distance_squared(cart, reference_cart, side, d));
}

struct ExciseArgs {
    const double *x, *side, *new_side;
    const int64_t* central;
    int N, d, mode, neighbours, center, capacity;
    double radius;
    int64_t* source;
    float* constrained_x;
    int32_t* counts;
    uint32_t* status;
};

// One workgroup per central atom.  LDS: the N distances (binary64) and the source atom of every output slot.  An atom's slot
// is its rank by (distance, atom index), found by counting -- no sort; in radius mode every atom closer than a member is a
// member, so the rank among all atoms is the rank among the members.
__global__ __launch_bounds__(kBlock) void excise_environments_kernel(ExciseArgs p)
{
    extern __shared__ double excise_lds[];
    double* dist = excise_lds;
    int* slot_source = reinterpret_cast<int*>(excise_lds + p.N);
    __shared__ int members;
    __shared__ uint32_t bits;
    const int e = blockIdx.x, N = p.N, d = p.d, cap = p.capacity;
    const int64_t c = p.central[e];
    int64_t* source = p.source + (int64_t)e * cap;
    float* out = p.constrained_x + (int64_t)e * cap * d;
    if (c < 0 || c >= N) {                                   // (the whole workgroup takes this branch: c is uniform)
        for (int s = threadIdx.x; s < cap; s += blockDim.x) {
            source[s] = 0;
            for (int a = 0; a < d; ++a) out[s * d + a] = 0.0f;
        }
        if (threadIdx.x == 0) {
            p.counts[e] = 0;
            if (p.status) atomicOr(p.status, MDX_STATUS_EXCISE_CENTRAL_INDEX);
        }
        return;
    }
    if (threadIdx.x == 0) { members = 0; bits = 0u; }
    for (int s = threadIdx.x; s < cap; s += blockDim.x) slot_source[s] = -1;     // (stays -1 only where NaN distances share a rank)
    double side[3], reference[3];
    for (int a = 0; a < d; ++a) {
        side[a] = p.side[a];
        reference[a] = p.x[c * d + a] * side[a];
    }
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        double cart[3];
        for (int a = 0; a < d; ++a) cart[a] = p.x[(int64_t)j * d + a] * side[a];
        dist[j] = image_distance(cart, reference, side, d);
    }
    __syncthreads();
    const int wanted = p.neighbours < N - 1 ? p.neighbours + 1 : N;         // nearest-neighbours mode: the centre and k more
    for (int j = threadIdx.x; j < N; j += blockDim.x) {
        const double dj = dist[j];
        if (p.mode == MDX_EXCISE_RADIUS && !(dj < p.radius)) continue;
        int rank = 0;
        for (int i = 0; i < N; ++i) {
            const double di = dist[i];
            rank += (di < dj || (di == dj && i < j)) ? 1 : 0;
        }
        if (p.mode == MDX_EXCISE_NEIGHBOURS && rank >= wanted) continue;
        atomicAdd(&members, 1);
        if (rank < cap) slot_source[rank] = j;
    }
    __syncthreads();
    const int count = members, kept = count < cap ? count : cap;
    for (int s = threadIdx.x; s < cap; s += blockDim.x) {
        if (s >= kept) {
            source[s] = 0;
            for (int a = 0; a < d; ++a) out[s * d + a] = 0.0f;
            continue;
        }
        const int j = slot_source[s];
        const int first = slot_source[0];                    // center_structure (base_excisor.py:65-70) centres slot 0
        if (j < 0 || first < 0) {
            source[s] = 0;
            for (int a = 0; a < d; ++a) out[s * d + a] = 0.0f;
            continue;
        }
        source[s] = j;
        bool outside = false;
        for (int a = 0; a < d; ++a) {
            double v = p.x[(int64_t)j * d + a];
            if (p.center) {
                v = v + (0.5 - p.x[(int64_t)first * d + a]);
                double r = fmod(v, 1.0);                     // numpy's mod: the sign of the divisor
                if (r != 0.0) { if (r < 0.0) r += 1.0; } else { r = 0.0; }
                v = r;
            }
            if (p.new_side) {                                // embed_structure_in_new_box (base_sample_maker.py:250-291)
                const double cart = (v - 0.5) * side[a] + 0.5 * p.new_side[a];
                if (!(cart < p.new_side[a] && cart > 0.0)) outside = true;
                v = cart * (1.0 / p.new_side[a]);            // the reference multiplies by the inverse cell
            }
            out[s * d + a] = (float)v;
        }
        if (outside) atomicOr(&bits, MDX_STATUS_EXCISE_OUTSIDE_BOX);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        p.counts[e] = count;
        uint32_t word = bits;
        if (count > cap) word |= MDX_STATUS_EXCISE_CAPACITY;
        if (p.status && word) atomicOr(p.status, word);
    }
}

struct EditMaskArgs {
    const float *x, *lattice;
    int lattice_stride;
    const int32_t *environment, *active, *counts;
    int64_t B;
    int N, d, E;
    double radius;
    uint8_t* keep;
};

__global__ __launch_bounds__(kBlock) void edit_keep_mask_kernel(EditMaskArgs p)
{
    const int64_t total = p.B * p.N;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = t / p.N;
        const int n = (int)(t - b * p.N);
        const int e = p.environment[b];
        const int active = e >= 0 && e < p.E ? p.active[e] : -1;
        if (active < 0 || active >= p.N || n < p.counts[e]) { p.keep[t] = 1; continue; }     // (no environment: nothing is edited)
        const float* row = p.x + b * p.N * p.d;
        double side[3], cart[3], reference[3];
        for (int a = 0; a < p.d; ++a) {
            side[a] = (double)p.lattice[b * p.lattice_stride + a];
            cart[a] = (double)row[n * p.d + a] * side[a];
            reference[a] = (double)row[active * p.d + a] * side[a];
        }
        p.keep[t] = image_distance(cart, reference, side, p.d) > p.radius ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The excise-and-random sample maker (active_learning_loop/sample_maker/excise_and_random_sample_maker.py:169-328)
// ---------------------------------------------------------------------------------------------------------------
struct ProposalArgs {
    uint64_t seed;
    uint32_t call;
    int64_t first_sample;
    int M, N, d, C, V;
    double* uniforms;
    int32_t *types, *voxels;
};

// a multiple of 2^-53 in [0, 1) from two Philox words: 27 high bits and 26 low bits
__device__ __forceinline__ double u01_binary64(uint32_t w0, uint32_t w1)
{
    return (double)(((uint64_t)(w0 >> 5) << 26) | (uint64_t)(w1 >> 6)) * 1.1102230246251565e-16;
}

// One workgroup per (sample, attempt).  LDS: one key per voxel, for the ranks of the voxels that the atoms of the last, partial
// round take (select_occupied_voxels, utils.py:203-212).
__global__ __launch_bounds__(kBlock) void random_fill_proposals_kernel(ProposalArgs p)
{
    extern __shared__ uint32_t proposal_keys[];
    const int64_t bm = blockIdx.x, b = bm / p.M;
    const uint32_t m = (uint32_t)(bm - b * p.M), sample = (uint32_t)(p.first_sample + b);
    const uint32_t k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32), call8 = p.call << 8;
    const int N = p.N, d = p.d, V = p.V;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        for (int a = 0; a < d; ++a) {
            const u32x4 r = philox4x32_10((uint32_t)n, call8 | (uint32_t)a, sample, (m << 8) | MDX_TAG_FILL_UNIFORM, k0, k1);
            p.uniforms[(bm * N + n) * d + a] = u01_binary64(r.v[0], r.v[1]);
        }
        const u32x4 r = philox4x32_10((uint32_t)n, call8, sample, (m << 8) | MDX_TAG_FILL_TYPE, k0, k1);
        p.types[bm * N + n] = (int32_t)__umulhi(r.v[0], (uint32_t)p.C);
    }
    if (!p.voxels) return;
    const int full = (N / V) * V, rest = N - full;
    for (int n = threadIdx.x; n < full; n += blockDim.x) p.voxels[bm * N + n] = n % V;
    if (rest == 0) return;                                   // (uniform over the workgroup)
    for (int v = threadIdx.x; v < V; v += blockDim.x)
        proposal_keys[v] = philox4x32_10((uint32_t)v, call8, sample, (m << 8) | MDX_TAG_FILL_VOXEL, k0, k1).v[0];
    __syncthreads();
    for (int v = threadIdx.x; v < V; v += blockDim.x) {
        const uint32_t key = proposal_keys[v];
        int rank = 0;
        for (int w = 0; w < V; ++w) {
            const uint32_t other = proposal_keys[w];
            rank += (other < key || (other == key && w < v)) ? 1 : 0;
        }
        if (rank < rest) p.voxels[bm * N + full + rank] = v;      // the ranks are a permutation: every slot is written once
    }
}

struct RandomFillArgs {
    const double *uniforms, *cx, *sides;
    const int32_t *types, *voxels, *counts, *active, *environment;
    const int64_t* ca;
    int E, K, N, d, M, voxel_mode;
    int partition[3];
    double threshold;
    double* x;
    int64_t* a;
    int32_t *active_out, *attempts;
    uint8_t* accepted;
    double* min_distance;
    uint32_t* status;
};

// is the pair (distance, index) `a` ahead of `b`: the smaller distance, the lower index among equal distances
__device__ __forceinline__ bool nearer(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// One workgroup per sample.  LDS: the N proposed sites and the N atoms of the structure (relative coordinates, binary64), the
// site behind every slot of the structure, one bit per taken site.  Every branch around a barrier is uniform over the
// workgroup: it depends on the sample's environment, the attempt and the decision thread 0 publishes.
__global__ __launch_bounds__(kBlock) void random_fill_environments_kernel(RandomFillArgs p)
{
    extern __shared__ double fill_lds[];
    constexpr int kWaves = kBlock / kWave;
    __shared__ double wave_best[kWaves];
    __shared__ int wave_index[kWaves];
    __shared__ double least_distance;
    __shared__ int decision;
    const int N = p.N, d = p.d, words = (N + 31) / 32;
    double* site = fill_lds;
    double* atom = fill_lds + (size_t)N * d;
    int* slot_site = reinterpret_cast<int*>(fill_lds + 2 * (size_t)N * d);
    uint32_t* taken = reinterpret_cast<uint32_t*>(slot_site + N);
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int e = p.environment[b];
    const bool known = e >= 0 && e < p.E;
    const int count = known ? p.counts[e] : 0;
    const int active = known ? p.active[e] : -1;
    double* out_x = p.x + b * N * d;
    int64_t* out_a = p.a + b * N;
    uint32_t bits = 0u;
    if (!known) bits = MDX_STATUS_RANDOM_FILL_ENVIRONMENT;
    else if (count > N || count > p.K) bits = MDX_STATUS_RANDOM_FILL_COUNT;
    else if (active < 0 || active >= count) bits = MDX_STATUS_RANDOM_FILL_ENVIRONMENT;       // (count < 1 ends here too)
    if (bits) {
        for (int s = tid; s < N; s += blockDim.x) {
            out_a[s] = 0;
            for (int a = 0; a < d; ++a) out_x[s * d + a] = 0.0;
        }
        if (tid == 0) {
            p.active_out[b] = 0; p.attempts[b] = 0; p.accepted[b] = 0; p.min_distance[b] = 0.0;
            if (p.status) atomicOr(p.status, bits);
        }
        return;
    }
    double side[3];
    for (int a = 0; a < d; ++a) side[a] = p.sides[e * d + a];
    const double* cx = p.cx + (int64_t)e * p.K * d;
    const double infinity = __builtin_inf();
    for (int m = 0; m < p.M; ++m) {
        const int64_t bm = b * p.M + m;
        // the sites of this attempt
        for (int n = tid; n < N; n += blockDim.x) {
            int v = p.voxel_mode ? p.voxels[bm * N + n] : 0;
            for (int a = d - 1; a >= 0; --a) {
                double value = p.uniforms[(bm * N + n) * d + a];
                if (p.voxel_mode) {
                    const int parts = p.partition[a], i = v % parts;
                    v /= parts;
                    value = (double)i * (1.0 / (double)parts) + value / (double)parts;
                }
                site[n * d + a] = value;
            }
        }
        for (int w = tid; w < words; w += blockDim.x) taken[w] = 0u;
        __syncthreads();
        // every constrained atom in order takes the nearest site still free
        for (int k = 0; k < count; ++k) {
            double reference[3];
            for (int a = 0; a < d; ++a) reference[a] = cx[k * d + a] * side[a];
            double best = infinity;
            int index = INT_MAX;
            for (int n = tid; n < N; n += blockDim.x) {
                if ((taken[n >> 5] >> (n & 31)) & 1u) continue;
                double cart[3];
                for (int a = 0; a < d; ++a) cart[a] = site[n * d + a] * side[a];
                const double distance = image_distance(cart, reference, side, d);
                if (nearer(distance, n, best, index)) { best = distance; index = n; }
            }
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) {
                const double other = __shfl_xor(best, o, kWave);
                const int other_index = __shfl_xor(index, o, kWave);
                if (nearer(other, other_index, best, index)) { best = other; index = other_index; }
            }
            if (lane == 0) { wave_best[wave] = best; wave_index[wave] = index; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < kWaves; ++w)
                    if (nearer(wave_best[w], wave_index[w], best, index)) { best = wave_best[w]; index = wave_index[w]; }
                if (index == INT_MAX)                        // only NaN distances: the lowest free site (count <= N: there is one)
                    for (index = 0; index < N - 1 && ((taken[index >> 5] >> (index & 31)) & 1u); ++index) {}
                taken[index >> 5] |= 1u << (index & 31);
                slot_site[k] = index;
            }
            __syncthreads();
        }
        // the structure: the constrained atoms, then the free sites in ascending order
        for (int s = tid; s < count; s += blockDim.x)
            for (int a = 0; a < d; ++a) atom[s * d + a] = cx[s * d + a];
        for (int n = tid; n < N; n += blockDim.x) {
            if ((taken[n >> 5] >> (n & 31)) & 1u) continue;
            int before = __popc(taken[n >> 5] & ((1u << (n & 31)) - 1u));
            for (int w = 0; w < (n >> 5); ++w) before += __popc(taken[w]);
            const int slot = count + n - before;
            slot_site[slot] = n;
            for (int a = 0; a < d; ++a) atom[slot * d + a] = site[n * d + a];
        }
        __syncthreads();
        // the least squared distance over the pairs i < j (the distance is symmetric, bit for bit)
        double least = infinity;
        for (int pair = tid; pair < N * N; pair += blockDim.x) {
            const int i = pair / N, j = pair - i * N;
            if (j <= i) continue;
            double first[3], second[3];
            for (int a = 0; a < d; ++a) { first[a] = atom[i * d + a] * side[a]; second[a] = atom[j * d + a] * side[a]; }
            least = fmin(least, image_distance_squared(second, first, side, d));
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) least = fmin(least, __shfl_xor(least, o, kWave));
        if (lane == 0) wave_best[wave] = least;
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < kWaves; ++w) least = fmin(least, wave_best[w]);
            least_distance = sqrt(least);
            decision = least_distance > p.threshold ? 1 : 0;
        }
        __syncthreads();
        if (decision || m == p.M - 1) {
            for (int s = tid; s < N; s += blockDim.x) {
                for (int a = 0; a < d; ++a) out_x[s * d + a] = atom[s * d + a];
                out_a[s] = s < count ? p.ca[(int64_t)e * p.K + s] : (int64_t)p.types[bm * N + slot_site[s]];
            }
            if (tid == 0) {
                p.active_out[b] = active; p.attempts[b] = m + 1; p.accepted[b] = (uint8_t)decision;
                p.min_distance[b] = least_distance;
            }
            return;
        }
    }
}

}  // namespace

// =================================================================================================================
// C ABI
// =================================================================================================================
extern "C" {

static int radius_graph_args_ok(const float* cart, const float* cell, float rc, int64_t batch, int N)
{
    if (batch < 0 || N < 1 || !(rc > 0.0f)) return MDX_ERR_INVALID_ARG;
    if (N > 5000) return MDX_ERR_UNSUPPORTED;    // structure tile (12 B per atom) kept under the 64 KiB default dynamic-LDS limit
    if (batch > 0 && (!cart || !cell)) return MDX_ERR_INVALID_ARG;
    return MDX_OK;
}

int mdx_radius_graph_count(const float* cart, const float* cell, float rc, int64_t batch, int N, int unique,
                           int64_t* counts, uint32_t* status, mdx_stream_t stream)
{
    const int ok = radius_graph_args_ok(cart, cell, rc, batch, N);
    if (ok != MDX_OK) return ok;
    if (batch == 0) return MDX_OK;
    if (!counts) return MDX_ERR_INVALID_ARG;
    const int chunks = (int)cdiv(N, kRowsPerBlock);
    const size_t lds = sizeof(float) * (3 * (size_t)N + 81);
    hipLaunchKernelGGL(radius_graph_kernel<false>, dim3((unsigned)(batch * chunks)), dim3(kBlock), lds, as_stream(stream),
                       cart, cell, rc, batch, N, unique, chunks, counts, (const int64_t*)nullptr, (int64_t*)nullptr,
                       (int32_t*)nullptr, (float*)nullptr, status, (int64_t)0, (const float*)nullptr, 0, 0.0f);
    return launch_status();
}

int mdx_radius_graph_fill_capped(const float* cart, const float* cell, float rc, int64_t batch, int N, int unique,
                                 const int64_t* offsets, int64_t capacity, int64_t* edges_out, int32_t* image_out,
                                 float* shifts_out, uint32_t* status, mdx_stream_t stream)
{
    const int ok = radius_graph_args_ok(cart, cell, rc, batch, N);
    if (ok != MDX_OK) return ok;
    if (capacity < 0) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return MDX_OK;
    if (!offsets || (capacity > 0 && !edges_out) || (!unique && capacity > 0 && !image_out)) return MDX_ERR_INVALID_ARG;
    const int chunks = (int)cdiv(N, kRowsPerBlock);
    const size_t lds = sizeof(float) * (3 * (size_t)N + 81);
    hipLaunchKernelGGL(radius_graph_kernel<true>, dim3((unsigned)(batch * chunks)), dim3(kBlock), lds, as_stream(stream),
                       cart, cell, rc, batch, N, unique, chunks, (int64_t*)nullptr, offsets, edges_out, image_out,
                       shifts_out, status, capacity, (const float*)nullptr, 0, 0.0f);
    return launch_status();
}

int64_t mdx_egnn_radius_graph_workspace_words(int64_t batch, int N)
{
    if (batch < 1 || N < 1 || N > kGraphMaxAtoms || batch > kGraphMaxBatch) return 0;
    return batch * N * (int64_t)cdiv(N, kWave) + batch;
}

int mdx_egnn_radius_graph(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride, float clip_min,
                          float rc, int64_t batch, int N, int64_t capacity, int64_t* counts, int64_t* offsets,
                          int64_t* n_edges, int64_t* edges_out, uint32_t* status, uint64_t* workspace, int64_t workspace_words,
                          mdx_stream_t stream)
{
    if (batch < 0 || N < 1 || !(rc > 0.0f) || capacity < 0 || lattice_stride < 3 || !(clip_min >= 0.0f)) return MDX_ERR_INVALID_ARG;
    if (N > 5000) return MDX_ERR_UNSUPPORTED;
    if (!n_edges) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return hipMemsetAsync(n_edges, 0, sizeof(int64_t), as_stream(stream)) == hipSuccess ? MDX_OK : MDX_ERR_HIP;
    if (!relative_coordinates || !lattice_parameters || !counts || !offsets || (capacity > 0 && !edges_out)) return MDX_ERR_INVALID_ARG;
    if (workspace_words < 0 || (workspace_words > 0 && !workspace)) return MDX_ERR_INVALID_ARG;
    const int64_t needed = mdx_egnn_radius_graph_workspace_words(batch, N);
    if (workspace && needed > 0) {
        if (workspace_words < needed) return MDX_ERR_INVALID_ARG;
        // sixteen wavefronts per structure while the launch still fits the chip at once (8 192 wavefront slots), four beyond
        if (N <= 16 || (N <= kWave && batch > 768))
            launch_graph_two_pass<256>(relative_coordinates, lattice_parameters, lattice_stride, clip_min, rc, batch, N, capacity,
                                       counts, offsets, n_edges, edges_out, status, workspace, as_stream(stream));
        else
            launch_graph_two_pass<1024>(relative_coordinates, lattice_parameters, lattice_stride, clip_min, rc, batch, N, capacity,
                                        counts, offsets, n_edges, edges_out, status, workspace, as_stream(stream));
        return launch_status();
    }
    const int chunks = (int)cdiv(N, kRowsPerBlock);
    const size_t lds = sizeof(float) * (3 * (size_t)N + 81);
    const dim3 grid((unsigned)(batch * chunks));
    hipLaunchKernelGGL(radius_graph_kernel<false>, grid, dim3(kBlock), lds, as_stream(stream), relative_coordinates,
                       (const float*)nullptr, rc, batch, N, 1, chunks, counts, (const int64_t*)nullptr, (int64_t*)nullptr,
                       (int32_t*)nullptr, (float*)nullptr, status, (int64_t)0, lattice_parameters, lattice_stride, clip_min);
    hipLaunchKernelGGL(offsets_scan_kernel, dim3(1), dim3(kScanBlock), 0, as_stream(stream), (const int64_t*)counts, batch * N,
                       offsets, n_edges);
    hipLaunchKernelGGL(radius_graph_kernel<true>, grid, dim3(kBlock), lds, as_stream(stream), relative_coordinates,
                       (const float*)nullptr, rc, batch, N, 1, chunks, (int64_t*)nullptr, (const int64_t*)offsets, edges_out,
                       (int32_t*)nullptr, (float*)nullptr, status, capacity, lattice_parameters, lattice_stride, clip_min);
    return launch_status();
}

int mdx_force_field_pseudo_force(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride,
                                 float clip_min, float rc, float two_strength, int64_t batch, int N, const float* score_in,
                                 float* out, uint32_t* status, mdx_stream_t stream)
{
    if (batch < 0 || N < 1 || !(rc > 0.0f) || lattice_stride < 3 || !(clip_min >= 0.0f)) return MDX_ERR_INVALID_ARG;
    if (N > 5000) return MDX_ERR_UNSUPPORTED;    // the structure tile in LDS, as the radius graph's
    if (batch == 0) return MDX_OK;
    if (!relative_coordinates || !lattice_parameters || !out) return MDX_ERR_INVALID_ARG;
    const int chunks = (int)cdiv(N, kRowsPerBlock);
    const size_t lds = sizeof(float) * (3 * (size_t)N + 81);
    hipLaunchKernelGGL(force_field_kernel, dim3((unsigned)(batch * chunks)), dim3(kBlock), lds, as_stream(stream),
                       relative_coordinates, lattice_parameters, lattice_stride, clip_min, rc, two_strength, N, chunks, score_in,
                       out, status);
    return launch_status();
}

int mdx_radius_graph_fill(const float* cart, const float* cell, float rc, int64_t batch, int N, int unique,
                          const int64_t* offsets, int64_t* edges_out, int32_t* image_out, float* shifts_out,
                          mdx_stream_t stream)
{
    return mdx_radius_graph_fill_capped(cart, cell, rc, batch, N, unique, offsets, INT64_MAX, edges_out, image_out, shifts_out,
                                        nullptr, stream);
}

int mdx_excise_environments(const double* relative_coordinates, const double* box_sides, int number_of_atoms, int spatial_dimension,
                            const int64_t* central_atoms, int number_of_environments, int mode, double radial_cutoff,
                            int number_of_neighbors, int center_atoms, const double* new_box_sides, int capacity,
                            int64_t* source_indices, float* constrained_x, int32_t* counts, uint32_t* status, mdx_stream_t stream)
{
    if (number_of_atoms < 1 || number_of_environments < 0 || capacity < 1) return MDX_ERR_INVALID_ARG;
    if (spatial_dimension < 1 || spatial_dimension > 3) return MDX_ERR_INVALID_ARG;
    if (mode != MDX_EXCISE_RADIUS && mode != MDX_EXCISE_NEIGHBOURS) return MDX_ERR_INVALID_ARG;
    if (mode == MDX_EXCISE_RADIUS ? !(radial_cutoff > 0.0) : number_of_neighbors < 1) return MDX_ERR_INVALID_ARG;
    if (number_of_atoms > MDX_EXCISE_MAX_ATOMS || capacity > MDX_EXCISE_MAX_ATOMS) return MDX_ERR_UNSUPPORTED;   // LDS: distances, slots
    if (number_of_environments == 0) return MDX_OK;
    if (!relative_coordinates || !box_sides || !central_atoms || !source_indices || !constrained_x || !counts)
        return MDX_ERR_INVALID_ARG;
    ExciseArgs a{};
    a.x = relative_coordinates; a.side = box_sides; a.new_side = new_box_sides; a.central = central_atoms;
    a.N = number_of_atoms; a.d = spatial_dimension; a.mode = mode; a.neighbours = number_of_neighbors;
    a.center = center_atoms ? 1 : 0; a.capacity = capacity; a.radius = radial_cutoff;
    a.source = source_indices; a.constrained_x = constrained_x; a.counts = counts; a.status = status;
    const size_t lds = sizeof(double) * (size_t)number_of_atoms + sizeof(int) * (size_t)capacity;
    hipLaunchKernelGGL(excise_environments_kernel, dim3((unsigned)number_of_environments), dim3(kBlock), lds, as_stream(stream), a);
    return launch_status();
}

int mdx_edit_keep_mask(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride,
                       const int32_t* sample_environment, const int32_t* active_atoms, const int32_t* counts,
                       int number_of_environments, double radius, int64_t batch, int number_of_atoms, int spatial_dimension, uint8_t* keep, mdx_stream_t stream)
{
    if (batch < 0 || number_of_atoms < 1 || spatial_dimension < 1 || spatial_dimension > 3) return MDX_ERR_INVALID_ARG;
    if (lattice_stride < spatial_dimension || !(radius >= 0.0) || number_of_environments < 0) return MDX_ERR_INVALID_ARG;
    if (batch == 0) return MDX_OK;
    if (!relative_coordinates || !lattice_parameters || !sample_environment || !active_atoms || !counts || !keep)
        return MDX_ERR_INVALID_ARG;
    EditMaskArgs a{};
    a.x = relative_coordinates; a.lattice = lattice_parameters; a.lattice_stride = lattice_stride;
    a.environment = sample_environment; a.active = active_atoms; a.counts = counts;
    a.B = batch; a.N = number_of_atoms; a.d = spatial_dimension; a.E = number_of_environments; a.radius = radius; a.keep = keep;
    hipLaunchKernelGGL(edit_keep_mask_kernel, dim3(flat_grid(batch * number_of_atoms)), dim3(kBlock), 0, as_stream(stream), a);
    return launch_status();
}

int mdx_random_fill_proposals(uint64_t seed, uint32_t call, int64_t first_sample, int64_t batch, int max_attempts,
                              int number_of_atoms, int spatial_dimension, int num_atom_types, int number_of_voxels, double* uniforms,
                              int32_t* types, int32_t* voxels, mdx_stream_t stream)
{
    if (batch < 0 || first_sample < 0 || max_attempts < 1 || number_of_atoms < 1 || num_atom_types < 1) return MDX_ERR_INVALID_ARG;
    if (spatial_dimension < 1 || spatial_dimension > 3 || number_of_voxels < 0) return MDX_ERR_INVALID_ARG;
    if ((number_of_voxels > 0) != (voxels != nullptr)) return MDX_ERR_INVALID_ARG;
    if (number_of_atoms > MDX_RANDOM_FILL_MAX_ATOMS || number_of_voxels > MDX_RANDOM_FILL_MAX_VOXELS) return MDX_ERR_UNSUPPORTED;
    if (call >= (1u << 24) || max_attempts >= (1 << 24) || first_sample + batch > 0x100000000LL) return MDX_ERR_UNSUPPORTED;
    if (batch * max_attempts > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;                     // one workgroup per (sample, attempt)
    if (batch == 0) return MDX_OK;
    if (!uniforms || !types) return MDX_ERR_INVALID_ARG;
    ProposalArgs a{};
    a.seed = seed; a.call = call; a.first_sample = first_sample; a.M = max_attempts; a.N = number_of_atoms;
    a.d = spatial_dimension; a.C = num_atom_types; a.V = number_of_voxels; a.uniforms = uniforms; a.types = types; a.voxels = voxels;
    hipLaunchKernelGGL(random_fill_proposals_kernel, dim3((unsigned)(batch * max_attempts)), dim3(kBlock),
                       sizeof(uint32_t) * (size_t)(number_of_voxels > 0 ? number_of_voxels : 1), as_stream(stream), a);
    return launch_status();
}

int mdx_random_fill_environments(const double* uniforms, const int32_t* types, const int32_t* voxels, const int32_t* partition,
                                 const double* constrained_x, const int64_t* constrained_a, const int32_t* counts,
                                 const int32_t* active, int number_of_environments, int constrained_capacity,
                                 const int32_t* sample_environment, const double* box_sides, int max_attempts,
                                 double minimal_interatomic_distance, int64_t batch, int number_of_atoms, int spatial_dimension,
                                 double* x, int64_t* a_out, int32_t* active_out, int32_t* attempts, uint8_t* accepted,
                                 double* min_distance, uint32_t* status, mdx_stream_t stream)
{
    if (batch < 0 || max_attempts < 1 || number_of_atoms < 2 || number_of_environments < 1 || constrained_capacity < 1)
        return MDX_ERR_INVALID_ARG;
    if (spatial_dimension < 1 || spatial_dimension > 3 || (partition != nullptr) != (voxels != nullptr)) return MDX_ERR_INVALID_ARG;
    if (!(minimal_interatomic_distance == minimal_interatomic_distance)) return MDX_ERR_INVALID_ARG;          // NaN
    if (number_of_atoms > MDX_RANDOM_FILL_MAX_ATOMS || constrained_capacity > MDX_RANDOM_FILL_MAX_ATOMS) return MDX_ERR_UNSUPPORTED;
    if (batch > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (batch == 0) return MDX_OK;
    if (!uniforms || !types || !constrained_x || !constrained_a || !counts || !active || !sample_environment || !box_sides)
        return MDX_ERR_INVALID_ARG;
    if (!x || !a_out || !active_out || !attempts || !accepted || !min_distance) return MDX_ERR_INVALID_ARG;
    RandomFillArgs r{};
    r.uniforms = uniforms; r.types = types; r.voxels = voxels; r.cx = constrained_x; r.ca = constrained_a; r.counts = counts;
    r.active = active; r.environment = sample_environment; r.sides = box_sides; r.E = number_of_environments;
    r.K = constrained_capacity; r.N = number_of_atoms; r.d = spatial_dimension; r.M = max_attempts;
    r.voxel_mode = partition ? 1 : 0;
    for (int k = 0; k < 3; ++k) r.partition[k] = 1;
    if (partition) {
        int64_t voxels_in_all = 1;
        for (int k = 0; k < spatial_dimension; ++k) {
            if (partition[k] < 1) return MDX_ERR_INVALID_ARG;
            r.partition[k] = partition[k];
            voxels_in_all *= partition[k];
            if (voxels_in_all > MDX_RANDOM_FILL_MAX_VOXELS) return MDX_ERR_UNSUPPORTED;
        }
    }
    r.threshold = minimal_interatomic_distance; r.x = x; r.a = a_out; r.active_out = active_out; r.attempts = attempts;
    r.accepted = accepted; r.min_distance = min_distance; r.status = status;
    const size_t lds = sizeof(double) * 2 * (size_t)number_of_atoms * spatial_dimension + sizeof(int) * (size_t)number_of_atoms +
                       sizeof(uint32_t) * (size_t)((number_of_atoms + 31) / 32);              // <= 53 376 B at the limits
    hipLaunchKernelGGL(random_fill_environments_kernel, dim3((unsigned)batch), dim3(kBlock), lds, as_stream(stream), r);
    return launch_status();
}

}  // extern "C"
