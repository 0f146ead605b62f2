// Stillinger-Weber energies and forces of a batch of periodic structures (LAMMPS `pair_style sw`, metal units): what the
// reference's energy oracle asks LAMMPS for (oracle/lammps_energy_oracle.py:56-158 through energy_oracle.py:44-131), as a closed
// formula over a periodic pair test like that of radius_graph_kernel / force_field_kernel.  The staging and the 27-image sweep
// here are other arithmetic, not a copy of theirs: binary64 positions from the raw sides, a cutoff per pair of types, three
// nested loops that leave an axis early.  See include/mdx_hip.h (mdx_stillinger_weber_energy_forces) for the contract.
//
//   stillinger_weber_kernel    one workgroup per structure, three phases separated by workgroup barriers:
//     0  stage: position = (double)relative * (double)side, atom types, the pair cutoffs a*sigma of the (ti,tj,tj) entries;
//        a side below the largest cutoff, a type outside the table or a non-finite coordinate ends the structure with NaNs
//     1  one wavefront per centre i: the 27-image sweep over all j, hits ranked by a lane scan, so the neighbour list of i
//        (displacement, j * 27 + image) is written to the workspace dense and sorted; the list cutoff is symmetric in (i, j),
//        so j lists i's opposite image with the exactly negated displacement
//     2  one wavefront per atom i, everything GATHERED (no float atomics): its halves of the pair terms, the triplets it is
//        the centre of, and -- for the force on it as an END atom -- the triplets of each neighbour centre c, read from c's
//        list.  Per-lane sums in a fixed order, a fixed xor-butterfly over the lanes, then the per-atom energies summed in a
//        fixed order: the same bits on every launch.
// 64-wide wavefronts are assumed (gfx950).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mdx_hip.h"
#include "mdx_launch.hpp"
#include "mdx_reduce.hpp"

using namespace mdx;

namespace {

constexpr int kWaves = kBlock / kWave;
constexpr int kMaxAtoms = 1024;
constexpr int kMaxTypes = 8;
constexpr int kSlot = 4;          // doubles per neighbour: dx, dy, dz, j * 27 + image
// columns of a parameter entry
constexpr int kEps = 0, kSigma = 1, kA = 2, kLambda = 3, kGamma = 4, kCos0 = 5, kBigA = 6, kBigB = 7, kP = 8, kQ = 9, kEntry = 10;
// reasons a structure ends with NaNs
constexpr int kSmallSide = 1, kBadType = 2, kOverflow = 4, kNotFinite = 8;

__device__ __forceinline__ const double* entry_of(const double* __restrict__ table, int n, int a, int b, int c)
{
    return table + (size_t)((a * n + b) * n + c) * kEntry;
}

// One leg of a triplet: displacement from the centre, its length, exp(gamma sigma / (r - a sigma)) and
// gamma sigma / (r - a sigma)^2 / r, with sigma, a, gamma of the (centre, end, end) entry.
struct Leg {
    double x, y, z, r, ex, slope;
};

__device__ __forceinline__ Leg make_leg(double x, double y, double z, double r, double cut, const double* __restrict__ pair_entry)
{
    Leg g;
    g.x = x; g.y = y; g.z = z; g.r = r;
    const double sg = pair_entry[kSigma] * pair_entry[kGamma];
    const double inv = 1.0 / (r - cut);
    g.ex = exp(sg * inv);
    g.slope = sg * inv * inv / r;
    return g;
}

// phi3 of the triplet (centre; legs 1, 2) with lambda, eps, cos theta0 of `triple`; f1 / f2: the forces on the end atoms of
// leg 1 / leg 2 (the centre takes -(f1 + f2)).
__device__ __forceinline__ double three_body(const Leg& a, const Leg& b, const double* __restrict__ triple, double* f1, double* f2)
{
    const double le = triple[kLambda] * triple[kEps];
    const double rinv12 = 1.0 / (a.r * b.r);
    const double cs = (a.x * b.x + a.y * b.y + a.z * b.z) * rinv12;
    const double delta = cs - triple[kCos0];
    const double strength = le * a.ex * b.ex;
    const double value = strength * delta * delta;
    const double facang = 2.0 * strength * delta;
    const double facang12 = facang * rinv12;
    const double c1 = value * a.slope + cs * facang / (a.r * a.r);
    const double c2 = value * b.slope + cs * facang / (b.r * b.r);
    f1[0] = a.x * c1 - b.x * facang12; f1[1] = a.y * c1 - b.y * facang12; f1[2] = a.z * c1 - b.z * facang12;
    f2[0] = b.x * c2 - a.x * facang12; f2[1] = b.y * c2 - a.y * facang12; f2[2] = b.z * c2 - a.z * facang12;
    return value;
}

__global__ __launch_bounds__(kBlock) void stillinger_weber_kernel(const float* __restrict__ relative, const float* __restrict__ lattice,
                                                                  int lattice_stride, const int64_t* __restrict__ atom_types,
                                                                  const double* __restrict__ table, int n_types, int N, int K,
                                                                  double* __restrict__ workspace, double* __restrict__ energies,
                                                                  double* __restrict__ forces, uint32_t* status)
{
    extern __shared__ double lds[];
    double* pos = lds;                                  // [N][3]
    double* e_atom = pos + 3 * N;                       // [N]
    double* cut = e_atom + N;                           // [kMaxTypes^2]: a sigma of entry (ti, tj, tj)
    int* type = reinterpret_cast<int*>(cut + kMaxTypes * kMaxTypes);   // [N]
    int* nn = type + N;                                 // [N]
    __shared__ int flags, overflow;
    const int64_t b = blockIdx.x;
    const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
    if (tid == 0) {
        flags = 0;
        overflow = 0;
    }
    double side[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) side[k] = (double)lattice[b * lattice_stride + k];
    for (int t = tid; t < n_types * n_types; t += kBlock) {
        const double* e = entry_of(table, n_types, t / n_types, t % n_types, t % n_types);
        cut[t] = e[kA] * e[kSigma];
    }
    __syncthreads();
    for (int i = tid; i < N; i += kBlock) {
        const int64_t t = atom_types[b * N + i];
        const bool known = t >= 0 && t < n_types;
        type[i] = known ? (int)t : 0;
        int bad = known ? 0 : kBadType;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double p = (double)relative[(b * N + i) * 3 + k] * side[k];
            pos[3 * i + k] = p;
            if (!finite_(p)) bad |= kNotFinite;
        }
        if (bad) atomicOr(&flags, bad);
    }
    if (tid == 0) {
        double largest = 0.0;
        for (int t = 0; t < n_types * n_types; ++t) largest = cut[t] > largest ? cut[t] : largest;
        // the +-1 sweep is complete only while every side reaches the largest cutoff (a NaN side fails the test too)
        if (!(side[0] >= largest && side[1] >= largest && side[2] >= largest)) atomicOr(&flags, kSmallSide);
    }
    __syncthreads();
    double* list = workspace + (size_t)b * N * K * kSlot;

    if (flags == 0) {
        // ---- phase 1: neighbour lists
        for (int i = wave; i < N; i += kWaves) {
            const double pix = pos[3 * i], piy = pos[3 * i + 1], piz = pos[3 * i + 2];
            const int ti = type[i];
            double* mine = list + (size_t)i * K * kSlot;
            int count = 0;
            for (int j0 = 0; j0 < N; j0 += kWave) {
                const int j = j0 + lane;
                uint32_t mask = 0;
                double djx = 0.0, djy = 0.0, djz = 0.0;
                if (j < N) {
                    const int tj = type[j];
                    const double c_ij = cut[ti * n_types + tj], c_ji = cut[tj * n_types + ti];
                    const double c = c_ij > c_ji ? c_ij : c_ji;
                    const double c2 = c * c;
                    djx = pos[3 * j] - pix; djy = pos[3 * j + 1] - piy; djz = pos[3 * j + 2] - piz;
                    for (int nx = 0; nx < 3; ++nx) {
                        const double dx = djx + (double)(nx - 1) * side[0];
                        if (!(__builtin_fabs(dx) < c)) continue;
                        for (int ny = 0; ny < 3; ++ny) {
                            const double dy = djy + (double)(ny - 1) * side[1];
                            if (!(__builtin_fabs(dy) < c)) continue;
                            for (int nz = 0; nz < 3; ++nz) {
                                const double dz = djz + (double)(nz - 1) * side[2];
                                const double r2 = (dx * dx + dy * dy) + dz * dz;
                                const int l = nx * 9 + ny * 3 + nz;
                                if (r2 < c2 && !(j == i && l == 13)) mask |= 1u << l;
                            }
                        }
                    }
                }
                const int cnt = __popc(mask);
                int incl = cnt;                          // inclusive prefix over the lanes
#pragma unroll
                for (int o = 1; o < kWave; o <<= 1) {
                    const int v = __shfl_up(incl, o, kWave);
                    if (lane >= o) incl += v;
                }
                const int total = __shfl(incl, kWave - 1, kWave);
                int slot = count + incl - cnt;
                while (mask) {
                    const int l = __ffs(mask) - 1;
                    mask &= mask - 1;
                    if (slot < K) {
                        double* out = mine + (size_t)slot * kSlot;
                        out[0] = djx + (double)(l / 9 - 1) * side[0];
                        out[1] = djy + (double)((l / 3) % 3 - 1) * side[1];
                        out[2] = djz + (double)(l % 3 - 1) * side[2];
                        out[3] = (double)(j * 27 + l);
                    }
                    ++slot;
                }
                count += total;
            }
            if (lane == 0) {
                nn[i] = count;
                if (count > K) atomicOr(&overflow, kOverflow);      // nothing is truncated: the structure ends with NaNs
            }
        }
    }
    __threadfence_block();
    __syncthreads();

    const int ended = flags | overflow;
    if (ended != 0) {
        const double nan = __builtin_nan("");
        if (tid == 0) {
            energies[b] = nan;
            const uint32_t bits = ((ended & kSmallSide) ? MDX_STATUS_CUTOFF_TOO_LARGE : 0u) |
                                  ((ended & kBadType) ? MDX_STATUS_SW_ATOM_TYPE : 0u) |
                                  ((ended & kOverflow) ? MDX_STATUS_SW_NEIGHBOURS : 0u);
            if (status && bits) atomicOr(status, bits);
        }
        if (forces)
            for (int i = tid; i < 3 * N; i += kBlock) forces[(size_t)b * N * 3 + i] = nan;
        return;
    }

    // ---- phase 2: per-atom energy and force
    for (int i = wave; i < N; i += kWaves) {
        const int ni = nn[i], ti = type[i];
        const double* mine = list + (size_t)i * K * kSlot;
        double e = 0.0, fx = 0.0, fy = 0.0, fz = 0.0;
        // this atom's half of each pair term
        for (int s = lane; s < ni; s += kWave) {
            const double dx = mine[s * kSlot], dy = mine[s * kSlot + 1], dz = mine[s * kSlot + 2];
            const int tj = type[(int)mine[s * kSlot + 3] / 27];
            const double r = sqrt((dx * dx + dy * dy) + dz * dz);
            const double c = cut[ti * n_types + tj];
            if (!(r < c)) continue;
            const double* p = entry_of(table, n_types, ti, tj, tj);
            const double sr = p[kSigma] / r;
            const double sp = pow(sr, p[kP]), sq = pow(sr, p[kQ]);
            const double inv = 1.0 / (r - c);
            const double ex = exp(p[kSigma] * inv);
            const double ae = p[kBigA] * p[kEps];
            const double value = ae * (p[kBigB] * sp - sq) * ex;
            const double slope = ae * (p[kQ] * sq - p[kP] * p[kBigB] * sp) / r * ex - value * p[kSigma] * inv * inv;
            e += 0.5 * value;
            const double g = slope / r;                  // F_i = +phi2'(r) d / r with d = r_j - r_i
            fx += g * dx; fy += g * dy; fz += g * dz;
        }
        // the triplets this atom is the centre of: first leg s1 (the same for every lane), second leg s2 > s1 over the lanes
        for (int s1 = 0; s1 < ni; ++s1) {
            const double ax = mine[s1 * kSlot], ay = mine[s1 * kSlot + 1], az = mine[s1 * kSlot + 2];
            const int tj = type[(int)mine[s1 * kSlot + 3] / 27];
            const double ra = sqrt((ax * ax + ay * ay) + az * az);
            const double ca = cut[ti * n_types + tj];
            if (!(ra < ca)) continue;
            const Leg first = make_leg(ax, ay, az, ra, ca, entry_of(table, n_types, ti, tj, tj));
            for (int s2 = s1 + 1 + lane; s2 < ni; s2 += kWave) {
                const double bx = mine[s2 * kSlot], by = mine[s2 * kSlot + 1], bz = mine[s2 * kSlot + 2];
                const int tk = type[(int)mine[s2 * kSlot + 3] / 27];
                const double rb = sqrt((bx * bx + by * by) + bz * bz);
                const double cb = cut[ti * n_types + tk];
                if (!(rb < cb)) continue;
                const Leg second = make_leg(bx, by, bz, rb, cb, entry_of(table, n_types, ti, tk, tk));
                double f1[3], f2[3];
                e += three_body(first, second, entry_of(table, n_types, ti, tj, tk), f1, f2);
                fx -= f1[0] + f2[0]; fy -= f1[1] + f2[1]; fz -= f1[2] + f2[2];
            }
        }
        // this atom as an END atom: for each neighbour centre c, every other leg of c (read from c's own list).  The leg towards
        // this atom is c's entry with the opposite image; the legs are ordered as in c's own sweep (by j * 27 + image).
        if (forces) {
            for (int s = 0; s < ni; ++s) {
                const int code = (int)mine[s * kSlot + 3];
                const int c = code / 27, l = code % 27;
                const int tc = type[c];
                const double ax = -mine[s * kSlot], ay = -mine[s * kSlot + 1], az = -mine[s * kSlot + 2];
                const double ra = sqrt((ax * ax + ay * ay) + az * az);
                const double ca = cut[tc * n_types + ti];
                if (!(ra < ca)) continue;
                const Leg towards = make_leg(ax, ay, az, ra, ca, entry_of(table, n_types, tc, ti, ti));
                const int own = i * 27 + (26 - l);
                const int nc = nn[c];
                const double* theirs = list + (size_t)c * K * kSlot;
                for (int u = lane; u < nc; u += kWave) {
                    const int other = (int)theirs[u * kSlot + 3];
                    if (other == own) continue;
                    const double bx = theirs[u * kSlot], by = theirs[u * kSlot + 1], bz = theirs[u * kSlot + 2];
                    const int tk = type[other / 27];
                    const double rb = sqrt((bx * bx + by * by) + bz * bz);
                    const double cb = cut[tc * n_types + tk];
                    if (!(rb < cb)) continue;
                    const Leg second = make_leg(bx, by, bz, rb, cb, entry_of(table, n_types, tc, tk, tk));
                    double f1[3], f2[3];
                    if (own < other) {
                        three_body(towards, second, entry_of(table, n_types, tc, ti, tk), f1, f2);
                        fx += f1[0]; fy += f1[1]; fz += f1[2];
                    } else {
                        three_body(second, towards, entry_of(table, n_types, tc, tk, ti), f1, f2);
                        fx += f2[0]; fy += f2[1]; fz += f2[2];
                    }
                }
            }
        }
        e = wave_sum(e);
        if (forces) {
            fx = wave_sum(fx); fy = wave_sum(fy); fz = wave_sum(fz);
        }
        if (lane == 0) {
            e_atom[i] = e;
            if (forces) {
                double* f = forces + ((size_t)b * N + i) * 3;
                f[0] = fx; f[1] = fy; f[2] = fz;
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        double e = 0.0;
        for (int i = lane; i < N; i += kWave) e += e_atom[i];
        e = wave_sum(e);
        if (lane == 0) energies[b] = e;
    }
}

}  // namespace

extern "C" {

int64_t mdx_stillinger_weber_workspace_doubles(int64_t batch, int number_of_atoms, int neighbour_capacity)
{
    if (batch < 0 || number_of_atoms < 1 || neighbour_capacity < 1) return 0;
    return batch * (int64_t)number_of_atoms * neighbour_capacity * kSlot;
}

int mdx_stillinger_weber_energy_forces(const float* relative_coordinates, const float* lattice_parameters, int lattice_stride,
                                       const int64_t* atom_types, const double* parameter_table, int n_types, int64_t batch,
                                       int number_of_atoms, int neighbour_capacity, double* workspace, int64_t workspace_doubles,
                                       double* energies, double* forces, uint32_t* status, mdx_stream_t stream)
{
    const int N = number_of_atoms;
    if (batch < 0 || N < 1 || n_types < 1 || lattice_stride < 3 || neighbour_capacity < 1) return MDX_ERR_INVALID_ARG;
    if (N > kMaxAtoms || n_types > kMaxTypes || batch > 0x7fffffffLL) return MDX_ERR_UNSUPPORTED;
    if (batch == 0) return MDX_OK;
    if (!relative_coordinates || !lattice_parameters || !atom_types || !parameter_table || !workspace || !energies)
        return MDX_ERR_INVALID_ARG;
    if (workspace_doubles < mdx_stillinger_weber_workspace_doubles(batch, N, neighbour_capacity)) return MDX_ERR_INVALID_ARG;
    const size_t lds = sizeof(double) * (4 * (size_t)N + kMaxTypes * kMaxTypes) + sizeof(int) * 2 * (size_t)N;
    hipLaunchKernelGGL(stillinger_weber_kernel, dim3((unsigned)batch), dim3(kBlock), lds, as_stream(stream), relative_coordinates,
                       lattice_parameters, lattice_stride, atom_types, parameter_table, n_types, N, neighbour_capacity, workspace,
                       energies, forces, status);
    return launch_status();
}

}  // extern "C"
