"""Tensor-level wrappers of the C ABI (include/mdx_hip.h).

Each function validates shapes, hands its tensors to the shared library through `_hip.call` -- which checks device, dtype
and contiguity of each against the header's parameter, appends torch's current HIP stream and raises on a non-zero status --
and returns torch tensors that PyTorch owns.  Nothing here computes on the CPU.
"""
import ctypes as C
import inspect
from collections import namedtuple
from dataclasses import dataclass
from functools import lru_cache
from typing import Any, Optional

import torch

from . import _hip
from ._hip import Mlp, PcFlags, Rng, Schedule, call, lib

F32, F64, I64, I32 = torch.float32, torch.float64, torch.int64, torch.int32


# ----------------------------------------------------------------------------------------------------------------
# S1
# ----------------------------------------------------------------------------------------------------------------
@dataclass
class DeviceSchedule:
    """Device-resident schedule tables + the mdx_schedule_t view handed to the kernels."""

    total_time_steps: int
    num_classes: int
    sigma_min: float
    time: torch.Tensor
    sigma: torch.Tensor
    sigma_squared: torch.Tensor
    g: torch.Tensor
    g_squared: torch.Tensor
    epsilon: torch.Tensor
    sqrt_2_epsilon: torch.Tensor
    beta: torch.Tensor
    alpha_bar: torch.Tensor
    q_matrix: torch.Tensor
    q_bar_matrix: torch.Tensor
    q_bar_tm1_matrix: torch.Tensor

    def __post_init__(self):
        self.c_struct = Schedule(self.total_time_steps, self.num_classes, float(self.sigma_min),
                                 self.time.data_ptr(), self.sigma.data_ptr(), self.g.data_ptr(),
                                 self.g_squared.data_ptr(), self.epsilon.data_ptr(), self.q_matrix.data_ptr(),
                                 self.q_bar_matrix.data_ptr(), self.q_bar_tm1_matrix.data_ptr())

    @property
    def device(self):
        return self.time.device


def noise_schedule_build(total_time_steps: int, schedule_type: str, time_delta: float, sigma_min: float,
                         sigma_max: float, corrector_step_epsilon: float, num_classes: int,
                         device: torch.device) -> DeviceSchedule:
    """S1: build the variance-exploding schedule tables on the device (mdx_noise_schedule_build)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _hip.MdxError(f"schedule tables are built on the GPU; got device {device}")
    T, Cn = int(total_time_steps), int(num_classes)
    st = {"exponential": 0, "linear": 1}[schedule_type]
    with torch.cuda.device(device):
        vec = [torch.empty(T, dtype=F32, device=device) for _ in range(9)]
        mats = [torch.empty(T, Cn, Cn, dtype=F32, device=device) for _ in range(3)]
        call("mdx_noise_schedule_build", T, st, float(time_delta), float(sigma_min), float(sigma_max),
             float(corrector_step_epsilon), Cn, *vec, *mats)
    time, sigma, sigma2, g, g2, eps, s2e, beta, ab = vec
    q, qb, qbm = mats
    return DeviceSchedule(T, Cn, float(sigma_min), time, sigma, sigma2, g, g2, eps, s2e, beta, ab, q, qb, qbm)


# ----------------------------------------------------------------------------------------------------------------
# step index / network inputs
# ----------------------------------------------------------------------------------------------------------------
def index_set(d_index: torch.Tensor, value: int):
    call("mdx_index_set", d_index, int(value))


def index_add(d_index: torch.Tensor, delta: int):
    call("mdx_index_add", d_index, int(delta))


def fill_time_sigma(sched: DeviceSchedule, mode: int, index_i: int, d_index: Optional[torch.Tensor],
                    time_out: torch.Tensor, sigma_out: torch.Tensor):
    batch = time_out.numel()
    assert sigma_out.numel() == batch
    call("mdx_fill_time_sigma", C.byref(sched.c_struct), mode, int(index_i), d_index, time_out, sigma_out, batch)


# ----------------------------------------------------------------------------------------------------------------
# P1 / P2 / P3 with explicit operands (mirror the reference's private update methods)
# ----------------------------------------------------------------------------------------------------------------
def relative_coordinates_update(x, s, z, score_weight=None, gaussian_noise_weight=None, sigma=None, out=None, weights=None):
    """P1.  The three scalars as host numbers, or -- `weights`, float32 [3] on the device: {score weight, noise weight,
    sigma} -- read by the kernel (no host synchronisation: AdaptiveCorrectorGenerator)."""
    assert x.shape == s.shape == z.shape
    out = torch.empty_like(x) if out is None else out
    if weights is not None:
        assert weights.numel() == 3
        call("mdx_relative_coordinates_update_dev", x, s, z, weights, x.numel(), out)
        return out
    call("mdx_relative_coordinates_update", x, s, z, float(score_weight), float(gaussian_noise_weight), float(sigma), x.numel(), out)
    return out


def lattice_parameters_update(l, s, z, score_weight=None, gaussian_noise_weight=None, sigma_n=None, out=None, weights=None):
    """P3; `weights` as in relative_coordinates_update."""
    assert l.shape == s.shape == z.shape
    out = torch.empty_like(l) if out is None else out
    if weights is not None:
        assert weights.numel() == 3
        call("mdx_lattice_parameters_update_dev", l, s, z, weights, l.numel(), out)
        return out
    call("mdx_lattice_parameters_update", l, s, z, float(score_weight), float(gaussian_noise_weight), float(sigma_n), l.numel(), out)
    return out


def atom_types_update(logits, atom_types, q, q_bar, q_bar_tm1, gumbel, u, small_epsilon: float, greedy: bool,
                      one_transition: bool, return_probabilities: bool = False):
    B, N, Cn = logits.shape
    assert atom_types.shape == (B, N) and gumbel.shape == (B, N, Cn)
    assert q.shape == q_bar.shape == q_bar_tm1.shape == (Cn, Cn)
    out = torch.empty_like(atom_types)
    p_out = torch.empty_like(logits) if return_probabilities else None
    call("mdx_atom_types_update", logits, atom_types, q, q_bar, q_bar_tm1, gumbel, u, B, N, Cn, float(small_epsilon),
         int(bool(greedy)), int(bool(one_transition)), out, p_out)
    return (out, p_out) if return_probabilities else out


# ----------------------------------------------------------------------------------------------------------------
# fused per-step update
# ----------------------------------------------------------------------------------------------------------------
def pc_step_update(sched: DeviceSchedule, mode: int, index_i: int, d_index: Optional[torch.Tensor], flags: PcFlags,
                   atom_types, x, l, logits, score_x, score_l, z_coordinates, gumbel, u, z_lattice, rng: Rng,
                   atom_types_out, x_out, l_out, status: Optional[torch.Tensor]):
    B, N, d = x.shape
    call("mdx_pc_step_update", C.byref(sched.c_struct), int(mode), int(index_i), d_index, C.byref(flags), atom_types, x, l,
         logits, score_x, score_l, z_coordinates, gumbel, u, z_lattice, rng, B, N, d, atom_types_out, x_out, l_out, status)


# ----------------------------------------------------------------------------------------------------------------
# adaptive corrector: batch statistics -> step size -> update (no host read in between)
# ----------------------------------------------------------------------------------------------------------------
def adaptive_corrector_statistics(sched: DeviceSchedule, index_i: int, d_index: Optional[torch.Tensor], score_x, score_l,
                                  z_coordinates, z_lattice_for_step_size, rng: Rng, use_fixed_lattice_parameters: bool,
                                  corrector_r: float, small_epsilon: float, workspace, totals, weights=None):
    """Stage 1 (mdx_adaptive_corrector_statistics): per-structure norms into workspace float32 [B,4], their fixed-order
    binary64 sums and counts into totals float64 [8]; with `weights` (float32 [6]) the step size follows in the same launch.
    A None z is regenerated in registers from `rng`."""
    B, N, d = score_x.shape
    assert workspace.numel() == 4 * B and totals.numel() == 8 and (weights is None or weights.numel() == 6)
    call("mdx_adaptive_corrector_statistics", C.byref(sched.c_struct), int(index_i), d_index, score_x, score_l, z_coordinates,
         z_lattice_for_step_size, rng, B, N, d, int(bool(use_fixed_lattice_parameters)), float(corrector_r),
         float(small_epsilon), workspace, totals, weights)


def adaptive_corrector_step_size(sched: DeviceSchedule, index_i: int, d_index: Optional[torch.Tensor], totals,
                                 number_of_atoms: int, spatial_dimension: int, use_fixed_lattice_parameters: bool,
                                 corrector_r: float, small_epsilon: float, weights):
    """Stage 2 (mdx_adaptive_corrector_step_size): weights float32 [6] = {eps, sqrt(2 eps), sigma, eps_L, sqrt(2 eps_L),
    sigma_n} from totals float64 [8] (all-reduced by the caller when the batch is sharded)."""
    assert totals.numel() == 8 and weights.numel() == 6
    call("mdx_adaptive_corrector_step_size", C.byref(sched.c_struct), int(index_i), d_index, totals, int(number_of_atoms),
         int(spatial_dimension), int(bool(use_fixed_lattice_parameters)), float(corrector_r), float(small_epsilon), weights)


def adaptive_corrector_update(sched: DeviceSchedule, mode: int, index_i: int, d_index: Optional[torch.Tensor], flags: PcFlags,
                              atom_types, x, l, logits, score_x, score_l, z_coordinates, gumbel, u, z_lattice, weights,
                              rng: Rng, atom_types_out, x_out, l_out, status: Optional[torch.Tensor]):
    """Stage 3 (mdx_adaptive_corrector_update): pc_step_update's operands; corrector: scalars from `weights`; predictor: atom
    types only."""
    B, N, d = x.shape
    call("mdx_adaptive_corrector_update", C.byref(sched.c_struct), int(mode), int(index_i), d_index, C.byref(flags), atom_types,
         x, l, logits, score_x, score_l, z_coordinates, gumbel, u, z_lattice, weights, rng, B, N, d, atom_types_out, x_out, l_out,
         status)


# ----------------------------------------------------------------------------------------------------------------
# F1 / F2 / R1
# ----------------------------------------------------------------------------------------------------------------
def noise_relative_coordinates(x0, z, sigma, out=None):
    """wrap(x0 + sigma z); sigma: one number, or a tensor of x0's shape (the reference's per-element sigmas)."""
    assert x0.shape == z.shape
    out = torch.empty_like(x0) if out is None else out
    if isinstance(sigma, torch.Tensor):
        assert sigma.shape == x0.shape, "sigmas array is expected to be of the same shape as the real_relative_coordinates array"
        call("mdx_noise_relative_coordinates_sigmas", x0, z, sigma, x0.numel(), out)
        return out
    call("mdx_noise_relative_coordinates", x0, z, float(sigma), x0.numel(), out)
    return out


def noise_lattice_parameters(l0, z, sigmas_n):
    """sigmas_n * z + l0, element by element (mdx_noise_lattice_parameters)."""
    assert l0.shape == z.shape == sigmas_n.shape
    out = torch.empty_like(l0)
    call("mdx_noise_lattice_parameters", l0, z, sigmas_n, l0.numel(), out)
    return out


def noise_atom_types(a0, q_bar, u):
    """q_bar: one [C, C] matrix for the call, or one per atom [*a0.shape, C, C]."""
    Cn = u.shape[-1]
    assert u.shape[:-1] == a0.shape
    out = torch.empty_like(a0)
    if q_bar.dim() > 2:
        assert q_bar.shape == tuple(a0.shape) + (Cn, Cn), "q_bar array first dimensions should match real_atom_types array"
        call("mdx_noise_atom_types_per_atom", a0, q_bar, u, a0.numel(), Cn, out)
        return out
    assert q_bar.shape == (Cn, Cn)
    call("mdx_noise_atom_types", a0, q_bar, u, a0.numel(), Cn, out)
    return out


def repaint_constrained_rows(sched: DeviceSchedule, index_i: int, d_index, constrained_x, constrained_a,
                             constrained_indices, z, u, rng: Rng, x_inout, a_inout):
    B, N, d = x_inout.shape
    K = constrained_x.shape[0]
    call("mdx_repaint_constrained_rows", C.byref(sched.c_struct), int(index_i), d_index, constrained_x, constrained_a,
         constrained_indices, K, z, u, rng, B, N, d, x_inout, a_inout)


def forward_diffusion_step(sched: DeviceSchedule, index_i: int, d_index, z, u, rng: Rng, x_inout, a_inout):
    """RePaint resampling: one forward-process step i -> i+1 on every atom, in place (mdx_forward_diffusion_step)."""
    B, N, d = x_inout.shape
    call("mdx_forward_diffusion_step", C.byref(sched.c_struct), int(index_i), d_index, z, u, rng, B, N, d, x_inout, a_inout)


def repaint_rows_per_sample(sched: DeviceSchedule, index_i: int, d_index, constrained_x, constrained_a, constrained_indices,
                            counts, sample_environment, z, u, rng: Rng, x_inout, a_inout):
    """mdx_repaint_constrained_rows with one constraint table per environment (mdx_repaint_rows_per_sample): tables
    constrained_x f32 [E,K,d], constrained_a / constrained_indices int64 [E,K], counts int32 [E]; sample b of the batch takes
    the first counts[e] rows of environment e = sample_environment[b] (int32 [B]).  In place on x_inout [B,N,d], a_inout [B,N]."""
    B, N, d = x_inout.shape
    E, K = constrained_a.shape
    assert constrained_x.shape == (E, K, d) and constrained_indices.shape == (E, K) and counts.shape == (E,)
    assert sample_environment.shape == (B,) and a_inout.shape == (B, N)
    call("mdx_repaint_rows_per_sample", C.byref(sched.c_struct), int(index_i), d_index, constrained_x, constrained_a,
         constrained_indices, counts, E, K, sample_environment, z, u, rng, B, N, d, x_inout, a_inout)


NoisedTrainingBatch = namedtuple("NoisedTrainingBatch", ["x0", "a0", "l0", "time_indices", "time", "sigma", "xt", "at", "lt", "q",
                                                         "q_bar", "q_bar_tm1"])
NOISING_INDEX_MESSAGE = "a dataset row, a time index or an atom type of a training batch is outside its range"


def noised_training_batch_buffers(batch: int, number_of_atoms: int, spatial_dimension: int, num_classes: int,
                                  device) -> NoisedTrainingBatch:
    """The twelve outputs of noise_training_batch for a batch of this size, uninitialised."""
    B, N, d, Cn, nl = batch, number_of_atoms, spatial_dimension, num_classes, spatial_dimension * (spatial_dimension + 1) // 2
    f = lambda *shape: torch.empty(*shape, dtype=F32, device=device)      # noqa: E731
    i = lambda *shape: torch.empty(*shape, dtype=I64, device=device)      # noqa: E731
    return NoisedTrainingBatch(x0=f(B, N, d), a0=i(B, N), l0=f(B, nl), time_indices=i(B), time=f(B), sigma=f(B), xt=f(B, N, d),
                               at=i(B, N), lt=f(B, nl), q=f(B, Cn, Cn), q_bar=f(B, Cn, Cn), q_bar_tm1=f(B, Cn, Cn))


def raise_noising_status(status: torch.Tensor):
    """One host read of a status word mdx_noise_training_batch reported into: its bit is cleared, then raised."""
    if _take_status_bits(status, _hip.STATUS_NOISING_INDEX) & _hip.STATUS_NOISING_INDEX:
        raise IndexError(NOISING_INDEX_MESSAGE)


def noise_training_batch(sched: DeviceSchedule, x0, a0, l0, batch: int, *, rows=None, row_offset: int = 0, cursor=None,
                         time_indices=None, z=None, u=None, z_lattice=None, rng: Optional[Rng] = None,
                         use_fixed_lattice_parameters: bool = False, out: Optional[NoisedTrainingBatch] = None,
                         status: Optional[torch.Tensor] = None) -> NoisedTrainingBatch:
    """`batch` rows of the device-resident dataset x0 f32 [M, N, d], a0 int64 [M, N], l0 f32 [M, d(d+1)/2], gathered and noised
    in ONE launch (mdx_noise_training_batch), no host read.  Structure b is row rows[p] (int64, e.g. a permutation; None: p) at
    p = row_offset + cursor * batch + b; `cursor` is an int32 device word or None (0).  `time_indices` int64 [batch], z
    [batch, N, d], u [batch, N, C], z_lattice [batch, nl] are pre-drawn; each None is drawn on the device from `rng`, keyed by
    the dataset row (include/mdx_hip.h).  `out` takes preallocated buffers (noised_training_batch_buffers), so that a captured
    launch writes where the step reads.  `status`: the int32 device word MDX_STATUS_NOISING_INDEX is OR-ed into."""
    _device_only("the training batch's noising", x0=x0, a0=a0, l0=l0, rows=rows, cursor=cursor, time_indices=time_indices, z=z, u=u,
                 z_lattice=z_lattice, status=status, schedule=sched.time,
                 **({} if out is None else {"out." + name: t for name, t in out._asdict().items()}))
    if x0.dim() != 3 or tuple(a0.shape) != tuple(x0.shape[:2]):
        raise ValueError(f"x0 has shape {tuple(x0.shape)} and a0 {tuple(a0.shape)}, expected [M, N, d] and [M, N]")
    M, N, d = x0.shape
    B, Cn, nl = int(batch), sched.num_classes, d * (d + 1) // 2
    if tuple(l0.shape) != (M, nl):
        raise ValueError(f"l0 has shape {tuple(l0.shape)}, expected {(M, nl)}")
    if rng is None:
        if time_indices is None or z is None or u is None or (z_lattice is None and not use_fixed_lattice_parameters):
            raise ValueError("a draw that is not given needs the device RNG request `rng`")
        rng = Rng(0, 0, 1, 0)
    if rows is not None and rows.dim() != 1:
        raise ValueError(f"rows has shape {tuple(rows.shape)}, expected [count]")
    out = noised_training_batch_buffers(B, N, d, Cn, x0.device) if out is None else out
    expected = dict(x0=(B, N, d), a0=(B, N), l0=(B, nl), time_indices=(B,), time=(B,), sigma=(B,), xt=(B, N, d), at=(B, N),
                    lt=(B, nl), q=(B, Cn, Cn), q_bar=(B, Cn, Cn), q_bar_tm1=(B, Cn, Cn), time_indices_in=(B,), z=(B, N, d),
                    u=(B, N, Cn), z_lattice=(B, nl))
    given = dict(out._asdict(), time_indices_in=time_indices, z=z, u=u, z_lattice=z_lattice)
    for name, t in given.items():
        if t is not None and t.numel() != torch.Size(expected[name]).numel():
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {expected[name]}")
    call("mdx_noise_training_batch", C.byref(sched.c_struct), x0, a0, l0, M, rows, 0 if rows is None else rows.numel(),
         int(row_offset), cursor, time_indices, z, u, z_lattice, rng, B, N, d, float(root_of_atom_count(N, d)),
         int(bool(use_fixed_lattice_parameters)), out.x0, out.a0, out.l0, out.time_indices, out.time, out.sigma, out.xt, out.at,
         out.lt, out.q, out.q_bar, out.q_bar_tm1, status)
    return out


class ExcisionCapacityError(_hip.MdxError):
    """MDX_STATUS_EXCISE_CAPACITY: an environment holds more atoms than the call's capacity; call again with a larger one."""


EXCISION_OUTSIDE_BOX = "Excised atoms are outside the new box. Use a larger box or smaller cutoff size for the excision."


def excise_environments(relative_coordinates, box_sides, central_atoms, radial_cutoff: Optional[float] = None,
                        number_of_neighbors: Optional[int] = None, center_atoms: bool = True, new_box_sides=None,
                        capacity: Optional[int] = None, status: Optional[torch.Tensor] = None):
    """The environments around `central_atoms` (int64 [E]) of ONE structure, in one launch (mdx_excise_environments): every atom
    within `radial_cutoff` of the central atom, or its `number_of_neighbors` nearest atoms and itself, ordered by (periodic
    distance, atom index) -- ties go to the lower index -- optionally translated so that slot 0 sits at the box centre and
    embedded in the orthogonal box `new_box_sides`.  relative_coordinates f64 [N,d] and box_sides f64 [d] on the device
    (float32 inputs are widened by the caller: the arithmetic is binary64 in the reference's operation order); N <= 4096, d <= 3.

    Returns (source_indices int64 [E,capacity], constrained_x f32 [E,capacity,d], counts int32 [E]), zero-padded; `capacity`
    defaults to N.  Without `status` the status word is read once after the call: a count above the capacity raises
    ExcisionCapacityError, an embedded atom outside the new box the reference's AssertionError, a central index outside
    [0, N) an IndexError.  With a caller's `status` (int32 [1]) nothing is read on the host."""
    for name, t in (("relative_coordinates", relative_coordinates), ("box_sides", box_sides), ("central_atoms", central_atoms)):
        if not t.is_cuda:
            raise _hip.MdxError(f"{name} lives on {t.device}: the excision kernel runs on the GPU only (no CPU fallback)")
    N, d = relative_coordinates.shape
    if d > 3 or N > _hip.EXCISE_MAX_ATOMS:
        raise _hip.MdxError(f"excision: at most 3 spatial dimensions and {_hip.EXCISE_MAX_ATOMS} atoms, got d = {d}, N = {N}")
    assert box_sides.shape == (d,) and central_atoms.dim() == 1
    assert (radial_cutoff is None) != (number_of_neighbors is None), "give a radial cutoff or a number of neighbours"
    E = central_atoms.shape[0]
    cap = N if capacity is None else int(capacity)
    dev = relative_coordinates.device
    source = torch.empty(E, cap, dtype=I64, device=dev)
    cx = torch.empty(E, cap, d, dtype=F32, device=dev)
    counts = torch.empty(E, dtype=I32, device=dev)
    own = status is None
    if own:
        status = torch.zeros(1, dtype=I32, device=dev)
    mode = _hip.EXCISE_RADIUS if number_of_neighbors is None else _hip.EXCISE_NEIGHBOURS
    call("mdx_excise_environments", relative_coordinates, box_sides, N, d, central_atoms, E, mode, float(radial_cutoff or 0.0),
         int(number_of_neighbors or 0), int(bool(center_atoms)), new_box_sides, cap, source, cx, counts, status)
    if own:
        word = int(status.item())
        if word & _hip.STATUS_EXCISE_CENTRAL_INDEX:
            raise IndexError(f"a central atom index is outside [0, {N})")
        if word & _hip.STATUS_EXCISE_CAPACITY:
            raise ExcisionCapacityError(f"an environment holds {int(counts.max())} atoms, more than the capacity {cap}")
        if word & _hip.STATUS_EXCISE_OUTSIDE_BOX:
            raise AssertionError(EXCISION_OUTSIDE_BOX)
    return source, cx, counts


def edit_keep_mask(relative_coordinates, lattice_parameters, sample_environment, active_atoms, counts, radius: float):
    """keep uint8 [B,N] of the excise-and-repaint sample edit (mdx_edit_keep_mask): atom n of sample b stays when it is one of
    the first counts[e] (constrained) atoms or lies further than `radius` from atom active_atoms[e], e = sample_environment[b]
    (all three int32), in the sample's own box lattice_parameters[b, :d]; binary64 distances on the widened float32 inputs."""
    B, N, d = relative_coordinates.shape
    assert lattice_parameters.dim() == 2 and lattice_parameters.shape[0] == B and lattice_parameters.shape[1] >= d
    assert sample_environment.shape == (B,) and active_atoms.shape == counts.shape and active_atoms.dim() == 1
    keep = torch.empty(B, N, dtype=torch.uint8, device=relative_coordinates.device)
    call("mdx_edit_keep_mask", relative_coordinates, lattice_parameters, lattice_parameters.shape[1], sample_environment,
         active_atoms, counts, counts.shape[0], float(radius), B, N, d, keep)
    return keep


RANDOM_FILL_TOO_MANY_CONSTRAINED = "There are more constrained atoms {} than total number of atoms {}."


def random_fill_proposals(seed: int, call: int, first_sample: int, batch: int, max_attempts: int, number_of_atoms: int,
                          spatial_dimension: int, num_atom_types: int, number_of_voxels: int, device):
    """The device draws of the excise-and-random maker (mdx_random_fill_proposals): uniforms f64 [B,M,N,d] in [0, 1), types
    int32 [B,M,N] in [0, num_atom_types) and, with number_of_voxels > 0, voxel occupancies int32 [B,M,N] (None otherwise) by
    the reference's rule: all voxels once per full round, the rest a random subset without replacement.  Philox keyed by
    (seed, call, first_sample + b, attempt): a sample's numbers do not depend on the batch it is drawn in."""
    device = torch.device(device)
    if device.type != "cuda":
        raise _hip.MdxError(f"the proposals are drawn on the GPU; got device {device} (no CPU fallback)")
    B, M, N, d = int(batch), int(max_attempts), int(number_of_atoms), int(spatial_dimension)
    with torch.cuda.device(device):
        uniforms = torch.empty(B, M, N, d, dtype=F64, device=device)
        types = torch.empty(B, M, N, dtype=I32, device=device)
        voxels = torch.empty(B, M, N, dtype=I32, device=device) if number_of_voxels else None
        _hip.call("mdx_random_fill_proposals", int(seed) & 0xFFFFFFFFFFFFFFFF, int(call), int(first_sample), B, M, N, d,
                  int(num_atom_types), int(number_of_voxels), uniforms, types, voxels)
    return uniforms, types, voxels


def random_fill_environments(uniforms, types, voxels, partition, constrained_x, constrained_a, counts, active,
                             sample_environment, box_sides, minimal_interatomic_distance: float,
                             status: Optional[torch.Tensor] = None):
    """Placement, retry and acceptance of the excise-and-random maker for a batch of samples, one workgroup per sample and all
    attempts in one launch (mdx_random_fill_environments).  Proposals uniforms f64 [B,M,N,d], types int32 [B,M,N], voxels int32
    [B,M,N] with the voxels per axis `partition` (a sequence of d ints) or both None; constraint tables constrained_x f64
    [E,K,d], constrained_a int64 [E,K], counts / active int32 [E]; sample_environment int32 [B]; box_sides f64 [E,d].

    Returns (x f64 [B,N,d], a int64 [B,N], active_out int32 [B], attempts int32 [B], accepted uint8 [B], min_distance f64 [B]).
    Without `status` the status word is read once after the call: more constrained atoms than atoms raises the reference's
    AssertionError, an environment or active index out of range an IndexError.  With a caller's `status` (int32 [1]) nothing is
    read on the host."""
    B, M, N, d = uniforms.shape
    E, K = constrained_a.shape
    if d > 3 or N > _hip.RANDOM_FILL_MAX_ATOMS or K > _hip.RANDOM_FILL_MAX_ATOMS:
        raise _hip.MdxError(f"random fill: at most 3 spatial dimensions and {_hip.RANDOM_FILL_MAX_ATOMS} atoms, "
                            f"got d = {d}, N = {N}, K = {K}")
    assert types.shape == (B, M, N) and constrained_x.shape == (E, K, d) and counts.shape == (E,) and active.shape == (E,)
    assert sample_environment.shape == (B,) and box_sides.shape == (E, d)
    assert (voxels is None) == (partition is None), "voxel occupancies and the partition go together"
    words = None
    if partition is not None:
        assert voxels.shape == (B, M, N) and len(partition) == d
        words = (C.c_int32 * d)(*[int(v) for v in partition])
    dev = uniforms.device
    x = torch.empty(B, N, d, dtype=F64, device=dev)
    a = torch.empty(B, N, dtype=I64, device=dev)
    active_out, attempts = torch.empty(B, dtype=I32, device=dev), torch.empty(B, dtype=I32, device=dev)
    accepted = torch.empty(B, dtype=torch.uint8, device=dev)
    min_distance = torch.empty(B, dtype=F64, device=dev)
    own = status is None
    if own:
        status = torch.zeros(1, dtype=I32, device=dev)
    call("mdx_random_fill_environments", uniforms, types, voxels, words, constrained_x, constrained_a, counts, active, E, K,
         sample_environment, box_sides, M, float(minimal_interatomic_distance), B, N, d, x, a, active_out, attempts, accepted,
         min_distance, status)
    if own:
        word = int(status.item())
        if word & _hip.STATUS_RANDOM_FILL_COUNT:
            raise AssertionError(RANDOM_FILL_TOO_MANY_CONSTRAINED.format(int(counts.max()), N))
        if word & _hip.STATUS_RANDOM_FILL_ENVIRONMENT:
            raise IndexError(f"a sample's environment is outside [0, {E}) or an active atom is not a constrained atom")
    return x, a, active_out, attempts, accepted, min_distance


# ----------------------------------------------------------------------------------------------------------------
# N1
# ----------------------------------------------------------------------------------------------------------------
def radius_graph(cartesian_positions, basis_vectors, radial_cutoff: float, unique: bool,
                 status: Optional[torch.Tensor] = None, want_shifts: bool = True):
    """Two-call radius graph.  Returns dict(counts [B,N], edges [E,2], image [E] | None, shifts [E,3] | None).

    The only host synchronisation is reading E = counts.sum() to size the outputs.
    """
    B, N, d = cartesian_positions.shape
    assert d == 3 and basis_vectors.shape == (B, 3, 3)
    dev = cartesian_positions.device
    counts = torch.empty(B, N, dtype=I64, device=dev)
    call("mdx_radius_graph_count", cartesian_positions, basis_vectors, float(radial_cutoff), B, N, int(bool(unique)), counts,
         status)
    inclusive = torch.cumsum(counts.view(-1), 0)
    offsets = inclusive - counts.view(-1)
    E = int(inclusive[-1].item()) if B * N > 0 else 0
    edges = torch.empty(E, 2, dtype=I64, device=dev)
    image = None if unique else torch.empty(E, dtype=I32, device=dev)
    shifts = None if (unique or not want_shifts) else torch.empty(E, 3, dtype=F32, device=dev)
    if E > 0:
        call("mdx_radius_graph_fill", cartesian_positions, basis_vectors, float(radial_cutoff), B, N, int(bool(unique)),
             offsets, edges, image, shifts)
    return dict(counts=counts, edges=edges, image=image, shifts=shifts)


def radius_graph_static(cartesian_positions, basis_vectors, radial_cutoff: float, capacity: int,
                        status: Optional[torch.Tensor] = None):
    """Unique-pair radius graph into a caller-sized edge list, with NO host synchronisation (capturable into a hipGraph):
    returns dict(counts [B*N], offsets [B*N], edges [capacity, 2], n_edges int64 [1] on the device).  Rows beyond
    n_edges are uninitialised; more than `capacity` edges sets STATUS_GRAPH_CAPACITY in `status`."""
    B, N, d = cartesian_positions.shape
    assert d == 3 and basis_vectors.shape == (B, 3, 3)
    dev = cartesian_positions.device
    counts = torch.empty(B * N, dtype=I64, device=dev)
    call("mdx_radius_graph_count", cartesian_positions, basis_vectors, float(radial_cutoff), B, N, 1, counts, status)
    inclusive = torch.cumsum(counts, 0)
    offsets = inclusive - counts
    edges = torch.empty(int(capacity), 2, dtype=I64, device=dev)
    call("mdx_radius_graph_fill_capped", cartesian_positions, basis_vectors, float(radial_cutoff), B, N, 1, offsets,
         int(capacity), edges, None, None, status)
    return dict(counts=counts, offsets=offsets, edges=edges, n_edges=inclusive[-1:])


def egnn_radius_graph(relative_coordinates, lattice_parameters, clip_min: float, radial_cutoff: float, capacity: int,
                      status: Optional[torch.Tensor] = None, two_launches: bool = True):
    """radius_graph_static for the graph EGNNScoreNetwork builds (egnn_score_network.py:236-247): relative coordinates
    [B,N,3] in the cell diag(max(lattice_parameters[:, :3], clip_min)) behind ONE call, no library kernel, no host read
    (mdx_egnn_radius_graph): hit masks + emission (two launches, every pair tested once) where that form applies
    (N <= 1024, B <= 2048) and `two_launches`, else count, device-side scan and fill.  Same dict as radius_graph_static."""
    B, N, d = relative_coordinates.shape
    assert d == 3 and lattice_parameters.dim() == 2 and lattice_parameters.shape[0] == B and lattice_parameters.shape[1] >= 3
    dev = relative_coordinates.device
    counts = torch.empty(B * N, dtype=I64, device=dev)
    offsets = torch.empty(B * N, dtype=I64, device=dev)
    n_edges = torch.empty(1, dtype=I64, device=dev)
    edges = torch.empty(int(capacity), 2, dtype=I64, device=dev)
    words = int(lib().mdx_egnn_radius_graph_workspace_words(B, N)) if two_launches else 0
    workspace = torch.empty(words, dtype=I64, device=dev) if words else None
    call("mdx_egnn_radius_graph", relative_coordinates, lattice_parameters, lattice_parameters.shape[1], float(clip_min),
         float(radial_cutoff), B, N, int(capacity), counts, offsets, n_edges, edges, status, workspace, words)
    return dict(counts=counts, offsets=offsets, edges=edges, n_edges=n_edges)


def force_field_pseudo_force(relative_coordinates, lattice_parameters, clip_min: float, radial_cutoff: float, strength: float,
                             score_in: Optional[torch.Tensor] = None, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The force-field wrapper's repulsive pseudo-force in relative coordinates [B,N,3] (mdx_force_field_pseudo_force): every
    (i, j, image) pair of the full radius graph of relative coordinates [B,N,3] in the cell diag(max(lattice_parameters[:, :3],
    clip_min)), tested in place -- one launch, no edge list, no host read.  With `score_in` [B,N,3] the result is score_in + the
    pseudo-force.  MDX_STATUS_CUTOFF_TOO_LARGE is OR-ed into `status` where the cutoff reaches the cell's crossing distance."""
    B, N, d = relative_coordinates.shape
    if d != 3:
        raise _hip.MdxError(f"force-field pseudo-force: spatial dimension 3 only (the reference's), got {d}")
    assert lattice_parameters.dim() == 2 and lattice_parameters.shape[0] == B and lattice_parameters.shape[1] >= 3
    if score_in is not None and score_in.shape != relative_coordinates.shape:
        raise ValueError(f"score_in has shape {tuple(score_in.shape)}, expected {tuple(relative_coordinates.shape)}")
    out = torch.empty(B, N, 3, dtype=F32, device=relative_coordinates.device)
    call("mdx_force_field_pseudo_force", relative_coordinates, lattice_parameters, lattice_parameters.shape[1], float(clip_min),
         float(radial_cutoff), float(2.0 * strength), B, N, score_in, out, status)
    return out


class StillingerWeberNeighbourCapacityError(_hip.MdxError):
    """MDX_STATUS_SW_NEIGHBOURS: an atom has more neighbours than the call's neighbour capacity; call again with a larger one."""


SW_NEIGHBOUR_CAPACITY = 64         # slots per atom of the neighbour lists (diamond Si has 4 inside a sigma, a dense random gas ~45)


def stillinger_weber_energy_forces(relative_coordinates, lattice_parameters, atom_types, parameter_table, with_forces: bool = True,
                                   neighbour_capacity: int = SW_NEIGHBOUR_CAPACITY, status: Optional[torch.Tensor] = None,
                                   workspace: Optional[torch.Tensor] = None):
    """Stillinger-Weber energies f64 [B] (eV) and Cartesian forces f64 [B,N,3] (eV/Angstrom; None without `with_forces`) of
    relative coordinates f32 [B,N,3] in the orthogonal boxes lattice_parameters[:, :3] (f32 [B, >=3]) with atom types int64 [B,N]
    and the device table f64 [n,n,n,10] of read_stillinger_weber_coefficients (mdx_stillinger_weber_energy_forces): one launch,
    binary64, gathered forces, the same bits on every launch.  Without `status` the device status word is read ONCE after the
    call and a side below the largest cutoff, an atom type outside the table (MASK included) or a neighbour overflow raises;
    with a caller's `status` (int32 [1]) nothing is read on the host -- the call can be captured -- and the caller inspects the
    bits (the affected structures hold NaNs).  `workspace`: f64, reused when large enough."""
    for name, t in (("relative_coordinates", relative_coordinates), ("lattice_parameters", lattice_parameters),
                    ("atom_types", atom_types), ("parameter_table", parameter_table)):
        if not t.is_cuda:
            raise _hip.MdxError(f"{name} lives on {t.device}: the Stillinger-Weber kernel runs on the GPU only (no CPU fallback)")
    B, N, d = relative_coordinates.shape
    if d != 3:
        raise _hip.MdxError(f"Stillinger-Weber: spatial dimension 3 only, got {d}")
    assert lattice_parameters.dim() == 2 and lattice_parameters.shape[0] == B and lattice_parameters.shape[1] >= 3
    assert atom_types.shape == (B, N)
    n = parameter_table.shape[0]
    assert parameter_table.shape == (n, n, n, 10), "the parameter table is [n_types, n_types, n_types, 10]"
    dev = relative_coordinates.device
    words = int(lib().mdx_stillinger_weber_workspace_doubles(B, N, int(neighbour_capacity)))
    if workspace is None or workspace.numel() < words:
        workspace = torch.empty(max(words, 1), dtype=F64, device=dev)
    energies = torch.empty(B, dtype=F64, device=dev)
    forces = torch.empty(B, N, 3, dtype=F64, device=dev) if with_forces else None
    own_status = status is None
    if own_status:
        status = torch.zeros(1, dtype=I32, device=dev)
    call("mdx_stillinger_weber_energy_forces", relative_coordinates, lattice_parameters, lattice_parameters.shape[1], atom_types,
         parameter_table, n, B, N, int(neighbour_capacity), workspace, workspace.numel(), energies, forces, status)
    if own_status:
        bits = int(status.item())
        if bits & _hip.STATUS_SW_ATOM_TYPE:
            raise _hip.MdxError(f"Stillinger-Weber: an atom type lies outside the parameter table's {n} types (a MASK among them?)")
        if bits & _hip.STATUS_CUTOFF_TOO_LARGE:
            raise _hip.MdxError("Stillinger-Weber: a box side is shorter than the largest cutoff a*sigma of the table: the 27-image "
                                "sweep would miss neighbours (MDX_STATUS_CUTOFF_TOO_LARGE)")
        if bits & _hip.STATUS_SW_NEIGHBOURS:
            raise StillingerWeberNeighbourCapacityError(
                f"Stillinger-Weber: an atom has more than neighbour_capacity={neighbour_capacity} neighbours (MDX_STATUS_SW_NEIGHBOURS)")
    return energies, forces


# ----------------------------------------------------------------------------------------------------------------
# analytical score network (csrc/mdx_analytical.hip)
# ----------------------------------------------------------------------------------------------------------------
ANALYTICAL_MAX_ATOMS, ANALYTICAL_MAX_PERMUTED_ATOMS = 1024, 8


def _device_only(what: str, **tensors):
    for name, t in tensors.items():
        if t is not None and not t.is_cuda:
            raise _hip.MdxError(f"{name} lives on {t.device}: {what} runs on the GPU only (no CPU fallback)")


def raise_analytical_bits(word: int):
    """The reference's two value assertions (score/wrapped_gaussian_score.py:155-159) for the bits of a status word read earlier."""
    if word & _hip.STATUS_ANALYTICAL_SIGMA:
        raise AssertionError("All values of sigma should be larger than zero.")
    if word & _hip.STATUS_ANALYTICAL_COORDINATES:
        raise AssertionError("the relative coordinates should all be in [0, 1)")


def _take_status_bits(status: torch.Tensor, mask: int) -> int:
    """The status word, by one host read; the bits of `mask` that were set in it are cleared (the other kernels' stay)."""
    word = int(status.item())
    if word & mask:
        status.bitwise_and_(~mask)
    return word


def raise_analytical_status(status: torch.Tensor):
    """One host read of a status word the analytical kernels reported into: their bits are cleared, then raised."""
    raise_analytical_bits(_take_status_bits(status, _hip.STATUS_ANALYTICAL_SIGMA | _hip.STATUS_ANALYTICAL_COORDINATES))


def wrapped_gaussian_sigma_normalized_score(relative_coordinates, sigmas, kmax: int, coordinates_bounded: bool = True,
                                            status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """sigma x score of the wrapped Gaussian, elementwise over f32 tensors of one shape (mdx_wrapped_gaussian_sigma_normalized_score):
    binary64 inside, the reference's three formulas and truncation.  Invalid values give NaN and their bit in `status`."""
    _device_only("the wrapped-Gaussian score", relative_coordinates=relative_coordinates, sigmas=sigmas, status=status)
    if relative_coordinates.shape != sigmas.shape:
        raise ValueError("relative_coordinates and sigmas must have the same shape")
    out = torch.empty_like(relative_coordinates)
    call("mdx_wrapped_gaussian_sigma_normalized_score", relative_coordinates, sigmas, relative_coordinates.numel(), int(kmax),
         int(bool(coordinates_bounded)), out, status)
    return out


def log_wrapped_gaussians(relative_coordinates, sigmas, kmax: int, row_length: int,
                          status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Log wrapped Gaussians of f32 tensors of one shape, summed over rows of `row_length` trailing elements: f32
    [numel / row_length] (mdx_log_wrapped_gaussians)."""
    _device_only("the log wrapped Gaussian", relative_coordinates=relative_coordinates, sigmas=sigmas, status=status)
    if relative_coordinates.shape != sigmas.shape:
        raise ValueError("relative_coordinates and sigmas must have the same shape")
    if row_length < 1 or relative_coordinates.numel() % row_length:
        raise ValueError(f"row_length {row_length} does not divide {relative_coordinates.numel()} elements")
    rows = relative_coordinates.numel() // row_length
    out = torch.empty(rows, dtype=F32, device=relative_coordinates.device)
    call("mdx_log_wrapped_gaussians", relative_coordinates, sigmas, rows, int(row_length), int(kmax), out, status)
    return out


def analytical_score(relative_coordinates, sigmas, equilibrium_relative_coordinates, sigma_d_square: float, kmax: int,
                     use_permutation_invariance: bool, with_probabilities: bool = False, status: Optional[torch.Tensor] = None):
    """(sigma-normalised score f32 [B,N,D], probabilities f32 [B] or None) of the analytical score network (mdx_analytical_score):
    relative_coordinates f32 [B,N,D]; sigmas f32 [B] (one per structure) or [B,N,D] (one per element); sites f32 [N,D].  One
    kernel, no host read: a structure with an invalid sigma or coordinate holds NaNs and its bit is OR-ed into `status`."""
    _device_only("the analytical score", relative_coordinates=relative_coordinates, sigmas=sigmas,
                 equilibrium_relative_coordinates=equilibrium_relative_coordinates, status=status)
    B, N, D = relative_coordinates.shape
    if equilibrium_relative_coordinates.shape != (N, D):
        raise ValueError(f"equilibrium_relative_coordinates has shape {tuple(equilibrium_relative_coordinates.shape)}, expected {(N, D)}")
    if sigmas.shape == relative_coordinates.shape:
        per_element = 1
    elif sigmas.numel() == B:
        per_element = 0
    else:
        raise ValueError(f"sigmas has shape {tuple(sigmas.shape)}: expected [{B}] or {tuple(relative_coordinates.shape)}")
    dev = relative_coordinates.device
    scores = torch.empty(B, N, D, dtype=F32, device=dev)
    probabilities = torch.empty(B, dtype=F32, device=dev) if with_probabilities else None
    call("mdx_analytical_score", relative_coordinates, sigmas, per_element, equilibrium_relative_coordinates,
         float(sigma_d_square), int(kmax), int(bool(use_permutation_invariance)), B, N, D, scores, probabilities, status)
    return scores, probabilities


# ----------------------------------------------------------------------------------------------------------------
# linear assignment, optimal transport, equivariant analytical score network (csrc/mdx_transport.hip)
# ----------------------------------------------------------------------------------------------------------------
TRANSPORT_MAX_ATOMS, TRANSPORT_MAX_OPERATIONS = _hip.TRANSPORT_MAX_ATOMS, _hip.TRANSPORT_MAX_OPERATIONS


def linear_assignment(cost_matrices, status: Optional[torch.Tensor] = None):
    """(col_idx int32 [M, n], costs f64 [M]) of the M assignment problems cost_matrices f32 or f64 [M, n, n], n <= 256
    (mdx_linear_assignment): col_idx[m, i] is the column of row i, costs[m] the optimum summed in row order.  A matrix with a
    non-finite entry gives col_idx -1, a NaN cost and STATUS_LAP_COST in `status`."""
    _device_only("the linear assignment", cost_matrices=cost_matrices, status=status)
    if cost_matrices.dim() != 3 or cost_matrices.shape[1] != cost_matrices.shape[2]:
        raise ValueError(f"cost_matrices has shape {tuple(cost_matrices.shape)}, expected [M, n, n]")
    if cost_matrices.dtype not in (F32, F64):
        raise TypeError(f"cost_matrices must be float32 or float64, got {cost_matrices.dtype}")
    M, n, _ = cost_matrices.shape
    col_idx = torch.empty(M, n, dtype=I32, device=cost_matrices.device)
    costs = torch.empty(M, dtype=F64, device=cost_matrices.device)
    call("mdx_linear_assignment", cost_matrices, int(cost_matrices.dtype == F64), M, n, col_idx, costs, status)
    return col_idx, costs


def transport_align(x, mu, point_group_operations, with_details: bool = False, status: Optional[torch.Tensor] = None):
    """Transporter.get_optimal_transport in one launch (mdx_transport_align): x f32 [B, N, D]; mu f32 [N, D] (shared) or
    [B, N, D]; point_group_operations f32 [O, D, D].  Returns the aligned image of mu f32 [B, N, D], and with `with_details`
    also (operation index int32 [B], col_idx int32 [B, N], costs f64 [B, O])."""
    _device_only("the optimal transport", x=x, mu=mu, point_group_operations=point_group_operations, status=status)
    B, N, D = x.shape
    O = point_group_operations.shape[0]
    if point_group_operations.shape != (O, D, D):
        raise ValueError(f"point_group_operations has shape {tuple(point_group_operations.shape)}, expected [O, {D}, {D}]")
    if mu.shape == (N, D):
        stride = 0
    elif mu.shape == (B, N, D):
        stride = N * D
    else:
        raise ValueError(f"mu has shape {tuple(mu.shape)}, expected {(N, D)} or {(B, N, D)}")
    dev = x.device
    aligned = torch.empty(B, N, D, dtype=F32, device=dev)
    operation_idx = torch.empty(B, dtype=I32, device=dev) if with_details else None
    col_idx = torch.empty(B, N, dtype=I32, device=dev) if with_details else None
    costs = torch.empty(B, O, dtype=F64, device=dev) if with_details else None
    call("mdx_transport_align", x, mu, stride, point_group_operations, O, B, N, D, aligned, operation_idx, col_idx, costs, status)
    return (aligned, operation_idx, col_idx, costs) if with_details else aligned


def equivariant_analytical_score(relative_coordinates, sigmas, equilibrium_relative_coordinates, point_group_operations,
                                 sigma_d_square: float, kmax: int, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The equivariant analytical score network's forward (mdx_equivariant_analytical_score): relative_coordinates f32 [B, N, D];
    sigmas f32 [B] (numel B); sites f32 [N, D]; point_group_operations f32 [O, D, D].  One kernel, no host read: a structure
    with an invalid sigma or a non-finite coordinate holds NaNs and its bit is OR-ed into `status`."""
    _device_only("the equivariant analytical score", relative_coordinates=relative_coordinates, sigmas=sigmas,
                 equilibrium_relative_coordinates=equilibrium_relative_coordinates, point_group_operations=point_group_operations,
                 status=status)
    B, N, D = relative_coordinates.shape
    O = point_group_operations.shape[0]
    if equilibrium_relative_coordinates.shape != (N, D):
        raise ValueError(f"equilibrium_relative_coordinates has shape {tuple(equilibrium_relative_coordinates.shape)}, expected {(N, D)}")
    if point_group_operations.shape != (O, D, D):
        raise ValueError(f"point_group_operations has shape {tuple(point_group_operations.shape)}, expected [O, {D}, {D}]")
    if sigmas.numel() != B:
        raise ValueError(f"sigmas has shape {tuple(sigmas.shape)}: expected one per structure, [{B}]")
    scores = torch.empty(B, N, D, dtype=F32, device=relative_coordinates.device)
    call("mdx_equivariant_analytical_score", relative_coordinates, sigmas, equilibrium_relative_coordinates,
         point_group_operations, O, float(sigma_d_square), int(kmax), B, N, D, scores, status)
    return scores


# ----------------------------------------------------------------------------------------------------------------
# optimal torus translation (csrc/mdx_optimal_translation.hip)
# ----------------------------------------------------------------------------------------------------------------
def optimal_translation(x, y, with_details: bool = False, status: Optional[torch.Tensor] = None):
    """The reference's find_squared_geodesic_distance_minimizing_translation in one launch (mdx_optimal_translation): x f32 [N, D]
    (shared by the batch) or [B, N, D]; y f32 [B, N, D].  Returns tau f32 [B, D], the translation in [-1/2, 1/2) that minimises
    D^2(x, y + tau) per structure and dimension, and with `with_details` also (squared_distance f64 [B, D], number_of_candidates
    int32 [B, D]).  No host read: an entry whose minimum sits on the boundary holds +inf (as the reference's does) and
    STATUS_TRANSLATION_NO_CANDIDATE is OR-ed into `status`; a structure with a non-finite coordinate holds NaN (count -1) and
    STATUS_ANALYTICAL_COORDINATES."""
    _device_only("the optimal translation", x=x, y=y, status=status)
    if y.dim() != 3:
        raise ValueError(f"y has shape {tuple(y.shape)}, expected [B, N, D]")
    B, N, D = y.shape
    if x.shape == (N, D):
        stride = 0
    elif x.shape == (B, N, D):
        stride = N * D
    else:
        raise ValueError(f"x has shape {tuple(x.shape)}, expected {(N, D)} or {(B, N, D)}")
    dev = y.device
    tau = torch.empty(B, D, dtype=F32, device=dev)
    squared_distance = torch.empty(B, D, dtype=F64, device=dev) if with_details else None
    number_of_candidates = torch.empty(B, D, dtype=I32, device=dev) if with_details else None
    call("mdx_optimal_translation", x, stride, y, B, N, D, tau, squared_distance, number_of_candidates, status)
    return (tau, squared_distance, number_of_candidates) if with_details else tau


# ----------------------------------------------------------------------------------------------------------------
# denoising loss (csrc/mdx_loss.hip)
# ----------------------------------------------------------------------------------------------------------------
LOSS_ALGORITHMS = {"mse": _hip.LOSS_MSE, "weighted_mse": _hip.LOSS_WEIGHTED_MSE}
LOSS_MAX_ATOMS, LOSS_MAX_LATTICE_PARAMETERS = _hip.LOSS_MAX_ATOMS, _hip.LOSS_MAX_LATTICE_PARAMETERS
LOSS_LOGITS_MESSAGE = "Logits are pathological: the probabilities do not sum to one."

DenoisingLoss = namedtuple("DenoisingLoss", ["target_x", "target_l", "loss_x", "loss_a", "loss_l", "per_structure", "q_atm1",
                                             "p_atm1", "vb_term", "ce_term"])


def binary32(value: float) -> float:
    """The binary32 neighbour of a Python float, as a Python float: what a 0-dim float32 buffer of the reference holds."""
    return float(torch.tensor(value, dtype=F32))


@lru_cache(maxsize=None)
def root_of_atom_count(number_of_atoms: int, degree: int) -> float:
    """n^(1 / degree) as the reference's scale_sigma_by_number_of_atoms makes it (utils/noise_utils.py:29): torch.pow of a
    binary32 HOST tensor, so that a sigma_n made from it has the reference's bits whatever the device's pow rounds to."""
    return float(torch.pow(torch.full((16,), float(number_of_atoms)), 1 / degree)[0])


def raise_loss_status(status: torch.Tensor):
    """One host read of a status word mdx_denoising_loss reported into: its bits are cleared, then raised -- the reference's
    value assertion on the logits (utils/d3pm_utils.py:144-145), the wrapped score's two, and an index outside its table."""
    word = _take_status_bits(status, _hip.STATUS_LOSS_LOGITS | _hip.STATUS_LOSS_INDEX | _hip.STATUS_ANALYTICAL_SIGMA |
                             _hip.STATUS_ANALYTICAL_COORDINATES)
    if word & _hip.STATUS_LOSS_LOGITS:
        raise AssertionError(LOSS_LOGITS_MESSAGE)
    if word & _hip.STATUS_LOSS_INDEX:
        raise IndexError("a time index outside the transition tables or an atom type outside [0, num_classes)")
    raise_analytical_bits(word)


def denoising_loss(*, x0=None, xt=None, target_x=None, predicted_x=None, sigma=None, a0=None, at=None, logits=None,
                   time_indices=None, q_matrices=None, q_bar_matrices=None, q_bar_tm1_matrices=None,
                   tables_per_structure: bool = False, l0=None, lt=None, predicted_l=None, sigma_n=None, sigma_n_divisor: float = 0.0,
                   kmax: int = 4,
                   x_algorithm: str = "mse", x_sigma0: float = 0.0, x_exponent: float = 0.0, l_algorithm: str = "mse",
                   l_sigma0: float = 0.0, l_exponent: float = 0.0, ce_weight: float = 0.001, eps: float = 1e-8,
                   lambda_weights=(1.0, 1.0, 1.0), with_terms: bool = False,
                   status: Optional[torch.Tensor] = None) -> DenoisingLoss:
    """The denoising loss of a noised batch in one launch (mdx_denoising_loss), no host read.  The three parts are independent,
    each present when its prediction (for A: a0) is given:
      X  predicted_x f32 [B, N, D]; sigma f32 with B elements, or [B, N, D]; the target from x0, xt f32 [B, N, D] (kmax), or
         `target_x` f32 [B, N, D] as given
      A  a0, at int64 [B, N], logits f32 [B, N, C], time_indices int64 [B]; the three transition tables f32 [T, C, C], read at
         the structure's time index, or with `tables_per_structure` [B, C, C], one row per structure.  Without tables only
         ce_term is made, without logits only q_atm1
      L  l0, lt, predicted_l f32 [B, P]; sigma_n f32 with B elements, or `sigma_n_divisor`: sigma_n = sigma / divisor in
         binary32 inside the kernel; the weights of weighted_mse take `sigma`
    x_sigma0, x_exponent, l_sigma0, l_exponent go to the kernel as given: the reference holds them in binary32 (`binary32`).
    lambda_weights is (A, X, L).  Returns a DenoisingLoss of f32 tensors, None where its part is absent: the two targets, the
    three unreduced losses, per_structure [B, 4] = (mean A, mean X, mean L, weighted aggregate), and with `with_terms` the
    atom-type intermediates q_atm1, p_atm1, vb_term, ce_term [B, N, C]."""
    return _denoising_loss_launch(x0, xt, target_x, predicted_x, sigma, a0, at, logits, time_indices, q_matrices, q_bar_matrices,
                                  q_bar_tm1_matrices, tables_per_structure, l0, lt, predicted_l, sigma_n, sigma_n_divisor, kmax,
                                  x_algorithm, x_sigma0, x_exponent, l_algorithm, l_sigma0, l_exponent, ce_weight, eps,
                                  lambda_weights, with_terms, status)


def _denoising_loss_launch(x0, xt, target_x, predicted_x, sigma, a0, at, logits, time_indices, q_matrices, q_bar_matrices,
                           q_bar_tm1_matrices, tables_per_structure, l0, lt, predicted_l, sigma_n, sigma_n_divisor, kmax,
                           x_algorithm, x_sigma0, x_exponent, l_algorithm, l_sigma0, l_exponent, ce_weight, eps, lambda_weights,
                           with_terms, status, with_gradient: bool = False, batch_divisor: Optional[float] = None):
    """The checks and the one call behind denoising_loss (mdx_denoising_loss) and, `with_gradient`,
    denoising_loss_and_gradient (mdx_denoising_loss_gradient)."""
    _device_only("the denoising loss", x0=x0, xt=xt, target_x=target_x, predicted_x=predicted_x, sigma=sigma, a0=a0, at=at,
                 logits=logits, time_indices=time_indices, q_matrices=q_matrices, q_bar_matrices=q_bar_matrices,
                 q_bar_tm1_matrices=q_bar_tm1_matrices, l0=l0, lt=lt, predicted_l=predicted_l, sigma_n=sigma_n, status=status)
    with_x, with_a, with_l = predicted_x is not None, a0 is not None, predicted_l is not None
    leading = predicted_x if with_x else a0 if with_a else predicted_l
    if leading is None:
        raise ValueError("one of predicted_x, a0 and predicted_l must be given")
    B, dev = leading.shape[0], leading.device
    N, D, Cn, P, T, per_element = 1, 1, 0, 0, 0, 0

    def expect(name, t, shape):
        if t is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")

    def per_structure_values(name, t):
        if t is not None and t.numel() != B:
            raise ValueError(f"{name} has shape {tuple(t.shape)}: expected one value per structure, [{B}]")

    def empty(present, *shape):
        return torch.empty(*shape, dtype=F32, device=dev) if present else None

    if with_x:
        if predicted_x.dim() != 3:
            raise ValueError(f"predicted_x has shape {tuple(predicted_x.shape)}, expected [B, N, D]")
        _, N, D = predicted_x.shape
        for name, t in (("x0", x0), ("xt", xt), ("target_x", target_x)):
            expect(name, t, (B, N, D))
        if target_x is None and (x0 is None or xt is None or sigma is None):
            raise ValueError("the coordinates' part needs x0, xt and sigma, or target_x")
    if sigma is not None:
        per_element = int(with_x and sigma.numel() != B and tuple(sigma.shape) == (B, N, D))
        if not per_element:
            per_structure_values("sigma", sigma)
    if with_a:
        if a0.dim() != 2 or (with_x and tuple(a0.shape) != (B, N)):
            raise ValueError(f"a0 has shape {tuple(a0.shape)}, expected {(B, N) if with_x else '[B, N]'}")
        N = a0.shape[1]
        tables = (q_matrices, q_bar_matrices, q_bar_tm1_matrices)
        if logits is None and tables[0] is None:
            raise ValueError("the atom types' part needs logits or the transition tables")
        Cn = logits.shape[-1] if logits is not None else tables[0].shape[-1]
        expect("at", at, (B, N))
        expect("logits", logits, (B, N, Cn))
        expect("time_indices", time_indices, (B,))
        if any(t is not None for t in tables):
            if any(t is None for t in tables) or at is None or time_indices is None:
                raise ValueError("the transition tables come as three, with at and time_indices")
            T = 0 if tables_per_structure else tables[0].shape[0]
            for name, t in zip(("q_matrices", "q_bar_matrices", "q_bar_tm1_matrices"), tables):
                expect(name, t, (B if tables_per_structure else T, Cn, Cn))
    if with_l:
        if predicted_l.dim() != 2:
            raise ValueError(f"predicted_l has shape {tuple(predicted_l.shape)}, expected [B, P]")
        P = predicted_l.shape[1]
        for name, t in (("l0", l0), ("lt", lt)):
            expect(name, t, (B, P))
        if l0 is None or lt is None or (sigma_n is None and not (sigma is not None and sigma_n_divisor > 0.0)):
            raise ValueError("the lattice parameters' part needs l0, lt and sigma_n (or sigma and sigma_n_divisor)")
        per_structure_values("sigma_n", sigma_n)
    with_tables = with_a and q_matrices is not None
    with_logits = with_a and logits is not None
    out = DenoisingLoss(
        target_x=empty(with_x and target_x is None, B, N, D), target_l=empty(with_l, B, P), loss_x=empty(with_x, B, N, D),
        loss_a=empty(with_tables and with_logits, B, N, Cn), loss_l=empty(with_l, B, P), per_structure=empty(True, B, 4),
        q_atm1=empty(with_terms and with_tables, B, N, Cn), p_atm1=empty(with_terms and with_tables and with_logits, B, N, Cn),
        vb_term=empty(with_terms and with_tables and with_logits, B, N, Cn), ce_term=empty(with_terms and with_logits, B, N, Cn))
    lambda_a, lambda_x, lambda_l = (float(w) for w in lambda_weights)
    detached = [None if t is None else t.detach() for t in (predicted_x, logits, predicted_l)] if with_gradient else \
        [predicted_x, logits, predicted_l]
    arguments = (x0, xt, target_x, detached[0], sigma, per_element, a0, at, detached[1], time_indices, q_matrices,
                 q_bar_matrices, q_bar_tm1_matrices, int(T), l0, lt, detached[2], sigma_n, float(sigma_n_divisor), B, int(N), int(D),
                 int(Cn), int(P), int(kmax), LOSS_ALGORITHMS[x_algorithm], float(x_sigma0), float(x_exponent),
                 LOSS_ALGORITHMS[l_algorithm], float(l_sigma0), float(l_exponent), float(ce_weight), float(eps), lambda_a, lambda_x,
                 lambda_l, out.target_x, out.target_l, out.loss_x, out.loss_a, out.loss_l, out.per_structure, out.q_atm1, out.p_atm1,
                 out.vb_term, out.ce_term)
    if not with_gradient:
        call("mdx_denoising_loss", *arguments, status)
        return out
    if B < 1:
        raise ValueError("the gradient of the denoising loss of an empty batch is not defined")
    divisor = float(B if batch_divisor is None else batch_divisor)
    if not divisor > 0.0:
        raise ValueError(f"batch_divisor must be positive, got {batch_divisor}")
    gradient_x, gradient_l = empty(with_x, B, N, D), empty(with_l, B, P)
    gradient_a = empty(with_tables and with_logits, B, N, Cn)
    sums, loss = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(1, dtype=F32, device=dev)
    call("mdx_denoising_loss_gradient", *arguments, divisor, gradient_x, gradient_a, gradient_l, sums, loss, status)
    loss = loss[0]
    if any(t is not None and t.requires_grad for t in (predicted_x, logits, predicted_l)):
        loss = _DenoisingLossFunction.apply(loss, predicted_x, logits, predicted_l, gradient_x, gradient_a, gradient_l)
    return DenoisingLossGradient(*out, gradient_x=gradient_x, gradient_a=gradient_a, gradient_l=gradient_l, loss=loss)


DenoisingLossGradient = namedtuple("DenoisingLossGradient", DenoisingLoss._fields + ("gradient_x", "gradient_a", "gradient_l", "loss"))


class _DenoisingLossFunction(torch.autograd.Function):
    """loss(predicted_x, logits, predicted_l) of mdx_denoising_loss_gradient for predictions that require grad: backward is
    grad_output x the kernel's own gradient buffers, no second launch.  A prediction that is absent, or that the loss does not
    depend on (logits without the tables), has no buffer and gets None."""

    @staticmethod
    def forward(ctx, loss, predicted_x, logits, predicted_l, gradient_x, gradient_a, gradient_l):
        ctx.save_for_backward(gradient_x, gradient_a, gradient_l)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_output):
        asked = ctx.needs_input_grad[1:4]
        return (None, *(grad_output * buffer if wanted and buffer is not None else None
                        for wanted, buffer in zip(asked, ctx.saved_tensors)), None, None, None)


def denoising_loss_and_gradient(*, batch_divisor: Optional[float] = None, **arguments) -> DenoisingLossGradient:
    """The denoising loss AND its gradient in one launch (mdx_denoising_loss_gradient, the family's one-workgroup total
    after it), no host read.  Takes the keyword arguments of `denoising_loss`, and `batch_divisor` (default: B).  Returns a
    DenoisingLossGradient: the fields of DenoisingLoss with the same bits, then
      gradient_x [B, N, D], gradient_a [B, N, C], gradient_l [B, P]   d loss / d predicted_x, logits, predicted_l (None where
                                                                       the part is absent; gradient_a needs logits and tables)
      loss (0-dim f32) = sum_b (lambda_x mean_x[b] + lambda_l mean_l[b] + lambda_a mean_a[b]) / batch_divisor, added in binary64
    When a prediction requires grad, loss carries it: its backward returns grad_output x the buffer for every prediction that
    asked, without a second launch."""
    unknown = sorted(set(arguments) - set(_DENOISING_LOSS_DEFAULTS))
    if unknown:
        raise TypeError(f"denoising_loss_and_gradient() got unexpected keyword arguments {unknown}")
    return _denoising_loss_launch(**{**_DENOISING_LOSS_DEFAULTS, **arguments}, with_gradient=True, batch_divisor=batch_divisor)


_DENOISING_LOSS_DEFAULTS = {name: parameter.default for name, parameter in inspect.signature(denoising_loss).parameters.items()}


ConsistencyLoss = namedtuple("ConsistencyLoss", ["target", "gradient", "per_structure", "loss"])


def _sigma_words(name: str, sigma, batch: int, device) -> torch.Tensor:
    """A Python float or a 0-dim tensor as a one-element f32 device word; a tensor with 1 or `batch` elements as it is (flat)."""
    if not isinstance(sigma, torch.Tensor):
        return torch.full((1,), float(sigma), dtype=F32, device=device)
    if sigma.numel() not in (1, batch):
        raise ValueError(f"{name} has shape {tuple(sigma.shape)}: expected one value, or one per structure, [{batch}]")
    return sigma.detach().to(dtype=F32).reshape(-1).contiguous()


class _ConsistencyLossFunction(torch.autograd.Function):
    """loss(score) of mdx_consistency_loss or mdx_regression_loss for a score that requires grad: backward is grad_output x the
    kernel's own gradient buffer (2 (s - target) / B; / (B N D) for the regression loss), no second launch."""

    @staticmethod
    def forward(ctx, score, loss, gradient):
        ctx.save_for_backward(gradient)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_output):
        gradient, = ctx.saved_tensors
        return grad_output * gradient, None, None


def consistency_loss(x_start, x_end, score=None, *, sigma_start, sigma_end, kmax: int = 4,
                     status: Optional[torch.Tensor] = None) -> ConsistencyLoss:
    """The consistency regularizer's target and loss (mdx_consistency_loss), no host read: x_start, x_end, score f32 [B, N, D];
    sigma_start, sigma_end a Python float, a 0-dim tensor, or a tensor with 1 or B elements (both alike).  Returns a
    ConsistencyLoss of f32 tensors: target [B, N, D] = sigma_start x the score of the wrapped Gaussian of width
    sqrt(sigma_start^2 - sigma_end^2) at wrap(x_start - x_end); gradient [B, N, D] = 2 (score - target) / B; per_structure [B],
    the sums of score (score - 2 target); loss (0-dim), their sum over B.  Without `score` only target is made.  When `score`
    requires grad, loss carries it: its backward returns grad_output x gradient.  An invalid sigma or coordinate gives NaNs
    and its bit in `status` (raise_analytical_status)."""
    _device_only("the consistency loss", x_start=x_start, x_end=x_end, score=score, status=status,
                 sigma_start=sigma_start if isinstance(sigma_start, torch.Tensor) else None,
                 sigma_end=sigma_end if isinstance(sigma_end, torch.Tensor) else None)
    if x_start.dim() != 3:
        raise ValueError(f"x_start has shape {tuple(x_start.shape)}, expected [B, N, D]")
    B, N, D = x_start.shape
    if B < 1:
        raise ValueError("the consistency loss of an empty batch is not defined")
    for name, t in (("x_end", x_end), ("score", score)):
        if t is not None and tuple(t.shape) != (B, N, D):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {(B, N, D)}")
    dev = x_start.device
    words_start, words_end = _sigma_words("sigma_start", sigma_start, B, dev), _sigma_words("sigma_end", sigma_end, B, dev)
    if words_start.numel() != words_end.numel():
        raise ValueError("sigma_start and sigma_end must both hold one value, or both one per structure")
    stride = int(words_start.numel() == B and B > 1)
    with_score = score is not None
    values = score.detach().contiguous() if with_score else None
    target = torch.empty(B, N, D, dtype=F32, device=dev)
    gradient = torch.empty(B, N, D, dtype=F32, device=dev) if with_score else None
    per_structure = torch.empty(B, dtype=F32, device=dev) if with_score else None
    sums = torch.empty(B, dtype=torch.float64, device=dev) if with_score else None
    loss = torch.empty(1, dtype=F32, device=dev) if with_score else None
    call("mdx_consistency_loss", x_start.detach().contiguous(), x_end.detach().contiguous(), values, words_start, words_end, stride,
         B, int(N), int(D), int(kmax), target, gradient, per_structure, sums, loss, status)
    if with_score:
        loss = _ConsistencyLossFunction.apply(score, loss[0], gradient) if score.requires_grad else loss[0]
    return ConsistencyLoss(target=target, gradient=gradient, per_structure=per_structure, loss=loss)


RegressionLoss = namedtuple("RegressionLoss", ["target", "gradient", "per_structure", "loss"])


def regression_loss(score=None, *, target=None, relative_coordinates=None, sigmas=None, equilibrium_relative_coordinates=None,
                    sigma_d_square: Optional[float] = None, kmax: Optional[int] = None, use_permutation_invariance: bool = False,
                    status: Optional[torch.Tensor] = None) -> RegressionLoss:
    """The regression regularizer's target and error (mdx_regression_loss), one call with no host read: score f32 [B, N, D]
    against a target that is either GIVEN (`target` f32 [B, N, D]) or the analytical score network's at `relative_coordinates`
    f32 [B, N, D] with `sigmas` (B values, one per structure), `equilibrium_relative_coordinates` f32 [N, D], `sigma_d_square`,
    `kmax` and `use_permutation_invariance` -- kernels.analytical_score's evaluation, kept in binary64 for the subtraction.
    Returns a RegressionLoss of f32 tensors: target [B, N, D] (the bits of kernels.analytical_score; the given tensor's values);
    gradient [B, N, D] = 2 (score - target) / (B N D); per_structure [B], the sums of (score - target)^2; loss (0-dim), their sum
    over B N D: mean((score - target)^2).  Without `score` (analytical target only) only target is made.  When `score` requires
    grad, loss carries it: its backward returns grad_output x gradient.  An invalid sigma or coordinate gives NaNs in its
    structure and in loss, and its bit in `status` (raise_analytical_status)."""
    given = target is not None
    _device_only("the regression loss", score=score, target=target, relative_coordinates=relative_coordinates,
                 sigmas=sigmas if isinstance(sigmas, torch.Tensor) else None,
                 equilibrium_relative_coordinates=equilibrium_relative_coordinates, status=status)
    if given:
        if score is None:
            raise ValueError("a given target needs a score to be compared with")
        if relative_coordinates is not None or sigmas is not None or equilibrium_relative_coordinates is not None:
            raise ValueError("give either target, or relative_coordinates, sigmas and equilibrium_relative_coordinates: not both")
        shaped = target
    else:
        missing = [name for name, value in (("relative_coordinates", relative_coordinates), ("sigmas", sigmas),
                                            ("equilibrium_relative_coordinates", equilibrium_relative_coordinates),
                                            ("sigma_d_square", sigma_d_square), ("kmax", kmax)) if value is None]
        if missing:
            raise ValueError(f"without a given target the analytical one needs {', '.join(missing)}")
        shaped = relative_coordinates
    if shaped.dim() != 3:
        raise ValueError(f"{'target' if given else 'relative_coordinates'} has shape {tuple(shaped.shape)}, expected [B, N, D]")
    B, N, D = shaped.shape
    if B < 1:
        raise ValueError("the regression loss of an empty batch is not defined")
    if score is not None and tuple(score.shape) != (B, N, D):
        raise ValueError(f"score has shape {tuple(score.shape)}, expected {(B, N, D)}")
    dev = shaped.device
    sites = None
    if not given:
        if tuple(equilibrium_relative_coordinates.shape) != (N, D):
            raise ValueError(f"equilibrium_relative_coordinates has shape {tuple(equilibrium_relative_coordinates.shape)}, "
                             f"expected {(N, D)}")
        if not isinstance(sigmas, torch.Tensor):
            sigmas = torch.full((B,), float(sigmas), dtype=F32, device=dev)
        if sigmas.numel() != B:
            raise ValueError(f"sigmas has shape {tuple(sigmas.shape)}: expected one value per structure, [{B}]")
        sigmas = sigmas.detach().to(dtype=F32).reshape(-1).contiguous()
        relative_coordinates = relative_coordinates.detach().to(dtype=F32).contiguous()
        sites = equilibrium_relative_coordinates.detach().to(dtype=F32).contiguous()
    with_score = score is not None
    values = score.detach().to(dtype=F32).contiguous() if with_score else None
    given_values = target.detach().to(dtype=F32).contiguous() if given else None
    out_target = torch.empty(B, N, D, dtype=F32, device=dev)
    gradient = torch.empty(B, N, D, dtype=F32, device=dev) if with_score else None
    per_structure = torch.empty(B, dtype=F32, device=dev) if with_score else None
    sums = torch.empty(B, dtype=torch.float64, device=dev) if with_score else None
    loss = torch.empty(1, dtype=F32, device=dev) if with_score else None
    call("mdx_regression_loss", relative_coordinates if not given else None, sigmas if not given else None, values, given_values,
         sites, 0.0 if given else float(sigma_d_square), 0 if given else int(kmax), int(bool(use_permutation_invariance)),
         B, int(N), int(D), out_target, gradient, per_structure, sums, loss, status)
    if with_score:
        loss = _ConsistencyLossFunction.apply(score, loss[0], gradient) if score.requires_grad else loss[0]
    return RegressionLoss(target=out_target, gradient=gradient, per_structure=per_structure, loss=loss)


# ----------------------------------------------------------------------------------------------------------------
# the optimizer step: multi-tensor Adam / AdamW and the gradients' global norm (csrc/mdx_optimizer.hip)
# ----------------------------------------------------------------------------------------------------------------
ADAM_CHUNK_ELEMENTS = _hip.ADAM_CHUNK_ELEMENTS       # elements per workgroup: the granule of the per-block table
ADAM_HYPER_NAMES = ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm", "gradient_scale")    # mdx_adam_hyper_fill's order


def adam_chunk_table(counts) -> tuple:
    """(block_tensor, block_offset): per workgroup the tensor it serves and its element offset in it, for tensors of `counts`
    elements each -- ceil(count / ADAM_CHUNK_ELEMENTS) workgroups per tensor, in table order.  Host lists; no device."""
    block_tensor, block_offset = [], []
    for k, count in enumerate(counts):
        if count < 1:
            raise ValueError(f"tensor {k} of the table has {count} elements: a tensor without elements is left out of it")
        for offset in range(0, count, ADAM_CHUNK_ELEMENTS):
            block_tensor.append(k)
            block_offset.append(offset)
    return block_tensor, block_offset


def adam_counter_slots(counts) -> tuple:
    """(slots, total): the entry of the step-counter array of each tensor's first chunk, for tensors of `counts` elements laid
    out one after another -- one entry per chunk of ADAM_CHUNK_ELEMENTS elements, none for a tensor without elements -- and
    the number of entries."""
    slots, total = [], 0
    for count in counts:
        slots.append(total)
        total += -(-int(count) // ADAM_CHUNK_ELEMENTS)
    return slots, total


def _adam_upload(values, dtype, device) -> torch.Tensor:
    """A host list as a device table (the one host-to-device copy of a plan: tests count its calls)."""
    return torch.tensor(values, dtype=dtype, device=device)


@dataclass
class AdamPlan:
    """The device tables of one parameter group for mdx_adam_step / mdx_gradient_norm, and the norm's workspace."""

    key: tuple
    addresses: Optional[torch.Tensor]      # int64 [tensors, 4]: p, g, exp_avg, exp_avg_sq
    counts: Optional[torch.Tensor]         # int64 [tensors]
    slots: Optional[torch.Tensor]          # int32 [tensors]: the entry of the step counters of each tensor's first chunk
    block_tensor: Optional[torch.Tensor]   # int32 [blocks]
    block_offset: Optional[torch.Tensor]   # int64 [blocks]
    number_of_blocks: int
    partials: Optional[torch.Tensor]       # f64 [blocks]
    norm: Optional[torch.Tensor]           # f64 [2]: the norm and its square
    device: Optional[torch.device]
    counters: int = 0                      # the step-counter entries the plan reaches: 1 + the highest


_ADAM_PLANS = {}
_ADAM_PLANS_KEPT = 64


def adam_plan(parameters, gradients=None, exp_avg=None, exp_avg_sq=None, slots=None, names=None) -> AdamPlan:
    """The tables of a parameter group, built once per tuple of (data pointers, count, slot) and cached under it: parameters
    with their gradients (default: each parameter's .grad), first and second moments, and the entry of the step-counter array
    of each one's first chunk (default: adam_counter_slots of the parameters' sizes: one entry per chunk, in order).  Refused before anything is uploaded or launched: a host tensor (MdxError), a dtype other
    than float32 or a non-contiguous tensor (ValueError naming it), moments or gradients of another size.  A tensor without
    elements is skipped: it takes no row of the tables."""
    parameters = list(parameters)
    count = len(parameters)
    gradients = [p.grad for p in parameters] if gradients is None else list(gradients)
    names = [f"parameters[{i}]" for i in range(count)] if names is None else list(names)
    slots = adam_counter_slots([p.numel() for p in parameters])[0] if slots is None else [int(s) for s in slots]
    if exp_avg is None or exp_avg_sq is None:
        raise ValueError("adam_plan needs the first and second moments (exp_avg, exp_avg_sq) of every parameter")
    exp_avg, exp_avg_sq = list(exp_avg), list(exp_avg_sq)
    if not (len(gradients) == len(exp_avg) == len(exp_avg_sq) == len(names) == len(slots) == count):
        raise ValueError("adam_plan: parameters, gradients, exp_avg, exp_avg_sq, slots and names must have one entry per parameter")
    rows, sizes, kept_slots = [], [], []
    for name, p, g, m, v, slot in zip(names, parameters, gradients, exp_avg, exp_avg_sq, slots):
        group = {name: p, name + ".grad": g, name + ".exp_avg": m, name + ".exp_avg_sq": v}
        if any(t is None for t in group.values()):
            raise ValueError(f"{name}: a parameter without a gradient or moments is left out of the plan, not passed as None")
        _device_only("the optimizer step", **group)
        for label, t in group.items():
            if t.dtype != F32:
                raise ValueError(f"{label} has dtype {t.dtype}: the optimizer step serves float32 only")
            if not t.is_contiguous():
                raise ValueError(f"{label} is not contiguous: the optimizer step addresses each tensor as one flat array")
            if t.numel() != p.numel():
                raise ValueError(f"{label} has {t.numel()} elements, {name} has {p.numel()}")
        if p.numel() == 0:
            continue
        rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()))
        sizes.append(p.numel())
        kept_slots.append(slot)
    key = tuple(row + (size, slot) for row, size, slot in zip(rows, sizes, kept_slots))
    plan = _ADAM_PLANS.get(key)
    if plan is not None:
        return plan
    if not rows:
        plan = AdamPlan(key, None, None, None, None, None, 0, None, None, None)
    else:
        device = next(p for p in parameters if p.numel()).device
        block_tensor, block_offset = adam_chunk_table(sizes)
        plan = AdamPlan(key, _adam_upload(rows, I64, device), _adam_upload(sizes, I64, device),
                        _adam_upload(kept_slots, I32, device), _adam_upload(block_tensor, I32, device),
                        _adam_upload(block_offset, I64, device), len(block_tensor),
                        torch.empty(len(block_tensor), dtype=F64, device=device), torch.empty(2, dtype=F64, device=device), device,
                        max(slot + -(-size // ADAM_CHUNK_ELEMENTS) for size, slot in zip(sizes, kept_slots)))
    if len(_ADAM_PLANS) >= _ADAM_PLANS_KEPT:
        _ADAM_PLANS.clear()
    _ADAM_PLANS[key] = plan
    return plan


def adam_hyper_fill(hyper, lr, beta1, beta2, eps, weight_decay, max_norm, gradient_scale):
    """Write the hyper-parameter buffer (f64 [ADAM_HYPER_COUNT], device) from host values: one tiny launch, no copy."""
    _device_only("the optimizer step", hyper=hyper)
    if hyper.numel() < _hip.ADAM_HYPER_COUNT:
        raise ValueError(f"hyper holds {hyper.numel()} values, mdx_adam_hyper_fill writes {_hip.ADAM_HYPER_COUNT}")
    call("mdx_adam_hyper_fill", float(lr), float(beta1), float(beta2), float(eps), float(weight_decay), float(max_norm),
         float(gradient_scale), hyper)


def gradient_norm(plan: AdamPlan) -> Optional[torch.Tensor]:
    """f64 [2] on the device: the 2-norm of all gradients of the plan and its square (mdx_gradient_norm: two launches, no host
    read, a fixed summation order).  The plan's own buffer: the next call overwrites it.  None for a plan without tensors."""
    if plan.number_of_blocks == 0:
        return None
    call("mdx_gradient_norm", plan.addresses, plan.counts, plan.block_tensor, plan.block_offset, plan.number_of_blocks,
         plan.partials, plan.norm)
    return plan.norm


def adam_step(plan: AdamPlan, steps, hyper, decoupled_weight_decay: bool, zero_gradients: bool = False, clip: bool = False,
              status: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """One Adam / AdamW step of every tensor of the plan in one launch (mdx_adam_step); with `clip`, gradient_norm first and
    the gradients scaled by min(1, max_norm / (norm + 1e-6)) inside the step: .grad itself is not rewritten.  steps int32: the
    counters, one entry per chunk at the plan's slots (adam_counter_slots); hyper f64 [ADAM_HYPER_COUNT] as adam_hyper_fill
    writes it.  Returns the norm buffer when one was computed.  A gradient that is not finite sets STATUS_OPTIMIZER_NONFINITE in
    `status` (int32 [1], optional)."""
    if plan.number_of_blocks == 0:
        return None
    _device_only("the optimizer step", steps=steps, hyper=hyper, status=status)
    if steps.numel() < plan.counters:
        raise ValueError(f"the plan reaches {plan.counters} step counters; steps holds {steps.numel()}")
    if hyper.numel() < _hip.ADAM_HYPER_COUNT:
        raise ValueError(f"hyper holds {hyper.numel()} values, expected {_hip.ADAM_HYPER_COUNT}")
    norm = gradient_norm(plan) if clip else None
    call("mdx_adam_step", plan.addresses, plan.counts, plan.slots, plan.block_tensor, plan.block_offset, plan.number_of_blocks,
         steps, hyper, norm, int(bool(decoupled_weight_decay)), int(bool(zero_gradients)), status)
    return norm


# ----------------------------------------------------------------------------------------------------------------
# sampling metrics: sort and two-sample Kolmogorov-Smirnov rank (csrc/mdx_metrics.hip)
# ----------------------------------------------------------------------------------------------------------------
KS_MAX_SAMPLES = _hip.KS_MAX_SAMPLES     # per sample: every product of a count and a reduced size stays below 2^48
KS_SORT_TILE = _hip.KS_SORT_TILE         # keys per workgroup of the radix sort: the granule at which it changes behaviour


def _ks_sample(name: str, values) -> torch.Tensor:
    """A sample as the kernels take it: a flat contiguous device tensor; refused before any launch otherwise."""
    if not isinstance(values, torch.Tensor):
        raise ValueError(f"{name} must be a torch.Tensor, got {type(values).__name__}")
    if values.numel() < 1:
        raise ValueError(f"{name} is empty: the Kolmogorov-Smirnov distance of an empty sample is not defined")
    if values.numel() > KS_MAX_SAMPLES:
        raise ValueError(f"{name} holds {values.numel()} values, more than KS_MAX_SAMPLES = {KS_MAX_SAMPLES}")
    if not values.is_cuda:
        raise ValueError(f"{name} lives on {values.device}: the Kolmogorov-Smirnov kernels run on the GPU only (no CPU fallback)")
    values = values.detach().reshape(-1)
    if values.dtype not in (F32, F64):
        values = values.to(F64)
    return values.contiguous()


def sort_keys(values, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ascending sort, f64 [n], of the n values of a device tensor (mdx_sort_keys): binary32 and binary64 are sorted in their
    own width and widened exactly, any other dtype is taken as binary64; -0.0 comes out as +0.0; `values` is not modified.  A
    hand-written radix sort: no vendor sort, no host read, capturable, the same bits on every replay.  A NaN sets
    STATUS_KS_NAN in `status` (int32 [1], optional) and leaves the output unspecified."""
    values = _ks_sample("values", values)
    if status is not None and not status.is_cuda:
        raise ValueError(f"status lives on {status.device}: the Kolmogorov-Smirnov kernels run on the GPU only")
    n, wide = values.numel(), int(values.dtype == F64)
    workspace = torch.empty(int(lib().mdx_sort_keys_workspace_bytes(n, wide)), dtype=torch.uint8, device=values.device)
    out = torch.empty(n, dtype=F64, device=values.device)
    call("mdx_sort_keys", values, n, wide, out, workspace, status)
    return out


def ks_two_sample_numerator(a, b, status: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [1] on the device: h = max over x of |c_a(x) n2/g - c_b(x) n1/g| with g = gcd(n1, n2) and c_s(x) the number of
    elements of sample s that are <= x (mdx_sort_keys on both samples, then mdx_ks_two_sample_sorted); the two-sided
    Kolmogorov-Smirnov distance is h / lcm(n1, n2).  Samples of different dtype are both taken as binary64.  No host read:
    the call can be captured; a NaN in either sample sets STATUS_KS_NAN in `status` (int32 [1], optional)."""
    a, b = _ks_sample("a", a), _ks_sample("b", b)
    if a.device != b.device:
        raise ValueError(f"a lives on {a.device} and b on {b.device}")
    if a.dtype != b.dtype:
        a, b = a.to(F64), b.to(F64)
    a_sorted, b_sorted = sort_keys(a, status), sort_keys(b, status)
    n1, n2 = a_sorted.numel(), b_sorted.numel()
    workspace = torch.empty(int(lib().mdx_ks_two_sample_workspace_bytes(n1, n2)), dtype=torch.uint8, device=a.device)
    numerator = torch.empty(1, dtype=I64, device=a.device)
    call("mdx_ks_two_sample_sorted", a_sorted, n1, b_sorted, n2, workspace, numerator)
    return numerator


def kolmogorov_limit_p_value(scaled_distance: float) -> float:
    """Kolmogorov's limiting law Q(lambda) = P(sup |B| > lambda) in binary64 host arithmetic, clipped to [0, 1]:
    2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 lambda^2) for lambda >= 1.18, 1 - sqrt(2 pi) / lambda sum_{k>=1} exp(-(2k-1)^2 pi^2 /
    (8 lambda^2)) below that, 1 for lambda <= 0 (scipy.stats.kstwobign.sf).  Either series needs a handful of terms there."""
    import math
    lam = float(scaled_distance)
    if math.isnan(lam):
        return lam
    if lam <= 0.0:
        return 1.0
    total = 0.0
    if lam >= 1.18:
        for k in range(1, 8):
            total += (-1.0) ** (k - 1) * math.exp(-2.0 * k * k * lam * lam)
        value = 2.0 * total
    else:
        for k in range(1, 8):
            total += math.exp(-((2 * k - 1) ** 2) * math.pi ** 2 / (8.0 * lam * lam))
        value = 1.0 - math.sqrt(2.0 * math.pi) / lam * total
    return min(1.0, max(0.0, value))


def ks_two_sample(a, b):
    """(distance, p_value), two Python floats, of the two-sided two-sample Kolmogorov-Smirnov test between the device tensors
    a and b: what the reference asks scipy.stats.ks_2samp for (metrics/kolmogorov_smirnov_metrics.py:59-75), computed where
    the samples are.  The distance is scipy's statistic, h / lcm(n1, n2) in one correctly rounded division of the integer
    numerator (ks_two_sample_numerator); the numerator and the status word are read here, the feature's one point of host
    contact.  A NaN in either sample gives (nan, nan), scipy's nan_policy='propagate'.
    DEVIATION from the reference: the p-value is Kolmogorov's limiting law at lambda = d sqrt(n1 n2 / (n1 + n2))
    (kolmogorov_limit_p_value), not scipy's method='auto' (exact path counting up to 10 000 samples, the finite-n kstwo law
    above): the two differ by a few per cent at p ~ 0.3 (profiles/r16_ks_metrics.md)."""
    import math
    a, b = _ks_sample("a", a), _ks_sample("b", b)            # the refusals, before anything is allocated on a device
    n1, n2 = a.numel(), b.numel()
    status = torch.zeros(1, dtype=I32, device=a.device)
    numerator = ks_two_sample_numerator(a, b, status)
    if _take_status_bits(status, _hip.STATUS_KS_NAN) & _hip.STATUS_KS_NAN:
        return float("nan"), float("nan")
    distance = int(numerator.item()) / math.lcm(n1, n2)
    return distance, kolmogorov_limit_p_value(distance * math.sqrt(n1 * n2 / (n1 + n2)))


# ----------------------------------------------------------------------------------------------------------------
# fused MLP score network
# ----------------------------------------------------------------------------------------------------------------
class MlpPack:
    """Device copy of an MLPScoreNetwork's parameters in the layout of mdx_mlp_t (transposed weights, [in, out]).

    Built from the module's state at construction; rebuild it if the parameters change."""

    def __init__(self, network, device):
        hp = network._hyper_params
        if getattr(network, "use_permutation_invariance", False) or getattr(network, "use_time_dependent_prefactor", False):
            raise _hip.MdxError("the fused MLP kernels implement the plain unconditional forward "
                                "(no permutation symmetrisation, no time prefactor)")
        n_hidden = len(network.mlp_layers)
        if n_hidden > _hip.MLP_MAX_HIDDEN:
            raise _hip.MdxError(f"at most {_hip.MLP_MAX_HIDDEN} hidden layers are supported by the fused MLP kernels")
        self._keep = []

        def wt(linear):
            t = linear.weight.detach().to(device=device, dtype=F32).t().contiguous()
            self._keep.append(t)
            return t.data_ptr()

        def bias(linear):
            t = linear.bias.detach().to(device=device, dtype=F32).contiguous()
            self._keep.append(t)
            return t.data_ptr()

        m = Mlp()
        m.number_of_atoms, m.spatial_dimension, m.num_classes = network._natoms, network.spatial_dimension, network.num_classes
        m.hidden_size, m.n_hidden = hp.hidden_dimensions_size, n_hidden
        m.e_coordinates = hp.relative_coordinates_embedding_dimensions_size
        m.e_noise, m.e_time = hp.noise_embedding_dimensions_size, hp.time_embedding_dimensions_size
        m.e_atom_type = hp.atom_type_embedding_dimensions_size
        m.e_lattice = hp.lattice_parameters_embedding_dimensions_size
        for name, layer in (("coordinates", network.relative_coordinates_embedding_layer),
                            ("noise", network.noise_embedding_layer), ("time", network.time_embedding_layer),
                            ("atom_type", network.atom_type_embedding_layer),
                            ("lattice", network.lattice_parameters_embedding_layer)):
            setattr(m, f"w_{name}_t", wt(layer))
            setattr(m, f"b_{name}", bias(layer))
        for k, layer in enumerate(network.mlp_layers):
            m.w_hidden_t[k] = wt(layer)
            m.b_hidden[k] = bias(layer)
        for name, layer in (("a", network.output_A_layer), ("x", network.output_X_layer), ("l", network.output_L_layer)):
            setattr(m, f"w_out_{name}_t", wt(layer))
            setattr(m, f"b_out_{name}", bias(layer))
        m.packed_image = None
        m.folded_input = None
        first, _, out = _folded_matrices(network, m)
        self.folded = _folded_layer(first, device)
        m.folded_output = None
        self.folded_out = _folded_layer(out, device)
        m.folded_padded = None
        if self.folded is not None and self.folded_out is not None:
            m.folded_input = self.folded.data_ptr()
            m.folded_output = self.folded_out.data_ptr()
            self.folded_padded = _pad_folded_layers(network, m, device)
            if self.folded_padded is not None:
                m.folded_padded = self.folded_padded.data_ptr()
        n_floats = lib().mdx_mlp_image_floats(C.byref(m))
        if n_floats > 0:      # the kernels' own layout, built once: kernel start-up becomes one coalesced copy
            self.image = torch.empty(n_floats, dtype=F32, device=device)
            with torch.cuda.device(device):
                call("mdx_mlp_pack_image", C.byref(m), self.image)
            m.packed_image = self.image.data_ptr()
        self.c_struct = m
        self.device = torch.device(device)
        self.number_of_atoms, self.num_classes, self.spatial_dimension = m.number_of_atoms, m.num_classes, m.spatial_dimension


def _folded_matrices(network, m):
    """The network as n_hidden linear maps, in binary64 on the host: ((W_first [H, F], b_first [H]) or None, [(W_k, b_k) of the
    middle hidden layers], (W_out [outputs, H], b_out) or None).  The ONLY place the folded products are formed, each rounded
    once by its user, so mdx_mlp_t.folded_input, folded_output and folded_padded hold the same bits.
    first: the five embedding layers folded into hidden layer 0 -- they are linear and no activation lies between them and the
    first hidden layer (mlp_score_network.py:299-344); its input is [cos (N d) | sin (N d) | sigma | t | atom-type embeddings
    (N e_a) | lattice emb. (e_l)].  None when hidden layer 0 does not have that input width (then nothing is folded).
    out: the last hidden layer (no activation follows it, mlp_score_network.py:337-344) folded into the three output heads,
    outputs ordered logits | score_x | score_l.  Needs >= 2 hidden layers."""
    f64 = torch.float64
    with torch.no_grad():
        w0 = network.mlp_layers[0].weight.detach().to(f64).cpu()           # [H, ec + en + et + N ea + el]
        b0 = network.mlp_layers[0].bias.detach().to(f64).cpu()
        ec, en, et = m.e_coordinates, m.e_noise, m.e_time
        na = m.number_of_atoms * m.e_atom_type
        o1, o2, o3, o4 = ec, ec + en, ec + en + et, ec + en + et + na
        if w0.shape[1] != o4 + m.e_lattice:
            return None, [], None
        cpu = lambda t: t.detach().to(f64).cpu()       # noqa: E731
        wc, bc = cpu(network.relative_coordinates_embedding_layer.weight), cpu(network.relative_coordinates_embedding_layer.bias)
        wn, bn = cpu(network.noise_embedding_layer.weight), cpu(network.noise_embedding_layer.bias)
        wt_, bt = cpu(network.time_embedding_layer.weight), cpu(network.time_embedding_layer.bias)
        first = torch.cat([w0[:, :o1] @ wc,                     # [H, 2 N d]: cos block then sin block, as the module
                           w0[:, o1:o2] @ wn,                   # [H, 1]  sigma
                           w0[:, o2:o3] @ wt_,                  # [H, 1]  time
                           w0[:, o3:o4],                        # [H, N ea]
                           w0[:, o4:]], dim=1)                  # [H, el]
        first_bias = b0 + w0[:, :o1] @ bc + w0[:, o1:o2] @ bn + w0[:, o2:o3] @ bt
        if len(network.mlp_layers) < 2:
            return (first, first_bias), [], None
        mids = [(cpu(layer.weight), cpu(layer.bias)) for layer in list(network.mlp_layers)[1:-1]]
        last = network.mlp_layers[-1]
        heads = (network.output_A_layer, network.output_X_layer, network.output_L_layer)
        w_heads = torch.cat([cpu(h.weight) for h in heads], dim=0)        # [N C + N d + nl, H]
        b_heads = torch.cat([cpu(h.bias) for h in heads], dim=0)
        return (first, first_bias), mids, (w_heads @ cpu(last.weight), w_heads @ cpu(last.bias) + b_heads)


def _folded_layer(folded, device):
    """mdx_mlp_t.folded_input / folded_output: one (W, b) of _folded_matrices as [quad image | bias], rounded once; None stays."""
    if folded is None:
        return None
    return torch.cat([_quad_image(folded[0]), folded[1]]).to(device=device, dtype=F32).contiguous()


def _pad_folded_layers(network, m, device):
    """mdx_mlp_t.folded_padded: the folded layers zero-padded to the fixed sizes of the padded register-resident family
    (64 neurons, 16 / 32 / 48 first-layer quads, 64 outputs), or None when the network is outside that family's limits.
    The same binary64 products as folded_input / folded_output, rounded once: the padded family and the generic folded forward
    compute the same bits."""
    n_hidden = len(network.mlp_layers)
    n_in = 2 * m.number_of_atoms * m.spatial_dimension + 2 + m.number_of_atoms * m.e_atom_type + m.e_lattice
    d = m.spatial_dimension
    n_out = m.number_of_atoms * m.num_classes + m.number_of_atoms * d + d * (d + 1) // 2
    if m.hidden_size > 64 or m.number_of_atoms > 8 or not 2 <= n_hidden <= 4 or n_out > 64 or n_in > 192:
        return None
    first, mids, out = _folded_matrices(network, m)
    if first is None or first[0].shape[1] != n_in:
        return None

    def padded(w, b, inputs):
        wp = torch.zeros(64, inputs, dtype=torch.float64)
        wp[: w.shape[0], : w.shape[1]] = w
        bp = torch.zeros(64, dtype=torch.float64)
        bp[: b.shape[0]] = b
        return [_quad_image(wp), bp]

    parts = padded(*first, 64 * ((n_in + 63) // 64))
    for w, b in mids + [out]:
        parts += padded(w, b, 64)
    return torch.cat(parts).to(device=device, dtype=F32).contiguous()


def _quad_image(matrix64: torch.Tensor) -> torch.Tensor:
    """[outputs, inputs] matrix -> the kernels' [ceil(inputs/4)][outputs][4] layout (inputs zero-padded)."""
    n_out, n_in = matrix64.shape
    quads = (n_in + 3) // 4
    padded = torch.zeros(n_out, quads * 4, dtype=matrix64.dtype)
    padded[:, :n_in] = matrix64
    return padded.t().reshape(quads, 4, n_out).permute(0, 2, 1).contiguous().reshape(-1)


def mlp_forward(pack: MlpPack, atom_types, x, l, time, sigma):
    """Fused forward of the MLP score network: returns (logits [B,N,C] with MASK = -inf, score_x, score_l)."""
    B, N, d = x.shape
    assert N == pack.number_of_atoms and d == pack.spatial_dimension
    logits = torch.empty(B, N, pack.num_classes, dtype=F32, device=x.device)
    score_x = torch.empty_like(x)
    score_l = torch.empty_like(l)
    call("mdx_mlp_forward", C.byref(pack.c_struct), atom_types, x, l, time, sigma, B, logits, score_x, score_l)
    return logits, score_x, score_l


# ----------------------------------------------------------------------------------------------------------------
# training the MLP score network: forward with an activation record, and the parameters' gradient (csrc/mdx_mlp_train.hip)
# ----------------------------------------------------------------------------------------------------------------
MLP_TRAIN_STRUCTURES_PER_SLAB = _hip.MLP_TRAIN_STRUCTURES_PER_SLAB     # structures one workgroup of the backward adds up


def mlp_train_layers(network) -> list:
    """[(name of the nn.Linear in the module, the nn.Linear)] of the unconditional forward, in the order of the address table
    and of the flat gradient buffer: the order named_parameters() gives these parameters."""
    names = ["relative_coordinates_embedding_layer", "noise_embedding_layer", "time_embedding_layer",
             "atom_type_embedding_layer", "lattice_parameters_embedding_layer"]
    layers = [(name, getattr(network, name)) for name in names]
    layers += [(f"mlp_layers.{k}", layer) for k, layer in enumerate(network.mlp_layers)]
    return layers + [(name, getattr(network, name)) for name in ("output_A_layer", "output_X_layer", "output_L_layer")]


def mlp_train_refusal(network) -> Optional[str]:
    """Why the training kernels do not cover this network, or None: they evaluate MLPScoreNetwork._single, nothing around it."""
    if getattr(network, "use_permutation_invariance", False):
        return "the fused MLP training kernels do not cover the permutation symmetrisation (use_permutation_invariance)"
    if getattr(network, "use_time_dependent_prefactor", False):
        return "the fused MLP training kernels do not cover the time-dependent prefactor (use_time_dependent_prefactor)"
    if len(network.mlp_layers) > _hip.MLP_MAX_HIDDEN:
        return f"the fused MLP training kernels serve at most {_hip.MLP_MAX_HIDDEN} hidden layers, the network has {len(network.mlp_layers)}"
    if network.num_classes > _hip.MAX_CLASSES:
        return f"the fused MLP training kernels serve at most {_hip.MAX_CLASSES} classes, the network has {network.num_classes}"
    return None


@dataclass
class MlpTrainPlan:
    """What mdx_mlp_train_forward / _backward need of one MLPScoreNetwork: the shape words, the device table of the parameters'
    addresses and the parameters themselves in table order (weight, bias per layer)."""

    key: tuple
    shape: Any                           # int32 [MLP_TRAIN_SHAPE_COUNT], host (ctypes)
    addresses: torch.Tensor              # int64 [2 layers], device
    names: list                          # the parameters' names in the module, in table order
    parameters: list
    sizes: list
    number_of_atoms: int
    spatial_dimension: int
    num_classes: int
    lattice_parameters: int
    record_floats: int
    parameter_count: int
    device: torch.device
    workspace: Optional[torch.Tensor] = None      # f64, grown on demand: the slabs of the last backward

    def workspace_doubles(self, batch: int) -> int:
        return int(lib().mdx_mlp_train_workspace_doubles(self.shape, int(batch)))

    def views(self, flat: torch.Tensor) -> list:
        """The per-parameter views of a flat gradient buffer, in table order, each of its parameter's shape."""
        return [piece.view(p.shape) for piece, p in zip(torch.split(flat, self.sizes), self.parameters)]


_MLP_TRAIN_PLANS = {}
_MLP_TRAIN_PLANS_KEPT = 16


def mlp_train_plan(network) -> MlpTrainPlan:
    """The plan of `network`, built once per tuple of (shape, data pointers) and cached under it -- the parameters are read in
    place, so an optimizer step needs no new plan, and a parameter that moved gets one.  Refused before anything is uploaded:
    a network the kernels do not cover (MdxError with the reason), a host parameter (MdxError), a parameter that is not float32
    or not contiguous (ValueError naming it)."""
    reason = mlp_train_refusal(network)
    if reason:
        raise _hip.MdxError(reason)
    hp = network._hyper_params
    words = (network._natoms, network.spatial_dimension, network.num_classes, hp.hidden_dimensions_size, len(network.mlp_layers),
             hp.relative_coordinates_embedding_dimensions_size, hp.noise_embedding_dimensions_size,
             hp.time_embedding_dimensions_size, hp.atom_type_embedding_dimensions_size,
             hp.lattice_parameters_embedding_dimensions_size)
    names, parameters = [], []
    for name, layer in mlp_train_layers(network):
        names += [name + ".weight", name + ".bias"]
        parameters += [layer.weight, layer.bias]
    _device_only("the MLP training step", **dict(zip(names, parameters)))
    for name, p in zip(names, parameters):
        if p.dtype != F32:
            raise ValueError(f"{name} has dtype {p.dtype}: the MLP training kernels serve float32 only")
        if not p.is_contiguous():
            raise ValueError(f"{name} is not contiguous: the MLP training kernels read each parameter as one [out, in] array")
    key = words + tuple(p.data_ptr() for p in parameters)
    plan = _MLP_TRAIN_PLANS.get(key)
    if plan is not None and all(held is p for held, p in zip(plan.parameters, parameters)):
        return plan
    shape = (C.c_int32 * _hip.MLP_TRAIN_SHAPE_COUNT)(*words)
    record_floats, parameter_count = lib().mdx_mlp_train_record_floats(shape), lib().mdx_mlp_train_parameter_count(shape)
    sizes = [p.numel() for p in parameters]
    if record_floats < 0 or parameter_count != sum(sizes):
        raise _hip.MdxError(f"the MLP training kernels do not serve the shape {words}: the library counts {parameter_count} "
                            f"parameters, the module's layers hold {sum(sizes)}")
    device = parameters[0].device
    d = network.spatial_dimension
    plan = MlpTrainPlan(key, shape, _adam_upload([p.data_ptr() for p in parameters], I64, device), names, parameters, sizes,
                        network._natoms, d, network.num_classes, d * (d + 1) // 2, int(record_floats), int(parameter_count), device)
    if len(_MLP_TRAIN_PLANS) >= _MLP_TRAIN_PLANS_KEPT:
        _MLP_TRAIN_PLANS.clear()
    _MLP_TRAIN_PLANS[key] = plan
    return plan


MlpTrainForward = namedtuple("MlpTrainForward", ["logits", "score_x", "score_l", "record"])
MlpTrainGradients = namedtuple("MlpTrainGradients", ["flat", "views"])


def mlp_train_forward(plan: MlpTrainPlan, atom_types, x, l, time, sigma) -> MlpTrainForward:
    """MLPScoreNetwork._single in one launch, on the module's own parameters (mdx_mlp_train_forward): the RAW head outputs --
    logits [B, N, C] without the -inf of the MASK class, score_x [B, N, d], score_l [B, nl] -- and the activation record
    [B, plan.record_floats] that mlp_train_backward reads.  time, sigma: [B, 1] or [B]."""
    _device_only("the MLP training forward", atom_types=atom_types, x=x, l=l, time=time, sigma=sigma)
    if x.dim() != 3 or tuple(x.shape[1:]) != (plan.number_of_atoms, plan.spatial_dimension):
        raise ValueError(f"x has shape {tuple(x.shape)}, expected [B, {plan.number_of_atoms}, {plan.spatial_dimension}]")
    B = x.shape[0]
    for name, t, shape in (("atom_types", atom_types, (B, plan.number_of_atoms)), ("l", l, (B, plan.lattice_parameters))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape}")
    for name, t in (("time", time), ("sigma", sigma)):
        if t.numel() != B:
            raise ValueError(f"{name} has shape {tuple(t.shape)}: expected one value per structure, [{B}, 1]")
    logits = torch.empty(B, plan.number_of_atoms, plan.num_classes, dtype=F32, device=x.device)
    score_x = torch.empty(B, plan.number_of_atoms, plan.spatial_dimension, dtype=F32, device=x.device)
    score_l = torch.empty(B, plan.lattice_parameters, dtype=F32, device=x.device)
    record = torch.empty(B, plan.record_floats, dtype=F32, device=x.device)
    call("mdx_mlp_train_forward", plan.shape, plan.addresses, atom_types, x, l, time, sigma, B, logits, score_x, score_l, record)
    return MlpTrainForward(logits, score_x, score_l, record)


def mlp_train_backward(plan: MlpTrainPlan, record, grad_logits, grad_x, grad_l, out=None, accumulate: bool = False,
                       scale: float = 1.0, workspace=None) -> MlpTrainGradients:
    """The gradient of every parameter of the plan from a forward's record and the cotangents of its three outputs, each of
    which may be None (mdx_mlp_train_backward: two launches, a fixed summation order, each element rounded to binary32 once).
    out: the flat float32 buffer [plan.parameter_count] in table order (default: a fresh one); `accumulate` adds its old value
    before the rounding, `scale` multiplies the sum (1 / accumulate_grad_batches).  workspace: f64, at least
    plan.workspace_doubles(B) (default: the plan's own, grown on demand).  Returns (flat, its per-parameter views)."""
    _device_only("the MLP training backward", record=record, grad_logits=grad_logits, grad_x=grad_x, grad_l=grad_l, out=out,
                 workspace=workspace)
    if record.dim() != 2 or record.shape[1] != plan.record_floats:
        raise ValueError(f"record has shape {tuple(record.shape)}, expected [B, {plan.record_floats}]")
    B = record.shape[0]
    expected = (("grad_logits", grad_logits, (B, plan.number_of_atoms, plan.num_classes)),
                ("grad_x", grad_x, (B, plan.number_of_atoms, plan.spatial_dimension)), ("grad_l", grad_l, (B, plan.lattice_parameters)))
    for name, t, shape in expected:
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {shape}")
    if out is None:
        if accumulate:
            raise ValueError("accumulate adds to the buffer's old value: it needs `out`")
        out = torch.empty(plan.parameter_count, dtype=F32, device=record.device)
    elif out.dim() != 1 or out.numel() != plan.parameter_count:
        raise ValueError(f"out has shape {tuple(out.shape)}, expected [{plan.parameter_count}]")
    needed = plan.workspace_doubles(B)
    if workspace is None:
        if plan.workspace is None or plan.workspace.numel() < needed:
            plan.workspace = torch.empty(max(needed, 1), dtype=F64, device=record.device)
        workspace = plan.workspace
    elif workspace.numel() < needed:
        raise ValueError(f"workspace holds {workspace.numel()} doubles, a batch of {B} needs {needed}")
    call("mdx_mlp_train_backward", plan.shape, plan.addresses, record, grad_logits, grad_x, grad_l, B, workspace,
         int(bool(accumulate)), float(scale), out)
    return MlpTrainGradients(out, plan.views(out))


class _MlpTrainFunction(torch.autograd.Function):
    """(logits, score_x, score_l) of mdx_mlp_train_forward as a function of the plan's parameters: backward is
    mdx_mlp_train_backward into a fresh flat buffer, whose per-parameter views autograd accumulates into .grad."""

    @staticmethod
    def forward(ctx, plan, atom_types, x, l, time, sigma, *parameters):
        out = mlp_train_forward(plan, atom_types, x, l, time, sigma)
        ctx.plan = plan
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(out.record, *parameters)       # the parameters: autograd refuses a backward after they changed
        return out.logits, out.score_x, out.score_l

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_logits, grad_x, grad_l):
        record = ctx.saved_tensors[0]
        given = [None if g is None else g.contiguous() for g in (grad_logits, grad_x, grad_l)]
        gradients = mlp_train_backward(ctx.plan, record, *given)
        return (None,) * 6 + tuple(view if wanted else None for view, wanted in zip(gradients.views, ctx.needs_input_grad[6:]))


def mlp_train_apply(plan: MlpTrainPlan, atom_types, x, l, time, sigma):
    """(logits, score_x, score_l) with a grad_fn that reaches the plan's parameters (raw logits: the caller fills the MASK class)."""
    return _MlpTrainFunction.apply(plan, atom_types, x, l, time, sigma, *plan.parameters)


NOISE_WORKSPACE_MAX_FLOATS = 1 << 28       # 1 GiB cap; longer segments are split into several launches by the library
NOISE_WORKSPACE_MIN_ITERATIONS = 1024       # first allocation holds at least this many iterations (within the cap)


class NoiseWorkspace:
    """The pre-drawn-noise buffer of mdx_mlp_pc_sample: sized by the library, grown on demand, owned by ONE caller (a
    generator or a bench loop), so that two samplers on different streams never share records.  A buffer that is
    replaced is handed to the allocator with record_stream, i.e. it is not reused before the launches that read it
    have completed."""

    def __init__(self):
        self.buffer = None

    def floats_needed(self, pack: "MlpPack", number_of_corrector_steps: int, atom_type_transition_in_corrector: bool,
                      n_iterations: int, batch: int) -> int:
        need = lib().mdx_mlp_pc_sample_workspace_floats(C.byref(pack.c_struct), int(number_of_corrector_steps),
                                                        int(bool(atom_type_transition_in_corrector)), int(n_iterations),
                                                        int(batch))
        if need < 0:
            raise _hip.MdxError("mdx_mlp_pc_sample_workspace_floats: invalid argument")
        return need

    def get(self, pack: "MlpPack", number_of_corrector_steps: int, atom_type_transition_in_corrector: bool,
            n_iterations: int, batch: int, device) -> torch.Tensor:
        need = self.floats_needed(pack, number_of_corrector_steps, atom_type_transition_in_corrector, n_iterations, batch)
        per_iteration = need // max(int(n_iterations), 1)
        need = max(min(need, NOISE_WORKSPACE_MAX_FLOATS), per_iteration, 1)
        buf = self.buffer
        if buf is None or buf.numel() < need or buf.device != torch.device(device):
            # allocate with headroom (a device allocation costs ~100 us, more than a short segment's kernels): room for
            # NOISE_WORKSPACE_MIN_ITERATIONS iterations of this shape, within the cap
            roomy = min(max(need, NOISE_WORKSPACE_MIN_ITERATIONS * per_iteration), max(NOISE_WORKSPACE_MAX_FLOATS, need))
            if buf is not None and buf.is_cuda:
                buf.record_stream(torch.cuda.current_stream(buf.device))
            buf = self.buffer = torch.empty(roomy, dtype=F32, device=device)
        return buf


def mlp_pc_sample(sched: DeviceSchedule, pack: MlpPack, flags: PcFlags, number_of_corrector_steps: int,
                  atom_type_transition_in_corrector: bool, start_index: int, n_iterations: int, rng: Rng,
                  atom_types, x, l, status, workspace: Optional[NoiseWorkspace] = None, options: int = 0,
                  caller_records: Optional[torch.Tensor] = None):
    """n_iterations x (predictor + M correctors) in one launch, composition updated in place.

    workspace: the caller's NoiseWorkspace -- the segment's draws are generated by the chip-filling pre-pass kernel
    into it (default product path); None: every wavefront draws in-kernel.  Both evaluate the same Philox
    specification: identical results.  caller_records: a float32 device tensor already holding the records (layout in
    include/mdx_hip.h) -- parity tests replay the reference's recorded draws this way (MLP_SAMPLE_CALLER_NOISE).
    options: MLP_SAMPLE_* bits of _hip.py, passed through to the library."""
    B = x.shape[0]
    work = None
    if caller_records is not None:
        work = caller_records
        options |= _hip.MLP_SAMPLE_CALLER_NOISE
    elif workspace is not None and B > 0 and n_iterations > 0:
        work = workspace.get(pack, number_of_corrector_steps, atom_type_transition_in_corrector, n_iterations, B,
                             x.device)
    call("mdx_mlp_pc_sample", C.byref(sched.c_struct), C.byref(pack.c_struct), C.byref(flags), int(number_of_corrector_steps),
         int(bool(atom_type_transition_in_corrector)), int(start_index), int(n_iterations), rng, B, atom_types, x, l, work,
         0 if work is None else work.numel(), int(options), status)


# ----------------------------------------------------------------------------------------------------------------
# EGNN helpers around the MFMA kernels: fused first message layer, sorted-segment reductions
# ----------------------------------------------------------------------------------------------------------------
def egnn_message_input(node_proj, edges, radial, bias, w_radial, silu: bool = True) -> torch.Tensor:
    """First message layer on an edge list: SiLU(P[src,:H] + P[dst,H:] + b + r w_r)  (mdx_egnn_message_input)."""
    E = edges.shape[0]
    H = bias.shape[0]
    assert node_proj.shape[1] == 2 * H and radial.numel() == E
    out = torch.empty(E, H, dtype=F32, device=node_proj.device)
    call("mdx_egnn_message_input", node_proj, edges, radial, bias, w_radial, E, H, int(bool(silu)), out)
    return out


def egnn_coord_head(hidden, w_out, coord_diff, offsets, degree, mean: bool) -> torch.Tensor:
    """Last coordinate-MLP layer (H -> 1, no bias) x coord_diff, summed (or averaged) over each node's sorted edges."""
    n_nodes, H, d = degree.shape[0], hidden.shape[1], coord_diff.shape[1]
    if hidden.shape[0] == 0:                                   # no edges at all
        return torch.zeros(n_nodes, d, dtype=F32, device=hidden.device)
    trans = torch.empty(n_nodes, d, dtype=F32, device=hidden.device)
    call("mdx_egnn_coord_head", hidden, w_out, coord_diff, offsets, degree, n_nodes, H, d, int(bool(mean)), trans)
    return trans


def segment_rows(data, offsets, degree, mean: bool) -> torch.Tensor:
    """Sum (or mean) of the rows of data [E,H] over each node's sorted edge segment -> [n_nodes, H]."""
    n_nodes, H = degree.shape[0], data.shape[1]
    if data.shape[0] == 0:
        return torch.zeros(n_nodes, H, dtype=F32, device=data.device)
    out = torch.empty(n_nodes, H, dtype=F32, device=data.device)
    call("mdx_segment_rows", data, offsets, degree, n_nodes, H, int(bool(mean)), out)
    return out


# ----------------------------------------------------------------------------------------------------------------
# fused EGNN edge chain on the matrix cores (csrc/mdx_egnn_chain.hip)
# ----------------------------------------------------------------------------------------------------------------
# "f32": exact binary32 MFMA (v_mfma_f32_32x32x2_f32); "f16x3": split-f16, three products per term, on
# v_mfma_f32_16x16x32_f16 (the default since round 3: the chip holds a higher clock on this shape); "f16x3_32x32": the same
# arithmetic on v_mfma_f32_32x32x16_f16 (the round-2 kernel, kept for A/B runs and as a second implementation in the tests)
EDGE_CHAIN_PRECISIONS = {"f32": 0, "f16x3": 2, "f16x3_32x32": 1}


def _pack_chain_image(weights, w_out, H: int, precision: str, tied_layers: int = 0):
    """(image, exponents) of mdx_egnn_chain_pack for device matrices `weights` ([H, H] each, nn.Linear layout) and the
    optional head row w_out [H].  exponents: int32 [len(weights) + 1] on the device -- the per-layer powers of two the
    split-f16 image is scaled by (zeros for "f32"), chosen and written by the library without a host read."""
    dev = weights[0].device
    keep = [w.detach().to(F32).contiguous() for w in weights]
    image = torch.empty(lib().mdx_egnn_chain_image_bytes(H, len(keep)), dtype=torch.uint8, device=dev)
    exponents = torch.empty(len(keep) + 1, dtype=I32, device=dev)
    array = (C.c_void_p * len(keep))(*[w.data_ptr() for w in keep])
    head = None if w_out is None else w_out.detach().reshape(-1).to(F32).contiguous()
    with torch.cuda.device(dev):
        call("mdx_egnn_chain_pack", array, len(keep), head, H, EDGE_CHAIN_PRECISIONS[precision], tied_layers, image, exponents)
    return image, exponents      # (the temporaries are freed in stream order: the image holds its own copy)


F16_ACTIVATION_EXPONENT = _hip.EGNN_F16_ACTIVATION_EXPONENT


class ActivationScales:
    """The per-position powers of two the split-f16 kernels carry a chain's activations with, and the maxima the exact-f32
    kernels collect for them (mdx_egnn_chain_t.activation_exponents / activation_maxima): two small device arrays owned by
    whoever owns the chain's parameters and SHARED by the chain's packs of every precision -- the f32 pass that follows a
    range report fills the maxima, adapt() turns them into exponents (on the device, no host read), and the split-f16
    launches that follow -- captured ones included: the kernels read the array at every launch -- carry the hot positions
    with more headroom."""

    def __init__(self, n_layers: int, device):
        self.count = n_layers + 2
        self.exponents = torch.full((self.count,), F16_ACTIVATION_EXPONENT, dtype=I32, device=device)
        self.maxima = torch.zeros(self.count, dtype=I32, device=device)

    def adapt(self):
        with torch.cuda.device(self.exponents.device):
            call("mdx_egnn_chain_adapt_activation_exponents", self.maxima, self.count, self.exponents)

    def reset(self):
        """The state of a new object: default exponents, no maxima.  (The exponents only ever go DOWN otherwise -- after a
        fallback the split-f16 kernels carry the hot positions with more headroom and fewer low bits, so a later sample() with
        the same (seed, call index) can differ in the last bits from one made before the fallback: results are a function of
        (seed, call index, exponents), and reset() restores the exponents' initial value.)"""
        self.exponents.fill_(F16_ACTIVATION_EXPONENT)
        self.maxima.zero_()

    def pointers(self, precision: str):
        """(activation_exponents, activation_maxima) of a pack of `precision`: the split kernels read the exponents, the
        exact-f32 kernels write the maxima."""
        return (None, self.maxima.data_ptr()) if precision == "f32" else (self.exponents.data_ptr(), None)


CHAIN_WIDTHS = (32, 64, 128, 256)       # the widths egnn_edge_chain_kernel is instantiated for


def chain_width(*widths) -> int:
    """The instantiated chain width that holds layers of these widths (0: none does)."""
    need = max(widths)
    return next((w for w in CHAIN_WIDTHS if w >= need), 0)


def _pad2(w: torch.Tensor, rows: int, cols: int) -> torch.Tensor:
    w = w.detach().to(F32)
    if tuple(w.shape) == (rows, cols):
        return w.contiguous()
    out = torch.zeros(rows, cols, dtype=F32, device=w.device)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def _pad1(v: torch.Tensor, n: int) -> torch.Tensor:
    return _pad2(v.reshape(1, -1), 1, n).reshape(-1)


def parameter_stamp(*tensors) -> tuple:
    """((storage address, version), ...) of the given tensors, None skipped: differs once a parameter was replaced or written
    in place, which is when whatever was built from the parameters has to be rebuilt."""
    return tuple((t.data_ptr(), t._version) for t in tensors if t is not None)


class ChainPack:
    """What the device images of a chain of H x H layers share (mdx_egnn_chain_t): the checks at construction, the weight image
    re-laid out by mdx_egnn_chain_pack for `precision` with its per-layer exponents, the bias rows, the activation scales and
    the C struct.  Built from the modules' parameters at construction; the owner's stamp tells when to rebuild.
    scales (ActivationScales, optional): shared with the owner's packs of the other precisions."""

    def __init__(self, precision: str, scales, supported: bool, not_covered: str):
        if precision not in EDGE_CHAIN_PRECISIONS:
            raise _hip.MdxError(f"chain precision must be one of {sorted(EDGE_CHAIN_PRECISIONS)}; got {precision!r}")
        if not supported:
            raise _hip.MdxError(not_covered)
        self.precision, self.scales = precision, scales

    def _build(self, H: int, weights, biases, n_message_layers: int, n_coord_layers: int = 0, w_out=None, tied_layers: int = 0,
               edge_vectors=(None, None), attention=(None, None)):
        """weights: the image's [H, H] matrices (w_out [H]: the optional head row); biases: one [H] row per chain layer;
        edge_vectors / attention: the edge chain's (bias_in, w_radial) / (att_w, att_b)."""
        self.hidden, self.device = H, weights[0].device
        self.image, self.exponents = _pack_chain_image(weights, w_out, H, self.precision, tied_layers)
        self.biases = torch.stack(biases).contiguous()
        assert self.scales is None or self.scales.count == n_message_layers + n_coord_layers + 2
        act = self.scales.pointers(self.precision) if self.scales is not None else (None, None)
        self.c_struct = _hip.EgnnChain(H, n_message_layers, n_coord_layers, EDGE_CHAIN_PRECISIONS[self.precision], 0, 0,
                                       self.image.data_ptr(), self.biases.data_ptr(),
                                       *(None if t is None else t.data_ptr() for t in edge_vectors),
                                       self.exponents.data_ptr(), *act,
                                       *(None if t is None else t.data_ptr() for t in attention))


class EdgeChainPack(ChainPack):
    """Device image of one E_GCL layer's per-edge MLP chain for mdx_egnn_edge_chain: the H -> H weight matrices of the
    message MLP (after its first layer) and of the coordinate MLP, plus the small vectors.

    Widths.  The kernel runs square layers of one width H in CHAIN_WIDTHS.  A message MLP of width m and a coordinate
    MLP of width c (the reference's DEFAULT hyper-parameters are m = 16, c = 32: models/score_networks/egnn_score_network.py:
    23-45) run at H = chain_width(m, c) with every matrix, bias and vector ZERO-PADDED: a padded neuron has zero weights and a
    zero bias, so its pre-activation is 0, SiLU(0) = 0, and it feeds zeros on -- the same function, bit for bit in exact
    arithmetic, at the price of multiplying zeros.  `hidden` = H, `message_width` = m: the message sums come out [.., H] with
    columns m .. H-1 zero."""

    def __init__(self, first_message_layer, message_layers, coord_layers, coord_out_layer, input_size: int, precision: str,
                 scales=None, attention_layer=None):
        """attention_layer: E_GCL.att_mlp's nn.Linear(m, 1) (its Sigmoid is the kernel's), or None."""
        message_layers, coord_layers = list(message_layers), list(coord_layers)
        layers = message_layers + coord_layers
        super().__init__(precision, scales, self.supported(first_message_layer, message_layers, coord_layers, coord_out_layer),
                         "this E_GCL shape is not covered by the fused edge chain (see mdx_egnn_edge_chain)")
        m = first_message_layer.out_features
        H = chain_width(m, coord_out_layer.in_features)
        self.message_width = m
        self.bias_in = _pad1(first_message_layer.bias, H)
        self.w_radial = _pad1(first_message_layer.weight.detach()[:, 2 * input_size], H)
        # [2H, n_in]: the per-node projections of the first message layer (source half | destination half) as ONE matrix
        w0 = first_message_layer.weight.detach().to(F32)
        self.proj_weight = torch.cat([_pad2(w0[:, :input_size], H, input_size),
                                      _pad2(w0[:, input_size:2 * input_size], H, input_size)], dim=0).contiguous()
        self.att_w = self.att_b = None
        if attention_layer is not None:
            if attention_layer.in_features != m or attention_layer.out_features != 1 or attention_layer.bias is None:
                raise _hip.MdxError("the attention gate of the fused edge chain is nn.Linear(message width, 1) with a bias")
            self.att_w = _pad1(attention_layer.weight, H)
            self.att_b = attention_layer.bias.detach().to(F32).reshape(-1).contiguous()
        self._build(H, [_pad2(layer.weight, H, H) for layer in layers], [_pad1(layer.bias, H) for layer in layers],
                    len(message_layers), len(coord_layers), w_out=_pad1(coord_out_layer.weight, H),
                    edge_vectors=(self.bias_in, self.w_radial), attention=(self.att_w, self.att_b))
        # the kernel's LDS: weight ring + small vectors + per-layer scale table + the source ids of the in-kernel aggregation
        # (+ the attention gate's weight row)
        lds = 4 * 32 * H * 4 + 4 * (len(layers) * H + 2 * H) + 16 * (_hip.EGNN_CHAIN_MAX_LAYERS + 4) + 4 * 4 * 32 + 4 * (_hip.EGNN_CHAIN_MAX_LAYERS + 2) + \
            (16 + 4 * (H + 4) if self.att_w is not None else 0)
        self.piece_sums_ok = lds <= 160 * 1024

    @staticmethod
    def supported(first_message_layer, message_layers, coord_layers, coord_out_layer) -> bool:
        """nn.Linear stacks m -> m (message, after the first layer), m -> c -> c ... (coordinate), c -> 1 without a bias (head),
        with chain_width(m, c) an instantiated width."""
        message_layers, coord_layers = list(message_layers), list(coord_layers)
        if len(message_layers) < 1 or len(coord_layers) < 1 or \
                len(message_layers) + len(coord_layers) > _hip.EGNN_CHAIN_MAX_LAYERS:
            return False
        m, c = first_message_layer.out_features, coord_out_layer.in_features
        widths_in = [m] * len(message_layers) + [m] + [c] * (len(coord_layers) - 1)
        widths_out = [m] * len(message_layers) + [c] * len(coord_layers)
        return (chain_width(m, c) != 0 and first_message_layer.bias is not None and
                all(l.in_features == i and l.out_features == o and l.bias is not None
                    for l, i, o in zip(message_layers + coord_layers, widths_in, widths_out)) and
                coord_out_layer.out_features == 1 and coord_out_layer.bias is None)


class RowChainPack(ChainPack):
    """Device image of a chain of H -> H nn.Linear layers applied to the rows of a matrix (mdx_mlp_chain_rows): every layer
    but the last is followed by SiLU.  Used for the per-node MLP of an EGNN layer after its first (2H -> H) layer."""

    def __init__(self, layers, precision: str, scales=None):
        layers = list(layers)
        super().__init__(precision, scales, self.supported(layers), "this layer stack is not covered by mdx_mlp_chain_rows")
        self._build(layers[0].in_features, [layer.weight for layer in layers],
                    [layer.bias.detach().to(F32) for layer in layers], len(layers))

    @staticmethod
    def supported(layers) -> bool:
        layers = list(layers)
        if not layers:
            return False
        H = layers[0].in_features
        return (H in CHAIN_WIDTHS and len(layers) <= _hip.EGNN_CHAIN_MAX_LAYERS and
                all(l.in_features == H and l.out_features == H and l.bias is not None for l in layers))


class NodeMlpPack(ChainPack):
    """Device image of a whole EGNN node MLP -- Linear(2H, H), SiLU, [Linear(H, H), SiLU]*, Linear(H, H) -- for
    mdx_node_mlp_rows: the first layer's [H, 2H] weight as two H x H chain layers."""

    def __init__(self, layers, precision: str, next_projection=None, scales=None):
        """next_projection: [2H, H] = the next graph layer's per-node projection weight (EdgeChainPack.proj_weight): its
        two H x H halves follow the MLP in the image, and node_mlp_rows also returns out @ next_projection.T.
        scales: ActivationScales(n_chain_layers(layers), device), shared between the precisions."""
        layers = list(layers)
        super().__init__(precision, scales, self.supported(layers), "this layer stack is not covered by mdx_node_mlp_rows")
        H = layers[0].out_features
        w0 = layers[0].weight.detach().to(F32)
        keep = [w0[:, :H].contiguous(), w0[:, H:].contiguous()] + [l.weight.detach().to(F32).contiguous() for l in layers[1:]]
        n = len(keep)
        self.projects = next_projection is not None and n + 2 <= _hip.EGNN_CHAIN_MAX_LAYERS
        if self.projects:
            assert tuple(next_projection.shape) == (2 * H, H)
            keep += [next_projection[:H].detach().to(F32).contiguous(), next_projection[H:].detach().to(F32).contiguous()]
        # tied: the two halves of the wide first layer (their accumulators continue one another) and the two halves of the
        # projection share a power of two each
        tied = (1 << 1) | ((1 << (n + 1)) if self.projects else 0)
        zeros = torch.zeros(H, dtype=F32, device=w0.device)
        self._build(H, keep, [layers[0].bias.detach().to(F32), zeros] + [l.bias.detach().to(F32) for l in layers[1:]], n,
                    tied_layers=tied)

    @staticmethod
    def n_chain_layers(layers) -> int:
        """chain layers of the MLP part of the image: the wide first layer counts twice"""
        return len(list(layers)) + 1

    @staticmethod
    def supported(layers) -> bool:
        layers = list(layers)
        if len(layers) < 2:
            return False
        H = layers[0].out_features
        return (H in CHAIN_WIDTHS and layers[0].in_features == 2 * H and len(layers) + 1 <= _hip.EGNN_CHAIN_MAX_LAYERS and
                all(l.in_features == H and l.out_features == H for l in layers[1:]) and all(l.bias is not None for l in layers))


def node_mlp_rows(pack: NodeMlpPack, node_in, add_residual: bool, status=None, agg=None, row_class=None):
    """(h if add_residual) + MLP([h | agg]) over the rows; with a pack built with next_projection: (out, out @
    next_projection.T [M, 2H]).  node_in [M, 2H] = [h | agg] (mdx_node_mlp_rows), or node_in = h [M, H] with agg [M, H] given
    separately (mdx_node_mlp_rows_split: the concatenation is never formed), or -- with row_class int64 [M] -- node_in =
    class rows [n_classes, H] and h = node_in[row_class], never formed either (mdx_node_mlp_rows_indexed; a class outside
    the rows: row 0 and MDX_STATUS_EGNN_TABLE in `status`)."""
    if row_class is not None:
        n_classes, W = node_in.shape
        M = row_class.shape[0]
        assert agg is not None and W == pack.hidden and tuple(agg.shape) == (M, W) and row_class.dtype == torch.int64
        out = torch.empty(M, pack.hidden, dtype=F32, device=agg.device)
        proj = torch.empty(M, 2 * pack.hidden, dtype=F32, device=agg.device) if pack.projects else None
        call("mdx_node_mlp_rows_indexed", C.byref(pack.c_struct), node_in, n_classes, row_class, agg, int(bool(add_residual)), M,
             None, out, proj, status)
        return (out, proj) if pack.projects else out
    M, W = node_in.shape
    out = torch.empty(M, pack.hidden, dtype=F32, device=node_in.device)
    proj = torch.empty(M, 2 * pack.hidden, dtype=F32, device=node_in.device) if pack.projects else None
    if agg is not None:
        assert W == pack.hidden and agg.shape == node_in.shape
        call("mdx_node_mlp_rows_split", C.byref(pack.c_struct), node_in, agg, int(bool(add_residual)), M, None, out, proj, status)
        return (out, proj) if pack.projects else out
    assert W == 2 * pack.hidden
    call("mdx_node_mlp_rows", C.byref(pack.c_struct), node_in, int(bool(add_residual)), M, None, out, proj, status)
    return (out, proj) if pack.projects else out


def mlp_chain_rows(pack: RowChainPack, x, residual=None, status=None) -> torch.Tensor:
    """residual + chain(x) over the rows of x [M, H] (mdx_mlp_chain_rows)."""
    M, H = x.shape
    assert H == pack.hidden and (residual is None or residual.shape == x.shape)
    out = torch.empty_like(x)
    call("mdx_mlp_chain_rows", C.byref(pack.c_struct), x, residual, M, None, out, status)
    return out


def egnn_edge_chain(pack: EdgeChainPack, node_proj, coord, edges, status=None, n_edges_dev=None, piece_sums: bool = False,
                    memo: Optional["EgnnTableMemo"] = None, sigma=None):
    """messages [E,H], edge_scalar [E] of the fused per-edge chain (mdx_egnn_edge_chain); edges sorted by source.
    n_edges_dev (int64 [1], device): the actual number of edge rows when `edges` is a capacity-sized list.
    piece_sums: the first output holds per-node piece sums instead of the messages, in the compact layout of
    mdx_egnn_piece_rows(E, n_nodes) = ceil(E / 16) + n_nodes rows (feed it to segment_combine with n_edges=E): no [E, H]
    buffer exists in that mode.
    memo (with sigma): the launch on the first layer's distance grid (mdx_egnn_edge_chain_keyed) -- the outputs are the memo's
    kept buffers, and the kernel returns at once while the memo's key holds the bits of sigma[0]."""
    E, H = edges.shape[0], pack.hidden
    pack.c_struct.message_mode = 1 if piece_sums else 0
    assert node_proj.shape[1] == 2 * H and coord.shape[0] == node_proj.shape[0]
    if memo is not None:
        assert not piece_sums and sigma is not None and tuple(memo.values.shape) == (E, H)
        call("mdx_egnn_edge_chain_keyed", C.byref(pack.c_struct), node_proj, coord, coord.shape[1], edges, E, n_edges_dev,
             memo.values, memo.scalars, status, memo.key, sigma)
        return memo.values, memo.scalars
    rows = lib().mdx_egnn_piece_rows(E, node_proj.shape[0]) if piece_sums else E
    messages = torch.empty(rows, H, dtype=F32, device=edges.device)
    scalar = torch.empty(E, dtype=F32, device=edges.device)
    call("mdx_egnn_edge_chain", C.byref(pack.c_struct), node_proj, coord, coord.shape[1], edges, E, n_edges_dev, messages, scalar,
         status)
    return messages, scalar


# ---- the per-node passes behind the edge chain (csrc/mdx_egnn_node.hip)
def segment_combine(pieces, n_edges: int, offsets, degree, mean: bool, left=None) -> torch.Tensor:
    """Sum (or mean) over each node's edges from the piece sums of egnn_edge_chain(..., piece_sums=True) over `n_edges` edge
    rows (the capacity that call was given) -> [n_nodes, H]; with `left` [n_nodes, H]: [left | sums], [n_nodes, 2H] (the
    node MLP's input, without a separate concatenation)."""
    n_nodes, H = degree.shape[0], pieces.shape[1]
    assert left is None or tuple(left.shape) == (n_nodes, H)
    assert pieces.shape[0] == lib().mdx_egnn_piece_rows(n_edges, n_nodes), "pieces: not the compact layout of n_edges, n_nodes"
    out = torch.empty(n_nodes, H if left is None else 2 * H, dtype=F32, device=pieces.device)
    call("mdx_segment_combine", pieces, n_edges, offsets, degree, n_nodes, H, int(bool(mean)), left, out)
    return out


def coord_flags(normalize: bool, tanh: bool) -> int:
    """MDX_EGNN_COORD_* bits of an E_GCL layer's coordinate update (models/egnn.py: `normalize`, `tanh`)."""
    return (_hip.EGNN_COORD_NORMALIZE if normalize else 0) | (_hip.EGNN_COORD_TANH if tanh else 0)


def egnn_node_gather(pieces, n_edges: int, offsets, degree, mean_messages: bool, left, edge_scalar, coord, edges,
                     mean_coords: bool, flags: int = 0):
    """segment_combine(..., left=left) and egnn_coord_aggregate(...) in one launch (mdx_egnn_node_gather):
    ([left | message sums] [n_nodes, 2H] (or the sums [n_nodes, H] when left is None), coord_out [n_nodes, D]).
    pieces None (left None too): the coordinate half alone, (None, coord_out) with the same bits."""
    if pieces is None:
        assert left is None
        coord_out = torch.empty_like(coord)
        call("mdx_egnn_node_gather", None, n_edges, offsets, degree, degree.shape[0], 4, int(bool(mean_messages)), None, None,
             edge_scalar, coord, coord.shape[1], edges, int(bool(mean_coords)), int(flags), coord_out)
        return None, coord_out
    n_nodes, H = degree.shape[0], pieces.shape[1]
    assert left is None or tuple(left.shape) == (n_nodes, H)
    assert pieces.shape[0] == lib().mdx_egnn_piece_rows(n_edges, n_nodes), "pieces: not the compact layout of n_edges, n_nodes"
    out = torch.empty(n_nodes, H if left is None else 2 * H, dtype=F32, device=pieces.device)
    coord_out = torch.empty_like(coord)
    call("mdx_egnn_node_gather", pieces, n_edges, offsets, degree, n_nodes, H, int(bool(mean_messages)), left, out, edge_scalar,
         coord, coord.shape[1], edges, int(bool(mean_coords)), int(flags), coord_out)
    return out, coord_out


# ---- the first graph layer on a distance grid (mdx_egnn_table_check: csrc/mdx_egnn_table.hip; mdx_egnn_table_gather:
# csrc/mdx_egnn_node.hip)
TABLE_INV_SPACING = 256.0        # h = 2^-8 between the even grid points: rho_k = k h / 2, k^2 < 2^24 keeps rho_k^2 exact
# largest midpoint error, relative to the class pair's largest |value|: the chain's own rounding noise sits at ~2e-6 of that
# (exact-f32 and split-f16 alike, measured at C3 / C4 -- csrc/mdx_egnn_table.hip), so the check is set 8x above it; an
# interpolation error that passes it is below the network's binary32 noise floor in the scores
TABLE_TOLERANCE = 2.0 ** -16


TABLE_NO_KEY = _hip.EGNN_TABLE_NO_KEY        # a NaN's bits in the key record = no table in memory


class EgnnTableMemo:
    """The first layer's distance table kept on the device between forwards (include/mdx_hip.h, "The table memoised on the
    device"): the table's values [n_classes^2 K, H] and scalars, the grid problem's per-node inputs (of which the chain reads
    `grid_proj` [G, 2H]), the check's workspace, and the KEY RECORD `key`, int32 [2] = (bits of the sigma the table was built
    at, or TABLE_NO_KEY; number of builds so far).  The kernels of a build compare key[0] with the forward's sigma[0] on the
    device and return at once when they agree; the verdict kernel writes the key.  One memo per first graph layer, device and
    precision (E_GCL.table_memo): the pointers of a captured iteration stay valid across a one-iteration switch of precision.
    `stamp`: whatever else the table depends on, kept by the owner, which calls reset() when it changes."""

    def __init__(self, n_classes: int, n_even: int, hidden: int, embedding_width: int, coord_dimension: int, device):
        K = 2 * n_even - 1
        rows, G = n_classes * n_classes * K, n_classes * (K + 1)
        self.n_classes, self.n_even = n_classes, n_even
        self.values = torch.zeros(rows, hidden, dtype=F32, device=device)
        self.scalars = torch.zeros(rows, dtype=F32, device=device)
        self.grid_z = torch.zeros(G, coord_dimension, dtype=F32, device=device)
        self.grid_h = torch.zeros(G, embedding_width, dtype=F32, device=device)
        self.grid_proj = torch.zeros(G, 2 * hidden, dtype=F32, device=device)
        self.workspace = torch.zeros(n_classes ** 2 * (hidden + 2), dtype=I32, device=device)      # (every check leaves it zeroed)
        self.worst = torch.zeros(1, dtype=F32, device=device)
        self.key = torch.tensor([TABLE_NO_KEY, 0], dtype=I32, device=device)
        self.stamp = None

    def reset(self):
        """No table in memory: the next forward builds one.  A fill on the stream (no host read; the build counter stays)."""
        self.key[:1].fill_(TABLE_NO_KEY)

    def builds(self) -> int:
        """The number of tables built so far (one host read: tests and evidence, not the hot path)."""
        return int(self.key[1].item())


@dataclass
class EgnnTable:
    """What the first graph layer needs to run on the grid: the grid problem's per-node projections [G, 2H] (the class
    embeddings at the batch's sigma through the layer's first weight), sigma [B] (checked to be uniform on the device), the
    nodes' classes [n_nodes] int64 (MASK = n_classes - 1) and the grid's size.  memo: the EgnnTableMemo that owns grid_proj and
    receives the table."""
    grid_proj: torch.Tensor
    sigma: torch.Tensor
    atom_types: torch.Tensor
    n_classes: int
    n_even: int
    memo: EgnnTableMemo


def egnn_table_points(coord_dimension: int) -> int:
    """Even grid points for the torus uplift of coord_dimension = 2 n_k components: rho <= 2 sqrt(n_k), and the cubic of the
    cell [m h, (m+1) h) reads points m - 1 .. m + 2."""
    import math
    return int(math.ceil(math.sqrt(2.0 * coord_dimension) * TABLE_INV_SPACING)) + 3


_TABLE_GRIDS = {}


def egnn_table_grid(n_classes: int, n_even: int, coord_dimension: int, device):
    """The grid problem (fixed for a shape, built once per device): node classes [G] int64, coordinates [G, D] and the sorted
    edge list [n_classes^2 K, 2].  Node a < n_classes is the source of class a at the origin; node n_classes + b K + r the
    destination of class b at (rho_r, 0, ..., 0), rho_r = r h for r < n_even and (r - n_even + 1/2) h after that; edge row
    p K + r, p = a n_classes + b, joins a to (b, r): the row layout of mdx_egnn_table_check."""
    key = (n_classes, n_even, coord_dimension, str(device))
    if key not in _TABLE_GRIDS:
        K = 2 * n_even - 1
        r = torch.arange(K, dtype=torch.float64)
        rho = torch.where(r < n_even, r, r - n_even + 0.5) / TABLE_INV_SPACING
        classes = torch.cat([torch.arange(n_classes), torch.arange(n_classes).repeat_interleave(K)])
        coord = torch.zeros(n_classes * (K + 1), coord_dimension, dtype=F32)
        coord[n_classes:, 0] = rho.to(F32).repeat(n_classes)
        a = torch.arange(n_classes).repeat_interleave(n_classes * K)
        dst = n_classes + torch.arange(n_classes * K).repeat(n_classes)
        edges = torch.stack([a, dst], dim=1)
        _TABLE_GRIDS[key] = (classes.to(device), coord.to(device), edges.contiguous().to(device))
    return _TABLE_GRIDS[key]


def egnn_table_check(table, table_scalar, n_classes: int, n_even: int, sigma, workspace, worst=None, status=None, key=None):
    """Midpoint check of the grid table (mdx_egnn_table_check): MDX_STATUS_EGNN_TABLE into `status` on failure.
    key (EgnnTableMemo.key): mdx_egnn_table_check_keyed -- the midpoints only when this forward built the table, the uniform-sigma
    check always, and the key record written last."""
    H = table.shape[1]
    assert table.shape[0] == n_classes * n_classes * (2 * n_even - 1) and workspace.numel() >= n_classes ** 2 * (H + 2)
    call("mdx_egnn_table_check_keyed", table, table_scalar, H, n_classes, n_even, sigma, sigma.numel(), TABLE_TOLERANCE, workspace,
         worst, status, key)


def egnn_table_gather(table, table_scalar, n_classes: int, n_even: int, atom_types, offsets, degree, mean_messages: bool, left,
                      coord, edges, mean_coords: bool, flags: int = 0, status=None):
    """egnn_node_gather's outputs with the messages and scalars interpolated from the grid table (mdx_egnn_table_gather)."""
    n_nodes, H = degree.shape[0], table.shape[1]
    assert left is None or tuple(left.shape) == (n_nodes, H)
    assert atom_types.shape[0] == n_nodes and table.shape[0] == n_classes * n_classes * (2 * n_even - 1)
    out = torch.empty(n_nodes, H if left is None else 2 * H, dtype=F32, device=table.device)
    coord_out = torch.empty_like(coord)
    call("mdx_egnn_table_gather", table, table_scalar, H, n_classes, n_even, TABLE_INV_SPACING, atom_types, offsets, degree,
         n_nodes, int(bool(mean_messages)), left, out, coord, coord.shape[1], edges, int(bool(mean_coords)), int(flags), coord_out,
         status)
    return out, coord_out


def egnn_node_inputs(x, k_vectors, sigma, atom_types, emb_weight, emb_bias, second=None, memo: Optional[EgnnTableMemo] = None,
                     with_h: bool = True):
    """z [n_nodes, 2 n_k] (torus uplift) and h [n_nodes, H] (embedding of [sigma | one_hot]) of EGNNScoreNetwork, one launch.
    x [B, N, 3] relative coordinates, sigma [B] (or [B,1]), atom_types [B, N] int64.
    second = (W2 [H2, F], b2 [H2]): a third output, the same input through that linear map (see mdx_egnn_node_inputs).
    memo: the launch on the class nodes of the first layer's distance grid (mdx_egnn_node_inputs_keyed) -- the outputs are the
    memo's kept buffers, and the kernel returns at once while the memo's key holds the bits of sigma[0].
    with_h=False: h is neither allocated nor written (None in its place); z keeps its bits."""
    B, N, d = x.shape
    assert d == 3 and k_vectors.shape[1] == 3
    n_nodes, n_k, (H, F) = B * N, k_vectors.shape[0], emb_weight.shape
    w2, b2 = second if second is not None else (None, None)
    assert second is None or (w2.shape[1] == F and b2.shape[0] == w2.shape[0])
    H2 = w2.shape[0] if second is not None else 0
    if memo is not None:
        z, h, h2 = memo.grid_z, memo.grid_h, memo.grid_proj
        assert second is not None and tuple(z.shape) == (n_nodes, 2 * n_k) and tuple(h.shape) == (n_nodes, H) and \
            tuple(h2.shape) == (n_nodes, H2)
    else:
        z = torch.empty(n_nodes, 2 * n_k, dtype=F32, device=x.device)
        h = torch.empty(n_nodes, H, dtype=F32, device=x.device) if with_h else None
        h2 = torch.empty(n_nodes, H2, dtype=F32, device=x.device) if second is not None else None
    call("mdx_egnn_node_inputs_keyed", x, k_vectors, n_k, sigma, N, atom_types, emb_weight, emb_bias, F, H, n_nodes, z, h, w2, b2,
         H2, h2, memo.key if memo is not None else None)
    return (z, h) if second is None else (z, h, h2)


def egnn_scores(z, x_hat, k_vectors):
    """S^alpha = z . Gamma^alpha . x_hat per node -> [n_nodes, 3]  (mdx_egnn_scores)."""
    n_nodes, n_k = z.shape[0], k_vectors.shape[0]
    assert z.shape == x_hat.shape == (n_nodes, 2 * n_k)
    out = torch.empty(n_nodes, 3, dtype=F32, device=z.device)
    call("mdx_egnn_scores", z, x_hat, k_vectors, n_k, n_nodes, out)
    return out


def egnn_outputs(z, x_hat, k_vectors, h, class_weight, class_bias, mask_class: int, n_zero: int):
    """(scores [n_nodes,3], logits [n_nodes,C] with the MASK logit at -inf, zeros [n_zero]) in one launch (mdx_egnn_outputs)."""
    n_nodes, n_k = z.shape[0], k_vectors.shape[0]
    C, H = class_weight.shape
    assert z.shape == x_hat.shape == (n_nodes, 2 * n_k) and h.shape == (n_nodes, H) and class_bias.shape == (C,)
    scores = torch.empty(n_nodes, 3, dtype=F32, device=z.device)
    logits = torch.empty(n_nodes, C, dtype=F32, device=z.device)
    zeros = torch.empty(int(n_zero), dtype=F32, device=z.device)
    call("mdx_egnn_outputs", z, x_hat, k_vectors, n_k, h, class_weight, class_bias, H, C, int(mask_class), n_nodes, scores, logits,
         zeros if n_zero else None, int(n_zero))
    return scores, logits, zeros


def egnn_coord_aggregate(edge_scalar, coord, edges, offsets, degree, mean: bool, flags: int = 0) -> torch.Tensor:
    """coord + segment sum/mean of (coord_i - coord_dst) * edge_scalar over each node's sorted edges (flags: coord_flags())."""
    out = torch.empty_like(coord)
    call("mdx_egnn_coord_aggregate", edge_scalar, coord, coord.shape[1], edges, offsets, degree, coord.shape[0], int(bool(mean)),
         int(flags), out)
    return out


# ----------------------------------------------------------------------------------------------------------------
# RNG fills / probes
# ----------------------------------------------------------------------------------------------------------------
RNG_UNIFORM, RNG_NORMAL, RNG_GUMBEL = 0, 1, 2


def rng_fill(kind: int, seed: int, call: int, draw: int, tag: int, n_items: int, width: int, device) -> torch.Tensor:
    out = torch.empty(n_items, width, dtype=F32, device=device)
    _hip.call("mdx_rng_fill", kind, int(seed) & 0xFFFFFFFFFFFFFFFF, int(call), int(draw), int(tag), n_items, width, out)
    return out


def math_probe(fn: int, x: torch.Tensor) -> torch.Tensor:
    """y = f(x) elementwise on the device (mdx_math_probe, tests only).  fn 0 logf, 1 expf, 2 sinpi, 3 cospi: the software
    sequences of the arithmetic contract; fn 4 cos(2 pi x), 5 sin(2 pi x): the hardware v_cos_f32 / v_sin_f32 (x in
    revolutions) that the folded forwards of mlp_pc_sample evaluate."""
    y = torch.empty_like(x)
    call("mdx_math_probe", fn, x, x.numel(), y)
    return y
