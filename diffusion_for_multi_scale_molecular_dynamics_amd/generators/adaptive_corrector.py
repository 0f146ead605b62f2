"""Adaptive-step Langevin corrector (src/.../generators/adaptive_corrector.py:17-148).

The predictor only updates the atom types; each corrector step uses
    eps = 2 (r * mean|z| / (mean|sigma s| / sigma))^2
with batch means, so the step needs reductions over the batch between the forward and the update.  Not one of the BASELINE
configurations.

rng_mode="device": three stream-ordered HIP stages with no host read (kernels.adaptive_corrector_*): per-structure norms with
the draws regenerated in registers and their fixed-order binary64 batch sums, the step size written to device words, and the
update that reads them.  The iteration therefore runs on the device-resident loop and is captured into a hipGraph like every
other generator's (use_hip_graph); the eager step methods call the same entry points, so a replay equals eager steps bit for
bit.  rng_mode="reference" keeps the reference's host draws, their order, and torch reductions.

Sharding a batch over ranks changes the batch means (SURVEY 8e caveat): with `sync_batch_statistics: true` and an initialised
process group the sums and counts of every rank's shard are added by ONE all-reduce of eight doubles per corrector step
(coordinates and lattice together), which reproduces the un-sharded step sizes; the collective is not captured, so that
combination launches the iteration eagerly.
"""
import warnings
from typing import Optional

import torch

from .. import kernels
from .._hip import MDX_CORRECTOR, MDX_PREDICTOR, STATUS_MASK_AT_LAST_STEP, MdxError
from ..models.score_networks.score_network import ScoreNetwork
from ..namespace import AXL
from ..noise_schedulers.noise_parameters import NoiseParameters
from ..utils.batch_statistics import global_means
from .langevin_generator import LangevinGenerator
from .predictor_corrector_axl_generator import PredictorCorrectorSamplingParameters
from .trajectory_initializer import TrajectoryInitializer


class AdaptiveCorrectorGenerator(LangevinGenerator):
    def __init__(self, noise_parameters: NoiseParameters, sampling_parameters: PredictorCorrectorSamplingParameters,
                 axl_network: ScoreNetwork, trajectory_initializer: Optional[TrajectoryInitializer] = None):
        super().__init__(noise_parameters=noise_parameters, sampling_parameters=sampling_parameters,
                         axl_network=axl_network, trajectory_initializer=trajectory_initializer)
        self.corrector_r = noise_parameters.corrector_r
        self.sync_batch_statistics = bool(getattr(sampling_parameters, "sync_batch_statistics", False))
        if self.fused_score_network:
            raise MdxError("the adaptive corrector needs batch reductions between the forward and the update: "
                           "use_hip_graph / fused_score_network do not apply")
        self._warned_sync_eager = False

    # ---------------------------------------------------------------------------------------------------------
    # rng_mode="device": statistics -> step size -> update on the device, by-value or device-resident time index
    # ---------------------------------------------------------------------------------------------------------
    def _sync_across_ranks(self) -> bool:
        return self.sync_batch_statistics and torch.distributed.is_available() and torch.distributed.is_initialized()

    def _step_buffers(self, batch: int, device):
        """Per-structure norms [B,4], their batch totals (float64 [8]) and the step's {eps, sqrt(2 eps), sigma} x (X, L)."""
        key = ("adaptive", batch)
        if key not in self._buffers:
            self._buffers[key] = (torch.empty(batch, 4, dtype=torch.float32, device=device),
                                  torch.empty(8, dtype=torch.float64, device=device),
                                  torch.empty(6, dtype=torch.float32, device=device))
        return self._buffers[key]

    def _device_predictor(self, comp: AXL, index_i: int, forces, d_index=None, in_place=False):
        """Atom types only (:41-63): one update launch with the Gumbel / binary draws made in registers."""
        sched = self._prepare(comp.X.device)
        batch = comp.X.shape[0]
        time_t, sigma_t = self._time_sigma(batch, comp.X.device)
        kernels.fill_time_sigma(sched, MDX_PREDICTOR, index_i, d_index, time_t, sigma_t)
        predictions = self._get_model_predictions(comp, time_t, sigma_t, forces)
        a_out = comp.A if in_place else torch.empty_like(comp.A)
        kernels.adaptive_corrector_update(sched, MDX_PREDICTOR, index_i, d_index, self._flags(True), comp.A, comp.X, comp.L,
                                          predictions.A.contiguous(), None, None, None, None, None, None, None, self._rng(0),
                                          a_out, None, None, self._status)
        return AXL(A=a_out, X=comp.X, L=comp.L), predictions

    def _device_corrector(self, comp: AXL, index_i: int, forces, corrector_number: int, d_index=None, in_place=False):
        """One corrector step (:97-148)."""
        x = comp.X
        device = x.device
        sched = self._prepare(device)
        batch, n, d = x.shape
        fixed = self.use_fixed_lattice_parameters
        time_t, sigma_t = self._time_sigma(batch, device)
        kernels.fill_time_sigma(sched, MDX_CORRECTOR, index_i, d_index, time_t, sigma_t)
        predictions = self._get_model_predictions(comp, time_t, sigma_t, forces)
        score_x = predictions.X.contiguous()
        score_l = self._lattice_score(predictions, comp)
        workspace, totals, weights = self._step_buffers(batch, device)
        rng = self._rng(1 + corrector_number)
        sync = self._sync_across_ranks()
        kernels.adaptive_corrector_statistics(sched, index_i, d_index, score_x, score_l, None, None, rng, fixed,
                                              self.corrector_r, self.small_epsilon, workspace, totals,
                                              None if sync else weights)
        if sync:
            torch.distributed.all_reduce(totals, op=torch.distributed.ReduceOp.SUM)
            kernels.adaptive_corrector_step_size(sched, index_i, d_index, totals, n, d, fixed, self.corrector_r,
                                                 self.small_epsilon, weights)
        x_out = x if in_place else torch.empty_like(x)
        l_out = comp.L if (fixed or in_place) else torch.empty_like(comp.L)
        kernels.adaptive_corrector_update(sched, MDX_CORRECTOR, index_i, d_index, self._flags(False), comp.A, x, comp.L, None,
                                          score_x, score_l, None, None, None, None, weights, rng, comp.A, x_out, l_out,
                                          self._status)
        return AXL(A=comp.A, X=x_out, L=l_out), predictions

    def _iteration_on_device_index(self, comp: AXL, forces: torch.Tensor, d_index: torch.Tensor,
                                   visits: Optional[int] = None):
        """Atom-types-only predictor + M x [forward -> statistics -> step size -> update] with i read from *d_index; in place,
        no host read, no allocation of its own after the first call (what IterationLoop captures)."""
        comp, _ = self._device_predictor(comp, 1, forces, d_index=d_index, in_place=True)
        for m in range(self.number_of_corrector_steps):
            comp, _ = self._device_corrector(comp, 0, forces, m, d_index=d_index, in_place=True)
        kernels.index_add(d_index, -1)
        return comp

    def _capture_safe(self, composition: AXL) -> bool:
        if self._sync_across_ranks():
            if not self._warned_sync_eager:
                warnings.warn("use_hip_graph=True with sync_batch_statistics=True in a process group: the all-reduce of the "
                              "batch totals is not captured; the sampler iteration is launched eagerly")
                self._warned_sync_eager = True
            return False
        return super()._capture_safe(composition)

    def _graph_key(self, start: AXL):
        return super()._graph_key(start) + ((self.corrector_r, self.sync_batch_statistics),)

    # ---------------------------------------------------------------------------------------------------------
    # the step methods; below the device branch: rng_mode="reference" (host draws in the reference's order, torch reductions)
    # ---------------------------------------------------------------------------------------------------------
    def predictor_step(self, composition_i: AXL, index_i: int, cartesian_forces: torch.Tensor) -> AXL:
        """Atom types only; X and L pass through (:41-63).  The reference still draws z and z_lattice."""
        assert 1 <= index_i <= self.number_of_discretization_steps
        if self._device_rng:
            out, predictions = self._device_predictor(composition_i, index_i, cartesian_forces)
            if self.record:
                self._record_step("predictor_step", ["composition_i", "composition_im1", "model_predictions_i"],
                                  [composition_i, out, predictions], index_i)
            return out
        device = composition_i.X.device
        sched = self._prepare(device)
        batch = composition_i.X.shape[0]
        time_t, sigma_t = self._time_sigma(batch, device)
        kernels.fill_time_sigma(sched, MDX_PREDICTOR, index_i, None, time_t, sigma_t)
        predictions = self._get_model_predictions(composition_i, time_t, sigma_t, cartesian_forces)
        idx = index_i - 1
        gumbel = self._draw_gumbel_sample(batch).to(device).contiguous()
        u = self._draw_binary_sample(batch).to(device).contiguous() if self.atom_type_greedy_sampling else None
        self._draw_coordinates_gaussian_sample(batch)          # drawn by the reference, unused here
        self._draw_lattice_gaussian_sample(batch)
        one = self.one_atom_type_transition_per_step and idx != 0
        a_im1 = kernels.atom_types_update(predictions.A.contiguous(), composition_i.A.contiguous(), sched.q_matrix[idx],
                                          sched.q_bar_matrix[idx], sched.q_bar_tm1_matrix[idx], gumbel, u,
                                          self.small_epsilon, self.atom_type_greedy_sampling, one)
        if idx == 0:
            self._status |= (a_im1 == self.masked_atom_type_index).any().to(torch.int32) * STATUS_MASK_AT_LAST_STEP
        out = AXL(A=a_im1, X=composition_i.X, L=composition_i.L)
        if self.record:
            self._record_step("predictor_step", ["composition_i", "composition_im1", "model_predictions_i"],
                              [composition_i, out, predictions], index_i)
        return out

    def _step_size(self, sigma, sigma_normalized_score, z, coordinates: bool) -> torch.Tensor:
        """eps_i (:97-148): norms over (atoms, space) per structure for the score, over the last axis for z."""
        dims = [-2, -1] if coordinates else -1
        score_mean, z_norm = global_means(torch.linalg.norm(sigma_normalized_score, dim=dims),
                                          torch.linalg.norm(z, dim=-1), self.sync_batch_statistics)
        score_norm = score_mean / sigma
        return 2 * (self.corrector_r * z_norm / score_norm.clip(min=self.small_epsilon)) ** 2

    def corrector_step(self, composition_i: AXL, index_i: int, cartesian_forces: torch.Tensor,
                       corrector_number: int = 0) -> AXL:
        assert 0 <= index_i <= self.number_of_discretization_steps - 1
        if self._device_rng:
            out, predictions = self._device_corrector(composition_i, index_i, cartesian_forces, corrector_number)
            if self.record_corrector:
                self._record_step("corrector_step", ["composition_i", "corrected_composition_i", "model_predictions_i"],
                                  [composition_i, out, predictions], index_i)
            return out
        device = composition_i.X.device
        sched = self._prepare(device)
        x = composition_i.X
        batch, n, d = x.shape
        time_t, sigma_t = self._time_sigma(batch, device)
        kernels.fill_time_sigma(sched, MDX_CORRECTOR, index_i, None, time_t, sigma_t)
        predictions = self._get_model_predictions(composition_i, time_t, sigma_t, cartesian_forces)
        sigma = sigma_t[0, 0]
        z = self._draw_coordinates_gaussian_sample(batch).to(device).contiguous()
        eps = self._step_size(sigma, predictions.X, z, coordinates=True)
        # the step size is a batch statistic: it stays on the device ({eps, sqrt(2 eps), sigma} read by the kernel)
        x_out = kernels.relative_coordinates_update(x.contiguous(), predictions.X.contiguous(), z,
                                                    weights=torch.stack([eps, torch.sqrt(2 * eps), sigma]).float())
        lattice = composition_i.L
        z_lattice = self._draw_lattice_gaussian_sample(batch).to(device)
        if not self.use_fixed_lattice_parameters:
            sigma_n = sigma / (n ** (1 / d))
            z_used = self._draw_lattice_gaussian_sample(batch).to(device).contiguous()   # the reference's 2nd draw
            score_l = self._lattice_score(predictions, composition_i)
            eps_l = self._step_size(sigma_n, score_l, z_lattice, coordinates=False)
            lattice = kernels.lattice_parameters_update(lattice.contiguous(), score_l, z_used,
                                                        weights=torch.stack([eps_l, torch.sqrt(2 * eps_l), sigma_n]).float())
        out = AXL(A=composition_i.A, X=x_out, L=lattice)
        if self.record_corrector:
            self._record_step("corrector_step", ["composition_i", "corrected_composition_i", "model_predictions_i"],
                              [composition_i, out, predictions], index_i)
        return out
