"""Consistency regularizer (src/.../regularizers/consistency_regularizer.py:29-308), after

    Daras, Giannis, et al. "Consistent diffusion models: Mitigating sampling drift by learning to be consistent."
    Advances in Neural Information Processing Systems 36 (2024),

adapted by the reference to score networks in a periodic space: B copies of one noised structure start at a random point of the
torus, the predictor-corrector sampler carries them a few steps down the schedule, and the network's sigma-normalised score at
the start is compared with the score of the wrapped Gaussian that links start and end,
    loss = sum s . (s - 2 t) / B,    t = sigma_start grad log K(x_start | x_end; sigma_start^2 - sigma_end^2).

Here the trajectory runs on the device (LangevinGenerator.sample_from_noisy_composition: eager, or the captured hipGraph loop
with `use_hip_graph` and `rng_mode: device`) and target, loss and d loss / d s come from ONE launch of the fused kernel
(kernels.consistency_loss, binary64 inside).  The host-side methods are plain torch on any device; get_score_target and
compute_regularizer_loss run on the GPU only.  What differs from the reference:
  * one LangevinGenerator is kept per trajectory network (the reference builds one per call), so that its device tables and
    its captured loop survive across calls; it is released with the network;
  * the batch's times are read on the host once, to pick the element; nothing is read after the trajectory has returned: the
    kernel's value assertions go to the device word `status` (kernels.raise_analytical_status(regularizer.status));
  * `last_call` keeps what the last call used and made (indices, compositions, score, target, per-structure sums, loss).
"""
import weakref
from dataclasses import dataclass
from typing import Any, AnyStr, Dict, Tuple, Union

import torch

from .. import kernels
from ..generators.langevin_generator import LangevinGenerator
from ..generators.predictor_corrector_axl_generator import PredictorCorrectorSamplingParameters
from ..models.score_networks.analytical_score_network import AnalyticalScoreNetwork, AnalyticalScoreNetworkParameters
from ..models.score_networks.score_network import ScoreNetwork
from ..namespace import AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION, TIME
from ..noise_schedulers.noise_parameters import NoiseParameters
from ..noise_schedulers.noise_scheduler import Noise
from .regularizer import Regularizer, RegularizerParameters


@dataclass(kw_only=True)
class ConsistencyRegularizerParameters(RegularizerParameters):
    """Parameters of the consistency regularizer (:29-43)."""

    type: str = "consistency"

    maximum_number_of_steps: int
    kmax_target_score: int = 4      # truncation of the wrapped Gaussian's sum in the target
    noise_parameters: NoiseParameters
    sampling_parameters: PredictorCorrectorSamplingParameters

    # a sanity check: the trajectories are then sampled with an analytical score network, not with the regularized network
    analytical_score_network_parameters: Union[AnalyticalScoreNetworkParameters, None] = None


class ConsistencyRegularizer(Regularizer):
    """Regularizer on the consistency between a score network and the sampler it drives."""

    def __init__(self, regularizer_parameters: ConsistencyRegularizerParameters):
        super().__init__(regularizer_parameters)
        self.noise_parameters = regularizer_parameters.noise_parameters
        self.sampling_parameters = regularizer_parameters.sampling_parameters

        self.maximum_number_of_steps = regularizer_parameters.maximum_number_of_steps
        self.kmax_target_score = regularizer_parameters.kmax_target_score

        self.analytical_score_network = None
        if regularizer_parameters.analytical_score_network_parameters:
            self.analytical_score_network = AnalyticalScoreNetwork(regularizer_parameters.analytical_score_network_parameters)

        # trajectory network -> (its generator, the schedule's Noise on the host, the device); the generator holds the network
        # weakly, so an entry goes when its network does
        self._generators = weakref.WeakKeyDictionary()
        self._noise_source = None      # the generator's, for the duration of a call: where the start's coordinates come from
        self.status = None             # int32 [1] device word of kernels.consistency_loss, made by the first call
        self.last_call = None

    def get_augmented_batch_for_fixed_time(self, composition: AXL, time: float, sigma: float):
        """The score network's input for a composition whose elements all sit at `time`, with noise `sigma` (:74-101)."""
        batch_size = composition.X.shape[0]
        device = composition.X.device
        ones = torch.ones(batch_size, 1, device=device)
        return {NOISY_AXL_COMPOSITION: composition, NOISE: sigma * ones, TIME: time * ones,
                CARTESIAN_FORCES: torch.zeros_like(composition.X)}

    def get_partial_trajectory_start_and_end(self, start_time: float, noise: Noise) -> Tuple[int, int, float, float]:
        """(start index, end index, end time, end sigma) of the trajectory that begins at `start_time` and makes
        maximum_number_of_steps steps, or stops at index 0 (:103-153).  Predictor(x_i, i) runs at noise.time[i - 1], so the
        start index is one past the schedule entry nearest to start_time; index 0 is the data: time and sigma 0.0."""
        start_index = int((noise.time - start_time).abs().argmin()) + 1
        end_index = max(start_index - self.maximum_number_of_steps, 0)
        if end_index == 0:
            return start_index, end_index, 0.0, 0.0
        return start_index, end_index, noise.time[end_index - 1], noise.sigma[end_index - 1]

    def generate_starting_composition(self, original_composition: AXL, batch_index: int) -> AXL:
        """A batch of copies of element `batch_index`, with random relative coordinates (:155-188): X of the original shape from
        the running call's noise source (outside a call: torch.rand on the CPU generator, as the reference), A and L repeated;
        all on the original's device."""
        shape = original_composition.X.shape
        batch_size, device = shape[0], original_composition.X.device
        if self._noise_source is None:
            coordinates = torch.rand(*shape).to(device)
        else:
            coordinates = self._noise_source.initial_coordinates(*shape, device)
        atom_types, lattice = original_composition.A[batch_index], original_composition.L[batch_index]
        return AXL(A=atom_types.unsqueeze(0).repeat(batch_size, *[1] * atom_types.dim()), X=coordinates,
                   L=lattice.unsqueeze(0).repeat(batch_size, *[1] * lattice.dim()))

    def _status_word(self, device: torch.device) -> torch.Tensor:
        if self.status is None or self.status.device != device:
            self.status = torch.zeros(1, dtype=torch.int32, device=device)
        return self.status

    def get_score_target(self, start_composition: AXL, end_composition: AXL, start_sigma: float, end_sigma: float) -> torch.Tensor:
        """start_sigma grad log K, the sigma-normalised target [B, N, D] (:190-228), by the fused kernel without a score."""
        kernels._device_only("the consistency target", start_relative_coordinates=start_composition.X,
                             end_relative_coordinates=end_composition.X)
        x_start = start_composition.X
        return kernels.consistency_loss(x_start, end_composition.X, sigma_start=start_sigma, sigma_end=end_sigma,
                                        kmax=self.kmax_target_score, status=self._status_word(x_start.device)).target

    def _trajectory_generator(self, trajectory_network, device: torch.device):
        """(the network's generator, its schedule's Noise on the host): made on the first call with this network and device."""
        device = LangevinGenerator._device(device)
        kept = self._generators.get(trajectory_network)
        if kept is None or kept[2] != device:
            generator = kept[0] if kept is not None else LangevinGenerator(
                noise_parameters=self.noise_parameters, sampling_parameters=self.sampling_parameters,
                axl_network=weakref.proxy(trajectory_network))
            generator._prepare(device)
            host_noise = Noise(*[t.cpu() for t in generator.noise])      # read once per generator and device
            kept = (generator, host_noise, device)
            self._generators[trajectory_network] = kept
        return kept[0], kept[1]

    def compute_regularizer_loss(self, score_network: ScoreNetwork, augmented_batch: Dict[AnyStr, Any]) -> torch.Tensor:
        """The regularizer's loss on one randomly picked element of the batch whose time leaves room for
        maximum_number_of_steps steps (:230-308); tensor(0.0) when there is none."""
        trajectory_network = self.analytical_score_network if self.analytical_score_network else score_network
        original_noisy_composition = augmented_batch[NOISY_AXL_COMPOSITION]
        device = original_noisy_composition.X.device
        batch_times = augmented_batch[TIME][:, 0]
        batch_size = len(batch_times)

        if device.type == "cuda":
            generator, host_noise = self._trajectory_generator(trajectory_network, device)
            schedule_times = host_noise.time
        else:      # a host batch can only be told that it has no valid time: the reference's time array
            p = self.noise_parameters
            generator, host_noise, schedule_times = None, None, torch.linspace(p.time_delta, 1.0, p.total_time_steps)

        # times from which maximum_number_of_steps steps do not reach the data manifold: the batch's times come to the host here
        host_times = batch_times.detach().cpu()
        valid_time_mask = host_times > schedule_times[self.maximum_number_of_steps]
        if not torch.any(valid_time_mask):
            return torch.tensor(0.0)
        kernels._device_only("the consistency regularizer", relative_coordinates=original_noisy_composition.X,
                             times=augmented_batch[TIME], noise_parameter=augmented_batch[NOISE])

        # the reference's draw on the CPU generator
        idx = torch.randint(int(valid_time_mask.sum()), ())
        random_batch_index = int(torch.arange(batch_size)[valid_time_mask][idx])

        start_time = augmented_batch[TIME][random_batch_index, 0]
        start_sigma = augmented_batch[NOISE][random_batch_index, 0]
        start_step_index, end_step_index, end_time, end_sigma = self.get_partial_trajectory_start_and_end(
            host_times[random_batch_index], host_noise)

        device_rng = generator.rng_mode == "device"
        if device_rng:
            generator._begin_call(device)      # one Philox call index per call, as LangevinGenerator.sample
        self._noise_source = generator.noise_source
        try:
            start_composition = self.generate_starting_composition(original_noisy_composition, random_batch_index)
            with torch.no_grad():
                end_composition = generator.sample_from_noisy_composition(
                    starting_noisy_composition=start_composition, starting_step_index=start_step_index,
                    ending_step_index=end_step_index)
        finally:
            self._noise_source = None
            if device_rng:
                generator.noise_source = None

        start_batch = self.get_augmented_batch_for_fixed_time(start_composition, start_time, start_sigma)
        start_normalized_score = score_network(start_batch).X

        out = kernels.consistency_loss(start_composition.X, end_composition.X, start_normalized_score, sigma_start=start_sigma,
                                       sigma_end=float(end_sigma), kmax=self.kmax_target_score, status=self._status_word(device))
        self.last_call = dict(batch_index=random_batch_index, start_step_index=start_step_index, end_step_index=end_step_index,
                              start_time=start_time, start_sigma=start_sigma, end_time=end_time, end_sigma=end_sigma,
                              start_composition=start_composition, end_composition=end_composition,
                              start_normalized_score=start_normalized_score, normalized_score_target=out.target,
                              per_structure=out.per_structure, loss=out.loss)
        return out.loss
