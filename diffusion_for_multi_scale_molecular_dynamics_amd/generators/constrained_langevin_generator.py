"""RePaint-style constrained sampling (src/.../generators/constrained_langevin_generator.py:24-182).

After every predictor step the constrained rows are replaced by the known atoms forward-noised to the current
time index -- kernels F1 + F2 fused with the scatter (mdx_repaint_constrained_rows).  In reference-RNG mode the
reference's full-size draws (including the throw-away random composition) are reproduced draw for draw.

PerSampleConstrainedLangevinGenerator (no reference counterpart) pins a DIFFERENT set of atoms in every group of samples of
one batch -- the environments the excise-and-repaint sample maker cuts out of a frame -- so that they share one captured loop
(mdx_repaint_rows_per_sample) instead of running one generator per environment.
"""
from typing import List, Optional

import torch

from .. import kernels
from .._hip import Rng
from ..models.score_networks.score_network import ScoreNetwork
from ..namespace import AXL
from ..noise_schedulers.noise_parameters import NoiseParameters
from .langevin_generator import LangevinGenerator
from .noise_sources import upload
from .predictor_corrector_axl_generator import PredictorCorrectorSamplingParameters
from .sampling_constraint import SamplingConstraint
from .trajectory_initializer import TrajectoryInitializer


class ConstrainedLangevinGenerator(LangevinGenerator):
    def __init__(self, noise_parameters: NoiseParameters, sampling_parameters: PredictorCorrectorSamplingParameters,
                 axl_network: ScoreNetwork, sampling_constraints: SamplingConstraint,
                 trajectory_initializer: Optional[TrajectoryInitializer] = None):
        super().__init__(noise_parameters=noise_parameters, sampling_parameters=sampling_parameters,
                         axl_network=axl_network, trajectory_initializer=trajectory_initializer)
        self.sampling_constraints = sampling_constraints
        number_of_constraints, spatial_dimension = sampling_constraints.constrained_relative_coordinates.shape
        assert len(sampling_constraints.elements) == sampling_parameters.num_atom_types, \
            "Inconsistent number of atom types vs. elements list"
        assert number_of_constraints <= self.number_of_atoms, "There are more constrained positions than atoms!"
        assert spatial_dimension <= self.spatial_dimension, \
            "The spatial dimension of the constrained relative coordinates is inconsistent"
        if sampling_constraints.constrained_indices is None:
            self.constraint_indices = torch.arange(number_of_constraints)
        else:
            self.constraint_indices = sampling_constraints.constrained_indices
        self._constraint_device = {}
        self.resampling_steps = int(getattr(sampling_parameters, "repaint_resampling_steps", 0) or 0)
        assert self.resampling_steps >= 0, "repaint_resampling_steps should be non-negative"

    def _constraint_on(self, device):
        if device not in self._constraint_device:
            c = self.sampling_constraints
            self._constraint_device[device] = (
                c.constrained_relative_coordinates.to(device=device, dtype=torch.float32).contiguous(),
                c.constrained_atom_types.to(device=device, dtype=torch.int64).contiguous(),
                self.constraint_indices.to(device=device, dtype=torch.int64).contiguous())
        return self._constraint_device[device]

    def _repaint(self, composition: AXL, index_i: int, d_index=None, draw_index_offset: int = 1) -> AXL:
        """In-place on composition.X / composition.A, like the reference (:159-160)."""
        x, a = composition.X, composition.A
        device = x.device
        batch = x.shape[0]
        sched = self._prepare(device)
        z = u = None
        if not self._device_rng:
            self.initialize(batch, device)                     # composition_0_known: drawn, only constrained rows kept
            if d_index is None and index_i > 0:                # noising_transform.py:154,179
                z = upload(self.noise_source.randn(x.shape), device)
                u = upload(self.noise_source.rand(batch, self.number_of_atoms, self.num_classes), device)
        # Philox draw id of the repaint noise: that of the predictor step it follows (index_i + 1)
        rng = self._rng(0)
        rng_index = index_i
        self._repaint_rows(sched, rng_index, d_index, z, u,
                           Rng(rng.seed, rng.call, rng.draw_stride, rng.draw_stride + rng.draw_offset, 0, rng.call_dev), x, a)
        return AXL(A=a, X=x, L=composition.L)

    def _repaint_rows(self, sched, index_i: int, d_index, z, u, rng: Rng, x: torch.Tensor, a: torch.Tensor):
        """The launch behind _repaint and _apply_constraint: one constraint for the whole batch."""
        cx, ca, cidx = self._constraint_on(x.device)
        kernels.repaint_constrained_rows(sched, index_i, d_index, cx, ca, cidx, z, u, rng, x, a)

    def _forward_step(self, composition: AXL, index_i: int, d_index=None) -> AXL:
        """Resampling: forward-noise the WHOLE composition from time index i back to i+1, in place
        (mdx_forward_diffusion_step; build-only, no reference counterpart).  Reference-RNG mode draws z then u."""
        x, a = composition.X, composition.A
        device = x.device
        z = u = None
        if not self._device_rng:
            z = upload(self.noise_source.randn(x.shape), device)
            u = upload(self.noise_source.rand(x.shape[0], self.number_of_atoms, self.num_classes), device)
        kernels.forward_diffusion_step(self._prepare(device), index_i, d_index, z, u, self._rng(0), x, a)
        return AXL(A=a, X=x, L=composition.L)

    def predictor_step(self, composition_i: AXL, index_i: int, cartesian_forces: torch.Tensor) -> AXL:
        raw = super().predictor_step(composition_i, index_i, cartesian_forces)
        return self._repaint(raw, index_i - 1)

    def _after_predictor(self, composition: AXL, index_i: int, d_index=None) -> AXL:
        return self._repaint(composition, index_i, d_index=d_index)

    def _apply_constraint(self, composition: AXL, device: torch.device) -> AXL:
        """Hard constraint (:74-82): the index-0 path of the repaint kernel copies the known rows unnoised."""
        x, a = composition.X, composition.A
        self._repaint_rows(self._prepare(x.device), 0, None, None, None, Rng(0, 0, 1, 0), x, a)
        return AXL(A=a, X=x, L=composition.L)

    def sample(self, number_of_samples: int, device: torch.device) -> AXL:
        composition = super().sample(number_of_samples=number_of_samples, device=device)
        return self._apply_constraint(composition, device)


class PerSampleConstrainedLangevinGenerator(ConstrainedLangevinGenerator):
    """Repaint with one constraint per ENVIRONMENT: a batch of E x S samples, S consecutive samples per environment, each
    environment pinning its own first K_e rows (K_e may differ).  What the reference does with E generators run one after
    another (active_learning_loop/sample_maker/excise_and_repaint_sample_maker.py:162-174) is one trajectory here.

    The tables live on the device at a fixed capacity [E, capacity] and are REWRITTEN IN PLACE by set_environments: a kept
    hipGraph (whose key holds no constraint pointer) reads whatever they hold when it is replayed.  A change of E or of the
    capacity allocates new tables and drops the kept graph.  sample(E * S, device) is the only batch size served."""

    def __init__(self, noise_parameters: NoiseParameters, sampling_parameters: PredictorCorrectorSamplingParameters,
                 axl_network: ScoreNetwork, elements: List[str], trajectory_initializer: Optional[TrajectoryInitializer] = None,
                 capacity: Optional[int] = None):
        d = sampling_parameters.spatial_dimension
        nothing = SamplingConstraint(elements=elements, constrained_relative_coordinates=torch.zeros(0, d),
                                     constrained_atom_types=torch.zeros(0, dtype=torch.int64))
        super().__init__(noise_parameters=noise_parameters, sampling_parameters=sampling_parameters, axl_network=axl_network,
                         sampling_constraints=nothing, trajectory_initializer=trajectory_initializer)
        self.capacity = self.number_of_atoms if capacity is None else int(capacity)
        assert 0 < self.capacity <= self.number_of_atoms, "the capacity is a number of atoms of the generated structure"
        self.number_of_environments = 0
        self.samples_per_environment = 0
        self._host_tables = None
        self._tables = None           # device: (cx [E,cap,d], ca [E,cap], cidx [E,cap], counts [E], environment of sample [E*S])

    def set_environments(self, tables, samples_per_environment: int):
        """tables: (constrained_x float32 [E,K,d], constrained_a int64 [E,K], constrained_indices int64 [E,K] or None for
        0 .. K-1, counts int32 [E]) on the host or the device, K <= capacity; rows k >= counts[e] are padding."""
        cx, ca, cidx, counts = tables
        E, K = ca.shape
        assert E > 0 and samples_per_environment > 0
        assert K <= self.capacity, f"{K} constrained rows per environment, the generator's capacity is {self.capacity}"
        assert cx.shape == (E, K, self.spatial_dimension) and counts.shape == (E,)
        if cidx is None:
            cidx = torch.arange(K, dtype=torch.int64, device=ca.device).repeat(E, 1)
        assert cidx.shape == (E, K)
        host_counts = counts.cpu()
        assert int(host_counts.min()) >= 0 and int(host_counts.max()) <= K, "counts outside the tables"
        used = torch.arange(K)[None, :] < host_counts[:, None]
        assert bool(((ca.cpu() >= 0) & (ca.cpu() < self.num_classes - 1))[used].all()), \
            "constrained atom types must index into `elements`."
        assert bool(((cidx.cpu() >= 0) & (cidx.cpu() < self.number_of_atoms))[used].all()), \
            "There are more constrained positions than atoms!"
        if (E, samples_per_environment) != (self.number_of_environments, self.samples_per_environment):
            self._tables = None       # other shapes: new tables, and the captured iteration that read the old ones goes
            self._buffers.pop("graph_loop", None)
        self.number_of_environments, self.samples_per_environment = E, int(samples_per_environment)
        self._host_tables = (cx.to(torch.float32), ca.to(torch.int64), cidx.to(torch.int64), counts.to(torch.int32))
        if self._tables is not None:
            self._write_tables(self._tables[0].device)

    def _write_tables(self, device):
        cx, ca, cidx, counts = self._host_tables
        E, K = ca.shape
        if self._tables is None or self._tables[0].device != device:
            cap, S = self.capacity, self.samples_per_environment
            self._buffers.pop("graph_loop", None)
            self._tables = (torch.zeros(E, cap, self.spatial_dimension, dtype=torch.float32, device=device),
                            torch.zeros(E, cap, dtype=torch.int64, device=device),
                            torch.zeros(E, cap, dtype=torch.int64, device=device),
                            torch.zeros(E, dtype=torch.int32, device=device),
                            torch.arange(E, dtype=torch.int32, device=device).repeat_interleave(S).contiguous())
        dx, da, di, dc, _ = self._tables
        dx[:, :K].copy_(cx)
        da[:, :K].copy_(ca)
        di[:, :K].copy_(cidx)
        dc.copy_(counts)
        return self._tables

    def _constraint_on(self, device):
        assert self._host_tables is not None, "set_environments() comes before sample()"
        if self._tables is None or self._tables[0].device != device:
            self._write_tables(device)
        return self._tables

    def sample_from_noisy_composition(self, starting_noisy_composition: AXL, starting_step_index: int,
                                      ending_step_index: int) -> AXL:
        self._constraint_on(starting_noisy_composition.X.device)      # the upload stays outside a capture of the iteration
        return super().sample_from_noisy_composition(starting_noisy_composition, starting_step_index, ending_step_index)

    def _repaint_rows(self, sched, index_i: int, d_index, z, u, rng: Rng, x: torch.Tensor, a: torch.Tensor):
        cx, ca, cidx, counts, environment = self._constraint_on(x.device)
        assert x.shape[0] == environment.shape[0], \
            f"a batch of {x.shape[0]} samples, but {self.number_of_environments} environments x {self.samples_per_environment}"
        kernels.repaint_rows_per_sample(sched, index_i, d_index, cx, ca, cidx, counts, environment, z, u, rng, x, a)
