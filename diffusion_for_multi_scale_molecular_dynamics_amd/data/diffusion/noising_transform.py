"""Forward noising of a batch (src/.../data/diffusion/noising_transform.py:30-200): to ONE time index, as the repaint generator
uses it (transform_given_time_index), or to a random time index per structure, as the denoising loss of a held-out batch needs
it (transform, _transform_from_noise_sample).  Optimal transport is outside this package's scope.

Stand-alone form of what mdx_repaint_constrained_rows fuses: kernels F1 (wrapped Gaussian on X), F2 (D3PM on A),
F3 (Gaussian on L).  Draw order = the reference's: X noise, then A noise, then L noise.
"""
from typing import Dict

import torch

from ... import kernels
from ...namespace import (ATOM_TYPES, LATTICE_PARAMETERS, NOISE, NOISY_ATOM_TYPES, NOISY_LATTICE_PARAMETERS,
                          NOISY_RELATIVE_COORDINATES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES, Q_MATRICES,
                          RELATIVE_COORDINATES, TIME, TIME_INDICES)
from ...noise_schedulers.noise_parameters import NoiseParameters
from ...noise_schedulers.noise_scheduler import Noise, NoiseScheduler
from ...noisers.atom_types_noiser import AtomTypesNoiser
from ...noisers.lattice_noiser import LatticeDataParameters, LatticeNoiser
from ...noisers.relative_coordinates_noiser import RelativeCoordinatesNoiser
from ...utils.d3pm_utils import class_index_to_onehot


class NoisingTransform:
    def __init__(self, noise_parameters: NoiseParameters, num_atom_types: int, spatial_dimension: int,
                 use_fixed_lattice_parameters: bool = False, use_optimal_transport: bool = True, device="cuda"):
        """The reference's signature and defaults (:37-44) + `device`.  Optimal transport (the default there) re-assigns atoms
        while noising a TRAINING batch: outside the sampling hot path, refused loudly rather than silently skipped -- the
        sampling path passes use_optimal_transport=False (generators/constrained_langevin_generator.py:71).  (The call the
        reference makes there, Transporter(identity).get_optimal_transport(x0, xt), exists in transport/transporter.py; this
        transform is not wired to it: tests/test_generator_gpu.py pins the refusal.)"""
        if use_optimal_transport:
            raise NotImplementedError("NoisingTransform(use_optimal_transport=True) is the training-time augmentation, outside "
                                      "this package's scope: pass use_optimal_transport=False (as the repaint generator does)")
        self.num_atom_types = num_atom_types
        self.noise_scheduler = NoiseScheduler(noise_parameters, num_classes=num_atom_types + 1, device=device)
        self.lattice_noiser = LatticeNoiser(LatticeDataParameters(
            spatial_dimension=spatial_dimension, use_fixed_lattice_parameters=use_fixed_lattice_parameters))

    def _check_batch(self, batch: Dict):
        """The fields a batch must hold, with their ranks (:46-60)."""
        for key in (RELATIVE_COORDINATES, ATOM_TYPES, LATTICE_PARAMETERS):
            assert key in batch, f"The field '{key}' is missing from the input."
        assert batch[RELATIVE_COORDINATES].dim() == 3 and batch[ATOM_TYPES].dim() == 2 and batch[LATTICE_PARAMETERS].dim() == 2

    def transform(self, batch: Dict) -> Dict:
        """The batch augmented with its noised copy at a random time index per structure (:82-96)."""
        self._check_batch(batch)
        batch_size = batch[RELATIVE_COORDINATES].shape[0]
        noise_sample = self.noise_scheduler.get_random_noise_sample(batch_size)
        return self._transform_from_noise_sample(batch, noise_sample)

    def _transform_from_noise_sample(self, batch: Dict, noise_sample: Noise) -> Dict:
        """Noise every element of the composition at the noise sample's per-structure parameters (:122-200): the three noisers
        with the reference's operands, in its draw order X, A, L.  The three transition matrices come back as expand() views
        of the per-structure rows [batch, 1, C, C] -> [batch, atoms, C, C], not copies; like the reference this updates `batch`
        and returns it."""
        x0, a0, l0 = batch[RELATIVE_COORDINATES], batch[ATOM_TYPES], batch[LATTICE_PARAMETERS]
        batch_size, natoms, d = x0.shape
        augmentation_data = dict()
        augmentation_data[TIME] = noise_sample.time.reshape(-1, 1)
        augmentation_data[TIME_INDICES] = noise_sample.indices
        augmentation_data[NOISE] = noise_sample.sigma.reshape(-1, 1)
        sigmas = noise_sample.sigma.reshape(-1, 1, 1).expand(x0.shape)
        xt = RelativeCoordinatesNoiser.get_noisy_relative_coordinates_sample(x0, sigmas)
        q_matrices, q_bar_matrices, q_bar_tm1_matrices = (
            m.unsqueeze(1).expand(batch_size, natoms, -1, -1)
            for m in (noise_sample.q_matrix, noise_sample.q_bar_matrix, noise_sample.q_bar_tm1_matrix))
        augmentation_data[Q_MATRICES] = q_matrices
        augmentation_data[Q_BAR_MATRICES] = q_bar_matrices
        augmentation_data[Q_BAR_TM1_MATRICES] = q_bar_tm1_matrices
        a0_onehot = class_index_to_onehot(a0, self.num_atom_types + 1)
        at = AtomTypesNoiser.get_noisy_atom_types_sample(a0_onehot, q_bar_matrices)
        # sigma / natoms^(1/d) (utils/noise_utils.py:29) with the root taken on the host, as the reference's host tensors take it
        sigmas_n = noise_sample.sigma.reshape(-1, 1) / torch.full_like(l0, kernels.root_of_atom_count(natoms, d))
        lt = self.lattice_noiser.get_noisy_lattice_parameters(l0, sigmas_n)
        augmentation_data[NOISY_ATOM_TYPES] = at
        augmentation_data[NOISY_RELATIVE_COORDINATES] = xt
        augmentation_data[NOISY_LATTICE_PARAMETERS] = lt
        batch.update(augmentation_data)
        return batch

    def transform_given_time_index(self, batch: Dict, index_i: int) -> Dict:
        """index_i is the one-based time index (t_1 = delta, ..., t_T = 1)  (:98-120)."""
        assert index_i > 0, "The time index should never be smaller than 1."
        idx = index_i - 1
        self._check_batch(batch)
        x0, a0, l0 = batch[RELATIVE_COORDINATES], batch[ATOM_TYPES], batch[LATTICE_PARAMETERS]
        t = self.noise_scheduler.tables
        bsz, natoms, d = x0.shape
        sigma = float(t.sigma[idx])
        out = dict(batch)
        out[TIME] = t.time[idx].expand(bsz).reshape(-1, 1)
        out[NOISE] = t.sigma[idx].expand(bsz).reshape(-1, 1)
        out[TIME_INDICES] = torch.full((bsz,), idx, dtype=torch.long, device=x0.device)
        out[Q_MATRICES] = t.q_matrix[idx].expand(bsz, natoms, -1, -1)
        out[Q_BAR_MATRICES] = t.q_bar_matrix[idx].expand(bsz, natoms, -1, -1)
        out[Q_BAR_TM1_MATRICES] = t.q_bar_tm1_matrix[idx].expand(bsz, natoms, -1, -1)
        out[NOISY_RELATIVE_COORDINATES] = RelativeCoordinatesNoiser.get_noisy_relative_coordinates_sample(x0, sigma)
        out[NOISY_ATOM_TYPES] = AtomTypesNoiser.get_noisy_atom_types_sample(a0, t.q_bar_matrix[idx])
        sigma_n = float(t.sigma[idx] / torch.tensor(float(natoms)) ** (1 / d))
        out[NOISY_LATTICE_PARAMETERS] = self.lattice_noiser.get_noisy_lattice_parameters(l0, sigma_n)
        return out
