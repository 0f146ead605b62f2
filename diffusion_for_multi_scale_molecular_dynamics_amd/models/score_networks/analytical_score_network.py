"""Analytical score network (src/.../models/score_networks/analytical_score_network.py:32-298): the exact score of wrapped
Gaussians of width sigma_d around equilibrium positions, optionally made permutation invariant by summing over all atomic
permutations.  For checking a sampler against a known target, not for production results.

Same hyper-parameters and state_dict as the reference (`translations_k` int64 [2 kmax + 1], `all_x0` f32 [P, N, D] with P = N!
under permutation invariance, else 1).  The forward is ONE HIP kernel (kernels.analytical_score, csrc/mdx_analytical.hip): every
term depends only on (atom, site, dimension), so the kernel enumerates the permutations over an N x N table built from the
sites in row 0 of `all_x0` -- the other rows are kept for the state_dict alone.  Binary64 inside, device tensors only.
One difference from the reference on invalid input: the kernel refuses a RAW coordinate outside [0, 1) (NaN outputs for that
structure and MDX_STATUS_ANALYTICAL_COORDINATES, raised as the reference's "should all be in [0, 1)" assertion), where the
reference wraps x - x0 first and so accepts any x; the samplers always hand over wrapped coordinates.
Limits of the kernel: number_of_atoms <= 1024, spatial_dimension <= 3, kmax <= 64, and <= 8 atoms under permutation invariance.
"""
from dataclasses import dataclass
from typing import Any, AnyStr, Dict, List, Tuple

import torch

from ... import kernels
from ...namespace import AXL, NOISE, NOISY_AXL_COMPOSITION
from ...score.wrapped_gaussian_score import get_coordinates_sigma_normalized_score, get_log_wrapped_gaussians
from ...utils.basis_transformations import map_relative_coordinates_to_unit_cell
from ...utils.symmetry_utils import get_all_permutation_indices
from ._exact_score_outputs import _ExactScoreOutputs
from .score_network import ScoreNetwork, ScoreNetworkParameters


@dataclass(kw_only=True)
class AnalyticalScoreNetworkParameters(ScoreNetworkParameters):
    """Specific Hyper-parameters for analytical score networks (:32-65)."""

    architecture: str = "analytical"
    number_of_atoms: int
    kmax: int                       # translations are [-kmax, .., kmax]
    equilibrium_relative_coordinates: List[List[float]]
    sigma_d: float                  # the width of the data distribution
    use_permutation_invariance: bool = False     # the number of permutations is number_of_atoms!

    def __post_init__(self):
        super().__post_init__()
        assert self.sigma_d > 0.0, "the sigma_d parameter should be positive."
        assert len(self.equilibrium_relative_coordinates) == self.number_of_atoms, \
            "There should be exactly one list of equilibrium coordinates per atom."
        for x in self.equilibrium_relative_coordinates:
            assert len(x) == self.spatial_dimension, \
                "The equilibrium coordinates should be consistent with the spatial dimension."


class AnalyticalScoreNetwork(_ExactScoreOutputs, ScoreNetwork):
    """Score network based on analytical integration of Gaussian distributions."""

    _device_copies_slot = "_sites_on"

    def __init__(self, hyper_params: AnalyticalScoreNetworkParameters):
        super().__init__(hyper_params)
        self.number_of_atomic_classes = hyper_params.num_atom_types + 1      # account for the MASK class.
        self.natoms = hyper_params.number_of_atoms
        self.nd = self.natoms * self.spatial_dimension
        self.kmax = hyper_params.kmax
        self.sigma_d_square = hyper_params.sigma_d**2
        self.use_permutation_invariance = hyper_params.use_permutation_invariance
        if self.use_permutation_invariance and self.natoms > kernels.ANALYTICAL_MAX_PERMUTED_ATOMS:
            raise NotImplementedError(f"permutation invariance over {self.natoms} atoms: the kernel enumerates at most "
                                      f"{kernels.ANALYTICAL_MAX_PERMUTED_ATOMS}! permutations")

        self.translations_k = torch.nn.Parameter(self._get_all_translations(self.kmax), requires_grad=False)
        self.number_of_translations = len(self.translations_k)
        self.equilibrium_relative_coordinates = torch.tensor(hyper_params.equilibrium_relative_coordinates, dtype=torch.float)
        if self.use_permutation_invariance:
            all_x0 = self._get_all_equilibrium_permutations(self.equilibrium_relative_coordinates)      # [natoms!, natoms, d]
        else:
            all_x0 = self.equilibrium_relative_coordinates.unsqueeze(0)                                 # [1, natoms, d]
        self.all_x0 = torch.nn.Parameter(all_x0, requires_grad=False)
        self._sites_on = None
        self._constants = None
        self.graph_status = None        # int32 [1] on the inputs' device, made by the first forward (generators/network_hooks.py)

    @staticmethod
    def _get_all_translations(kmax: int) -> torch.Tensor:
        return torch.arange(-kmax, kmax + 1)

    @staticmethod
    def _get_all_equilibrium_permutations(relative_coordinates: torch.Tensor) -> torch.Tensor:
        perm_indices, _ = get_all_permutation_indices(relative_coordinates.shape[0])
        return relative_coordinates[perm_indices]

    def get_log_wrapped_gaussians_and_normalized_scores_centered_on_equilibrium_positions(
            self, relative_coordinates: torch.tensor, sigmas_t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(log wrapped Gaussians [P, batch], sigma-normalised scores [P, batch, natoms, d]) centred on each of the P rows of
        all_x0 (:135-215), through the two elementwise kernels of score/wrapped_gaussian_score.py.  The forward does not come
        through here: it never builds the P copies."""
        assert relative_coordinates.shape == sigmas_t.shape, "relative_coordinates and sigmas_t have different shapes."
        assert len(relative_coordinates.shape) == 3, "relative_coordinates should have 3 dimensions."
        effective_sigmas = torch.sqrt(self.sigma_d_square + sigmas_t**2)
        all_x0 = self.all_x0.to(relative_coordinates.device)
        number_of_equilibrium_positions = all_x0.shape[0]
        u = map_relative_coordinates_to_unit_cell(relative_coordinates.unsqueeze(0) - all_x0.unsqueeze(1))   # [P, B, N, d]
        repeated_sigmas_t = sigmas_t.unsqueeze(0).expand_as(u).contiguous()
        repeated_effective_sigmas = effective_sigmas.unsqueeze(0).expand_as(u).contiguous()
        wrapped_gaussians = get_log_wrapped_gaussians(u, repeated_effective_sigmas, self.kmax)
        effective_sigma_normalized_scores = get_coordinates_sigma_normalized_score(u, repeated_effective_sigmas, self.kmax)
        sigma_normalized_scores = repeated_sigmas_t * (effective_sigma_normalized_scores / repeated_effective_sigmas)
        assert wrapped_gaussians.shape[0] == number_of_equilibrium_positions
        return wrapped_gaussians, sigma_normalized_scores

    def get_probabilities_and_normalized_scores(self, relative_coordinates: torch.tensor,
                                                sigmas_t: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(probabilities P(x, t) [batch], normalised scores sigma S(x, t) [batch, natoms, d]) for sigmas_t of the shape of
        relative_coordinates (:217-255).  An invalid sigma or coordinate raises the reference's assertion (one host read)."""
        assert relative_coordinates.shape == sigmas_t.shape, "relative_coordinates and sigmas_t have different shapes."
        assert len(relative_coordinates.shape) == 3, "relative_coordinates should have 3 dimensions."
        status = torch.zeros(1, dtype=torch.int32, device=relative_coordinates.device) if relative_coordinates.is_cuda else None
        scores, probabilities = kernels.analytical_score(
            relative_coordinates.to(torch.float32).contiguous(), sigmas_t.to(torch.float32).contiguous(),
            *self._copies_on(relative_coordinates.device, self.all_x0[0]), self.sigma_d_square, self.kmax, self.use_permutation_invariance,
            with_probabilities=True, status=status)
        kernels.raise_analytical_status(status)
        return probabilities, scores

    def _forward_unchecked(self, batch: Dict[AnyStr, Any], conditional: bool = False) -> AXL:
        """AXL(A = logits (0, .., 0, -inf): one possible atom type, X = the analytical score, L = zeros in the reference's
        shape [batch, natoms, d]) (:257-298), all on the inputs' device.  `conditional` does nothing, as in the reference.
        Invalid inputs do not raise here (no host read): their structures hold NaNs and check_status() reports them."""
        xt = batch[NOISY_AXL_COMPOSITION].X
        sigmas = batch[NOISE].to(xt.device)         # [batch_size, 1]
        batch_size = xt.shape[0]
        scores, _ = kernels.analytical_score(xt.to(torch.float32).contiguous(), sigmas.to(torch.float32).contiguous(),
                                             *self._copies_on(xt.device, self.all_x0[0]), self.sigma_d_square, self.kmax,
                                             self.use_permutation_invariance, status=self._status_on(xt.device) if xt.is_cuda else None)
        return self._as_axl(scores, batch_size, xt.device)
