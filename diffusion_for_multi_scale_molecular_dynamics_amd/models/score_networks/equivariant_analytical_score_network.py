"""Equivariant analytical score network (src/.../models/score_networks/equivariant_analytical_score_network.py): the score of
wrapped Gaussians of width sigma_d around the image of the equilibrium sites that the Transporter aligns with the input -- a
translation (atan2 centre), a cubic point-group operation and a permutation found by the Hungarian algorithm.  For exploring and
debugging, not for production results.

Same hyper-parameters and state_dict as the reference (`equilibrium_relative_coordinates` f32 [N, D], `symmetries` f32 [O, D, D]).
The forward is ONE HIP kernel (kernels.equivariant_analytical_score, csrc/mdx_transport.hip): every operation's assignment
problem is solved on the device, where the reference solves batch x operations problems one by one on the host; nothing reads
the host, so the forward can be captured into a hipGraph.  Binary64 inside, device tensors only.  Any finite coordinate is
accepted (the reference wraps everything here).  Limits of the kernel: number_of_atoms <= 256, spatial_dimension <= 3, kmax <= 64.
"""
from dataclasses import dataclass
from typing import Any, AnyStr, Dict, List

import torch

from ... import kernels
from ...namespace import AXL, NOISE, NOISY_AXL_COMPOSITION
from ...score.wrapped_gaussian_score import get_coordinates_sigma_normalized_score
from ...transport.transporter import Transporter
from ...utils.basis_transformations import map_relative_coordinates_to_unit_cell
from ...utils.geometric_utils import get_cubic_point_group_symmetries
from ._exact_score_outputs import _ExactScoreOutputs
from .score_network import ScoreNetwork, ScoreNetworkParameters


@dataclass(kw_only=True)
class EquivariantAnalyticalScoreNetworkParameters(ScoreNetworkParameters):
    """Specific Hyper-parameters for equivariant analytical score networks (:21-51)."""

    architecture: str = "equivariant_analytical"
    number_of_atoms: int
    kmax: int                       # translations are [-kmax, .., kmax]
    equilibrium_relative_coordinates: List[List[float]]
    sigma_d: float                  # the width of the data distribution
    use_point_group_symmetries: bool = True

    def __post_init__(self):
        # (as in the reference, the base class's __post_init__ is not called here)
        assert self.sigma_d > 0.0, "the sigma_d parameter should be positive."
        assert len(self.equilibrium_relative_coordinates) == self.number_of_atoms, \
            "There should be exactly one list of equilibrium coordinates per atom."
        for x in self.equilibrium_relative_coordinates:
            assert len(x) == self.spatial_dimension, \
                "The equilibrium coordinates should be consistent with the spatial dimension."


class EquivariantAnalyticalScoreNetwork(_ExactScoreOutputs, ScoreNetwork):
    """Score network based on analytical integration of Gaussian distributions, equivariant by optimal transport."""

    _device_copies_slot = "_on_device"

    def __init__(self, hyper_params: EquivariantAnalyticalScoreNetworkParameters):
        super().__init__(hyper_params)
        self.number_of_atomic_classes = hyper_params.num_atom_types + 1      # account for the MASK class.
        self.natoms = hyper_params.number_of_atoms
        self.spatial_dimension = hyper_params.spatial_dimension
        self.nd = self.natoms * self.spatial_dimension
        self.kmax = hyper_params.kmax
        self.sigma_d_square = hyper_params.sigma_d**2
        if self.natoms > kernels.TRANSPORT_MAX_ATOMS:
            raise NotImplementedError(f"{self.natoms} atoms: the assignment kernel keeps a problem in one wavefront's registers, "
                                      f"at most {kernels.TRANSPORT_MAX_ATOMS} atoms")

        self.equilibrium_relative_coordinates = torch.nn.Parameter(
            torch.tensor(hyper_params.equilibrium_relative_coordinates), requires_grad=False)
        if hyper_params.use_point_group_symmetries:
            symmetries = get_cubic_point_group_symmetries(spatial_dimension=self.spatial_dimension)
        else:
            symmetries = torch.eye(self.spatial_dimension).unsqueeze(0)
        self.symmetries = torch.nn.Parameter(symmetries, requires_grad=False)
        self.transporter = Transporter(self.symmetries)
        self._on_device = None
        self._constants = None
        self.graph_status = None        # int32 [1] on the inputs' device, made by the first forward (generators/network_hooks.py)

    def get_nearest_equilibrium_coordinates(self, relative_coordinates: torch.Tensor) -> torch.Tensor:
        """The symmetry-group image of the equilibrium coordinates aligned with each structure of relative_coordinates
        [batch_size, num_atoms, spatial_dimension]: same shape (:93-107).  One kernel; the sites are shared, not repeated."""
        return kernels.transport_align(relative_coordinates.to(torch.float32).contiguous(),
                                       *self._copies_on(relative_coordinates.device, self.equilibrium_relative_coordinates, self.symmetries))

    def _get_jacobian_matrix(self, x: torch.Tensor) -> torch.Tensor:
        """J_ij = d c_j / d x_i of the translation-invariant coordinates c(x), diagonal in the spatial index:
        [batch_size, spatial_dimension, natoms, natoms] for x [batch_size, natoms, spatial_dimension] (:109-154).  The reference
        keeps it out of the score ("doesn't work at the moment"); it is here for the same callers."""
        batch_size, natoms, spatial_dimension = x.shape
        two_pi = 2 * torch.pi
        cosines, sines = torch.cos(two_pi * x), torch.sin(two_pi * x)
        u_mean, v_mean = cosines.mean(dim=1), sines.mean(dim=1)
        denominator = u_mean**2 + v_mean**2
        shape = (batch_size, spatial_dimension, natoms, natoms)
        cos_prefactor = (u_mean / denominator)[:, :, None, None].expand(shape)
        sin_prefactor = (v_mean / denominator)[:, :, None, None].expand(shape)
        cos_term = (cosines / natoms).transpose(1, 2)[:, :, :, None].expand(shape)
        sin_term = (sines / natoms).transpose(1, 2)[:, :, :, None].expand(shape)
        identity = torch.eye(natoms, device=x.device)[None, None].expand(shape)
        return identity - (cos_prefactor * cos_term + sin_prefactor * sin_term)

    def get_normalized_scores(self, xt: torch.tensor, sigmas_t: torch.Tensor) -> torch.Tensor:
        """Sigma-normalised scores [batch, natoms, d] centred on the aligned equilibrium image, for sigmas_t of the shape of xt
        (:156-193): the alignment kernel, then the elementwise wrapped-Gaussian kernel (one host read for its assertions).
        The forward does not come through here: its sigmas are one per structure and everything is one kernel."""
        assert xt.shape == sigmas_t.shape, "xt and sigmas_t have different shapes."
        assert len(xt.shape) == 3, "relative_coordinates should have 3 dimensions."
        effective_sigmas = torch.sqrt(self.sigma_d_square + sigmas_t**2)
        x_invariant = self.transporter.get_translation_invariant(xt)
        mu_invariant = self.get_nearest_equilibrium_coordinates(xt)
        u = map_relative_coordinates_to_unit_cell(x_invariant - mu_invariant)
        effective_sigma_normalized_scores = get_coordinates_sigma_normalized_score(u, effective_sigmas, self.kmax)
        return sigmas_t * effective_sigma_normalized_scores / effective_sigmas

    def _forward_unchecked(self, batch: Dict[AnyStr, Any], conditional: bool = False) -> AXL:
        """AXL(A = logits (0, .., 0, -inf): one possible atom type, X = the score, L = zeros [batch, natoms, d]) (:195-241),
        all on the inputs' device.  `conditional` does nothing, as in the reference.  Invalid inputs do not raise here (no host
        read): their structures hold NaNs and check_status() reports them."""
        xt = batch[NOISY_AXL_COMPOSITION].X
        sigmas = batch[NOISE].to(xt.device)         # [batch_size, 1]
        sites, symmetries = self._copies_on(xt.device, self.equilibrium_relative_coordinates, self.symmetries)
        scores = kernels.equivariant_analytical_score(xt.to(torch.float32).contiguous(), sigmas.to(torch.float32).contiguous(),
                                                      sites, symmetries, self.sigma_d_square, self.kmax,
                                                      status=self._status_on(xt.device) if xt.is_cuda else None)
        return self._as_axl(scores, xt.shape[0], xt.device)
