"""The symmetry-group image of one point of the hyper-torus that lies closest to another (src/.../transport/transporter.py:13-196).

The reference copies its [batch, operations, n, n] cost matrices to the host and solves them one by one with scipy; here the two
assignment methods run on the device solver (kernels.linear_assignment) and get_optimal_transport is ONE kernel
(kernels.transport_align: centres, costs, every operation's assignment, the choice and the image, in binary64, without the cost
matrices ever existing).  Nothing reads the host.  Device tensors only; at most 256 atoms, 48 operations, 3 dimensions.
"""
from typing import Tuple

import torch

from .. import kernels
from ..utils.basis_transformations import map_relative_coordinates_to_unit_cell
from .distance import get_geodesic_displacements


class Transporter:
    """Finds a symmetry group operation (translation, point group operation, permutation) that aligns two points on the
    hyper-torus.  It does not seek the minimal distance: it aims to be a fully equivariant function."""

    def __init__(self, point_group_operations: torch.Tensor):
        """point_group_operations: [number_of_point_group_operations, spatial_dimension, spatial_dimension]."""
        self.point_group_operations = point_group_operations
        self.number_of_point_group_operations = len(self.point_group_operations)
        self._operations_on = None

    def _operations(self, device) -> torch.Tensor:
        """The operations as f32 on `device`, copied there once (a call inside a captured loop must not upload)."""
        source = self.point_group_operations
        key = (device, source.data_ptr(), source._version)
        if self._operations_on is None or self._operations_on[0] != key:
            self._operations_on = (key, source.detach().to(device=device, dtype=torch.float32).contiguous())
        return self._operations_on[1]

    @staticmethod
    def get_atan2_translation(x: torch.Tensor) -> torch.Tensor:
        """The atan2 centre of x [batch, natoms, d]: [batch, d] (:36-42)."""
        two_pi = 2 * torch.pi
        x_bar = torch.cos(two_pi * x).mean(dim=1)
        y_bar = torch.sin(two_pi * x).mean(dim=1)
        return torch.atan2(y_bar, x_bar) / two_pi

    def get_translation_invariant(self, x: torch.Tensor) -> torch.Tensor:
        """x with its atan2 centre removed, wrapped into the unit cell (:44-48)."""
        x_com = self.get_atan2_translation(x).unsqueeze(1).expand_as(x)
        return map_relative_coordinates_to_unit_cell(x - x_com)

    def _get_all_cost_matrices(self, x_minus_x_com: torch.Tensor, mu_minus_mu_com: torch.Tensor) -> torch.Tensor:
        """Squared geodesic distances between every atom of x and every atom of every point-group image of mu:
        [batch, operations, natoms (x), natoms (mu)] (:50-72)."""
        operations = self.point_group_operations.to(mu_minus_mu_com)
        point_group_mu = torch.einsum("oij,bnj->boni", operations, mu_minus_mu_com)
        array_x = x_minus_x_com[:, None, :, None, :]
        array_mu = point_group_mu[:, :, None, :, :]
        return (get_geodesic_displacements(array_x, array_mu)**2).sum(dim=-1)

    def _solve_linear_assigment_problem(self, computed_cost_matrices: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(the lowest-cost operation's permutation matrix [batch, natoms, natoms], that operation [batch, d, d]) for cost
        matrices [batch, operations, natoms, natoms] (:74-116): every problem in one launch, the first minimum over the
        operations by torch.argmin."""
        batch_size, number_of_operations, natoms, _ = computed_cost_matrices.shape
        col_idx, costs = kernels.linear_assignment(computed_cost_matrices.reshape(-1, natoms, natoms).contiguous())
        lowest = costs.reshape(batch_size, number_of_operations).argmin(dim=1)
        batch_range = torch.arange(batch_size, device=lowest.device)
        chosen_col_idx = col_idx.reshape(batch_size, number_of_operations, natoms)[batch_range, lowest].long()
        identity = torch.eye(natoms, device=computed_cost_matrices.device)
        permutations = identity[chosen_col_idx].transpose(1, 2)          # eye(n)[:, col_idx] per structure
        return permutations, self.point_group_operations.to(computed_cost_matrices.device)[lowest]

    def _find_permutation_and_cost(self, cost_matrix: torch.Tensor):
        """(permutation matrix eye(n)[:, col_idx] that minimises Tr[permutation . cost_matrix], the minimised cost) of one
        n x n cost matrix (:118-135) -- on the device here, where the reference wants it on the host."""
        col_idx, _ = kernels.linear_assignment(cost_matrix.unsqueeze(0).contiguous())
        col_idx = col_idx[0].long()
        n = cost_matrix.shape[0]
        cost = cost_matrix[torch.arange(n, device=cost_matrix.device), col_idx].sum()
        return torch.eye(n, device=cost_matrix.device)[:, col_idx], cost

    def get_optimal_transport(self, x: torch.Tensor, mu: torch.Tensor) -> torch.Tensor:
        """The symmetry-group image of mu chosen so that the choice is equivariant under symmetry operations on x (:137-196):
        x, mu [batch_size, number_of_atoms, spatial_dimension] -> aligned mu, same shape, f32."""
        return kernels.transport_align(x.to(torch.float32).contiguous(), mu.to(torch.float32).contiguous(),
                                       self._operations(x.device))
