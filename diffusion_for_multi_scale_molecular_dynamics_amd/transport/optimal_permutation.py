"""The permutation that aligns two sets of points on the hyper-torus (src/.../transport/optimal_permutation.py): the reference
solves the assignment problem with scipy on the host, here it is the device solver (kernels.linear_assignment).  Device tensors
only."""
import torch

from .. import kernels
from .distance import get_squared_geodesic_distance_cost_matrix


def get_optimal_permutation(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The permutation matrix pi [number_of_atoms, number_of_atoms] such that pi.y is the shortest squared geodesic distance
    away from x (:8-29); x, y [number_of_atoms, spatial_dimension].  The matrix is eye(n)[col_idx, :], as in the reference, on
    the inputs' device."""
    cost_matrix = get_squared_geodesic_distance_cost_matrix(x, y)
    col_idx, _ = kernels.linear_assignment(cost_matrix.unsqueeze(0).contiguous())
    n = cost_matrix.shape[0]
    return torch.eye(n, device=cost_matrix.device)[col_idx[0].long(), :]
