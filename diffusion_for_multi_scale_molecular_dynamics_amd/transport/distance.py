"""Geodesic displacements and distances on the hyper-torus (src/.../transport/distance.py), plain torch on the inputs' device."""
import torch

TWOPI = 2 * torch.pi


def get_geodesic_displacements(x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    """The geodesic displacement x2 - x1 along every dimension, in [-1/2, 1/2]: atan2(sin, cos) of 2 pi (x2 - x1), over 2 pi
    (:9-26).  Inputs [(batch dimensions), spatial_dimension], same shape out."""
    theta = TWOPI * (x2 - x1)
    return torch.atan2(torch.sin(theta), torch.cos(theta)) / TWOPI


def get_squared_geodesic_distance(x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    """The squared geodesic distance between two configurations [number_of_atoms, spatial_dimension] (:29-39): a scalar."""
    return (get_geodesic_displacements(x1, x2)**2).sum()


def get_squared_geodesic_distance_cost_matrix(x1: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
    """Squared geodesic distances between every point of x1 [n1, d] and every point of x2 [n2, d]: [n1, n2] (:42-68)."""
    n1, d = x1.shape
    n2, d_ = x2.shape
    assert d == d_, "The spatial dimensions are inconsistent. Review input."
    displacements = get_geodesic_displacements(x1.unsqueeze(1).expand(n1, n2, d), x2.unsqueeze(0).expand(n1, n2, d))
    return (displacements**2).sum(dim=2)
