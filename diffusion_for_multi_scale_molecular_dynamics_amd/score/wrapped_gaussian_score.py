"""Wrapped Gaussian score (src/.../score/wrapped_gaussian_score.py:41-419): the perturbation kernel on a torus,

    K(x, x0) ~ sum_{k in Z} exp[- |x - x0 + k|^2 / 2 sigma^2],

its sigma-normalised score sigma x d/dx ln K and its logarithm, each truncated to k in [-kmax, kmax] as the reference does.
The two tensor functions run on HIP kernels (csrc/mdx_analytical.hip: binary64 inside, one rounding of the result to binary32)
and take device tensors only; the reference's shape assertions are kept, and its two VALUE assertions come back through the
kernels' status word (one host read per call).  get_sigma_normalized_score_brute_force is the reference's plain-float loop on
the host: a checker, not a tensor path.
"""
from typing import Optional

import numpy as np
import torch

from .. import kernels

SIGMA_THRESHOLD = torch.Tensor([1.0 / np.sqrt(2.0 * np.pi)])
U_THRESHOLD = torch.Tensor([0.5])


def _status(device) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=device)


def get_log_wrapped_gaussians(relative_coordinates: torch.tensor, sigmas: torch.tensor, kmax: int):
    """[..., number_of_atoms, spatial_dimension] -> [...]: the log of the wrapped Gaussians, summed over the last two
    dimensions (:41-92)."""
    assert sigmas.device == relative_coordinates.device, "relative_coordinates and sigmas should be on the same device."
    assert relative_coordinates.shape == sigmas.shape, "The relative coordinates and sigmas array should have the same shape."
    assert len(relative_coordinates.shape) >= 3, "relative_coordinates should have at least 3 dimensions."
    shape = relative_coordinates.shape
    status = _status(relative_coordinates.device) if relative_coordinates.is_cuda else None
    out = kernels.log_wrapped_gaussians(relative_coordinates.to(torch.float32).contiguous(), sigmas.to(torch.float32).contiguous(),
                                        kmax, shape[-2] * shape[-1], status=status)
    kernels.raise_analytical_status(status)
    return out.reshape(shape[:-2])


def get_sigma_normalized_score_brute_force(u: float, sigma: float, kmax: Optional[int] = None) -> float:
    """The plain sum over k in [-kmax, kmax] (default: max(1, round(10 sigma))), in Python floats on the host (:95-128)."""
    z = 0.0
    sigma2_derivative_z = 0.0

    if kmax is None:
        kmax = np.max([1, np.round(10 * sigma)])

    for k in np.arange(-kmax, kmax + 1):
        upk = u + k
        exp = np.exp(-0.5 * upk**2 / sigma**2)

        z += exp
        sigma2_derivative_z += -upk * exp

    sigma2_score = sigma2_derivative_z / z
    sigma_score = sigma2_score / sigma

    return sigma_score


def get_coordinates_sigma_normalized_score(relative_coordinates: torch.Tensor, sigmas: torch.Tensor, kmax: int,
                                           coordinates_bounded: bool = True) -> torch.Tensor:
    """sigma x score of the wrapped Gaussian for tensors of any (equal) shape (:131-198): formula 1a for sigma <= 1/sqrt(2 pi)
    and u < 0.5, 1b for u >= 0.5, the Ewald form for larger sigma."""
    assert kmax >= 0, "kmax must be a non negative integer"
    assert sigmas.shape == relative_coordinates.shape, "The relative_coordinates and sigmas inputs should have the same shape"
    assert sigmas.device == relative_coordinates.device, "relative_coordinates and sigmas should be on the same device."
    status = _status(relative_coordinates.device) if relative_coordinates.is_cuda else None
    out = kernels.wrapped_gaussian_sigma_normalized_score(relative_coordinates.to(torch.float32).contiguous(),
                                                          sigmas.to(torch.float32).contiguous(), kmax, coordinates_bounded,
                                                          status=status)
    kernels.raise_analytical_status(status)
    return out
