"""The sigma-normalised score of the (non-wrapped) Gaussian kernel of the lattice parameters: src/.../score/gaussian_score.py:16-38.

Inside the denoising loss this target is made by the fused kernel (mdx_denoising_loss); this is the reference's function for a
plugin that calls it by name, one elementwise expression on tensors of any device.
"""
import torch


def get_lattice_sigma_normalized_score(noisy_l: torch.Tensor, real_l: torch.Tensor, sigma_n: torch.Tensor) -> torch.Tensor:
    """-(noisy_l - real_l) / sigma_n"""
    sigma_score = -(noisy_l - real_l) / sigma_n
    return sigma_score
