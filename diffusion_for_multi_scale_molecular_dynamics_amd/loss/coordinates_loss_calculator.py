"""The unreduced loss of the relative coordinates (and of the lattice parameters): src/.../loss/coordinates_loss_calculator.py:7-120.

Float32 device tensors without autograd go through the fused loss kernel (mdx_denoising_loss with the target given: binary64
inside, one rounding); anything else -- host tensors are refused -- is the reference's own torch expression, which autograd can
follow.
"""
import torch

from .. import kernels
from .loss_parameters import LossParameters, MSELossParameters, WeightedMSELossParameters


def _kernel_operands(*tensors) -> bool:
    return all(t.dtype == torch.float32 for t in tensors) and not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


class CoordinatesLossCalculator(torch.nn.Module):
    """Class to calculate the loss."""

    def __init__(self, loss_parameters: LossParameters):
        super().__init__()
        self.loss_parameters = loss_parameters

    def calculate_unreduced_loss(self, predicted_normalized_scores: torch.tensor,
                                 target_normalized_conditional_scores: torch.tensor, sigmas: torch.Tensor) -> torch.tensor:
        """All three of one shape [batch_size, ...]; returns the unreduced loss of that shape: its mean is the loss."""
        raise NotImplementedError


class MSELossCalculator(CoordinatesLossCalculator):
    """(predicted - target)^2."""

    algorithm = "mse"

    def __init__(self, loss_parameters: MSELossParameters):
        super().__init__(loss_parameters)
        self.mse_loss = torch.nn.MSELoss(reduction="none")

    def _kernel_scalars(self) -> dict:
        return dict(x_algorithm=self.algorithm)

    def _weights(self, sigmas):
        return None

    def calculate_unreduced_loss(self, predicted_normalized_scores: torch.tensor,
                                 target_normalized_conditional_scores: torch.tensor, sigmas: torch.Tensor) -> torch.tensor:
        predicted, target = predicted_normalized_scores, target_normalized_conditional_scores
        assert predicted.shape == target.shape == sigmas.shape, "Inconsistent shapes"
        kernels._device_only("the denoising loss", predicted_normalized_scores=predicted,
                             target_normalized_conditional_scores=target, sigmas=sigmas)
        if _kernel_operands(predicted, target, sigmas) and predicted.dim() >= 1 and predicted.numel() > 0:
            # [B, N, D] as it is, any other shape as [B, elements, 1]: one workgroup per leading entry
            shape = tuple(predicted.shape) if predicted.dim() == 3 and predicted.shape[2] <= 3 else (predicted.shape[0], -1, 1)
            operands = [t.reshape(shape).contiguous() for t in (predicted, target, sigmas)]
            out = kernels.denoising_loss(predicted_x=operands[0], target_x=operands[1], sigma=operands[2], **self._kernel_scalars())
            return out.loss_x.reshape(predicted.shape)
        unreduced_loss = self.mse_loss(predicted, target)
        weights = self._weights(sigmas)
        return unreduced_loss if weights is None else unreduced_loss * weights


class WeightedMSELossCalculator(MSELossCalculator):
    """(predicted - target)^2 (exp(exponent (sigmas - sigma0)) + 1); sigma0 and exponent are 0-dim float32 buffers, as in the
    reference (:81-82): their binary32 values are what enters the arithmetic in any precision."""

    algorithm = "weighted_mse"

    def __init__(self, loss_parameters: WeightedMSELossParameters):
        super().__init__(loss_parameters)
        self.register_buffer("sigma0", torch.tensor(loss_parameters.sigma0))
        self.register_buffer("exponent", torch.tensor(loss_parameters.exponent))
        self._scalars = dict(x_algorithm=self.algorithm, x_sigma0=kernels.binary32(loss_parameters.sigma0),
                             x_exponent=kernels.binary32(loss_parameters.exponent))

    def _kernel_scalars(self) -> dict:
        return self._scalars

    def _exponential_weights(self, sigmas):
        return torch.exp(self.exponent * (sigmas - self.sigma0)) + 1.0

    def _weights(self, sigmas):
        return self._exponential_weights(sigmas)
