"""The discrete-diffusion (D3PM) loss of the atom types: src/.../loss/atom_type_loss_calculator.py:9-266.

The methods take the reference's operands: one-hot vectors [batch, atoms, classes] and transition matrices per atom
[batch, atoms, classes, classes].  When those matrices are an expand() of one matrix per structure -- what
NoisingTransform returns -- and the other operands are float32 device tensors outside autograd, the work is done by the fused
loss kernel (mdx_denoising_loss, binary64 inside) on the per-structure rows; the [batch, atoms, classes, classes] broadcast is
never materialised.  Any other operands are evaluated with utils/d3pm_utils, as the reference does.
"""
import torch

from .. import kernels
from ..utils.d3pm_utils import class_index_to_onehot, get_probability_at_previous_time_step
from .loss_parameters import AtomTypeLossParameters


def _per_structure_rows(matrices: torch.Tensor):
    """The contiguous [batch, classes, classes] tensor a [batch, atoms, classes, classes] view expands, or None."""
    if matrices.dim() != 4 or not matrices.is_cuda or matrices.dtype != torch.float32:
        return None
    if matrices.shape[1] != 1 and matrices.stride(1) != 0:
        return None
    rows = matrices[:, 0]
    return rows if rows.is_contiguous() else None


def _class_indices(one_hot: torch.Tensor):
    """The class indices of strict one-hot vectors [batch, atoms, classes] on the device, or None (one host read)."""
    if one_hot.dim() != 3 or not one_hot.is_cuda:
        return None
    indices = one_hot.argmax(dim=-1)
    if not bool((class_index_to_onehot(indices, one_hot.shape[-1]) == one_hot.to(torch.float)).all()):
        return None
    return indices.contiguous()


def _outside_autograd(*tensors) -> bool:
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


def _kernel_logits(predicted_logits: torch.Tensor) -> bool:
    return (predicted_logits.is_cuda and predicted_logits.dim() == 3 and predicted_logits.dtype == torch.float32
            and _outside_autograd(predicted_logits))


class D3PMLossCalculator(torch.nn.Module):
    """Class to calculate the discrete diffusion loss."""

    def __init__(self, loss_parameters: AtomTypeLossParameters):
        super().__init__()
        self.ce_weight = loss_parameters.ce_weight      # weight of the cross-entropy component
        self.eps = loss_parameters.eps

    @staticmethod
    def _refuse_host(**tensors):
        kernels._device_only("the denoising loss", **tensors)

    @staticmethod
    def _fused(one_hot_a0, one_hot_at, q_matrices, q_bar_matrices, q_bar_tm1_matrices, predicted_logits=None):
        """The kernel's operands when the reference's operands allow it, else None."""
        if predicted_logits is not None and not _kernel_logits(predicted_logits):
            return None
        tables = [_per_structure_rows(m) for m in (q_matrices, q_bar_matrices, q_bar_tm1_matrices)]
        if any(t is None for t in tables):
            return None
        a0, at = _class_indices(one_hot_a0), _class_indices(one_hot_at)
        if a0 is None or at is None:
            return None
        operands = dict(a0=a0, at=at, q_matrices=tables[0], q_bar_matrices=tables[1], q_bar_tm1_matrices=tables[2],
                        tables_per_structure=True, with_terms=True)
        if predicted_logits is not None:
            operands["logits"] = predicted_logits.contiguous()
        return operands

    def cross_entropy_loss_term(self, predicted_logits: torch.Tensor, one_hot_real_atom_types: torch.Tensor) -> torch.Tensor:
        """-log p~(a_0 | a_t) at the real class, the MASK column squashed to 0  (:19-48).  [batch, atoms, classes]."""
        self._refuse_host(predicted_logits=predicted_logits, one_hot_real_atom_types=one_hot_real_atom_types)
        a0 = _class_indices(one_hot_real_atom_types) if _kernel_logits(predicted_logits) else None
        if a0 is not None:
            return kernels.denoising_loss(a0=a0, logits=predicted_logits.contiguous(), eps=self.eps, with_terms=True).ce_term
        nll_term = -torch.nn.functional.log_softmax(predicted_logits, dim=-1)
        nll_term[..., -1] = 0.0
        return one_hot_real_atom_types * nll_term

    def variational_bound_loss_term(self, predicted_logits: torch.Tensor, one_hot_real_atom_types: torch.Tensor,
                                    one_hot_noisy_atom_types: torch.Tensor, q_matrices: torch.Tensor,
                                    q_bar_matrices: torch.Tensor, q_bar_tm1_matrices: torch.Tensor,
                                    time_indices: torch.Tensor) -> torch.Tensor:
        """t == 1: -log p(a_0 | a_1); t != 1: KL[q(a_{t-1} | a_t, a_0) || p(a_{t-1} | a_t)]  (:50-126).  [batch, atoms, classes]."""
        self._refuse_host(predicted_logits=predicted_logits, one_hot_real_atom_types=one_hot_real_atom_types,
                          one_hot_noisy_atom_types=one_hot_noisy_atom_types, q_matrices=q_matrices,
                          q_bar_matrices=q_bar_matrices, q_bar_tm1_matrices=q_bar_tm1_matrices, time_indices=time_indices)
        fused = self._fused(one_hot_real_atom_types, one_hot_noisy_atom_types, q_matrices, q_bar_matrices, q_bar_tm1_matrices,
                            predicted_logits)
        if fused is not None:
            return kernels.denoising_loss(time_indices=time_indices.to(torch.int64).contiguous(), ce_weight=self.ce_weight,
                                          eps=self.eps, **fused).vb_term
        q_atm1_given_at_and_a0 = self.get_q_atm1_given_at_and_a0(
            one_hot_a0=one_hot_real_atom_types, one_hot_at=one_hot_noisy_atom_types, q_matrices=q_matrices,
            q_bar_matrices=q_bar_matrices, q_bar_tm1_matrices=q_bar_tm1_matrices, small_epsilon=self.eps)
        p_atm1_given_at = self.get_p_atm1_given_at(
            predicted_logits=predicted_logits, one_hot_at=one_hot_noisy_atom_types, q_matrices=q_matrices,
            q_bar_matrices=q_bar_matrices, q_bar_tm1_matrices=q_bar_tm1_matrices, small_epsilon=self.eps)
        log_p = torch.log(p_atm1_given_at.clip(min=self.eps))
        variational_bound_loss = torch.nn.functional.kl_div(log_p, q_atm1_given_at_and_a0, reduction="none")
        first_time_step_mask = time_indices == 0
        variational_bound_loss[first_time_step_mask] = \
            -log_p[first_time_step_mask] * one_hot_real_atom_types[first_time_step_mask]
        return variational_bound_loss

    @classmethod
    def get_q_atm1_given_at_and_a0(cls, one_hot_a0: torch.Tensor, one_hot_at: torch.Tensor, q_matrices: torch.Tensor,
                                   q_bar_matrices: torch.Tensor, q_bar_tm1_matrices: torch.Tensor,
                                   small_epsilon: float) -> torch.Tensor:
        """q(a_{t-1} | a_t, a_0)  (:128-165).  [batch, atoms, classes]."""
        cls._refuse_host(one_hot_a0=one_hot_a0, one_hot_at=one_hot_at, q_matrices=q_matrices, q_bar_matrices=q_bar_matrices,
                         q_bar_tm1_matrices=q_bar_tm1_matrices)
        fused = cls._fused(one_hot_a0, one_hot_at, q_matrices, q_bar_matrices, q_bar_tm1_matrices)
        if fused is not None:
            zeros = torch.zeros(one_hot_a0.shape[0], dtype=torch.int64, device=one_hot_a0.device)
            return kernels.denoising_loss(time_indices=zeros, eps=small_epsilon, **fused).q_atm1
        return get_probability_at_previous_time_step(
            probability_at_zeroth_timestep=one_hot_a0, one_hot_probability_at_current_timestep=one_hot_at,
            q_matrices=q_matrices, q_bar_matrices=q_bar_matrices, q_bar_tm1_matrices=q_bar_tm1_matrices,
            small_epsilon=small_epsilon, probability_at_zeroth_timestep_are_logits=False)

    @classmethod
    def get_p_atm1_given_at(cls, predicted_logits: torch.Tensor, one_hot_at: torch.Tensor, q_matrices: torch.Tensor,
                            q_bar_matrices: torch.Tensor, q_bar_tm1_matrices: torch.Tensor,
                            small_epsilon: float) -> torch.Tensor:
        """p(a_{t-1} | a_t) from the logits of p(a_0 | a_t)  (:167-208).  [batch, atoms, classes]."""
        cls._refuse_host(predicted_logits=predicted_logits, one_hot_at=one_hot_at, q_matrices=q_matrices,
                         q_bar_matrices=q_bar_matrices, q_bar_tm1_matrices=q_bar_tm1_matrices)
        # (the kernel's a_0 is only read by the terms this method does not return: a_t stands in for it)
        fused = cls._fused(one_hot_at, one_hot_at, q_matrices, q_bar_matrices, q_bar_tm1_matrices, predicted_logits)
        if fused is not None:
            zeros = torch.zeros(one_hot_at.shape[0], dtype=torch.int64, device=one_hot_at.device)
            return kernels.denoising_loss(time_indices=zeros, eps=small_epsilon, **fused).p_atm1
        return get_probability_at_previous_time_step(
            probability_at_zeroth_timestep=predicted_logits, one_hot_probability_at_current_timestep=one_hot_at,
            q_matrices=q_matrices, q_bar_matrices=q_bar_matrices, q_bar_tm1_matrices=q_bar_tm1_matrices,
            small_epsilon=small_epsilon, probability_at_zeroth_timestep_are_logits=True)

    def calculate_unreduced_loss(self, predicted_logits: torch.Tensor, one_hot_real_atom_types: torch.Tensor,
                                 one_hot_noisy_atom_types: torch.Tensor, time_indices: torch.Tensor, q_matrices: torch.Tensor,
                                 q_bar_matrices: torch.Tensor, q_bar_tm1_matrices: torch.Tensor) -> torch.Tensor:
        """The variational-bound term plus ce_weight times the cross-entropy term  (:210-266).  [batch, atoms, classes]; its
        mean is the loss."""
        self._refuse_host(predicted_logits=predicted_logits, one_hot_real_atom_types=one_hot_real_atom_types,
                          one_hot_noisy_atom_types=one_hot_noisy_atom_types, time_indices=time_indices, q_matrices=q_matrices,
                          q_bar_matrices=q_bar_matrices, q_bar_tm1_matrices=q_bar_tm1_matrices)
        fused = self._fused(one_hot_real_atom_types, one_hot_noisy_atom_types, q_matrices, q_bar_matrices, q_bar_tm1_matrices,
                            predicted_logits)
        if fused is not None:
            fused["with_terms"] = False
            return kernels.denoising_loss(time_indices=time_indices.to(torch.int64).contiguous(), ce_weight=self.ce_weight,
                                          eps=self.eps, **fused).loss_a
        vb_term = self.variational_bound_loss_term(predicted_logits, one_hot_real_atom_types, one_hot_noisy_atom_types,
                                                   q_matrices, q_bar_matrices, q_bar_tm1_matrices, time_indices)
        ce_term = self.cross_entropy_loss_term(predicted_logits, one_hot_real_atom_types)
        return vb_term + self.ce_weight * ce_term
