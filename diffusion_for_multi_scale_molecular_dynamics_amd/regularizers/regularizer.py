"""The regularizers' base class and parameters (src/.../regularizers/regularizer.py:10-89): an auxiliary loss beside score
matching, weighted by `regularizer_lambda_weight` and left out during the first `number_of_burn_in_epochs` epochs."""
from dataclasses import dataclass
from typing import Any, AnyStr, Dict

import torch

from ..models.score_networks.score_network import ScoreNetwork


@dataclass(kw_only=True)
class RegularizerParameters:
    """Base hyper-parameters of a regularizer (:10-23)."""

    type: str                                # which regularizer
    regularizer_lambda_weight: float = 1.0   # the prefactor of the regularizer's loss
    number_of_burn_in_epochs: int = 0        # epochs without regularization at the start of training

    def __post_init__(self):
        assert self.regularizer_lambda_weight > 0.0, "The regularizer weight must be positive."


class Regularizer(torch.nn.Module):
    """Base class of the regularizers (:26-89)."""

    def __init__(self, regularizer_parameters: RegularizerParameters):
        super().__init__()
        self.regularizer_parameters = regularizer_parameters
        self.weight = regularizer_parameters.regularizer_lambda_weight
        self.number_of_burn_in_epochs = regularizer_parameters.number_of_burn_in_epochs

    def can_regularizer_run(self):
        """Can the regularizer be executed from the global context?"""
        return True

    def compute_weighted_regularizer_loss(self, score_network: ScoreNetwork, augmented_batch: Dict[AnyStr, Any],
                                          current_epoch: int) -> torch.Tensor:
        """weight x compute_regularizer_loss on a batch that holds all the score network needs; tensor(0.0) during burn-in."""
        if current_epoch < self.number_of_burn_in_epochs:
            return torch.tensor(0.0)
        score_network._check_batch(augmented_batch)
        return self.weight * self.compute_regularizer_loss(score_network, augmented_batch)

    def compute_regularizer_loss(self, score_network: ScoreNetwork, augmented_batch: Dict[AnyStr, Any]) -> torch.Tensor:
        raise NotImplementedError("This method must be implemented in a child class.")
