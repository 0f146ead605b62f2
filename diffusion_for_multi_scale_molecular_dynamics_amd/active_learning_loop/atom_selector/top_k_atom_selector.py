"""The k most uncertain atoms (src/.../active_learning_loop/atom_selector/top_k_atom_selector.py:9-45)."""
from dataclasses import dataclass

import numpy as np

from .base_atom_selector import BaseAtomSelector, BaseAtomSelectorParameters


@dataclass(kw_only=True)
class TopKAtomSelectorParameters(BaseAtomSelectorParameters):
    algorithm: str = "top_k"
    top_k_environment: int

    def __post_init__(self):
        assert self.top_k_environment > 0, f"top_k_environment should be positive. Got {self.top_k_environment}"


class TopKAtomSelector(BaseAtomSelector):
    def __init__(self, atom_selector_parameters: TopKAtomSelectorParameters):
        super().__init__(atom_selector_parameters)
        self.top_k = atom_selector_parameters.top_k_environment

    def select_central_atoms(self, uncertainty_per_atom: np.array) -> np.array:
        """:40-45 -- the last k of numpy's ascending argsort, reversed."""
        return np.argsort(uncertainty_per_atom)[-self.top_k:][::-1]
