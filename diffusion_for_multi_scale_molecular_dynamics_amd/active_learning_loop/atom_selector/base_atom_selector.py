"""Atom selection skeleton (src/.../active_learning_loop/atom_selector/base_atom_selector.py:7-30)."""
from abc import ABC, abstractmethod
from dataclasses import dataclass

import numpy as np


@dataclass(kw_only=True)
class BaseAtomSelectorParameters:
    algorithm: str


class BaseAtomSelector(ABC):
    def __init__(self, atom_selector_parameters: BaseAtomSelectorParameters):
        self.atom_selector_parameters = atom_selector_parameters

    @abstractmethod
    def select_central_atoms(self, uncertainty_per_atom: np.array) -> np.array:
        """Indices of the selected atoms, from the highest uncertainty to the lowest."""
