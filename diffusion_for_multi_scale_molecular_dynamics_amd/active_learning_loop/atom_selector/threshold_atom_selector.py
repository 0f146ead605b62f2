"""Every atom above an uncertainty threshold (src/.../active_learning_loop/atom_selector/threshold_atom_selector.py:9-47)."""
from dataclasses import dataclass

import numpy as np

from .base_atom_selector import BaseAtomSelector, BaseAtomSelectorParameters


@dataclass(kw_only=True)
class ThresholdAtomSelectorParameters(BaseAtomSelectorParameters):
    algorithm: str = "threshold"
    uncertainty_threshold: float

    def __post_init__(self):
        assert self.uncertainty_threshold > 0., "Only positive uncertainty thresholds are allowed."


class ThresholdAtomSelector(BaseAtomSelector):
    def __init__(self, atom_selector_parameters: ThresholdAtomSelectorParameters):
        super().__init__(atom_selector_parameters)
        self.atom_selection_threshold = atom_selector_parameters.uncertainty_threshold

    def select_central_atoms(self, uncertainty_per_atom: np.array) -> np.array:
        """:39-47 -- the atoms above the threshold in ascending order of uncertainty (numpy's argsort), reversed."""
        above = np.where(uncertainty_per_atom > self.atom_selection_threshold)[0]
        return above[np.argsort(uncertainty_per_atom[above])][::-1]
