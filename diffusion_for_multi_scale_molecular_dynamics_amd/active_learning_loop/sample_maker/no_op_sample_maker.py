"""The trivial sample maker (src/.../active_learning_loop/sample_maker/no_op_sample_maker.py:13-43): the control of an
active-learning campaign.  The frame itself is the one sample; its active atoms are all the selected atoms."""
from dataclasses import dataclass
from typing import Any, Dict, List, Tuple

import numpy as np

from ...namespace import AXL
from ..atom_selector.base_atom_selector import BaseAtomSelector
from .base_sample_maker import BaseSampleMaker, BaseSampleMakerArguments


@dataclass(kw_only=True)
class NoOpSampleMakerArguments(BaseSampleMakerArguments):
    algorithm: str = "noop"
    sample_box_strategy: str = "noop"


class NoOpSampleMaker(BaseSampleMaker):
    def __init__(self, sample_maker_arguments: BaseSampleMakerArguments, atom_selector: BaseAtomSelector):
        super().__init__(sample_maker_arguments, atom_selector)

    def make_samples(self, structure: AXL, uncertainty_per_atom: np.array
                     ) -> Tuple[List[AXL], List[np.array], List[Dict[str, Any]]]:
        """([the structure], [the selected atoms], [the info dictionary of the whole structure]) (:32-39)."""
        selected = self.atom_selector.select_central_atoms(uncertainty_per_atom)
        return [structure], [selected], [self._create_sample_info_dictionary(structure)]

    def filter_made_samples(self, structures: List[AXL]) -> List[AXL]:
        return structures
