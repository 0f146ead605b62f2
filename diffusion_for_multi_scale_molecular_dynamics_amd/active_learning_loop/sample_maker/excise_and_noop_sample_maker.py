"""Excise and do nothing (src/.../active_learning_loop/sample_maker/excise_and_noop_sample_maker.py:9-46): the second control.
Every sample of an environment is the excised environment itself, in the new box."""
from dataclasses import dataclass
from typing import Any, Dict, List, Tuple

from ...namespace import AXL
from .base_sample_maker import BaseExciseSampleMaker, BaseExciseSampleMakerArguments


@dataclass(kw_only=True)
class ExciseAndNoOpSampleMakerArguments(BaseExciseSampleMakerArguments):
    algorithm: str = "excise_and_noop"


class ExciseAndNoOpSampleMaker(BaseExciseSampleMaker):
    def make_samples_from_constrained_substructure(self, substructure: AXL, active_atom_index: int, num_samples: int = 1
                                                   ) -> Tuple[List[AXL], List[int], List[Dict[str, Any]]]:
        """`num_samples` times the substructure, its active atom and its info dictionary (:39-42)."""
        infos = [self._create_sample_info_dictionary(substructure) for _ in range(num_samples)]
        return num_samples * [substructure], num_samples * [active_atom_index], infos

    def filter_made_samples(self, structures: List[AXL]) -> List[AXL]:
        return structures
