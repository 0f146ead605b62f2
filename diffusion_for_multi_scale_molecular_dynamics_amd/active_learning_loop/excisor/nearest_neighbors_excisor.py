"""The central atom and its N nearest atoms (src/.../active_learning_loop/excisor/nearest_neighbors_excisor.py:13-67)."""
from dataclasses import dataclass
from typing import Tuple

from ...namespace import AXL
from .base_excisor import BaseEnvironmentExcision, BaseEnvironmentExcisionArguments


@dataclass(kw_only=True)
class NearestNeighborsExcisionArguments(BaseEnvironmentExcisionArguments):
    algorithm: str = "nearest_neighbors"
    number_of_neighbors: int = 4  # besides the central atom itself

    def __post_init__(self):
        assert self.number_of_neighbors > 0, \
            f"Number of neighbors to include is expected to be positive. Got {self.number_of_neighbors}"


class NearestNeighborsExcision(BaseEnvironmentExcision):
    def __init__(self, excision_arguments: NearestNeighborsExcisionArguments):
        super().__init__(excision_arguments)
        self.number_of_neighbors = excision_arguments.number_of_neighbors

    def _kernel_mode(self):
        return dict(number_of_neighbors=self.number_of_neighbors)

    def _excise_one_environment(self, structure: AXL, central_atom_idx: int) -> Tuple[AXL, int]:
        """The number_of_neighbors + 1 atoms nearest the central atom (periodic distance), nearest first (:48-67)."""
        return self._excise_one_with_kernel(structure, central_atom_idx)
