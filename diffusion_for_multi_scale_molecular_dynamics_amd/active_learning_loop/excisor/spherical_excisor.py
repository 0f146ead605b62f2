"""Every atom within a radius of the central atom (src/.../active_learning_loop/excisor/spherical_excisor.py:13-68)."""
from dataclasses import dataclass
from typing import Tuple

from ...namespace import AXL
from .base_excisor import BaseEnvironmentExcision, BaseEnvironmentExcisionArguments


@dataclass(kw_only=True)
class SphericalExcisionArguments(BaseEnvironmentExcisionArguments):
    algorithm: str = "spherical_cutoff"
    radial_cutoff: float = 3.0  # Angstrom

    def __post_init__(self):
        assert self.radial_cutoff > 0, f"Radial cutoff is expected to be positive. Got {self.radial_cutoff}"


class SphericalExcision(BaseEnvironmentExcision):
    def __init__(self, excision_arguments: SphericalExcisionArguments):
        super().__init__(excision_arguments)
        self.radial_cutoff = excision_arguments.radial_cutoff

    def _kernel_mode(self):
        return dict(radial_cutoff=self.radial_cutoff)

    def _excise_one_environment(self, structure: AXL, central_atom_idx: int) -> Tuple[AXL, int]:
        """The atoms closer than radial_cutoff (periodic distance), nearest first: the central atom is atom 0 (:45-68)."""
        return self._excise_one_with_kernel(structure, central_atom_idx)
