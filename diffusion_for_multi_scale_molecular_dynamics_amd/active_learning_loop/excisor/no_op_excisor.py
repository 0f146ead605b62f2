"""The whole structure as its own environment (src/.../active_learning_loop/excisor/no_op_excisor.py:9-22)."""
from dataclasses import dataclass
from typing import Tuple

from ...namespace import AXL
from .base_excisor import BaseEnvironmentExcision, BaseEnvironmentExcisionArguments


@dataclass(kw_only=True)
class NoOpExcisionArguments(BaseEnvironmentExcisionArguments):
    algorithm: str = "noop"


class NoOpExcision(BaseEnvironmentExcision):
    def _excise_one_environment(self, structure: AXL, central_atom_idx: int) -> Tuple[AXL, int]:
        return structure, central_atom_idx
