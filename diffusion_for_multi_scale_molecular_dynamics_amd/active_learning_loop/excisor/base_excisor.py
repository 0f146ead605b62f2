"""Environment excision skeleton (src/.../active_learning_loop/excisor/base_excisor.py:10-88).

The two real excisors cut ALL the environments of a frame in one launch of mdx_excise_environments (one workgroup per central
atom; binary64 in the reference's operation order) instead of a Python loop over the central atoms; the AXLs that come back are
numpy, as in the reference.  There is no CPU fallback: without a GPU the excisors raise.  float32 structures are widened to
binary64 on the host before the launch; the returned X are rows of the caller's own array.

One rule is this package's own: atoms at EQUAL distance from the central atom are ordered by atom index, the lower first (the
reference sorts with numpy's argsort, which leaves the order of ties unspecified)."""
from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from ... import kernels
from ..._hip import STATUS_EXCISE_CENTRAL_INDEX, STATUS_EXCISE_OUTSIDE_BOX, MdxError
from ...namespace import AXL


@dataclass(kw_only=True)
class BaseEnvironmentExcisionArguments:
    algorithm: str


def _excise_on_device(structure: AXL, central_atoms_indices, radial_cutoff: Optional[float] = None,
                      number_of_neighbors: Optional[int] = None, center_atoms: bool = True, new_box_sides=None):
    """One launch for every central atom.  Returns device tensors (source_indices int64 [E,K], constrained_x float32 [E,K,d],
    counts int32 [E]) with K = the largest environment, and the counts on the host.  The capacity is guessed (64 atoms, or the
    neighbour count) and the launch repeated once with the true maximum when an environment is larger."""
    if not torch.cuda.is_available():
        raise MdxError("environment excision runs on the GPU only (mdx_excise_environments; there is no CPU fallback)")
    device = torch.device("cuda", torch.cuda.current_device())
    x_host = np.ascontiguousarray(np.asarray(structure.X, dtype=np.float64))
    n, d = x_host.shape
    assert np.isfinite(x_host).all(), "the relative coordinates must be finite"
    x = torch.from_numpy(x_host).to(device)
    sides = torch.from_numpy(np.ascontiguousarray(np.asarray(structure.L, dtype=np.float64)[:d])).to(device)
    central = torch.from_numpy(np.ascontiguousarray(np.asarray(central_atoms_indices, dtype=np.int64)).reshape(-1)).to(device)
    new_sides = None if new_box_sides is None else \
        torch.from_numpy(np.ascontiguousarray(np.asarray(new_box_sides, dtype=np.float64)[:d])).to(device)
    capacity = min(n, 64 if number_of_neighbors is None else number_of_neighbors + 1)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    while True:
        status.zero_()
        source, cx, counts = kernels.excise_environments(x, sides, central, radial_cutoff, number_of_neighbors, center_atoms,
                                                         new_sides, capacity, status)
        host_counts = counts.cpu().numpy()
        largest = int(host_counts.max()) if len(host_counts) else 0
        if largest <= capacity:
            break
        capacity = largest
    word = int(status.item())
    if word & STATUS_EXCISE_CENTRAL_INDEX:
        raise IndexError(f"a central atom index is outside [0, {n})")
    if word & STATUS_EXCISE_OUTSIDE_BOX:
        raise AssertionError(kernels.EXCISION_OUTSIDE_BOX)
    largest = max(largest, 1)
    return source[:, :largest].contiguous(), cx[:, :largest].contiguous(), counts, host_counts


class BaseEnvironmentExcision(ABC):
    def __init__(self, excision_arguments: BaseEnvironmentExcisionArguments):
        self.arguments = excision_arguments

    def _kernel_mode(self) -> Optional[dict]:
        """radial_cutoff= or number_of_neighbors= of mdx_excise_environments; None: this excisor has no kernel form."""
        return None

    def excise_environments(self, structure: AXL, central_atoms_indices: np.array, center_atoms: bool = True
                            ) -> Tuple[List[AXL], List[int]]:
        """The environments around the central atoms and the index of the central atom in each (:41-52)."""
        mode = self._kernel_mode()
        if mode is None:
            excised_environments, excised_central_atoms_indices = [], []
            for atom_index in central_atoms_indices:
                environment, excised_atom_index = self._excise_one_environment(structure, atom_index)
                if center_atoms:
                    environment = self.center_structure(environment, excised_atom_index)
                excised_environments.append(environment)
                excised_central_atoms_indices.append(excised_atom_index)
            return excised_environments, excised_central_atoms_indices
        if len(central_atoms_indices) == 0:
            return [], []
        source, _, _, counts = _excise_on_device(structure, central_atoms_indices, center_atoms=False, **mode)
        return self.environments_from_source_indices(structure, source.cpu().numpy(), counts, center_atoms), [0] * len(counts)

    @classmethod
    def environments_from_source_indices(cls, structure: AXL, source_indices: np.ndarray, counts: np.ndarray,
                                         center_atoms: bool = True) -> List[AXL]:
        """The numpy AXLs of the environments whose atoms the kernel named (rows of the caller's arrays, sorted from the central
        atom outwards: the central atom is atom 0)."""
        environments = []
        for row, count in zip(source_indices, counts):
            chosen = row[:count]
            environment = AXL(A=structure.A[chosen], X=structure.X[chosen, :], L=structure.L)
            environments.append(cls.center_structure(environment, 0) if center_atoms else environment)
        return environments

    def excise_constraint_tables(self, structure: AXL, central_atoms_indices: np.array, new_lattice_parameters: np.array):
        """What the batched repaint generator pins, straight from the kernel and still on the device: (source_indices int64
        [E,K], constrained_x float32 [E,K,d] centred and embedded in the new box, counts int32 [E], counts on the host).
        Raises the reference's "outside the new box" assertion.  None for an excisor without a kernel form."""
        mode = self._kernel_mode()
        if mode is None:
            return None
        return _excise_on_device(structure, central_atoms_indices, center_atoms=True, new_box_sides=new_lattice_parameters, **mode)

    @staticmethod
    def center_structure(structure: AXL, atom_index: int) -> AXL:
        """Translate so that atom `atom_index` sits at the centre of the box (:65-74): mod(x + (0.5 - x_c), 1)."""
        centre = structure.X[atom_index, :]
        translation = np.ones_like(centre) * 0.5 - centre
        return AXL(A=structure.A, X=np.mod(structure.X + translation, 1), L=structure.L)

    @abstractmethod
    def _excise_one_environment(self, structure: AXL, central_atom_idx: int) -> Tuple[AXL, int]:
        """The environment of one central atom, uncentred, and the central atom's index in it."""

    def _excise_one_with_kernel(self, structure: AXL, central_atom_idx: int) -> Tuple[AXL, int]:
        source, _, _, counts = _excise_on_device(structure, [central_atom_idx], center_atoms=False, **self._kernel_mode())
        return self.environments_from_source_indices(structure, source.cpu().numpy(), counts, center_atoms=False)[0], 0
