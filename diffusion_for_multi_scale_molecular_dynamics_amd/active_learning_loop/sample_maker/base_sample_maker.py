"""Sample maker skeletons (src/.../active_learning_loop/sample_maker/base_sample_maker.py:24-386): from a structure with
per-atom uncertainties to new candidate structures around the uncertain atoms."""
from abc import ABC, abstractmethod
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from ...namespace import AXL
from ...utils.basis_transformations import (get_positions_from_coordinates, get_reciprocal_basis_vectors,
                                            get_relative_coordinates_from_cartesian_positions,
                                            map_lattice_parameters_to_unit_cell_vectors,
                                            map_numpy_unit_cell_to_lattice_parameters)
from ..atom_selector.base_atom_selector import BaseAtomSelector
from ..excisor.base_excisor import BaseEnvironmentExcision
from .namespace import AXL_STRUCTURE_IN_NEW_BOX, AXL_STRUCTURE_IN_ORIGINAL_BOX

_UNLIMITED_CONSTRAINED_STRUCTURE = -1


@dataclass(kw_only=True)
class BaseSampleMakerArguments:
    algorithm: str
    sample_box_strategy: str = "fixed"
    sample_box_size: Optional[float] = None

    element_list: List[str]

    def __post_init__(self):
        assert self.sample_box_strategy in ["fixed", "noop"], \
            f"Sample box making strategy {self.sample_box_strategy} is not implemented."
        if self.sample_box_strategy == "fixed":
            assert self.sample_box_size is not None
            box_size = np.array(self.sample_box_size)
            unit_cell = np.diag(box_size) if box_size.ndim == 1 else box_size
            self.new_box_lattice_parameters = map_numpy_unit_cell_to_lattice_parameters(unit_cell)


class BaseSampleMaker(ABC):
    def __init__(self, sample_maker_arguments: BaseSampleMakerArguments, atom_selector: BaseAtomSelector, **kwargs):
        self.arguments = sample_maker_arguments
        self.atom_selector = atom_selector
        self.sample_box_strategy = sample_maker_arguments.sample_box_strategy

    @abstractmethod
    def make_samples(self, structure: AXL, uncertainty_per_atom: np.array
                     ) -> Tuple[List[AXL], List[np.array], List[Dict[str, Any]]]:
        """(sample structures, the active atoms' indices -- one array per sample --, information dictionaries)"""

    @abstractmethod
    def filter_made_samples(self, structures: List[AXL]) -> List[AXL]:
        """The samples that pass this maker's rejection rules."""

    def make_filtered_samples(self, structure: AXL, uncertainty_per_atom: np.array) -> List[AXL]:
        """make_samples, then filter_made_samples on what it returns (:113-115)."""
        return self.filter_made_samples(self.make_samples(structure, uncertainty_per_atom))

    def make_new_lattice_parameters(self, structure: AXL) -> np.array:
        """The box of the generated structures (:126-134): the structure's own ("noop") or the configured one ("fixed")."""
        match self.arguments.sample_box_strategy:
            case "noop":
                return structure.L
            case "fixed":
                return self.arguments.new_box_lattice_parameters
            case _:
                raise NotImplementedError(f"{self.arguments.sample_box_strategy} is an invalid box making strategy.")

    def _create_sample_info_dictionary(self, axl_structure: AXL) -> Dict[str, Any]:
        """The constrained atoms are the first atoms of a sample: their indices (:155-157)."""
        return dict(constrained_atom_indices=list(range(len(axl_structure.X))))


@dataclass(kw_only=True)
class BaseExciseSampleMakerArguments(BaseSampleMakerArguments):
    max_constrained_substructure: int = _UNLIMITED_CONSTRAINED_STRUCTURE      # environments considered; -1: all of them
    number_of_samples_per_substructure: int = 1

    def __post_init__(self):
        super().__post_init__()
        assert (self.max_constrained_substructure == _UNLIMITED_CONSTRAINED_STRUCTURE
                or self.max_constrained_substructure > 0), \
            ("max_constrained_substructure should be greater than 0 or be "
             f"equal to {_UNLIMITED_CONSTRAINED_STRUCTURE}."
             f"Got {self.max_constrained_substructure}")


class BaseExciseSampleMaker(BaseSampleMaker):
    """A sample maker that cuts the environments of the uncertain atoms out of the structure first."""

    def __init__(self, sample_maker_arguments: BaseExciseSampleMakerArguments, atom_selector: BaseAtomSelector,
                 environment_excisor: BaseEnvironmentExcision):
        super().__init__(sample_maker_arguments, atom_selector)
        self.environment_excisor = environment_excisor

    @abstractmethod
    def make_samples_from_constrained_substructure(self, substructure: AXL, active_atom_index: int, num_samples: int = 1
                                                   ) -> Tuple[List[AXL], List[int], List[Dict[str, Any]]]:
        """`num_samples` samples around one constrained substructure: (samples, active atom index per sample, info)."""

    @staticmethod
    def embed_structure_in_new_box(structure_with_centered_atoms: AXL, new_lattice_parameters: np.array) -> AXL:
        """The centred atoms keep their Cartesian offsets from the box centre and move to the centre of the new (orthogonal) box
        (:238-299): ((x - 0.5) L + 0.5 L_new) times the inverse of the new cell; an atom outside (0, L_new) is refused."""
        old_cell = map_lattice_parameters_to_unit_cell_vectors(torch.tensor(structure_with_centered_atoms.L))
        new_cell = map_lattice_parameters_to_unit_cell_vectors(torch.tensor(new_lattice_parameters))
        x = structure_with_centered_atoms.X
        offsets = get_positions_from_coordinates(torch.tensor(x - np.ones_like(x) * 0.5), basis_vectors=old_cell)
        d = x.shape[-1]
        centre = get_positions_from_coordinates((torch.ones(1, d) * 0.5).to(new_cell), basis_vectors=new_cell)
        positions = offsets + centre
        sides = torch.diag(new_cell)
        for axis in range(d):
            assert (torch.max(positions[:, axis]) < sides[axis]) and (torch.min(positions[:, axis]) > 0), \
                "Excised atoms are outside the new box. Use a larger box or smaller cutoff size for the excision."
        new_x = get_relative_coordinates_from_cartesian_positions(positions, get_reciprocal_basis_vectors(new_cell))
        return AXL(A=structure_with_centered_atoms.A, X=new_x.numpy(), L=new_lattice_parameters)

    def _excise(self, structure: AXL, uncertainty_per_atom: np.array) -> Tuple[List[AXL], List[int]]:
        """The centred environments of the selected atoms, at most max_constrained_substructure of them (:323-347)."""
        central_atom_indices = self.atom_selector.select_central_atoms(uncertainty_per_atom)
        environments, central_indices = self.environment_excisor.excise_environments(structure, central_atom_indices,
                                                                                     center_atoms=True)
        assert len(environments) == len(central_atom_indices), \
            "Number of excised environment do not match the number of central atom index. Something went wrong."
        limit = self.arguments.max_constrained_substructure
        if limit != _UNLIMITED_CONSTRAINED_STRUCTURE and limit < len(environments):
            environments, central_indices = environments[:limit], central_indices[:limit]
        return environments, central_indices

    def _in_new_box(self, environment: AXL) -> AXL:
        if self.sample_box_strategy == "fixed":
            return self.embed_structure_in_new_box(environment, self.arguments.new_box_lattice_parameters)
        return environment          # "noop"

    def _excise_tables(self, structure: AXL, uncertainty_per_atom: np.array):
        """(centred environments, the same in the new box, central atom indices, the float32 constraint tables
        of the repaint generator).  Shared by the makers that batch a frame's environments.  With a kernel
        excisor and a fixed box the tables come from ONE launch and stay on the device; the numpy structures of the
        information dictionaries are assembled on the host from the atoms the kernel named."""
        excisor = self.environment_excisor
        kernel_tables = None
        if self.sample_box_strategy == "fixed" and excisor._kernel_mode() is not None:
            central = self.atom_selector.select_central_atoms(uncertainty_per_atom)
            limit = self.arguments.max_constrained_substructure
            if limit != _UNLIMITED_CONSTRAINED_STRUCTURE:
                central = central[:limit]
            if len(central) == 0:
                return [], [], [], None
            kernel_tables = excisor.excise_constraint_tables(structure, central, self.arguments.new_box_lattice_parameters)
            source, cx, counts, host_counts = kernel_tables
            environments = excisor.environments_from_source_indices(structure, source.cpu().numpy(), host_counts, True)
            central_indices = [0] * len(environments)
        else:
            environments, central_indices = self._excise(structure, uncertainty_per_atom)
        in_new_box = [self._in_new_box(environment) for environment in environments]
        for embedded, central in zip(in_new_box, central_indices):
            assert central < len(embedded.X), \
                ("The active atom index is larger than the number of constrained atoms: "
                 "this should be impossible, something is wrong. Review code!")
        if kernel_tables is not None:
            ca = torch.from_numpy(np.asarray(structure.A, dtype=np.int64)).to(source.device)[source]
            return environments, in_new_box, central_indices, (cx, ca, None, counts)
        if not environments:
            return [], [], [], None
        E, K, d = len(in_new_box), max(len(e.X) for e in in_new_box), in_new_box[0].X.shape[-1]
        cx, ca = torch.zeros(E, K, d), torch.zeros(E, K, dtype=torch.int64)
        for e, embedded in enumerate(in_new_box):
            cx[e, :len(embedded.X)] = torch.FloatTensor(embedded.X)
            ca[e, :len(embedded.X)] = torch.LongTensor(embedded.A)
        counts = torch.tensor([len(e.X) for e in in_new_box], dtype=torch.int32)
        return environments, in_new_box, central_indices, (cx, ca, None, counts)

    @staticmethod
    def _with_structures(sample_info: Dict[str, Any], environment: AXL, environment_in_new_box: AXL) -> Dict[str, Any]:
        sample_info.update({AXL_STRUCTURE_IN_ORIGINAL_BOX: environment, AXL_STRUCTURE_IN_NEW_BOX: environment_in_new_box})
        return sample_info

    def make_samples(self, structure: AXL, uncertainty_per_atom: np.array
                     ) -> Tuple[List[AXL], List[np.array], List[Dict[str, Any]]]:
        """One call of make_samples_from_constrained_substructure per excised environment, in the selector's order (:323-386).
        `structure` holds numpy arrays."""
        samples, active_indices, infos = [], [], []
        for environment, central_atom_index in zip(*self._excise(structure, uncertainty_per_atom)):
            in_new_box = self._in_new_box(environment)
            new_samples, new_active, new_infos = self.make_samples_from_constrained_substructure(
                substructure=in_new_box, active_atom_index=central_atom_index,
                num_samples=self.arguments.number_of_samples_per_substructure)
            samples += new_samples
            active_indices += [np.array([index]) for index in new_active]
            infos += [self._with_structures(info, environment, in_new_box) for info in new_infos]
        return samples, active_indices, infos
