"""Excise and random (src/.../active_learning_loop/sample_maker/excise_and_random_sample_maker.py:22-367): the baseline of the
excise-and-repaint campaigns.  The same excision, but the rest of the small box is filled with atoms at random sites ("true_random":
anywhere in the cell; "voxel_random": one atom per voxel of a near-cubic partition, at a random place inside it) and random
types.  Every constrained atom, in order, replaces the proposed site nearest to it that is still free; a structure whose least
interatomic distance is not above `minimal_interatomic_distance` is drawn again, at most `max_attempts` times.

batch_environments = True (this package's own switch; an attribute, not a configuration field) cuts all environments of a frame
with the one-launch excision and fills all E x S samples in ONE launch of mdx_random_fill_environments, one workgroup per
sample, all attempts on the device.  The constraint tables are binary64, built from the embedded environments that also go into
the information dictionaries: a sample's constrained atoms are those arrays' numbers bit for bit, and a generated atom is a
proposed coordinate unchanged (or the voxel's corner + u / p, rounded as numpy rounds it).  Equal distances go to the LOWER
site index (numpy's argsort leaves them unspecified).

rng_mode (an attribute; default "reference", as the repaint maker's generator without an `rng_mode` in its sampling parameters):
  "reference"  the proposals are drawn on the host from numpy's GLOBAL generator through generate_random_relative_coordinates,
               select_occupied_voxels and generate_atom_types, for all max_attempts attempts of sample 0, then of sample 1, ...
               The reference's loop draws an attempt only when the one before it was rejected, so the two consume the stream
               differently: equal in distribution, not draw for draw.
  "device"     mdx_random_fill_proposals: Philox keyed by (torch.initial_seed(), the frame's call index, sample, attempt).
batch_environments = False is the reference's flow -- host numpy, one environment, one sample, one attempt after the other -- and
the only mode that reproduces the reference's stream position by position."""
import logging
from dataclasses import dataclass
from typing import Any, Dict, List, Tuple

import numpy as np
import torch

from ... import kernels
from ..._hip import MdxError
from ...namespace import AXL
from ...utils.basis_transformations import map_lattice_parameters_to_unit_cell_vectors
from ..atom_selector.base_atom_selector import BaseAtomSelector
from ..excisor.base_excisor import BaseEnvironmentExcision
from ..utils import get_distances_from_reference_point, partition_relative_coordinates_for_voxels, select_occupied_voxels
from .base_sample_maker import BaseExciseSampleMaker, BaseExciseSampleMakerArguments


@dataclass(kw_only=True)
class ExciseAndRandomSampleMakerArguments(BaseExciseSampleMakerArguments):
    algorithm: str = "excise_and_random"
    total_number_of_atoms: int                      # atoms of a sample, the excised ones included
    random_coordinates_algorithm: str = "true_random"
    max_attempts: int = 10
    minimal_interatomic_distance: float = 0.5       # Angstrom

    def __post_init__(self):
        super().__post_init__()
        assert self.random_coordinates_algorithm in ["true_random", "voxel_random"], \
            ("Random coordinates algorithm should be true_random or voxel_random."
             f"Got {self.random_coordinates_algorithm}")


class ExciseAndRandomSampleMaker(BaseExciseSampleMaker):
    batch_environments: bool = True
    rng_mode: str = "reference"

    def __init__(self, sample_maker_arguments: ExciseAndRandomSampleMakerArguments, atom_selector: BaseAtomSelector,
                 environment_excisor: BaseEnvironmentExcision):
        super().__init__(sample_maker_arguments, atom_selector, environment_excisor)
        self.num_atom_types = len(sample_maker_arguments.element_list)
        self._call_counter = 0                      # rng_mode "device": one Philox call index per frame
        self.last_attempts = None                   # batched path: the attempt returned for every sample of the last frame

    # -----------------------------------------------------------------------------------------------------------
    # the draws (numpy's global generator; the reference's tests patch these)
    # -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def generate_random_relative_coordinates(n_atoms: int, spatial_dimension: int = 3) -> np.ndarray:
        """Uniform relative coordinates [n_atoms, spatial_dimension] (:82)."""
        return np.random.random((n_atoms, spatial_dimension))

    @staticmethod
    def generate_atom_types(n_atoms: int, num_atom_types: int) -> np.array:
        """Uniform atom types [n_atoms] in [0, num_atom_types), whatever a dataset's composition (:98)."""
        return np.random.randint(0, num_atom_types, size=(n_atoms,))

    @staticmethod
    def sort_atoms_indices_by_distance(target_point: np.array, atom_relative_coordinates: np.ndarray,
                                       lattice_parameters: np.array) -> np.array:
        """Atom indices from the nearest to `target_point` to the farthest, by periodic distance (:118-121)."""
        return np.argsort(get_distances_from_reference_point(atom_relative_coordinates, target_point, lattice_parameters))

    def generate_relative_coordinates_true_random(self, spatial_dimension) -> np.ndarray:
        return self.generate_random_relative_coordinates(self.arguments.total_number_of_atoms, spatial_dimension)

    def _box_sides(self, lattice_parameters) -> np.ndarray:
        return map_lattice_parameters_to_unit_cell_vectors(torch.tensor(lattice_parameters)).diag().numpy()

    def generate_relative_coordinates_voxel_random(self, lattice_parameters) -> np.ndarray:
        """One atom per occupied voxel: the voxel's corner + u / (voxels per axis) (:135-167).  Draws u, then the occupancy."""
        number_of_atoms = self.arguments.total_number_of_atoms
        corners, voxels_per_axis = partition_relative_coordinates_for_voxels(self._box_sides(lattice_parameters), number_of_atoms)
        spatial_dimension, number_of_voxels = corners.shape
        inside = self.generate_random_relative_coordinates(number_of_atoms, spatial_dimension)
        inside /= voxels_per_axis
        occupied = select_occupied_voxels(number_of_voxels, number_of_atoms)
        return corners[:, occupied].transpose() + inside

    # -----------------------------------------------------------------------------------------------------------
    # one structure, one sample, one environment (the reference's flow, host numpy)
    # -----------------------------------------------------------------------------------------------------------
    def make_single_structure(self, constrained_structure: AXL, active_atom_index: int) -> Tuple[AXL, int]:
        """One attempt (:180-260): N proposed atoms; constrained atom k, in order, takes the place of the nearest proposed atom
        that no earlier one took.  Returns the structure -- the constrained atoms first, in their order, then the proposed atoms
        left, in theirs -- and the active atom's index in it."""
        constrained_x, constrained_a, lattice = constrained_structure.X, constrained_structure.A, constrained_structure.L
        match self.arguments.random_coordinates_algorithm:
            case "true_random":
                proposed_x = self.generate_relative_coordinates_true_random(constrained_x.shape[-1])
            case "voxel_random":
                proposed_x = self.generate_relative_coordinates_voxel_random(lattice)
            case _:
                proposed_x = constrained_x
        atom_types = self.generate_atom_types(self.arguments.total_number_of_atoms, self.num_atom_types)
        coordinates = proposed_x.copy()
        taken = []
        for x, a in zip(constrained_x, constrained_a):
            for site in self.sort_atoms_indices_by_distance(x, proposed_x, lattice):
                if site not in taken:
                    taken.append(site)
                    coordinates[site], atom_types[site] = x, a
                    break
        assert 0 <= active_atom_index < len(taken), "The new active atom index is not set. Something went wrong."
        generated = np.ones(len(proposed_x), dtype=bool)
        generated[taken] = False
        structure = AXL(A=np.concatenate([atom_types[taken], atom_types[generated]]),
                        X=np.vstack([coordinates[taken], coordinates[generated]]), L=lattice)
        return structure, int(active_atom_index)         # (the constrained atoms keep their order: so does the active one)

    @staticmethod
    def get_shortest_distance_between_atoms(atom_relative_coordinates: np.ndarray, lattice_parameters: np.array) -> float:
        """The least periodic distance between two atoms (:275-284): per atom the second smallest of its distances to all
        atoms (the smallest is its distance to itself), the least of those."""
        return min(np.partition(get_distances_from_reference_point(atom_relative_coordinates, x, lattice_parameters), 1)[1]
                   for x in atom_relative_coordinates)

    def _warn_not_separated(self, how_many: int = None):
        text = (f"A sample structure with all inter-atomic distances larger than {self.arguments.minimal_interatomic_distance} "
                f"could not be generated in {self.arguments.max_attempts} attempts. The last generated structure is returned.")
        logging.warning(text if how_many is None else f"{text} ({how_many} samples of this frame)")

    def make_single_sample_from_constrained_substructure(self, constrained_structure: AXL, active_atom_index: int
                                                         ) -> Tuple[AXL, int]:
        """Attempts until the least interatomic distance exceeds minimal_interatomic_distance, at most max_attempts; the last
        one is returned, with a warning, when none does (:302-328)."""
        count, total = constrained_structure.X.shape[0], self.arguments.total_number_of_atoms
        assert count <= total, kernels.RANDOM_FILL_TOO_MANY_CONSTRAINED.format(count, total)
        structure, active = None, None
        for _ in range(self.arguments.max_attempts):
            structure, active = self.make_single_structure(constrained_structure, active_atom_index)
            if self.get_shortest_distance_between_atoms(structure.X, structure.L) > self.arguments.minimal_interatomic_distance:
                return structure, active
        self._warn_not_separated()
        return structure, active

    def make_samples_from_constrained_substructure(self, substructure: AXL, active_atom_index: int, num_samples: int = 1
                                                   ) -> Tuple[List[AXL], List[int], List[Dict[str, Any]]]:
        """`num_samples` random fills around one substructure already in the new box (:352-363)."""
        samples, active_indices, infos = [], [], []
        for _ in range(num_samples):
            structure, active = self.make_single_sample_from_constrained_substructure(substructure, active_atom_index)
            samples.append(structure)
            active_indices.append(active)
            infos.append(self._create_sample_info_dictionary(substructure))
        return samples, active_indices, infos

    def filter_made_samples(self, structures: List[AXL]) -> List[AXL]:
        return structures

    # -----------------------------------------------------------------------------------------------------------
    # all environments of a frame in one launch
    # -----------------------------------------------------------------------------------------------------------
    def _voxel_partition(self, lattice_parameters):
        """(voxels per axis, number of voxels) of voxel_random, None for true_random."""
        if self.arguments.random_coordinates_algorithm != "voxel_random":
            return None, 0
        corners, voxels_per_axis = partition_relative_coordinates_for_voxels(self._box_sides(lattice_parameters),
                                                                             self.arguments.total_number_of_atoms)
        return [int(p) for p in voxels_per_axis], int(corners.shape[1])

    def _host_proposals(self, batch: int, spatial_dimension: int, number_of_voxels: int, device):
        """rng_mode "reference": per sample, per attempt: the coordinates, the voxel occupancy, the types -- the order of one
        make_single_structure."""
        N, M = self.arguments.total_number_of_atoms, self.arguments.max_attempts
        uniforms = np.empty((batch, M, N, spatial_dimension))
        types = np.empty((batch, M, N), dtype=np.int32)
        voxels = np.empty((batch, M, N), dtype=np.int32) if number_of_voxels else None
        for b in range(batch):
            for m in range(M):
                uniforms[b, m] = self.generate_random_relative_coordinates(N, spatial_dimension)
                if voxels is not None:
                    voxels[b, m] = select_occupied_voxels(number_of_voxels, N)
                types[b, m] = self.generate_atom_types(N, self.num_atom_types)
        return tuple(None if t is None else torch.from_numpy(t).to(device) for t in (uniforms, types, voxels))

    def make_samples(self, structure: AXL, uncertainty_per_atom: np.array
                     ) -> Tuple[List[AXL], List[np.array], List[Dict[str, Any]]]:
        if not self.batch_environments:
            return super().make_samples(structure, uncertainty_per_atom)
        assert self.rng_mode in ("reference", "device"), f"unknown rng_mode {self.rng_mode}"
        environments, in_new_box, central_indices, _ = self._excise_tables(structure, uncertainty_per_atom)
        if not environments:
            return [], [], []
        if not torch.cuda.is_available():
            raise MdxError("the batched random fill runs on the GPU only (mdx_random_fill_environments; there is no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
        S, N, M = self.arguments.number_of_samples_per_substructure, self.arguments.total_number_of_atoms, self.arguments.max_attempts
        E, K, d = len(in_new_box), max(len(e.X) for e in in_new_box), in_new_box[0].X.shape[-1]
        cx, ca, sides = np.zeros((E, K, d)), np.zeros((E, K), dtype=np.int64), np.zeros((E, d))
        for e, embedded in enumerate(in_new_box):
            count = len(embedded.X)
            assert count <= N, kernels.RANDOM_FILL_TOO_MANY_CONSTRAINED.format(count, N)
            cx[e, :count], ca[e, :count], sides[e] = embedded.X, embedded.A, self._box_sides(embedded.L)
        counts = np.array([len(e.X) for e in in_new_box], dtype=np.int32)
        partition, number_of_voxels = self._voxel_partition(in_new_box[0].L)
        for embedded in in_new_box[1:]:
            assert self._voxel_partition(embedded.L)[0] == partition, "the environments of a frame share one voxel partition"
        B = E * S
        if self.rng_mode == "device":
            uniforms, types, voxels = kernels.random_fill_proposals(torch.initial_seed(), self._call_counter, 0, B, M, N, d,
                                                                    self.num_atom_types, number_of_voxels, device)
            self._call_counter += 1
        else:
            uniforms, types, voxels = self._host_proposals(B, d, number_of_voxels, device)
        on_device = lambda array: torch.from_numpy(array).to(device)        # noqa: E731
        x, a, active, attempts, accepted, _ = kernels.random_fill_environments(
            uniforms, types, voxels, partition, on_device(cx), on_device(ca), on_device(counts),
            on_device(np.asarray(central_indices, dtype=np.int32)), torch.arange(E, dtype=torch.int32).repeat_interleave(S).to(device),
            on_device(sides), self.arguments.minimal_interatomic_distance)
        x, a, active, accepted = x.cpu().numpy(), a.cpu().numpy(), active.cpu().numpy(), accepted.cpu().numpy()
        self.last_attempts = attempts.cpu().numpy()                         # 1-based, per sample: the attempt returned
        if not accepted.all():
            self._warn_not_separated(int((accepted == 0).sum()))
        samples, active_indices, infos = [], [], []
        for e, (environment, embedded) in enumerate(zip(environments, in_new_box)):
            for b in range(e * S, (e + 1) * S):
                samples.append(AXL(A=a[b], X=x[b], L=embedded.L))
                active_indices.append(np.array([int(active[b])]))
                infos.append(self._with_structures(self._create_sample_info_dictionary(embedded), environment, embedded))
        return samples, active_indices, infos
