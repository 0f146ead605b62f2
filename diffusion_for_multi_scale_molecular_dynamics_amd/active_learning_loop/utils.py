"""Host helpers of the active-learning loop (src/.../active_learning_loop/utils.py): numpy and pandas on small arrays.  The
distances of a whole frame's environments are computed on the GPU (mdx_excise_environments, mdx_edit_keep_mask); the function
of that name here serves callers with one numpy structure, in the same arithmetic."""
from typing import List, Optional, Tuple

import numpy as np
import pandas as pd
import torch

from ..utils.basis_transformations import get_positions_from_coordinates, map_lattice_parameters_to_unit_cell_vectors


def get_structures_for_retraining(prediction_df: pd.DataFrame, criteria_threshold: Optional[float] = None,
                                  number_of_structures: Optional[int] = None, evaluation_criteria: str = "nbh_grades",
                                  structure_index: str = "structure_index") -> List[pd.DataFrame]:
    """The structures whose WORST atom has the highest criterion (:37-62): at or above the threshold if one is given, the first
    `number_of_structures` of them if a number is given, one dataframe per structure."""
    assert criteria_threshold is not None or number_of_structures is not None, \
        "criteria_threshold or number_of_structures should be set."
    worst = prediction_df[[evaluation_criteria, structure_index]].groupby(structure_index).max()
    worst = worst.sort_values(by=evaluation_criteria, ascending=False)
    if criteria_threshold is not None:
        worst = worst[worst[evaluation_criteria] >= criteria_threshold]
    chosen = worst.index.to_list()
    if number_of_structures is not None:
        chosen = chosen[:number_of_structures]
    return [prediction_df[prediction_df[structure_index] == index] for index in chosen]


def extract_target_region(structure_df: pd.DataFrame, extraction_radius: float,
                          evaluation_criteria: str = "nbh_grades") -> pd.DataFrame:
    """The atom with the worst criterion and the atoms within `extraction_radius` of it, without periodic images (:84-95;
    obsolete in the reference: the excisors replace it).  Adds the column `distance_squared` to the frame, as the reference."""
    target = structure_df[evaluation_criteria].idxmax()
    centre = structure_df.loc[target][["x", "y", "z"]]
    structure_df.loc[:, "distance_squared"] = structure_df.apply(
        lambda row: sum([(row[axis] - centre[axis]) ** 2 for axis in ["x", "y", "z"]]), axis=1)
    return structure_df.loc[structure_df["distance_squared"] <= extraction_radius ** 2, ["x", "y", "z", "species"]]


def get_distances_from_reference_point(atom_relative_coordinates: np.ndarray, reference_point_relative_coordinates: np.array,
                                       lattice_parameters: np.array) -> np.ndarray:
    """Periodic distances (Angstrom) of atoms [natom, d] from one point [d] in an orthogonal box (:113-135): the Cartesian
    difference, per dimension the least of D^2, (D - L)^2, (D + L)^2, the square root of the sum -- in the arrays' own dtype."""
    basis_vectors = map_lattice_parameters_to_unit_cell_vectors(torch.tensor(lattice_parameters))
    positions = get_positions_from_coordinates(torch.tensor(atom_relative_coordinates), basis_vectors).numpy()
    reference = get_positions_from_coordinates(torch.tensor(reference_point_relative_coordinates).unsqueeze(0),
                                               basis_vectors).numpy()
    sides = torch.diag(basis_vectors).numpy()
    difference = positions - reference
    squared = np.minimum(difference ** 2, (difference - sides) ** 2)
    squared = np.minimum(squared, (difference + sides) ** 2)
    return np.sqrt(squared.sum(axis=-1))


def find_partition_sizes(box_size: np.array, n_voxel: int) -> np.array:
    """Voxels per axis of an orthorhombic box for about `n_voxel` voxels of near-cubic shape (:153-164): the sides scaled by
    (n_voxel / volume)^(1/d), rounded, at least 1."""
    assert box_size.ndim == 1
    assert np.all(box_size > 0)
    scale = (n_voxel / np.prod(box_size)) ** (1 / box_size.shape[0])
    return np.round(box_size * scale).clip(min=1).astype(int)


def partition_relative_coordinates_for_voxels(box_size: np.array, n_voxel: int) -> Tuple[np.ndarray, np.array]:
    """The voxels' corners in relative coordinates [d, number of voxels] and the partition (:182-188)."""
    partition = find_partition_sizes(box_size, n_voxel)
    meshes = np.meshgrid(*[np.linspace(0, 1, p, endpoint=False) for p in partition], indexing="ij")
    return np.stack(meshes).reshape(len(meshes), -1), partition


def select_occupied_voxels(num_voxels, num_atoms) -> np.array:
    """Voxel indices for `num_atoms` atoms with as few voxels shared as possible (:203-212): all of them once per full round,
    the rest drawn without replacement from numpy's global generator."""
    if num_atoms == num_voxels:
        return np.arange(num_voxels)
    if num_atoms < num_voxels:
        return np.random.choice(np.arange(num_voxels), size=num_atoms, replace=False)
    return np.concatenate((np.arange(num_voxels), select_occupied_voxels(num_voxels, num_atoms - num_voxels)))
