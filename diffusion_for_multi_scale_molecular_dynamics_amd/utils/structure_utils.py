"""Pair distances under periodic boundary conditions (src/.../utils/structure_utils.py:41-121), on the HIP radius graph.

Third consumer of kernel N1 (full mode: one edge per (source, destination, image) with its lattice shift).  The
reference returns the distances as an unordered bag (it feeds histograms / KS metrics); here they come out ordered by
(structure, source, destination, image).

Beside them, the energies the reference's `oracle:` block asks LAMMPS for (oracle/lammps_energy_oracle.py:56-158 through
oracle/energy_oracle.py:44-131): the Stillinger-Weber potential of every sample, evaluated by a HIP kernel on the same periodic
pair test -- the coefficient file reader, the parameters of the block and the reference's sample contract.
"""
import logging
import os
import warnings
from dataclasses import dataclass
from typing import AnyStr, Dict, List, Tuple

import torch

from .. import kernels
from ..data.element_types import ElementTypes
from ..namespace import ATOM_TYPES, AXL_COMPOSITION, LATTICE_PARAMETERS, RELATIVE_COORDINATES

logger = logging.getLogger(__name__)


def compute_distances_in_batch(cartesian_positions: torch.Tensor, unit_cell: torch.Tensor,
                               max_distance: float) -> torch.Tensor:
    """All distances 0 < |p_i - (p_j + image)| <= max_distance over the 27 nearest images, for every structure."""
    batch_size, n_atoms, d = cartesian_positions.shape
    assert d in (1, 2, 3) and unit_cell.shape == (batch_size, d, d)
    from .neighbors import embed_in_three_dimensions
    cart, cell = embed_in_three_dimensions(cartesian_positions, unit_cell, max_distance)     # (1-D / 2-D: see there)
    out = kernels.radius_graph(cart, cell, max_distance, unique=False, status=None)
    edges, shifts = out["edges"], out["shifts"]
    structure = torch.repeat_interleave(torch.arange(batch_size, device=cart.device), out["counts"].sum(dim=1))
    flat = cart.reshape(batch_size * n_atoms, 3)
    base = structure * n_atoms
    displacement = flat.index_select(0, base + edges[:, 1]) + shifts - flat.index_select(0, base + edges[:, 0])
    return torch.linalg.norm(displacement, dim=1)


def get_orthogonal_basis_vectors(batch_size: int, cell_dimensions: List[float]) -> torch.Tensor:
    """[batch_size, d, d]: diag(cell_dimensions), once per structure (:124-139)."""
    return torch.diag(torch.tensor(cell_dimensions, dtype=torch.float32)).expand(batch_size, -1, -1).clone()


def compute_distances(cartesian_positions: torch.Tensor, basis_vectors: torch.Tensor, max_distance: float) -> torch.Tensor:
    """The lengths of the edges of the periodic radius graph (get_periodic_adjacency_information: the cutoff must be below the
    shortest cell-crossing distance, unlike compute_distances_in_batch's 27-image sweep) (:142-165)."""
    from .neighbors import get_periodic_adjacency_information
    info = get_periodic_adjacency_information(cartesian_positions, basis_vectors, radial_cutoff=max_distance)
    source, destination = info.adjacency_matrix
    displacement = cartesian_positions[info.edge_batch_indices, destination] - \
        cartesian_positions[info.edge_batch_indices, source] + info.shifts
    distances = torch.linalg.norm(displacement, dim=-1)
    return distances[distances > 0.0]


# ----------------------------------------------------------------------------------------------------------------
# Stillinger-Weber energies (the reference's `oracle:` block)
# ----------------------------------------------------------------------------------------------------------------
@dataclass(kw_only=True)
class StillingerWeberParameters:
    """`oracle: {name: stillinger_weber, sw_coeff_filename: ...}` with the configuration's `elements` (the fields of the
    reference's LammpsOracleParameters, lammps_energy_oracle.py:22-27): the same potential, evaluated here."""
    name: str = "stillinger_weber"
    sw_coeff_filename: str          # a LAMMPS .sw file; the package ships none
    elements: List[str]             # unique elements; atom type = index in the sorted list (ElementTypes)

    def __post_init__(self):
        assert self.name == "stillinger_weber", f"StillingerWeberParameters describe `name: stillinger_weber`, got '{self.name}'"
        ElementTypes.validate_elements(self.elements)


SW_COLUMNS = ("epsilon", "sigma", "a", "lambda", "gamma", "costheta0", "A", "B", "p", "q")
_SW_PAIR_COLUMNS = (0, 1, 2, 4, 6, 7, 8, 9)           # what the (i, j, j) entry lends to the pair term and to a leg
_SW_TRIPLE_COLUMNS = (0, 3, 5)                        # epsilon, lambda, costheta0: what the (i, j, k) entry lends to phi3


def read_stillinger_weber_coefficients(path, elements: List[str]) -> torch.Tensor:
    """The float64 [n, n, n, 10] table (columns SW_COLUMNS) of a LAMMPS .sw file for `elements`, indexed by atom type = index in
    the sorted element list, entry (t_i, t_j, t_k) = the file's `element_i element_j element_k` line.  LAMMPS's format: `#`
    starts a comment, an entry is 3 symbols and 11 numbers and may span lines, entries of other elements are ignored.
    Refused, with a message: a missing or repeated triplet, tol != 0, and tables whose result would depend on the ORDER in which
    LAMMPS meets the neighbours -- pair parameters of (i, j, j) and (j, i, i) that differ (epsilon among them), or epsilon,
    lambda, costheta0 of (i, j, k) and (i, k, j) that differ."""
    symbols = ElementTypes(elements).elements
    n = len(symbols)
    assert 1 <= n <= 8, f"Stillinger-Weber tables of 1 to 8 elements are supported, got {n}"
    assert os.path.isfile(path), f"The SW file '{path}' does not exist."
    with open(path) as fd:
        words = [w for line in fd for w in line.split("#", 1)[0].split()]
    if len(words) % 14:
        raise ValueError(f"{path}: {len(words)} words are not a whole number of entries of 3 elements and 11 numbers")
    table = torch.full((n, n, n, 10), float("nan"), dtype=torch.float64)
    for k in range(0, len(words), 14):
        triplet = words[k:k + 3]
        try:
            numbers = [float(w) for w in words[k + 3:k + 14]]
        except ValueError:
            raise ValueError(f"{path}: the entry of {' '.join(triplet)} does not hold 11 numbers: {words[k + 3:k + 14]}") from None
        if not all(e in symbols for e in triplet):
            continue
        index = tuple(symbols.index(e) for e in triplet)
        if not torch.isnan(table[index][0]):
            raise ValueError(f"{path}: the entry of {' '.join(triplet)} appears twice")
        if numbers[10] != 0.0:
            raise ValueError(f"{path}: the entry of {' '.join(triplet)} has tol = {numbers[10]}: only tol = 0 is supported")
        table[index] = torch.tensor(numbers[:10], dtype=torch.float64)
    for i in range(n):
        for j in range(n):
            for k in range(n):
                if torch.isnan(table[i, j, k, 0]):
                    raise ValueError(f"{path}: no entry for the triplet {symbols[i]} {symbols[j]} {symbols[k]}")
    for i in range(n):
        for j in range(n):
            a, b = table[i, j, j], table[j, i, i]
            if a[0] != b[0]:
                raise ValueError(f"{path}: epsilon of {symbols[i]} {symbols[j]} {symbols[j]} ({a[0]}) and of {symbols[j]} "
                                 f"{symbols[i]} {symbols[i]} ({b[0]}) differ: the pair energy would depend on the order of the atoms")
            for c in _SW_PAIR_COLUMNS:
                if a[c] != b[c]:
                    raise ValueError(f"{path}: {SW_COLUMNS[c]} of {symbols[i]} {symbols[j]} {symbols[j]} and of {symbols[j]} "
                                     f"{symbols[i]} {symbols[i]} differ: the pair term would depend on the order of the atoms")
            for k in range(n):
                for c in _SW_TRIPLE_COLUMNS:
                    if table[i, j, k, c] != table[i, k, j, c]:
                        raise ValueError(f"{path}: {SW_COLUMNS[c]} of {symbols[i]} {symbols[j]} {symbols[k]} and of {symbols[i]} "
                                         f"{symbols[k]} {symbols[j]} differ: the three-body term would depend on the order of the "
                                         f"neighbours")
    return table


def compute_stillinger_weber_energies_and_forces(samples: Dict[AnyStr, torch.Tensor], parameters: StillingerWeberParameters,
                                                 device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(energies f64 [B] in eV, Cartesian forces f64 [B, N, 3] in eV/Angstrom), on the GPU, of samples in the reference's
    contract (energy_oracle.py:44-131): a dictionary with AXL_COMPOSITION or with the three separate keys; the lattice angles
    are ignored (orthogonal boxes); a structure with a negative side has its sides clipped to 1.0 with a warning, and one with a
    side below 3.0 Angstrom gets energy 0 and zero forces with a warning (lammps_energy_oracle.py:124-130).  Inputs on the CPU
    are moved to `device` (default: the current GPU); the inputs are not modified."""
    assert LATTICE_PARAMETERS in samples or AXL_COMPOSITION in samples, \
        f"the field '{LATTICE_PARAMETERS}' or '{AXL_COMPOSITION}' must be present in the sample dictionary"
    assert AXL_COMPOSITION in samples or ATOM_TYPES in samples, \
        f"the field '{AXL_COMPOSITION}' or '{ATOM_TYPES}' must be present in the sample dictionary"
    x = samples[RELATIVE_COORDINATES] if RELATIVE_COORDINATES in samples else samples[AXL_COMPOSITION].X
    lattice = samples[LATTICE_PARAMETERS] if LATTICE_PARAMETERS in samples else samples[AXL_COMPOSITION].L
    a = samples[ATOM_TYPES] if ATOM_TYPES in samples else samples[AXL_COMPOSITION].A
    x, lattice, a = torch.as_tensor(x), torch.as_tensor(lattice), torch.as_tensor(a)
    if device is None:
        device = x.device if x.is_cuda else torch.device("cuda")
    table = read_stillinger_weber_coefficients(parameters.sw_coeff_filename, parameters.elements).to(device)
    x = x.detach().to(device=device, dtype=torch.float32).contiguous()
    a = a.detach().to(device=device, dtype=torch.int64).contiguous()
    sides = lattice.detach().to(device=device, dtype=torch.float32)[:, :3].clone()
    B, N, _ = x.shape
    negative = sides.min(dim=1).values < 0
    if bool(negative.any()):
        warnings.warn("Got a negative lattice parameter. Clipping to 1.0 Angstrom")
        sides = torch.where(negative[:, None], sides.clip(min=1.0), sides)
    small = sides.min(dim=1).values < 3.0
    if bool(small.any()):
        warnings.warn("Got a box with a side length smaller than 3.0 Angstrom. Skipping this example.")
    keep = torch.nonzero(~small).flatten()
    energies = torch.zeros(B, dtype=torch.float64, device=device)
    forces = torch.zeros(B, N, 3, dtype=torch.float64, device=device)
    if keep.numel() == 0:
        return energies, forces
    whole = keep.numel() == B
    x_k, a_k, sides_k = (x, a, sides.contiguous()) if whole else (x[keep].contiguous(), a[keep].contiguous(), sides[keep].contiguous())
    capacity = kernels.SW_NEIGHBOUR_CAPACITY
    while True:
        try:
            e_k, f_k = kernels.stillinger_weber_energy_forces(x_k, sides_k, a_k, table, neighbour_capacity=capacity)
            break
        except kernels.StillingerWeberNeighbourCapacityError:
            if capacity >= 27 * N:
                raise
            capacity = min(2 * capacity, 27 * N)
    if whole:
        return e_k, f_k
    energies[keep] = e_k
    forces[keep] = f_k
    return energies, forces
