"""The excise-and-random cases shared by tests/golden/make_golden_excise_and_random.py (which runs with the REFERENCE on its
path) and the tests: the settings of the recorded cases and a numpy restatement of the batched algorithm written for the tests
(what the GPU tests compare the kernels with).  Nothing here imports the package or the reference.  The frame, the central atoms
and the excisors are those of tests/excise_cases.py."""
import numpy as np

import excise_cases as ec

SAMPLES_PER_ENVIRONMENT, MAX_ATTEMPTS = 3, 4
DEFAULT_THRESHOLD = 0.5
THRESHOLD_CANDIDATES = [0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0]      # the generator takes the first that meets its conditions
ALGORITHMS = ["true_random", "voxel_random"]
EXCISORS = {"spherical": dict(algorithm="spherical_cutoff", radial_cutoff=ec.RADIAL_CUTOFF),
            "nearest_neighbors": dict(algorithm="nearest_neighbors", number_of_neighbors=ec.NUMBER_OF_NEIGHBORS)}
# N = 8 in the 6.5 Angstrom box of the excise-and-repaint cases: 2 x 2 x 2 voxels, one atom each.  N = 24: a cubic box gives
# 3 x 3 x 3 = 27 voxels whatever its side, so this shape takes an 8.0 x 8.0 x 6.4 box: 3 x 3 x 2 = 18 voxels, all of them once
# and 6 of them twice.
SHAPES = {"n8": dict(total_number_of_atoms=8, sample_box_size=[ec.NEW_BOX] * 3, partition=[2, 2, 2]),
          "n24": dict(total_number_of_atoms=24, sample_box_size=[8.0, 8.0, 6.4], partition=[3, 3, 2])}
PROPOSAL_SEED = 4711
MARGIN_THRESHOLD, MARGIN_ASSIGNMENT = 1e-6, 1e-9                    # Angstrom: what the generator asserts


def case_name(shape, algorithm, excisor):
    return f"{shape}_{algorithm}_{excisor}"


def case_names():
    return [case_name(s, a, x) for s in SHAPES for a in ALGORITHMS for x in EXCISORS]


def proposals(shape: str, algorithm: str, batch: int, spatial_dimension: int = 3):
    """The pre-drawn tables of a case: uniforms f64 [B,M,N,d], types int64 [B,M,N], voxels int64 [B,M,N] (None for
    true_random) by the reference's occupancy rule: all voxels once per full round, then a random subset."""
    settings = SHAPES[shape]
    N, M = settings["total_number_of_atoms"], MAX_ATTEMPTS
    rng = np.random.default_rng([PROPOSAL_SEED, N, ALGORITHMS.index(algorithm)])
    uniforms = rng.random((batch, M, N, spatial_dimension))
    types = rng.integers(0, 1, size=(batch, M, N))                   # one element (Si)
    voxels = None
    if algorithm == "voxel_random":
        V = int(np.prod(settings["partition"]))
        voxels = np.empty((batch, M, N), dtype=np.int64)
        for b in range(batch):
            for m in range(M):
                rounds, rest = divmod(N, V)
                voxels[b, m] = np.concatenate([np.tile(np.arange(V), rounds), rng.permutation(V)[:rest]])
    return uniforms, types, voxels


# ------------------------------------------------------------------------------------------------------------------
# the tests' checker: the batched algorithm restated in numpy, binary64
# ------------------------------------------------------------------------------------------------------------------
def sites(uniforms, voxels=None, partition=None):
    """The proposed sites [N,d]: the uniforms, or corner + u / p with numpy's linspace corner i (1 / p)."""
    if voxels is None:
        return np.array(uniforms, dtype=np.float64)
    partition = np.asarray(partition)
    index = np.stack(np.unravel_index(np.asarray(voxels), partition), axis=-1)
    return index * (1.0 / partition) + np.asarray(uniforms, dtype=np.float64) / partition


def squared_distances(x, reference, sides):
    delta = x * sides - reference * sides
    squared = np.minimum(np.minimum(delta ** 2, (delta - sides) ** 2), (delta + sides) ** 2)
    total = squared[..., 0]
    for axis in range(1, squared.shape[-1]):                         # the sum in dimension order
        total = total + squared[..., axis]
    return total


def place(proposed, constrained_x, sides):
    """The site each constrained atom takes: in order, the nearest free one by (distance, site index).  Also the least gap
    between the nearest and the second nearest free site met on the way (inf when there never were two)."""
    taken, gap = [], np.inf
    for x in constrained_x:
        distance = np.sqrt(squared_distances(proposed, x, sides))
        free = [n for n in np.lexsort((np.arange(len(proposed)), distance)) if n not in taken]
        if len(free) > 1:
            gap = min(gap, distance[free[1]] - distance[free[0]])
        taken.append(int(free[0]))
    return taken, gap


def shortest_distance(x, sides):
    """The least periodic distance over all pairs i != j: the least sum of squares, one square root."""
    n = len(x)
    if n < 2:
        return np.inf
    squared = squared_distances(x[:, None, :], x[None, :, :], sides)
    return float(np.sqrt(squared[~np.eye(n, dtype=bool)].min()))


def attempt(uniforms, types, voxels, partition, constrained_x, constrained_a, sides):
    """One attempt: (A, X, least distance, assignment gap)."""
    proposed = sites(uniforms, voxels, partition)
    taken, gap = place(proposed, constrained_x, sides)
    free = [n for n in range(len(proposed)) if n not in taken]
    x = np.vstack([np.asarray(constrained_x, dtype=np.float64).reshape(-1, proposed.shape[1]), proposed[free]])
    a = np.concatenate([np.asarray(constrained_a, dtype=np.int64), np.asarray(types, dtype=np.int64)[free]])
    return a, x, shortest_distance(x, sides), gap


def fill(uniforms, types, voxels, partition, constrained_x, constrained_a, sides, threshold):
    """One sample: attempts m = 0, 1, ... of uniforms [M,N,d], types [M,N], voxels [M,N] | None until the least distance
    exceeds the threshold; the last one otherwise.  dict(A, X, attempts (1-based), accepted, min_distance)."""
    sides = np.asarray(sides, dtype=np.float64)
    for m in range(len(uniforms)):
        a, x, least, _ = attempt(uniforms[m], types[m], None if voxels is None else voxels[m], partition, constrained_x,
                                 constrained_a, sides)
        if least > threshold:
            return dict(A=a, X=x, attempts=m + 1, accepted=True, min_distance=least)
    return dict(A=a, X=x, attempts=len(uniforms), accepted=False, min_distance=least)
