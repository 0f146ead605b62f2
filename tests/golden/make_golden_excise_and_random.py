"""Generate tests/golden/excise_and_random/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_excise_and_random.py

The reference's ExciseAndRandomSampleMaker (src/.../active_learning_loop/sample_maker/excise_and_random_sample_maker.py) on the
frame of tests/excise_cases.py with the settings of tests/excise_random_cases.py: the environments of atoms 20, 54 and 40, 3
samples each, at most 4 attempts; both algorithms, both excisors, N = 8 and N = 24 -- one file per case.  The maker's three draws
(generate_random_relative_coordinates, generate_atom_types, select_occupied_voxels) are patched to serve attempt m of sample b from
tables drawn beforehand with a seeded np.random.default_rng, so what is recorded is a function of the recorded proposals alone.

  <case>.npz   uniforms f64 [B,M,N,3], types int64 [B,M,N], voxels int64 [B,M,N] (voxel_random), partition, box [6];
               constrained_x f64 [E,K,3] / constrained_a int64 [E,K] / counts [E] / central [E]: the embedded environments;
               distances f64 [B,M]: the reference's shortest distance of EVERY attempt;
               thresholds [2]: 0.5 Angstrom and the larger one; for t = 0, 1:
               t<t>_A [B,N], t<t>_X [B,N,3], t<t>_L [B,6], t<t>_active [B], t<t>_attempts [B] (1-based), t<t>_accepted [B],
               t<t>_constrained [B] (the info dictionaries' constrained counts)
The larger threshold of a shape is the first of THRESHOLD_CANDIDATES at which, over the shape's recorded samples, one is accepted
at attempt 1, one at a later attempt and one exhausts its attempts.  The script asserts the margins that make the fixtures
insensitive to rounding: no attempt's shortest distance within 1e-6 Angstrom of a threshold, and at every placement step the
nearest and the second nearest free site at least 1e-9 Angstrom apart."""
import os
import sys
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

import excise_cases as ec  # noqa: E402
import excise_random_cases as rc  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.atom_selector.atom_selector_factory import (  # noqa: E402
    create_atom_selector, create_atom_selector_parameters)
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.excisor.excisor_factory import (  # noqa: E402
    create_excisor, create_excisor_parameters)
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.sample_maker import \
    excise_and_random_sample_maker as reference_module  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.utils import \
    get_distances_from_reference_point  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.namespace import AXL  # noqa: E402

DIRECTORY = "excise_and_random"
ReferenceMaker = reference_module.ExciseAndRandomSampleMaker


class Served(ReferenceMaker):
    """The reference's maker; it only keeps count of the sample and the attempt the patched draws serve."""

    sample, attempt = -1, 0

    def make_single_sample_from_constrained_substructure(self, constrained_structure, active_atom_index):
        self.sample, self.attempt = self.sample + 1, 0
        out = super().make_single_sample_from_constrained_substructure(constrained_structure, active_atom_index)
        self.attempts_returned.append(self.attempt)
        return out

    def make_single_structure(self, constrained_structure, active_atom_index):
        out = super().make_single_structure(constrained_structure, active_atom_index)
        self.attempt += 1
        return out


def run(shape, algorithm, excisor_name, threshold, tables, pinned=None):
    """The reference's make_samples with the draws served from `tables`.  `pinned` = (environment, sample, attempt): one
    make_single_structure of that attempt instead, for the margins."""
    settings = rc.SHAPES[shape]
    uniforms, types, voxels = tables
    arguments = reference_module.ExciseAndRandomSampleMakerArguments(
        element_list=["Si"], sample_box_size=settings["sample_box_size"], total_number_of_atoms=settings["total_number_of_atoms"],
        number_of_samples_per_substructure=rc.SAMPLES_PER_ENVIRONMENT, random_coordinates_algorithm=algorithm,
        max_attempts=rc.MAX_ATTEMPTS, minimal_interatomic_distance=threshold)
    selector = create_atom_selector(create_atom_selector_parameters(
        dict(algorithm="threshold", uncertainty_threshold=ec.UNCERTAINTY_THRESHOLD)))
    maker = Served(arguments, selector, create_excisor(create_excisor_parameters(rc.EXCISORS[excisor_name])))
    maker.attempts_returned = []
    at = lambda: (maker.sample, maker.attempt)          # noqa: E731
    with mock.patch.object(ReferenceMaker, "generate_random_relative_coordinates",
                           staticmethod(lambda n_atoms, spatial_dimension=3: uniforms[at()].copy())), \
            mock.patch.object(ReferenceMaker, "generate_atom_types", staticmethod(lambda n_atoms, num_atom_types: types[at()].copy())), \
            mock.patch.object(reference_module, "select_occupied_voxels", lambda num_voxels, num_atoms: voxels[at()].copy()):
        if pinned is not None:
            embedded, central, maker.sample, maker.attempt = pinned
            return maker.make_single_structure(embedded, central)[0]
        a, x, lattice = ec.source_frame()
        samples, active, infos = maker.make_samples(AXL(A=a, X=x, L=lattice), ec.uncertainties())
    return maker, samples, active, infos


def margins(shape, algorithm, excisor_name, tables, embedded_environments):
    """(the reference's shortest distance of every attempt [B,M], the least placement gap over all attempts)."""
    S, M = rc.SAMPLES_PER_ENVIRONMENT, rc.MAX_ATTEMPTS
    B = len(embedded_environments) * S
    distances, gap = np.zeros((B, M)), np.inf
    for b in range(B):
        embedded = embedded_environments[b // S]
        for m in range(M):
            structure = run(shape, algorithm, excisor_name, rc.DEFAULT_THRESHOLD, tables, pinned=(embedded, 0, b, m))
            distances[b, m] = ReferenceMaker.get_shortest_distance_between_atoms(structure.X, structure.L)
            proposed = rc.sites(tables[0][b, m], None if tables[2] is None else tables[2][b, m], rc.SHAPES[shape]["partition"])
            taken = []
            for x in embedded.X:
                distance = get_distances_from_reference_point(proposed, x, embedded.L)
                free = [n for n in np.argsort(distance) if n not in taken]
                gap = min(gap, distance[free[1]] - distance[free[0]])
                taken.append(free[0])
            assert np.array_equal(structure.X[len(taken):], np.delete(proposed, taken, axis=0))
    return distances, gap


def golden_shape(shape):
    settings = rc.SHAPES[shape]
    N, S, M = settings["total_number_of_atoms"], rc.SAMPLES_PER_ENVIRONMENT, rc.MAX_ATTEMPTS
    B = len(ec.CENTRAL_ATOMS) * S
    cases = [(algorithm, excisor) for algorithm in rc.ALGORITHMS for excisor in rc.EXCISORS]
    tables = {algorithm: rc.proposals(shape, algorithm, B) for algorithm in rc.ALGORITHMS}
    recorded = {}
    for algorithm, excisor in cases:                       # the default threshold; the environments; the margins
        maker, samples, active, infos = run(shape, algorithm, excisor, rc.DEFAULT_THRESHOLD, tables[algorithm])
        embedded = [infos[e * S]["axl_structure_in_new_box"] for e in range(len(ec.CENTRAL_ATOMS))]
        distances, gap = margins(shape, algorithm, excisor, tables[algorithm], embedded)
        assert gap >= rc.MARGIN_ASSIGNMENT, f"{shape} {algorithm} {excisor}: two free sites {gap:.3e} Angstrom apart in distance"
        if algorithm == "voxel_random":
            partition = reference_module.partition_relative_coordinates_for_voxels(np.array(settings["sample_box_size"]), N)[1]
            assert list(partition) == settings["partition"], partition
        recorded[algorithm, excisor] = dict(embedded=embedded, distances=distances, runs=[(maker, samples, active, infos)])
    larger = None
    for candidate in rc.THRESHOLD_CANDIDATES:
        runs = {case: run(shape, case[0], case[1], candidate, tables[case[0]]) for case in cases}
        attempts = np.concatenate([r[0].attempts_returned for r in runs.values()])
        accepted = np.concatenate([[ReferenceMaker.get_shortest_distance_between_atoms(s.X, s.L) > candidate for s in r[1]]
                                   for r in runs.values()])
        apart = min(np.abs(recorded[case]["distances"] - candidate).min() for case in cases)
        if (accepted & (attempts == 1)).any() and (accepted & (attempts > 1)).any() and (~accepted).any() \
                and apart >= rc.MARGIN_THRESHOLD:
            larger = candidate
            break
    assert larger is not None, f"{shape}: no candidate threshold shows acceptance at once, acceptance on retry and exhaustion"
    for case in cases:
        recorded[case]["runs"].append(runs[case])
    for algorithm, excisor in cases:
        record = recorded[algorithm, excisor]
        assert np.abs(record["distances"] - rc.DEFAULT_THRESHOLD).min() >= rc.MARGIN_THRESHOLD
        uniforms, types, voxels = tables[algorithm]
        embedded = record["embedded"]
        E, K = len(embedded), max(len(e.X) for e in embedded)
        cx, ca = np.zeros((E, K, 3)), np.zeros((E, K), dtype=np.int64)
        for e, environment in enumerate(embedded):
            cx[e, :len(environment.X)], ca[e, :len(environment.X)] = environment.X, environment.A
        out = dict(uniforms=uniforms, types=types, partition=np.array(settings["partition"], dtype=np.int64),
                   box=np.asarray(embedded[0].L, dtype=np.float64), constrained_x=cx, constrained_a=ca,
                   counts=np.array([len(e.X) for e in embedded], dtype=np.int64), central=np.zeros(E, dtype=np.int64),
                   distances=record["distances"], thresholds=np.array([rc.DEFAULT_THRESHOLD, larger]))
        if voxels is not None:
            out["voxels"] = voxels
        for t, (maker, samples, active, infos) in enumerate(record["runs"]):
            threshold = out["thresholds"][t]
            attempts = np.array(maker.attempts_returned, dtype=np.int64)
            accepted = np.array([ReferenceMaker.get_shortest_distance_between_atoms(s.X, s.L) > threshold for s in samples])
            # the attempt returned is the first above the threshold, or the last
            for b in range(B):
                above = np.flatnonzero(record["distances"][b] > threshold)
                assert attempts[b] == (above[0] + 1 if len(above) else M) and accepted[b] == bool(len(above))
            out.update({f"t{t}_A": np.stack([s.A for s in samples]), f"t{t}_X": np.stack([s.X for s in samples]),
                        f"t{t}_L": np.stack([np.asarray(s.L, dtype=np.float64) for s in samples]),
                        f"t{t}_active": np.array([int(i[0]) for i in active], dtype=np.int64), f"t{t}_attempts": attempts,
                        f"t{t}_accepted": accepted,
                        f"t{t}_constrained": np.array([len(i["constrained_atom_indices"]) for i in infos], dtype=np.int64)})
        mg.save(os.path.join(DIRECTORY, rc.case_name(shape, algorithm, excisor) + ".npz"), numpy_version=np.array(np.__version__),
                **out)
    print(f"{shape}: larger threshold {larger}")


if __name__ == "__main__":
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    for shape_name in rc.SHAPES:
        golden_shape(shape_name)
