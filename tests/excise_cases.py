"""The excise-and-repaint cases shared by tests/golden/make_golden_excise_and_repaint.py (which runs with the REFERENCE on its
path) and the tests: the source frame, the settings, and a numpy restatement of the excision written for the tests.  Nothing
here imports the package or the reference."""
import itertools

import numpy as np

BOX, NEW_BOX = 10.86, 6.5
CENTRAL_ATOMS = [20, 54, 40]         # two neighbours of the vacancy and one bulk atom
RADIAL_CUTOFF, NUMBER_OF_NEIGHBORS = 3.0, 4
SAMPLE_EDIT_RADIUS = 2.0
N_ATOMS, SAMPLES_PER_ENVIRONMENT, BASE_SEED, NET_SEED = 8, 3, 2025, 1234
NOISE = dict(total_time_steps=10, schedule_type="linear", time_delta=1e-5, sigma_min=1e-4, sigma_max=0.2,
             corrector_step_epsilon=2.5e-8)
SAMPLING = dict(algorithm="predictor_corrector", number_of_atoms=N_ATOMS, num_atom_types=1, number_of_samples=SAMPLES_PER_ENVIRONMENT,
                spatial_dimension=3, number_of_corrector_steps=1, use_fixed_lattice_parameters=True, cell_dimensions=[NEW_BOX] * 3)
UNCERTAINTY_THRESHOLD, TOP_K = 0.65, 3

_DIAMOND = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                     [.75, .75, .25]])


def diamond_sites(cells: int) -> np.ndarray:
    """Relative coordinates of cells^3 diamond cells, cell by cell (8 atoms each)."""
    return np.array([(np.array(cell) + site) / cells for cell in itertools.product(range(cells), repeat=3) for site in _DIAMOND])


def source_frame():
    """Diamond Si 2x2x2 in a 10.86 Angstrom box, sites perturbed by N(0, 0.012) and wrapped, atom 17 deleted: (A int64 [63],
    X float64 [63,3], L float64 [6])."""
    x = np.mod(diamond_sites(2) + np.random.default_rng(7).normal(0, 0.012, (64, 3)), 1)
    x = np.delete(x, 17, axis=0)
    return np.zeros(len(x), dtype=np.int64), x, np.array([BOX, BOX, BOX, 0.0, 0.0, 0.0])


def uncertainties():
    """Every atom below 0.5 except the three central atoms, in descending order 20, 54, 40."""
    u = 0.1 + 0.4 * np.random.default_rng(11).random(63)
    u[CENTRAL_ATOMS] = [0.9, 0.8, 0.7]
    return u


# ------------------------------------------------------------------------------------------------------------------
# the tests' checker: the excision restated in numpy, binary64, with the package's tie rule
# ------------------------------------------------------------------------------------------------------------------
def distances(x, reference, sides):
    delta = x * sides - reference * sides
    squared = np.minimum(np.minimum(delta ** 2, (delta - sides) ** 2), (delta + sides) ** 2)
    return np.sqrt(squared.sum(axis=-1))


def excise(x, sides, central, radial_cutoff=None, number_of_neighbors=None, center=True, new_sides=None):
    """(source indices, X float64 of the environment, outside-the-new-box flag) of ONE central atom: members ordered by
    (distance, atom index) -- np.lexsort, so equal distances go to the lower index --, centred on slot 0, embedded."""
    x, sides = np.asarray(x, dtype=np.float64), np.asarray(sides, dtype=np.float64)
    distance = distances(x, x[central], sides)
    order = np.lexsort((np.arange(len(x)), distance))
    if radial_cutoff is not None:
        order = order[distance[order] < radial_cutoff]
    else:
        order = order[:number_of_neighbors + 1]
    out = x[order]
    if center:
        out = np.mod(out + (0.5 - out[0]), 1)
    outside = False
    if new_sides is not None:
        new_sides = np.asarray(new_sides, dtype=np.float64)
        positions = (out - 0.5) * sides + 0.5 * new_sides
        outside = bool(((positions >= new_sides) | (positions <= 0)).any())
        out = positions * (1.0 / new_sides)
    return order, out, outside
