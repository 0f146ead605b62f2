"""Generate tests/golden/excise_and_repaint/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_excise_and_repaint.py

The reference's atom selectors, excisors and ExciseAndRepaintSampleMaker (src/.../active_learning_loop/) on the frame and
settings of tests/excise_cases.py: diamond Si 2x2x2 with a vacancy, the environments of atoms 20, 54 and 40 moved into a 6.5
Angstrom box and repainted to 8 atoms by the MLP of tests/nets.py::mlp_net, T = 10, 3 samples per environment, CPU.

  frame.npz               A, X, L of the frame, the uncertainty vector, what the threshold and the top-k selector return
  spherical.npz           the spherical excisor (3.0 Angstrom): count [E]; source [E,K] (-1 padded; recovered from the excised
  nearest_neighbors.npz   coordinates), A [E,K], X_raw / X_centred / X_embedded f64 [E,K,3] (0 padded) and X_constraint f32, the
                          embedded coordinates after the torch.FloatTensor(...) of create_sampling_constraints; the 4-neighbour one
  samples.npz             net/* the MLP's state_dict; for `seq` (the unpatched maker after ONE torch.manual_seed(BASE_SEED)) and
                          `per_env` (a subclass that calls torch.manual_seed(BASE_SEED + e) before environment e):
                          <run>_A [E*S,N], <run>_X [E*S,N,3], <run>_L [E*S,6]   the samples without the edit
                          <run>_keep [E*S,N] bool, <run>_edited_count [E*S]     the edit at SAMPLE_EDIT_RADIUS
                          <run>_edited_A / _edited_X                            the edited samples, 0 padded
                          <run>_active [E*S], <run>_constrained [E*S]           the active index and the info's constrained count
The script asserts the margins that make the fixtures insensitive to rounding: the sorted distances of an environment's members
and of the first atom left out >= 1e-3 Angstrom apart, no
distance within 1e-2 of the cutoff, no generated atom within 1e-3 of the edit radius."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

import excise_cases as ec  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.atom_selector.atom_selector_factory import (  # noqa: E402
    create_atom_selector, create_atom_selector_parameters)
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.excisor.excisor_factory import (  # noqa: E402
    create_excisor, create_excisor_parameters)
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.sample_maker.excise_and_repaint_sample_maker import (  # noqa: E402
    ExciseAndRepaintSampleMaker, ExciseAndRepaintSampleMakerArguments)
from diffusion_for_multi_scale_molecular_dynamics.active_learning_loop.utils import \
    get_distances_from_reference_point  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.namespace import AXL  # noqa: E402

DIRECTORY = "excise_and_repaint"
EXCISORS = {"spherical": dict(algorithm="spherical_cutoff", radial_cutoff=ec.RADIAL_CUTOFF),
            "nearest_neighbors": dict(algorithm="nearest_neighbors", number_of_neighbors=ec.NUMBER_OF_NEIGHBORS)}


def save(name, **arrays):
    mg.save(os.path.join(DIRECTORY, name), **arrays)


def frame():
    a, x, lattice = ec.source_frame()
    return AXL(A=a, X=x, L=lattice)


def selectors():
    u = ec.uncertainties()
    threshold = create_atom_selector(create_atom_selector_parameters(
        dict(algorithm="threshold", uncertainty_threshold=ec.UNCERTAINTY_THRESHOLD))).select_central_atoms(u)
    top_k = create_atom_selector(create_atom_selector_parameters(
        dict(algorithm="top_k", top_k_environment=ec.TOP_K))).select_central_atoms(u)
    assert list(threshold) == ec.CENTRAL_ATOMS and list(top_k) == ec.CENTRAL_ATOMS
    return u, threshold, top_k


def golden_frame():
    structure = frame()
    u, threshold, top_k = selectors()
    save("frame.npz", A=structure.A, X=structure.X, L=structure.L, uncertainty=u, threshold_selection=np.asarray(threshold),
         top_k_selection=np.asarray(top_k))


def golden_excisor(name):
    structure = frame()
    excisor = create_excisor(create_excisor_parameters(EXCISORS[name]))
    central = np.array(ec.CENTRAL_ATOMS)
    raw, _ = excisor.excise_environments(structure, central, center_atoms=False)
    centred, indices = excisor.excise_environments(structure, central, center_atoms=True)
    assert list(indices) == [0] * len(central)
    new_lattice = np.array([ec.NEW_BOX] * 3 + [0.0] * 3)
    embedded = [ExciseAndRepaintSampleMaker.embed_structure_in_new_box(e, new_lattice) for e in centred]
    E, K = len(central), max(len(e.X) for e in raw)
    count = np.array([len(e.X) for e in raw], dtype=np.int64)
    source = np.full((E, K), -1, dtype=np.int64)
    A = np.zeros((E, K), dtype=np.int64)
    X = {key: np.zeros((E, K, 3)) for key in ("raw", "centred", "embedded")}
    constraint = np.zeros((E, K, 3), dtype=np.float32)
    for e, c in enumerate(central):
        k = count[e]
        distance = get_distances_from_reference_point(structure.X, structure.X[c], structure.L)
        ordered = np.sort(distance)[:k + 1]                      # the members and the first atom left out
        assert np.diff(ordered).min() >= 1e-3, "two atoms at nearly the same distance: the order could flip on rounding"
        if name == "spherical":
            assert np.abs(distance - ec.RADIAL_CUTOFF).min() >= 1e-2, "an atom nearly on the cutoff"
        source[e, :k] = [int(np.flatnonzero((structure.X == row).all(axis=1))[0]) for row in raw[e].X]
        A[e, :k] = raw[e].A
        X["raw"][e, :k], X["centred"][e, :k], X["embedded"][e, :k] = raw[e].X, centred[e].X, embedded[e].X
        constraint[e, :k] = torch.FloatTensor(embedded[e].X).numpy()
    save(name + ".npz", count=count, source=source, A=A, X_raw=X["raw"], X_centred=X["centred"], X_embedded=X["embedded"],
         X_constraint=constraint)


def _maker(cls, net, radius):
    arguments = ExciseAndRepaintSampleMakerArguments(element_list=["Si"], sample_box_size=[ec.NEW_BOX] * 3,
                                                     number_of_samples_per_substructure=ec.SAMPLES_PER_ENVIRONMENT,
                                                     sample_edit_radius=radius)
    selector = create_atom_selector(create_atom_selector_parameters(
        dict(algorithm="threshold", uncertainty_threshold=ec.UNCERTAINTY_THRESHOLD)))
    excisor = create_excisor(create_excisor_parameters(EXCISORS["spherical"]))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sampling = mg.PredictorCorrectorSamplingParameters(**ec.SAMPLING)
    return cls(arguments, selector, excisor, mg.NoiseParameters(**ec.NOISE), sampling, net, device="cpu")


class SeededPerEnvironment(ExciseAndRepaintSampleMaker):
    """The reference's maker, reseeded with BASE_SEED + e before environment e."""

    environment = 0

    def make_samples_from_constrained_substructure(self, substructure, active_atom_index, num_samples=1):
        torch.manual_seed(ec.BASE_SEED + self.environment)
        self.environment += 1
        return super().make_samples_from_constrained_substructure(substructure, active_atom_index, num_samples)


def golden_samples():
    net = mg._mlp(ec.N_ATOMS, 1, seed=ec.NET_SEED)
    structure, u = frame(), ec.uncertainties()
    out = mg._state_dict_np(net)
    removed = 0
    for run, cls in (("seq", ExciseAndRepaintSampleMaker), ("per_env", SeededPerEnvironment)):
        torch.manual_seed(ec.BASE_SEED)
        plain, active, infos = _maker(cls, net, None).make_samples(structure, u)
        torch.manual_seed(ec.BASE_SEED)
        edited, active_again, _ = _maker(cls, net, ec.SAMPLE_EDIT_RADIUS).make_samples(structure, u)
        B, N = len(plain), ec.N_ATOMS
        assert B == len(ec.CENTRAL_ATOMS) * ec.SAMPLES_PER_ENVIRONMENT and all((a == b).all() for a, b in zip(active, active_again))
        constrained = np.array([len(info["constrained_atom_indices"]) for info in infos], dtype=np.int64)
        keep = np.zeros((B, N), dtype=bool)
        edited_A, edited_X = np.zeros((B, N), dtype=plain[0].A.dtype), np.zeros((B, N, 3), dtype=plain[0].X.dtype)
        for b, (sample, after) in enumerate(zip(plain, edited)):
            distance = get_distances_from_reference_point(sample.X, sample.X[int(active[b][0])], sample.L)
            generated = distance[constrained[b]:]
            assert np.abs(generated - ec.SAMPLE_EDIT_RADIUS).min() >= 1e-3, "a generated atom nearly on the edit radius"
            keep[b] = (np.arange(N) < constrained[b]) | (distance > ec.SAMPLE_EDIT_RADIUS)
            assert np.array_equal(after.X, sample.X[keep[b]]) and np.array_equal(after.A, sample.A[keep[b]])
            edited_A[b, :len(after.A)], edited_X[b, :len(after.X)] = after.A, after.X
        removed += int((~keep).sum())
        out.update({f"{run}_A": np.stack([s.A for s in plain]), f"{run}_X": np.stack([s.X for s in plain]),
                    f"{run}_L": np.stack([s.L for s in plain]), f"{run}_keep": keep,
                    f"{run}_edited_count": keep.sum(axis=1).astype(np.int64), f"{run}_edited_A": edited_A,
                    f"{run}_edited_X": edited_X, f"{run}_active": np.array([int(a[0]) for a in active], dtype=np.int64),
                    f"{run}_constrained": constrained})
    assert removed > 0, "the edit radius removes nothing: the edit would go unchecked"
    save("samples.npz", numpy_version=np.array(np.__version__), **out)


if __name__ == "__main__":
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    golden_frame()
    for excisor_name in EXCISORS:
        golden_excisor(excisor_name)
    golden_samples()
