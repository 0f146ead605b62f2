"""CPU tests of the random and no-op sample makers and their factory: what the dataclasses and the factory refuse, the no-op
makers' results, and the host flow of ExciseAndRandomSampleMaker (make_single_structure, get_shortest_distance_between_atoms)
and the tests' numpy restatement of the batched algorithm (tests/excise_random_cases.py) against the reference's recorded
samples (tests/golden/excise_and_random/, made by tests/golden/make_golden_excise_and_random.py) -- exactly: a sample's
coordinates are copies of the inputs or one correctly rounded divide, multiply and add.  Everything that reaches a kernel is in
tests/test_excise_and_random_gpu.py.

The reference's own test files of these makers are not run here: tests/active_learning_loop/sample_maker/base_test_sample_maker.py,
which all three build on, imports pymatgen and the reference's structure_converter at module level; neither exists on the
machines this suite runs on, so none of the three files can be collected."""
import dataclasses
import logging
from unittest import mock

import numpy as np
import pytest

import excise_cases as ec
import excise_random_cases as rc
from conftest import load_golden

PKG = "diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop."


def _modules():
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker import (
        excise_and_noop_sample_maker, excise_and_random_sample_maker, excise_and_repaint_sample_maker, no_op_sample_maker,
        sample_maker_factory)
    return (sample_maker_factory, no_op_sample_maker, excise_and_noop_sample_maker, excise_and_random_sample_maker,
            excise_and_repaint_sample_maker)


def _axl():
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL
    return AXL


def _parameters():
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.atom_selector.atom_selector_factory import \
        create_atom_selector_parameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.excisor.excisor_factory import \
        create_excisor_parameters
    return (create_atom_selector_parameters(dict(algorithm="top_k", top_k_environment=ec.TOP_K)),
            create_excisor_parameters(rc.EXCISORS["spherical"]), create_excisor_parameters(dict(algorithm="noop")))


def test_factory_builds_the_four_makers():
    import nets
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
        PredictorCorrectorSamplingParameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    factory, noop, excise_noop, excise_random, excise_repaint = _modules()
    selector, excisor, noop_excisor = _parameters()
    assert list(factory.SAMPLE_MAKER_PARAMETERS_BY_NAME) == ["noop", "excise_and_noop", "excise_and_repaint", "excise_and_random"]
    box = dict(element_list=["Si"], sample_box_size=[ec.NEW_BOX] * 3)
    parameters = factory.create_sample_maker_parameters(dict(algorithm="noop", element_list=["Si"]))
    assert type(parameters) is noop.NoOpSampleMakerArguments and parameters.sample_box_strategy == "noop"
    for given in (None, noop_excisor):
        assert type(factory.create_sample_maker(parameters, selector, given)) is noop.NoOpSampleMaker
    parameters = factory.create_sample_maker_parameters(dict(algorithm="excise_and_noop", number_of_samples_per_substructure=2, **box))
    maker = factory.create_sample_maker(parameters, selector, excisor)
    assert type(maker) is excise_noop.ExciseAndNoOpSampleMaker and maker.environment_excisor.arguments.radial_cutoff == ec.RADIAL_CUTOFF
    parameters = factory.create_sample_maker_parameters(dict(algorithm="excise_and_random", total_number_of_atoms=8,
                                                             random_coordinates_algorithm="voxel_random", **box))
    maker = factory.create_sample_maker(parameters, selector, excisor)
    assert type(maker) is excise_random.ExciseAndRandomSampleMaker and maker.num_atom_types == 1
    assert (parameters.max_attempts, parameters.minimal_interatomic_distance) == (10, 0.5)
    assert maker.batch_environments is True and maker.rng_mode == "reference"
    assert not {"batch_environments", "rng_mode"} & {f.name for f in dataclasses.fields(parameters)}
    parameters = factory.create_sample_maker_parameters(dict(algorithm="excise_and_repaint", number_of_samples_per_substructure=3, **box))
    maker = factory.create_sample_maker(parameters, selector, excisor, NoiseParameters(**ec.NOISE),
                                        PredictorCorrectorSamplingParameters(**ec.SAMPLING), nets.mlp_net(8, 1))
    assert type(maker) is excise_repaint.ExciseAndRepaintSampleMaker
    assert hasattr(type(maker).__mro__[1], "_excise_tables") and "_excise_tables" not in vars(type(maker))      # shared, in the base


def test_factory_consistency_assertions():
    factory, *_ = _modules()
    selector, excisor, noop_excisor = _parameters()
    with pytest.raises(AssertionError, match="Sample maker method excise is not implemented"):
        factory.create_sample_maker_parameters(dict(algorithm="excise", element_list=["Si"]))
    parameters = factory.create_sample_maker_parameters(dict(algorithm="noop", element_list=["Si"]))
    with pytest.raises(AssertionError, match="nonsensical to specify an excisor different from 'noop'"):
        factory.create_sample_maker(parameters, selector, excisor)
    for algorithm, more in (("excise_and_noop", {}), ("excise_and_random", dict(total_number_of_atoms=8)), ("excise_and_repaint", {})):
        parameters = factory.create_sample_maker_parameters(dict(algorithm=algorithm, element_list=["Si"],
                                                                 sample_box_size=[ec.NEW_BOX] * 3, **more))
        for given in (None, noop_excisor):
            with pytest.raises(AssertionError, match="nonsensical to specify a NoOp excisor"):
                factory.create_sample_maker(parameters, selector, given)
    parameters.algorithm = "excise"
    with pytest.raises(AssertionError, match="is not implemented"):
        factory.create_sample_maker(parameters, selector, excisor)


def test_arguments_refuse_what_the_reference_refuses():
    _, noop, excise_noop, excise_random, _ = _modules()
    box = dict(element_list=["Si"], sample_box_size=[ec.NEW_BOX] * 3)
    with pytest.raises(TypeError):
        excise_random.ExciseAndRandomSampleMakerArguments(**box)                          # total_number_of_atoms has no default
    with pytest.raises(AssertionError, match="Random coordinates algorithm should be true_random or voxel_random.Got grid"):
        excise_random.ExciseAndRandomSampleMakerArguments(total_number_of_atoms=8, random_coordinates_algorithm="grid", **box)
    with pytest.raises(AssertionError, match="max_constrained_substructure should be greater than 0"):
        excise_random.ExciseAndRandomSampleMakerArguments(total_number_of_atoms=8, max_constrained_substructure=0, **box)
    with pytest.raises(AssertionError):
        excise_noop.ExciseAndNoOpSampleMakerArguments(element_list=["Si"])                # a fixed box needs its size
    with pytest.raises(AssertionError, match="Sample box making strategy grow is not implemented"):
        noop.NoOpSampleMakerArguments(element_list=["Si"], sample_box_strategy="grow")
    arguments = excise_random.ExciseAndRandomSampleMakerArguments(total_number_of_atoms=8, **box)
    assert arguments.algorithm == "excise_and_random" and arguments.random_coordinates_algorithm == "true_random"
    assert excise_noop.ExciseAndNoOpSampleMakerArguments(**box).algorithm == "excise_and_noop"


def test_no_op_makers():
    factory, noop, excise_noop, _, _ = _modules()
    selector, excisor, _ = _parameters()
    a, x, lattice = ec.source_frame()
    structure, u = _axl()(A=a, X=x, L=lattice), ec.uncertainties()
    maker = factory.create_sample_maker(noop.NoOpSampleMakerArguments(element_list=["Si"]), selector)
    samples, active, infos = maker.make_samples(structure, u)
    assert len(samples) == len(active) == len(infos) == 1 and samples[0] is structure
    assert list(active[0]) == ec.CENTRAL_ATOMS and infos[0] == dict(constrained_atom_indices=list(range(63)))
    assert maker.filter_made_samples(samples) is samples
    maker = excise_noop.ExciseAndNoOpSampleMaker(
        excise_noop.ExciseAndNoOpSampleMakerArguments(element_list=["Si"], sample_box_size=[ec.NEW_BOX] * 3), None, None)
    substructure = _axl()(A=a[:4], X=x[:4], L=lattice)
    samples, active, infos = maker.make_samples_from_constrained_substructure(substructure, 2, num_samples=3)
    assert all(s is substructure for s in samples) and active == [2, 2, 2] and len(infos) == 3
    assert infos[0] == dict(constrained_atom_indices=[0, 1, 2, 3]) and infos[0] is not infos[1]


def _cases():
    return [(shape, algorithm, excisor) for shape in rc.SHAPES for algorithm in rc.ALGORITHMS for excisor in rc.EXCISORS]


def _maker(shape, algorithm, threshold, **more):
    excise_random = _modules()[3]
    settings = rc.SHAPES[shape]
    arguments = excise_random.ExciseAndRandomSampleMakerArguments(
        element_list=["Si"], sample_box_size=settings["sample_box_size"], total_number_of_atoms=settings["total_number_of_atoms"],
        number_of_samples_per_substructure=rc.SAMPLES_PER_ENVIRONMENT, random_coordinates_algorithm=algorithm,
        max_attempts=rc.MAX_ATTEMPTS, minimal_interatomic_distance=float(threshold), **more)
    return excise_random, excise_random.ExciseAndRandomSampleMaker(arguments, None, None)


@pytest.mark.parametrize("shape,algorithm,excisor", _cases())
def test_host_flow_reproduces_the_recorded_samples(shape, algorithm, excisor, caplog):
    """make_samples_from_constrained_substructure on the recorded embedded environments, its three draws patched -- as the
    golden generator patches the reference's -- to serve attempt m of sample b from the recorded proposals."""
    g = load_golden(f"excise_and_random/{rc.case_name(shape, algorithm, excisor)}.npz")
    uniforms, types, voxels = g["uniforms"], g["types"], g["voxels"] if "voxels" in g else None
    S, AXL = rc.SAMPLES_PER_ENVIRONMENT, _axl()
    assert np.array_equal(uniforms, rc.proposals(shape, algorithm, len(uniforms))[0])
    for t, threshold in enumerate(g["thresholds"]):
        module, maker = _maker(shape, algorithm, threshold)
        cursor = dict(sample=-1, attempt=0)
        at = lambda: (cursor["sample"], cursor["attempt"])          # noqa: E731
        single_structure, single_sample = maker.make_single_structure, maker.make_single_sample_from_constrained_substructure
        attempts = []

        def counted_structure(*args):
            out = single_structure(*args)
            cursor["attempt"] += 1
            return out

        def counted_sample(*args):
            cursor.update(sample=cursor["sample"] + 1, attempt=0)
            out = single_sample(*args)
            attempts.append(cursor["attempt"])
            return out

        maker.make_single_structure, maker.make_single_sample_from_constrained_substructure = counted_structure, counted_sample
        cls = module.ExciseAndRandomSampleMaker
        with mock.patch.object(cls, "generate_random_relative_coordinates", staticmethod(lambda n, d=3: uniforms[at()].copy())), \
                mock.patch.object(cls, "generate_atom_types", staticmethod(lambda n, c: types[at()].copy())), \
                mock.patch.object(module, "select_occupied_voxels", lambda v, n: voxels[at()].copy()), \
                caplog.at_level(logging.WARNING):
            caplog.clear()
            for e, count in enumerate(g["counts"]):
                environment = AXL(A=g["constrained_a"][e, :count], X=g["constrained_x"][e, :count], L=g["box"])
                samples, active, infos = maker.make_samples_from_constrained_substructure(environment, int(g["central"][e]), S)
                for s, (sample, index, info) in enumerate(zip(samples, active, infos)):
                    b = e * S + s
                    assert np.array_equal(sample.X, g[f"t{t}_X"][b]) and sample.X.dtype == np.float64, (t, b)
                    assert np.array_equal(sample.A, g[f"t{t}_A"][b]) and np.array_equal(sample.L, g[f"t{t}_L"][b])
                    assert index == g[f"t{t}_active"][b] and len(info["constrained_atom_indices"]) == g[f"t{t}_constrained"][b]
                    least = maker.get_shortest_distance_between_atoms(sample.X, sample.L)
                    assert (least > threshold) == bool(g[f"t{t}_accepted"][b])
                    assert least == g["distances"][b, attempts[b] - 1]
        assert np.array_equal(attempts, g[f"t{t}_attempts"])
        warnings = [r for r in caplog.records if "could not be generated in 4 attempts" in r.getMessage()]
        assert len(warnings) == int((~g[f"t{t}_accepted"]).sum())                    # one warning per exhausted sample, as the reference


@pytest.mark.parametrize("shape,algorithm,excisor", _cases())
def test_restatement_reproduces_the_recorded_samples(shape, algorithm, excisor):
    g = load_golden(f"excise_and_random/{rc.case_name(shape, algorithm, excisor)}.npz")
    voxels = g["voxels"] if "voxels" in g else None
    partition = list(g["partition"]) if voxels is not None else None
    S, sides = rc.SAMPLES_PER_ENVIRONMENT, g["box"][:3]
    assert list(g["partition"]) == rc.SHAPES[shape]["partition"]
    for t, threshold in enumerate(g["thresholds"]):
        for b in range(len(g["uniforms"])):
            e = b // S
            count = g["counts"][e]
            got = rc.fill(g["uniforms"][b], g["types"][b], None if voxels is None else voxels[b], partition,
                          g["constrained_x"][e, :count], g["constrained_a"][e, :count], sides, threshold)
            assert np.array_equal(got["X"], g[f"t{t}_X"][b]) and np.array_equal(got["A"], g[f"t{t}_A"][b]), (t, b)
            assert got["attempts"] == g[f"t{t}_attempts"][b] and got["accepted"] == bool(g[f"t{t}_accepted"][b])
            assert abs(got["min_distance"] - g["distances"][b, got["attempts"] - 1]) <= 1e-12


def test_the_fixtures_hold_every_branch():
    """What the generator asserted when it made them: at the larger threshold of each shape a sample is accepted at once, one on
    a retry and one never; no distance within 1e-6 Angstrom of a threshold; the N = 24 partition has fewer voxels than atoms."""
    for shape in rc.SHAPES:
        attempts, accepted = [], []
        for algorithm in rc.ALGORITHMS:
            for excisor in rc.EXCISORS:
                g = load_golden(f"excise_and_random/{rc.case_name(shape, algorithm, excisor)}.npz")
                assert g["thresholds"][0] == rc.DEFAULT_THRESHOLD and g["thresholds"][1] in rc.THRESHOLD_CANDIDATES
                assert min(np.abs(g["distances"] - t).min() for t in g["thresholds"]) >= rc.MARGIN_THRESHOLD
                attempts.append(g["t1_attempts"])
                accepted.append(g["t1_accepted"])
        attempts, accepted = np.concatenate(attempts), np.concatenate(accepted)
        assert (accepted & (attempts == 1)).any() and (accepted & (attempts > 1)).any() and (~accepted).any()
        assert (attempts[~accepted] == rc.MAX_ATTEMPTS).all()
    g = load_golden("excise_and_random/n24_voxel_random_spherical.npz")
    assert np.prod(g["partition"]) == 18 < 24 and (np.bincount(g["voxels"][0, 0], minlength=18) >= 1).all()
    assert sorted(np.bincount(g["voxels"][0, 0], minlength=18)) == [1] * 12 + [2] * 6


def test_host_draws_and_helpers():
    """The draws come from numpy's global generator in the reference's order; the voxel coordinates are corner + u / p."""
    module, maker = _maker("n24", "voxel_random", 0.5)
    np.random.seed(3)
    u = np.random.random((24, 3))
    chosen = np.random.choice(np.arange(18), size=6, replace=False)
    np.random.seed(3)
    x = maker.generate_relative_coordinates_voxel_random(np.array([8.0, 8.0, 6.4, 0.0, 0.0, 0.0]))
    occupied = np.concatenate([np.arange(18), chosen])
    assert np.array_equal(x, rc.sites(u, occupied, [3, 3, 2]))
    np.random.seed(5)
    want = (np.random.random((24, 3)), np.random.randint(0, 1, size=(24,)))
    np.random.seed(5)
    assert np.array_equal(maker.generate_relative_coordinates_true_random(3), want[0])
    assert np.array_equal(maker.generate_atom_types(24, 1), want[1])
    order = maker.sort_atoms_indices_by_distance(np.array([0.99, 0.5, 0.5]), np.array([[0.5, 0.5, 0.5], [0.02, 0.5, 0.5], [0.9, 0.5, 0.5]]),
                                                 np.array([8.0, 8.0, 6.4, 0.0, 0.0, 0.0]))
    assert list(order) == [1, 2, 0]                                                         # across the cell boundary
    AXL = _axl()
    with pytest.raises(AssertionError, match="There are more constrained atoms 25 than total number of atoms 24."):
        maker.make_single_sample_from_constrained_substructure(AXL(A=np.zeros(25, dtype=int), X=np.random.random((25, 3)),
                                                                   L=np.array([8.0, 8.0, 6.4, 0.0, 0.0, 0.0])), 0)
    assert maker.filter_made_samples([1, 2]) == [1, 2]


def test_abi_names_the_two_entry_points():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    with pytest.raises(_hip.MdxError, match="no CPU fallback"):
        kernels.random_fill_proposals(1, 0, 0, 1, 1, 4, 3, 1, 0, "cpu")
    assert {"mdx_random_fill_proposals", "mdx_random_fill_environments"} <= set(_hip.ABI_SYMBOLS)
    assert (_hip.STATUS_RANDOM_FILL_COUNT, _hip.STATUS_RANDOM_FILL_ENVIRONMENT) == (4096, 8192)
    assert (_hip.RANDOM_FILL_MAX_ATOMS, _hip.RANDOM_FILL_MAX_VOXELS) == (1024, 4096)
    assert (_hip.TAG_FILL_UNIFORM, _hip.TAG_FILL_TYPE, _hip.TAG_FILL_VOXEL) == (11, 12, 13)
