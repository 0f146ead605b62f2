"""The host side of the optimal-transport modules and the equivariant analytical score network: imports, hyper-parameters,
state_dict layout, the refusal of host tensors, and what this package leaves out (fixtures: tests/golden/transport/, made by
tests/golden/make_golden_transport.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError

BLOCK = dict(architecture="equivariant_analytical", spatial_dimension=1, number_of_atoms=2, num_atom_types=1, kmax=5,
             equilibrium_relative_coordinates=[[0.25], [0.75]], sigma_d=0.01)
NETWORK_CASES = ["d1_n3", "d2_n3", "d3_n5", "d3_n8", "d3_n8_identity", "d3_n2_ties", "toy1d", "d3_n64", "d3_n65"]


def fixture(name):
    return np.load(os.path.join(GOLDEN, "transport", name + ".npz"))


def network_of(case, **changes):
    """The network a fixture was made with (`changes` override its hyper-parameters)."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.equivariant_analytical_score_network import (
        EquivariantAnalyticalScoreNetwork, EquivariantAnalyticalScoreNetworkParameters)
    kw = dict(spatial_dimension=int(case["D"]), number_of_atoms=int(case["N"]), num_atom_types=1, kmax=int(case["kmax"]),
              sigma_d=float(case["sigma_d"]), equilibrium_relative_coordinates=case["sites"].tolist(),
              use_point_group_symmetries=bool(case["symmetries"]))
    kw.update(changes)
    return EquivariantAnalyticalScoreNetwork(EquivariantAnalyticalScoreNetworkParameters(**kw)).eval()


def test_the_modules_import_with_the_references_names():
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks import equivariant_analytical_score_network as network
    from diffusion_for_multi_scale_molecular_dynamics_amd.transport import distance, optimal_permutation, transporter
    assert distance.TWOPI == 2 * torch.pi
    for module, names in ((distance, ("get_geodesic_displacements", "get_squared_geodesic_distance",
                                      "get_squared_geodesic_distance_cost_matrix")),
                          (optimal_permutation, ("get_optimal_permutation",)),
                          (network, ("EquivariantAnalyticalScoreNetwork", "EquivariantAnalyticalScoreNetworkParameters"))):
        assert all(callable(getattr(module, name)) for name in names)
    for name in ("get_atan2_translation", "get_translation_invariant", "_get_all_cost_matrices", "_solve_linear_assigment_problem",
                 "_find_permutation_and_cost", "get_optimal_transport"):
        assert callable(getattr(transporter.Transporter, name))
    for name in ("get_nearest_equilibrium_coordinates", "_get_jacobian_matrix", "get_normalized_scores", "_forward_unchecked",
                 "capture_safe", "check_status"):
        assert callable(getattr(network.EquivariantAnalyticalScoreNetwork, name))
    assert not os.path.exists(os.path.join(os.path.dirname(transporter.__file__), "optimal_translation.py"))
    # plain torch on any device: the geodesic displacement is the difference folded into [-1/2, 1/2]
    x1, x2 = torch.tensor([[0.1, 0.9]]), torch.tensor([[0.9, 0.1]])
    assert torch.allclose(distance.get_geodesic_displacements(x1, x2), torch.tensor([[-0.2, 0.2]]), atol=1e-6)
    assert abs(float(distance.get_squared_geodesic_distance(x1, x2)) - 0.08) < 1e-6
    assert distance.get_squared_geodesic_distance_cost_matrix(torch.rand(3, 2), torch.rand(4, 2)).shape == (3, 4)


def test_parameters_refuse_what_the_reference_refuses():
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.equivariant_analytical_score_network import (
        EquivariantAnalyticalScoreNetwork, EquivariantAnalyticalScoreNetworkParameters)
    parameters = EquivariantAnalyticalScoreNetworkParameters(**BLOCK)
    assert parameters.architecture == "equivariant_analytical" and parameters.use_point_group_symmetries is True
    for bad in (dict(sigma_d=0.0), dict(sigma_d=-0.1), dict(number_of_atoms=3), dict(equilibrium_relative_coordinates=[[0.25, 0.5], [0.75, 0.5]])):
        with pytest.raises(AssertionError):
            EquivariantAnalyticalScoreNetworkParameters(**dict(BLOCK, **bad))
    assert EquivariantAnalyticalScoreNetwork(parameters).symmetries.shape == (2, 1, 1)
    identity_only = EquivariantAnalyticalScoreNetwork(EquivariantAnalyticalScoreNetworkParameters(**dict(BLOCK, use_point_group_symmetries=False)))
    assert torch.equal(identity_only.symmetries, torch.eye(1).unsqueeze(0))
    sites = torch.rand(257, 3).tolist()
    with pytest.raises(NotImplementedError, match="256"):
        EquivariantAnalyticalScoreNetwork(EquivariantAnalyticalScoreNetworkParameters(**dict(
            BLOCK, spatial_dimension=3, number_of_atoms=257, equilibrium_relative_coordinates=sites)))


@pytest.mark.parametrize("name", NETWORK_CASES)
def test_state_dict_layout_is_the_references(name):
    case = fixture(name)
    state = network_of(case).state_dict()
    assert list(state) == list(case["state_keys"]) == ["equilibrium_relative_coordinates", "symmetries"]
    assert [str(tuple(v.shape)) for v in state.values()] == list(case["state_shapes"])
    assert [str(v.dtype) for v in state.values()] == list(case["state_dtypes"])
    assert torch.equal(state["equilibrium_relative_coordinates"], torch.from_numpy(case["sites"]))
    assert torch.equal(state["symmetries"], torch.from_numpy(case["operations"]))


def test_the_package_does_not_import_scipy():
    code = ("import sys, pkgutil, importlib\n"
            "import diffusion_for_multi_scale_molecular_dynamics_amd as p\n"
            "for m in pkgutil.walk_packages(p.__path__, p.__name__ + '.'):\n"
            "    importlib.import_module(m.name)\n"
            "assert not [m for m in sys.modules if m == 'scipy' or m.startswith('scipy.')], 'scipy was imported'\n")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    package = os.path.join(ROOT, "diffusion_for_multi_scale_molecular_dynamics_amd")
    for folder, _, files in os.walk(package):
        for file in files:
            if file.endswith(".py"):
                text = open(os.path.join(folder, file)).read()
                assert "import scipy" not in text and "from scipy" not in text, file


def test_host_tensors_are_refused():
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION, TIME
    from diffusion_for_multi_scale_molecular_dynamics_amd.transport.optimal_permutation import get_optimal_permutation
    from diffusion_for_multi_scale_molecular_dynamics_amd.transport.transporter import Transporter
    network = network_of(fixture("d3_n5"))
    transporter = Transporter(torch.eye(3).unsqueeze(0))
    x = torch.rand(2, 5, 3)
    batch = {NOISY_AXL_COMPOSITION: AXL(A=torch.zeros(2, 5, dtype=torch.long), X=x, L=torch.ones(2, 6)), TIME: torch.ones(2, 1),
             NOISE: torch.full((2, 1), 0.1), CARTESIAN_FORCES: torch.zeros_like(x)}
    for call in (lambda: network(batch, conditional=False), lambda: network.get_nearest_equilibrium_coordinates(x),
                 lambda: network.get_normalized_scores(x, torch.full_like(x, 0.1)),
                 lambda: transporter.get_optimal_transport(x, x), lambda: transporter._find_permutation_and_cost(torch.rand(4, 4)),
                 lambda: transporter._solve_linear_assigment_problem(torch.rand(2, 1, 4, 4)),
                 lambda: get_optimal_permutation(x[0], x[1]), lambda: kernels.linear_assignment(torch.rand(1, 3, 3)),
                 lambda: kernels.transport_align(x, x, torch.eye(3).unsqueeze(0)),
                 lambda: kernels.equivariant_analytical_score(x, torch.ones(2), x[0], torch.eye(3).unsqueeze(0), 0.01, 2)):
        with pytest.raises(MdxError, match="no CPU fallback"):
            call()
    # the reference's shape assertions come first
    with pytest.raises(AssertionError):
        network.get_normalized_scores(x, torch.full_like(x, 0.1)[:1])


def test_the_factory_still_refuses_the_architecture():
    """A statement of scope: the network is reached through the plugin API (any ScoreNetwork goes into a generator), not through
    the factory or the sample_diffusion CLI."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks import score_network_factory as factory
    assert "equivariant_analytical" not in factory.EXACT_SCORE_NETWORKS_BY_ARCH
    with pytest.raises(AssertionError, match="not implemented"):
        factory.create_score_network_parameters(dict(BLOCK))
