"""The regression regularizer and the regularizer factory without a GPU: the C ABI's new entry and its argument refusals, the
names, fields, defaults and signatures against the reference's source text, the factory on the reference's own YAML blocks, the
refusals (unknown type, fokker_planck, host tensors), burn-in, and the fixtures' own float64 agreement."""
import ast
import ctypes as C
import dataclasses
import inspect
import os

import numpy as np
import pytest
import torch
import yaml

from denoising_loss_cases import excess
from regression_cases import (ANALYTICAL_CASES, DIRECTORY, GIVEN_CASES, OPERAND_CASES, WHOLE_CALL_CASES, YAML, augmented_batch,
                              fixture, formula64, mlp, regularizer, target_parameters)

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, regularizers
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.analytical_score_network import (
    AnalyticalScoreNetwork, AnalyticalScoreNetworkParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.equivariant_analytical_score_network import \
    EquivariantAnalyticalScoreNetwork
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers import (
    REGULARIZER_PARAMETERS_BY_TYPE, REGULARIZERS_BY_TYPE, RegressionRegularizer, RegressionRegularizerParameters,
    create_regularizer, create_regularizer_parameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers.consistency_regularizer import (
    ConsistencyRegularizer, ConsistencyRegularizerParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers.regularizer import Regularizer, RegularizerParameters

REFERENCE_REGULARIZERS = "/root/reference/src/diffusion_for_multi_scale_molecular_dynamics/regularizers"
# the `regularizer:` block of the reference's consistency_with_analytical_guide_regularizer/specific_config.yaml (settings only)
CONSISTENCY_BLOCK = """
regularizer:
    type: consistency
    maximum_number_of_steps: 5
    number_of_burn_in_epochs: 0
    regularizer_lambda_weight: 0.001
    noise:
      total_time_steps: 100
      sigma_min: 0.001
      sigma_max: 0.2
    sampling:
      num_atom_types: 1
      number_of_atoms: 2
      number_of_samples: 64
      spatial_dimension: 1
      number_of_corrector_steps: 0
      use_fixed_lattice_parameters: True
      cell_dimensions: [[1.0]]
    analytical_score_network:
      architecture: "analytical"
      spatial_dimension: 1
      number_of_atoms: 2
      num_atom_types: 1
      kmax: 5
      equilibrium_relative_coordinates:
        - [0.25]
        - [0.75]
      sigma_d: 0.01
      use_permutation_invariance: True
"""


def _toy_block():
    with open(os.path.join(DIRECTORY, YAML)) as stream:
        return yaml.safe_load(stream)["regularizer"]


def test_the_entry_is_in_the_abi():
    assert "mdx_regression_loss" in _hip.ABI_SYMBOLS and _hip.ABI_VERSION == 14
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdx_hip.h")).read()
    assert "MDX_API int mdx_regression_loss(" in header and "#define MDX_ABI_VERSION 14" in header
    f = _hip.ABI.functions["mdx_regression_loss"]
    assert f.streamed and f.params[-2] == ("uint32_t*", "status")
    assert [name for _, name in f.params] == [
        "relative_coordinates", "sigmas", "score", "given_target", "equilibrium_relative_coordinates", "sigma_d_square", "kmax",
        "use_permutation_invariance", "batch", "number_of_atoms", "spatial_dimension", "target", "gradient", "per_structure", "sums",
        "loss", "status", "stream"]
    kinds = dict((name, kind) for kind, name in f.params)
    assert kinds["sigmas"] == kinds["given_target"] == "const float*" and kinds["sums"] == "double*" and kinds["batch"] == "int64_t"
    assert kinds["target"] == kinds["gradient"] == kinds["per_structure"] == kinds["loss"] == "float*"
    assert hasattr(_hip.lib(), "mdx_regression_loss")


def test_the_kernels_argument_refusals_need_no_gpu():
    """Every refusal returns before anything is launched: the entry is called with placeholder addresses that are never read."""
    f = _hip.lib().mdx_regression_loss
    p = C.c_void_p(64)

    def status(x=p, sigma=p, score=p, given=None, sites=p, sigma_d_square=0.0025, kmax=4, permutations=0, batch=2, atoms=5, dimension=3,
               target=p, gradient=p, per_structure=p, sums=p, loss=p):
        return f(x, sigma, score, given, sites, sigma_d_square, kmax, permutations, batch, atoms, dimension, target, gradient,
                 per_structure, sums, loss, None, None)

    invalid, unsupported = _hip.ERR_INVALID_ARG, _hip.ERR_UNSUPPORTED
    assert status(batch=0) == 0 and status(batch=0, given=p, x=None, sigma=None, sites=None) == 0      # MDX_OK, nothing launched
    assert status(batch=-1) == status(atoms=0) == status(dimension=0) == invalid
    assert status(kmax=-1) == status(sigma_d_square=0.0) == status(sigma_d_square=float("nan")) == invalid
    assert status(x=None) == status(sigma=None) == status(sites=None) == invalid
    assert status(kmax=65) == status(dimension=4) == status(atoms=1025) == status(batch=2**31) == unsupported
    assert status(atoms=9, permutations=1) == unsupported and status(batch=0, atoms=8, permutations=1) == 0
    # without a score only the target is made; the total needs the sums
    assert status(score=None, batch=0, gradient=None, per_structure=None, sums=None, loss=None) == 0
    for name in ("gradient", "per_structure", "sums", "loss"):
        others = {other: None for other in ("gradient", "per_structure", "sums", "loss") if other != name}
        assert status(score=None, **others) == invalid, name
    assert status(score=None, target=None, gradient=None, per_structure=None, sums=None, loss=None) == invalid
    assert status(sums=None) == invalid and status(sums=None, loss=None, batch=0) == 0
    # given-target mode: the analytical limits do not apply, a score is required, N D must fit an int
    assert status(given=p, batch=0, atoms=5000, dimension=7, kmax=-3, sigma_d_square=0.0, x=None, sigma=None, sites=None) == 0
    assert status(given=p, score=None, gradient=None, per_structure=None, sums=None, loss=None) == invalid
    assert status(given=p, atoms=2**30, dimension=2) == unsupported and status(given=p, batch=0, atoms=2**30, dimension=1) == 0


def _dataclass_fields(tree, class_name):
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    bases = [ast.unparse(b) for b in node.bases]
    fields = [(item.target.id, ast.unparse(item.annotation), None if item.value is None else ast.unparse(item.value))
              for item in node.body if isinstance(item, ast.AnnAssign)]
    return bases, fields


def _signatures(tree, name):
    """{function or public method: [(parameter, default source or None), ..]} of a class, or of the module's functions."""
    body = tree.body if name is None else next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name).body
    out = {}
    for item in body:
        if isinstance(item, ast.FunctionDef) and (not item.name.startswith("_") or item.name == "__init__"):
            positional = item.args.posonlyargs + item.args.args
            defaults = [None] * (len(positional) - len(item.args.defaults)) + [ast.unparse(d) for d in item.args.defaults]
            out[item.name] = [(a.arg, None if a.annotation is None else ast.unparse(a.annotation), d)
                              for a, d in zip(positional, defaults)]
    return out


@pytest.mark.skipif(not os.path.isdir(REFERENCE_REGULARIZERS), reason="the reference is not on this machine")
def test_names_fields_defaults_and_signatures_are_the_references():
    ours = ast.parse(inspect.getsource(regularizers))
    theirs = ast.parse(open(os.path.join(REFERENCE_REGULARIZERS, "regression_regularizer.py")).read())
    assert _dataclass_fields(ours, "RegressionRegularizerParameters") == _dataclass_fields(theirs, "RegressionRegularizerParameters") == \
        (["RegularizerParameters"], [("type", "str", "'regression'"), ("score_network_parameters", "ScoreNetworkParameters", None)])
    their_methods = _signatures(theirs, "RegressionRegularizer")
    assert set(their_methods) == {"__init__", "compute_regularizer_loss"}
    assert _signatures(ours, "RegressionRegularizer") == their_methods
    factory = ast.parse(open(os.path.join(REFERENCE_REGULARIZERS, "regularizer_factory.py")).read())
    their_functions = _signatures(factory, None)
    assert set(their_functions) == {"create_regularizer", "create_regularizer_parameters"}
    assert _signatures(ours, None) == their_functions
    tables = {ast.unparse(n.targets[0]): {k.arg for k in n.value.keywords} for n in factory.body if isinstance(n, ast.Assign)}
    assert tables == {"REGULARIZERS_BY_TYPE": {"fokker_planck", "regression", "consistency"},
                      "REGULARIZER_PARAMETERS_BY_TYPE": {"fokker_planck", "regression", "consistency"}}
    # the reference's assertion texts
    text = open(os.path.join(REFERENCE_REGULARIZERS, "regularizer_factory.py")).read()
    for fragment in ("is not implemented. Possible choices are", "is not implemented.", "Possible choices are"):
        assert fragment in text and fragment in inspect.getsource(regularizers)


def test_the_dataclass_and_the_class():
    fields = {f.name: f.default for f in dataclasses.fields(RegressionRegularizerParameters)}
    assert fields["type"] == "regression" and fields["score_network_parameters"] is dataclasses.MISSING
    assert fields["regularizer_lambda_weight"] == 1.0 and fields["number_of_burn_in_epochs"] == 0
    assert issubclass(RegressionRegularizerParameters, RegularizerParameters) and issubclass(RegressionRegularizer, Regularizer)
    with pytest.raises(TypeError):
        RegressionRegularizerParameters()                              # score_network_parameters is required
    with pytest.raises(AssertionError, match="weight must be positive"):
        regularizer(weight=0.0)
    r = regularizer("analytical_perm", weight=2.5)
    assert type(r.target_score_network) is AnalyticalScoreNetwork and r.target_score_network.use_permutation_invariance
    assert r.weight == 2.5 and r.can_regularizer_run() is True
    assert (r.rng_mode, r.seed, r.status, r.last_call) == ("reference", 0, None, None)
    assert "target_score_network.all_x0" in dict(r.named_parameters())            # a submodule: it moves with the regularizer
    assert type(regularizer("equivariant").target_score_network) is EquivariantAnalyticalScoreNetwork
    assert set(REGULARIZERS_BY_TYPE) == set(REGULARIZER_PARAMETERS_BY_TYPE) == {"regression", "consistency"}
    assert REGULARIZERS_BY_TYPE == dict(regression=RegressionRegularizer, consistency=ConsistencyRegularizer)
    assert REGULARIZER_PARAMETERS_BY_TYPE == dict(regression=RegressionRegularizerParameters,
                                                  consistency=ConsistencyRegularizerParameters)


def test_the_factory_on_the_references_regression_block():
    block = _toy_block()
    network_block = dict(block["score_network"])
    parameters = create_regularizer_parameters(block, dict(spatial_dimension=1, elements=["Si"]))
    assert "type" not in block and "score_network" not in block            # popped, as the reference pops them
    assert type(parameters) is RegressionRegularizerParameters and parameters.type == "regression"
    assert parameters.regularizer_lambda_weight == 1.0 and parameters.number_of_burn_in_epochs == 0
    assert parameters.score_network_parameters == AnalyticalScoreNetworkParameters(**network_block)
    network = parameters.score_network_parameters
    assert (network.architecture, network.number_of_atoms, network.spatial_dimension, network.kmax, network.sigma_d,
            network.use_permutation_invariance) == ("analytical", 2, 1, 5, 0.01, True)
    assert network.equilibrium_relative_coordinates == [[0.25], [0.75]]
    made = create_regularizer(parameters)
    assert type(made) is RegressionRegularizer and type(made.target_score_network) is AnalyticalScoreNetwork
    assert made.target_score_network.all_x0.shape == (2, 2, 1) and made.weight == 1.0
    # the toy operand case holds the same network
    g = fixture("toy_perm2_d1")
    assert (int(g["kmax"]), float(g["sigma_d"]), bool(g["permutations"])) == (5, 0.01, True) and g["sites"].tolist() == [[0.25], [0.75]]
    # a global parameter that disagrees with the block is the score-network factory's assertion
    with pytest.raises(AssertionError, match="inconsistent configuration values for spatial_dimension"):
        create_regularizer_parameters(_toy_block(), dict(spatial_dimension=3))


def test_the_factory_on_the_references_consistency_block():
    block = yaml.safe_load(CONSISTENCY_BLOCK)["regularizer"]
    parameters = create_regularizer_parameters(block, {})
    assert type(parameters) is ConsistencyRegularizerParameters and parameters.type == "consistency"
    assert (parameters.maximum_number_of_steps, parameters.regularizer_lambda_weight, parameters.kmax_target_score) == (5, 0.001, 4)
    assert (parameters.noise_parameters.total_time_steps, parameters.noise_parameters.sigma_max) == (100, 0.2)
    assert (parameters.sampling_parameters.number_of_samples, parameters.sampling_parameters.number_of_corrector_steps) == (64, 0)
    assert type(parameters.analytical_score_network_parameters) is AnalyticalScoreNetworkParameters
    assert parameters.analytical_score_network_parameters.use_permutation_invariance is True
    made = create_regularizer(parameters)
    assert type(made) is ConsistencyRegularizer and type(made.analytical_score_network) is AnalyticalScoreNetwork
    without = yaml.safe_load(CONSISTENCY_BLOCK)["regularizer"]
    del without["analytical_score_network"]
    assert create_regularizer_parameters(without, {}).analytical_score_network_parameters is None


def test_unknown_types_and_fokker_planck_are_refused():
    with pytest.raises(AssertionError, match=r"Regularizer Type nothing is not implemented\.Possible choices are dict_keys"):
        create_regularizer_parameters(dict(type="nothing"), {})
    with pytest.raises(AssertionError, match=r"Regularizer type nothing is not implemented\. Possible choices are dict_keys"):
        create_regularizer(RegularizerParameters(type="nothing"))
    with pytest.raises(NotImplementedError, match="autograd through the score network's inputs"):
        create_regularizer_parameters(dict(type="fokker_planck", regularizer_lambda_weight=1.0), {})
    with pytest.raises(NotImplementedError, match="autograd through the score network's inputs"):
        create_regularizer(RegularizerParameters(type="fokker_planck"))
    with pytest.raises(KeyError):
        create_regularizer_parameters(dict(regularizer_lambda_weight=1.0), {})          # no type, as in the reference


def test_burn_in_returns_zero_and_a_host_batch_is_refused(monkeypatch):
    g = fixture("analytical")
    r = regularizer("analytical")
    r.number_of_burn_in_epochs = 2
    for epoch in (0, 1):          # neither the network nor the batch is looked at
        out = r.compute_weighted_regularizer_loss(None, None, current_epoch=epoch)
        assert isinstance(out, torch.Tensor) and out.dim() == 0 and float(out) == 0.0

    def no_kernel(name, *args):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(kernels, "call", no_kernel)
    net = mlp(g)
    state = torch.get_rng_state()
    with pytest.raises(MdxError, match="no CPU fallback"):
        r.compute_weighted_regularizer_loss(net, augmented_batch(g, "cpu"), current_epoch=2)
    assert torch.equal(torch.get_rng_state(), state) and r.last_call is None and r.status is None      # refused before any draw
    x = torch.from_numpy(g["drawn_X"])
    with pytest.raises(MdxError, match="no CPU fallback"):
        kernels.regression_loss(x, target=x)
    with pytest.raises(MdxError, match="no CPU fallback"):
        kernels.regression_loss(x, relative_coordinates=x, sigmas=torch.ones(4), equilibrium_relative_coordinates=x[0],
                                sigma_d_square=0.0025, kmax=4)


def test_the_fixtures_hold_what_their_names_say():
    sizes = {case: fixture(case)["s"][0].size for case in OPERAND_CASES}
    assert [sizes[c] for c in ("n1_d1", "n5_d3", "n65_d2", "n216_d3", "given_n5_d3", "given_n700_d3")] == [1, 15, 130, 648, 15, 2100]
    assert [fixture(c)["s"].shape[0] for c in ("n1_d1", "n5_d3", "n65_d2", "n216_d3", "perm3_d2", "perm8_d3")] == [1, 3, 2, 2, 3, 2]
    threshold = 1.0 / np.sqrt(2.0 * np.pi)
    effective = lambda g: np.sqrt(float(g["sigma_d"])**2 + g["sigma"].astype(np.float64)**2)
    assert effective(fixture("ewald")).min() > threshold and (effective(fixture("n5_d3")) > threshold).tolist() == [False, False, True]
    assert [bool(fixture(c)["permutations"]) for c in ANALYTICAL_CASES] == [False] * 6 + [True] * 3
    assert fixture("perm8_d3")["x"].shape == (2, 8, 3) and fixture("toy_perm2_d1")["x"].shape == (4, 2, 1)
    g = fixture("placed")
    difference = g["x"][0].astype(np.float64) - g["sites"].astype(np.float64)
    assert np.all(difference[0] == 0.0) and np.all(np.abs(difference[1]) == 0.5) and np.all(difference[2] == 1.0 - 2.0**-24)
    assert np.all(g["target64"][0, 0] == 0.0)
    for case in GIVEN_CASES:
        assert np.array_equal(fixture(case)["target64"], fixture(case)["target"].astype(np.float64))
    for case in WHOLE_CALL_CASES:
        g = fixture(case)
        assert g["drawn_X"].shape == g["s"].shape == g["target"].shape == g["target64"].shape == (4, 4, 3)
        assert float(g["weight"]) == 2.5 and np.array_equal(g["weighted_loss"], np.float32(2.5) * g["loss"])
        assert target_parameters(g, equivariant=case == "equivariant").number_of_atoms == 4


@pytest.mark.parametrize("case", OPERAND_CASES)
def test_formula64_agrees_with_the_fixture(case):
    """regression_cases.formula64 (numpy) on the recorded score and binary64 target, rounded once to binary32, is within the GPU
    tests' bound of the reference-side record (torch): the bound holds for an evaluation in another library and order."""
    g = fixture(case)
    out = formula64(g["s"], g["target64"])
    assert np.all(g["per_structure64"] > 0.0) and np.all(np.isfinite(g["per_structure64"])) and float(g["loss64"]) > 0.0
    for name in ("target", "gradient", "per_structure", "loss"):
        assert excess(out[name].astype(np.float32), g[name + "64"]) <= 0.0, name
    # scores were drawn so that |s - t| is of the order of |t|
    errors, target = np.abs(g["s"].astype(np.float64) - g["target64"]), np.abs(g["target64"])
    assert 0.05 < np.linalg.norm(errors) / np.linalg.norm(target) < 5.0
