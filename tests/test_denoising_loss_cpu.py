"""The denoising loss without a GPU: the parameter objects of the reference's `loss:` blocks, the factory, the refusal of host
tensors, the C ABI's new entry and what the fixtures hold."""
import dataclasses
import glob
import os
import re

import numpy as np
import pytest
import torch
import yaml

from denoising_loss_cases import ALGORITHMS, CASES, fixture
from test_reference_yaml_surface import REFERENCE

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
from diffusion_for_multi_scale_molecular_dynamics_amd.loss import (LOSS_BY_ALGO, create_loss_calculator, denoising_loss)
from diffusion_for_multi_scale_molecular_dynamics_amd.loss.atom_type_loss_calculator import D3PMLossCalculator
from diffusion_for_multi_scale_molecular_dynamics_amd.loss.coordinates_loss_calculator import (MSELossCalculator,
                                                                                                 WeightedMSELossCalculator)
from diffusion_for_multi_scale_molecular_dynamics_amd.loss.lattice_loss_calculator import LatticeLossCalculator
from diffusion_for_multi_scale_molecular_dynamics_amd.loss.loss_parameters import (LOSS_PARAMETERS_BY_ALGO, AtomTypeLossParameters,
                                                                                     MSELossParameters, WeightedMSELossParameters,
                                                                                     create_loss_parameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL
from diffusion_for_multi_scale_molecular_dynamics_amd.score.gaussian_score import get_lattice_sigma_normalized_score


def test_the_entry_is_in_the_abi():
    assert "mdx_denoising_loss" in _hip.ABI_SYMBOLS and _hip.ABI_VERSION == 14
    assert (_hip.STATUS_LOSS_LOGITS, _hip.STATUS_LOSS_INDEX) == (65536, 131072)
    assert (_hip.LOSS_MSE, _hip.LOSS_WEIGHTED_MSE, _hip.LOSS_MAX_ATOMS, _hip.LOSS_MAX_LATTICE_PARAMETERS) == (0, 1, 1024, 6)
    f = _hip.ABI.functions["mdx_denoising_loss"]
    assert f.streamed and f.params[-2] == ("uint32_t*", "status")
    # the tables are [T, C, C] pointers and the scalars of weighted_mse doubles: the caller decides their rounding
    kinds = dict((name, kind) for kind, name in f.params)
    assert kinds["q_matrices"] == kinds["q_bar_tm1_matrices"] == "const float*" and kinds["time_indices"] == "const int64_t*"
    assert kinds["x_sigma0"] == kinds["l_exponent"] == kinds["eps"] == kinds["lambda_a"] == "double"
    assert hasattr(_hip.lib(), "mdx_denoising_loss")


def test_defaults_and_the_factory():
    parameters = create_loss_parameters({})
    assert parameters == AXL(A=AtomTypeLossParameters(), X=MSELossParameters(), L=MSELossParameters())
    assert (parameters.A.ce_weight, parameters.A.eps, parameters.A.lambda_weight) == (0.001, 1e-8, 1.0)
    assert LOSS_PARAMETERS_BY_ALGO == dict(mse=MSELossParameters, weighted_mse=WeightedMSELossParameters, d3pm=AtomTypeLossParameters)
    assert LOSS_BY_ALGO == dict(mse=MSELossCalculator, weighted_mse=WeightedMSELossCalculator)
    block = dict(loss=dict(coordinates=dict(algorithm="weighted_mse", sigma0=0.3, lambda_weight=2.0), atom_types=dict(algorithm="d3pm", eps=1e-6)))
    parameters = create_loss_parameters(block)
    assert parameters.X == WeightedMSELossParameters(sigma0=0.3, lambda_weight=2.0) and parameters.X.exponent == 23.0259
    assert parameters.A == AtomTypeLossParameters(eps=1e-6) and parameters.L == MSELossParameters()
    calculator = create_loss_calculator(parameters)
    assert isinstance(calculator.A, D3PMLossCalculator) and isinstance(calculator.X, WeightedMSELossCalculator)
    assert type(calculator.L) is MSELossCalculator
    # sigma0 and exponent are 0-dim float32 buffers, as in the reference: their binary32 values enter the arithmetic
    assert calculator.X.sigma0.dtype == torch.float32 and calculator.X.sigma0.dim() == 0
    assert list(calculator.X.state_dict()) == ["sigma0", "exponent"]
    assert calculator.X._kernel_scalars() == dict(x_algorithm="weighted_mse", x_sigma0=float(np.float32(0.3)),
                                                  x_exponent=float(np.float32(23.0259)))
    assert kernels.binary32(0.2) == float(np.float32(0.2)) != 0.2
    with pytest.raises(AssertionError, match="The identifier field 'algorithm' is missing"):
        create_loss_parameters(dict(loss=dict(coordinates=dict(sigma0=0.1))))
    with pytest.raises(AssertionError, match="The option field 'huber' is missing"):
        create_loss_parameters(dict(loss=dict(coordinates=dict(algorithm="huber"))))
    with pytest.raises(AssertionError, match="Algorithm d3pm is not implemented"):
        create_loss_calculator(AXL(A=AtomTypeLossParameters(), X=AtomTypeLossParameters(), L=MSELossParameters()))
    with pytest.raises(TypeError):
        LatticeLossCalculator()                      # as in the reference: its constructor passes no parameters on


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_the_loss_blocks_of_the_references_yaml_templates():
    """Every YAML file of the reference with a `model: loss:` block gives the reference's parameter objects: the blocks' own values
    where they set one, the reference's defaults elsewhere (compared with the dataclasses' defaults as its source states them)."""
    seen = 0
    for path in sorted(glob.glob(os.path.join(REFERENCE, "**", "*.yaml"), recursive=True)):
        try:
            with open(path) as f:
                configuration = yaml.safe_load(f)
        except yaml.YAMLError:
            continue
        model = configuration.get("model") if isinstance(configuration, dict) else None
        if not isinstance(model, dict) or "loss" not in model:
            continue
        seen += 1
        parameters = create_loss_parameters(model)
        for field, key in (("X", "coordinates"), ("A", "atom_types"), ("L", "lattice_parameters")):
            block = model["loss"].get(key, dict(algorithm="d3pm" if field == "A" else "mse"))
            own = getattr(parameters, field)
            assert type(own) is LOSS_PARAMETERS_BY_ALGO[block["algorithm"]], (path, key)
            assert {k: getattr(own, k) for k in block} == block, (path, key)
            defaults = {f.name: f.default for f in dataclasses.fields(own) if f.name not in block}
            assert {k: getattr(own, k) for k in defaults} == defaults, (path, key)
    assert seen >= 5, seen
    source = open(os.path.join(REFERENCE, "src", "diffusion_for_multi_scale_molecular_dynamics", "loss", "loss_parameters.py")).read()
    for name, value in re.findall(r"^    (\w+): (?:float|str) = ([^#\n]+)", source, flags=re.M):
        owners = [c for c in LOSS_PARAMETERS_BY_ALGO.values() if name in {f.name for f in dataclasses.fields(c)}]
        assert owners and any(repr(getattr(c(), name)) == repr(eval(value)) for c in owners), (name, value)


def test_host_tensors_are_refused():
    g = fixture("c3_n5_d3_p6")
    t = lambda name: torch.from_numpy(g[name])
    calculator = create_loss_calculator(create_loss_parameters({}))
    with pytest.raises(MdxError, match="lives on cpu.*no CPU fallback"):
        calculator.X.calculate_unreduced_loss(t("predicted_x"), t("target_x32"), t("noise").reshape(-1, 1, 1).expand(-1, 5, 3))
    one_hot = torch.nn.functional.one_hot(t("a0"), 3).float()
    with pytest.raises(MdxError, match="predicted_logits lives on cpu.*no CPU fallback"):
        calculator.A.cross_entropy_loss_term(t("logits"), one_hot)
    matrices = [t(name)[t("time_indices")][:, None].expand(-1, 5, -1, -1) for name in ("table_q", "table_q_bar", "table_q_bar_tm1")]
    with pytest.raises(MdxError, match="lives on cpu.*no CPU fallback"):
        calculator.A.calculate_unreduced_loss(t("logits"), one_hot, one_hot, t("time_indices"), *matrices)
    with pytest.raises(MdxError, match="x0 lives on cpu.*no CPU fallback"):
        kernels.denoising_loss(x0=t("x0"), xt=t("xt"), predicted_x=t("predicted_x"), sigma=t("noise")[:, 0])
    batch = {"relative_coordinates": t("x0"), "atom_types": t("a0"), "lattice_parameters": t("l0"),
             "noisy_relative_coordinates": t("xt"), "noisy_atom_types": t("at"), "noisy_lattice_parameters": t("lt"),
             "noise_parameter": t("noise"), "time": t("time"), "time_indices": t("time_indices"), "q_matrices": matrices[0],
             "q_bar_matrices": matrices[1], "q_bar_tm1_matrices": matrices[2]}

    def network(batch, conditional=None):
        raise AssertionError("a host batch is refused before the network runs")
    with pytest.raises(MdxError, match="atom_types lives on cpu.*no CPU fallback"):
        denoising_loss(network, batch)
    # the lattice target is one elementwise expression of the reference, on any device
    assert torch.equal(get_lattice_sigma_normalized_score(t("lt"), t("l0"), t("sigma_n")[:, None]), t("target_l32"))


def test_what_the_fixtures_hold():
    """Every time index once, index 0 included; both branches of the wrapped score; reachable pairs only; every record finite;
    the placed rows are what the generator says; float64 is the yardstick because the reference's own float32 target is far off."""
    worst_float32_target = 0.0
    for case in CASES:
        g = fixture(case)
        C, N, D, P = g["shape"]
        assert np.array_equal(g["time_indices"], np.arange(12)) and g["table_q"].shape == (12, C, C)
        assert g["noise"].min() < 0.398942 < g["noise"].max() and np.array_equal(g["noise"][:, 0], g["table_sigma"])
        assert (((g["at"] == g["a0"]) | (g["at"] == C - 1))).all() and (g["a0"] < C - 1).all()
        assert np.isneginf(g["logits"][..., -1]).all() and np.isfinite(g["logits"][..., :-1]).all()
        assert np.array_equal((g["noise"][:, 0] / g["sigma_n_divisor"]).astype(np.float32), g["sigma_n"])
        for key, value in g.items():
            if key.endswith(("64", "32")) and value.dtype.kind == "f":
                assert np.isfinite(value).all(), (case, key)
        for algorithm in ALGORITHMS:
            assert g[f"{algorithm}_per_structure64"].shape == (12, 4) and g[f"{algorithm}_loss_x64"].shape == (12, N, D)
        worst_float32_target = max(worst_float32_target, float(g["float32_target_error"]))
        if case != "placed":
            assert np.array_equal(g["xt"], g["transform_xt"]) and np.array_equal(g["at"], g["transform_at"])
    assert 1e-6 < worst_float32_target < 1e-3
    assert np.abs(fixture("clip")["logits"][..., :-1]).min() == 30.0
    g = fixture("placed")
    assert np.array_equal(g["xt"][5], g["x0"][5]) and (np.abs(g["xt"][6] - g["x0"][6]) == 0.5).all()
    assert (g["at"][7] == 2).all() and np.array_equal(g["at"][8], g["a0"][8]) and np.array_equal(g["lt"], g["transform_lt"])
    assert 0.4 < float(fixture("c8_n65_d2_p3")["masked_fraction"]) < 0.7
    assert (float(fixture("sigma0_control")["sigma0"]), float(fixture("sigma0_control")["exponent"])) == (0.1, 200.0)
    assert (float(fixture("clip")["sigma0"]), float(fixture("clip")["exponent"])) == (0.2, 23.0259)
