"""tests/mlp_train_cases.py without a GPU: the float64 restatement of the MLP score network's backward against torch's float64
autograd of the real module, five restated mistakes against the bar, and the surface of the feature (header, ABI, Makefile,
the module's attribute)."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import mlp_cases as mc
import mlp_train_cases as tc
from conftest import ROOT

CPU_SHAPES = (mc.TEMPLATE, mc.ONE_LANE, mc.ALL_ODD, mc.D1)
CPU_BATCH = 5


def autograd64(shape, inputs, cots):
    """{layer: (dW, db)} by torch's float64 autograd of the real module, MASK fill included."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION, TIME
    network = copy.deepcopy(mc.build_network(shape)).double()
    batch = {NOISY_AXL_COMPOSITION: AXL(A=torch.from_numpy(inputs.a), X=torch.from_numpy(inputs.x).double(),
                                        L=torch.from_numpy(inputs.l).double()),
             TIME: torch.from_numpy(inputs.time).double()[:, None], NOISE: torch.from_numpy(inputs.sigma).double()[:, None],
             CARTESIAN_FORCES: torch.zeros(inputs.x.shape, dtype=torch.float64)}
    out = network(batch, conditional=False)
    given = [(o, torch.from_numpy(c).double()) for o, c in zip((out.A, out.X, out.L), cots) if c is not None]
    layers = dict(mc.linears(network))
    parameters = [p for name in tc.layer_names(shape) for p in (layers[name].weight, layers[name].bias)]
    gradients = torch.autograd.grad([o for o, _ in given], parameters, [c for _, c in given], allow_unused=True)
    gradients = [torch.zeros_like(p) if g is None else g for p, g in zip(parameters, gradients)]
    return {name: (gradients[2 * k].numpy(), gradients[2 * k + 1].numpy()) for k, name in enumerate(tc.layer_names(shape))}


@pytest.mark.parametrize("shape", CPU_SHAPES, ids=mc.shape_id)
@pytest.mark.parametrize("null", (None,) + tc.NULL_PARTS)
def test_restatement_is_the_module_s_float64_autograd(shape, null):
    inputs = mc.make_inputs(shape, CPU_BATCH, False)
    weights = mc.weights_of(shape)
    acts = tc.activations(shape, weights, inputs)
    module = mc.module_forward(shape, inputs)
    mine = tc.outputs(shape, weights, acts)
    assert np.allclose(mine[1], module[1], rtol=1e-12, atol=1e-13) and np.allclose(mine[2], module[2], rtol=1e-12, atol=1e-13)
    real = np.isfinite(module[0])
    assert np.allclose(mine[0][real], module[0][real], rtol=1e-12, atol=1e-13) and not real[..., -1].any()
    cots = tc.cotangents(shape, CPU_BATCH, null)
    gradients = tc.backward(shape, weights, acts, cots)
    want = tc.flat(shape, autograd64(shape, inputs, cots))
    got, s_abs = tc.flat(shape, gradients.value), tc.flat(shape, gradients.s_abs)
    assert got.shape == want.shape == (tc.parameter_count(shape),)
    assert np.all(np.abs(got - want) <= 1e-12 * s_abs + 1e-300), float(np.max(np.abs(got - want) / (s_abs + 1e-300)))
    assert np.all(np.abs(got) <= s_abs * (1.0 + 1e-12)) and np.count_nonzero(got) > got.size // 8


def test_record_layout_round_trips():
    shape = mc.ALL_ODD
    acts = tc.activations(shape, mc.weights_of(shape), mc.make_inputs(shape, 3, False))
    record = np.concatenate([acts.circle, acts.sigma[:, None], acts.time[:, None], acts.classes.astype(np.float64), acts.lattice,
                             acts.features] + acts.hidden_in + [acts.heads_in] + acts.z, axis=1)
    assert record.shape == (3, tc.record_floats(shape))
    back = tc.parse_record(shape, record)
    assert np.array_equal(back.classes, acts.classes) and np.array_equal(back.heads_in, acts.heads_in)
    assert all(np.array_equal(a, b) for a, b in zip(back.z + back.hidden_in, acts.z + acts.hidden_in))
    assert np.array_equal(back.features, acts.features) and np.array_equal(back.circle, acts.circle)


@pytest.mark.parametrize("mistake", tc.MISTAKES)
def test_restated_mistakes_leave_the_bar(mistake):
    shape, B = mc.TEMPLATE, tc.STRUCTURES_PER_SLAB + 1
    inputs, weights = mc.make_inputs(shape, B, False), mc.weights_of(shape)
    acts = tc.activations(shape, weights, inputs)
    cots = tc.cotangents(shape, B)
    right = tc.backward(shape, weights, acts, cots)
    wrong = tc.flat(shape, tc.backward(shape, weights, acts, cots, mistake).value)
    worst, where = tc.excess(shape, wrong, right)
    print(mistake, worst, where)
    assert worst > 4.0
    # and the right answer rounded to binary32 is inside it
    rounded = tc.flat(shape, right.value).astype(np.float32)
    assert tc.excess(shape, rounded, right)[0] <= 1.0


def test_header_declares_the_entry_points_and_the_abi_version_stays():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    names = ("mdx_mlp_train_record_floats", "mdx_mlp_train_parameter_count", "mdx_mlp_train_workspace_doubles",
             "mdx_mlp_train_forward", "mdx_mlp_train_backward")
    assert set(names) <= set(_hip.ABI_SYMBOLS) and _hip.ABI_VERSION == 14
    assert _hip.MLP_TRAIN_STRUCTURES_PER_SLAB == tc.STRUCTURES_PER_SLAB and _hip.MLP_TRAIN_SHAPE_COUNT == len(tc.shape_words(mc.TEMPLATE))
    forward, backward = _hip.ABI.functions["mdx_mlp_train_forward"], _hip.ABI.functions["mdx_mlp_train_backward"]
    assert forward.streamed and backward.streamed
    assert [p for _, p in backward.params][2:6] == ["record", "grad_logits", "grad_x", "grad_l"]
    assert ("double", "scale") in backward.params and ("int", "accumulate") in backward.params
    makefile = open(os.path.join(_hip.CSRC, "Makefile")).read()
    objects = re.search(r"^OBJS\s*=(.*?)(?<!\\)\n", makefile, flags=re.S | re.M).group(1)
    assert "mdx_mlp_train.o" in objects.split() and os.path.isfile(os.path.join(_hip.CSRC, "mdx_mlp_train.hip"))
    source = open(os.path.join(_hip.CSRC, "mdx_mlp_train.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", source)               # no atomics in the arithmetic, no ticket
    assert os.path.isfile(os.path.join(ROOT, "profiles", "r22_mlp_training.md"))


def test_library_sizes_the_record_and_the_buffers():
    import ctypes
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    _hip.build()
    lib = _hip.lib()
    for shape in tc.SHAPES:
        words = (ctypes.c_int32 * _hip.MLP_TRAIN_SHAPE_COUNT)(*tc.shape_words(shape))
        assert lib.mdx_mlp_train_record_floats(words) == tc.record_floats(shape)
        assert lib.mdx_mlp_train_parameter_count(words) == tc.parameter_count(shape)
        for B in tc.BATCHES:
            slabs = -(-B // tc.STRUCTURES_PER_SLAB)
            assert lib.mdx_mlp_train_workspace_doubles(words, B) == slabs * tc.parameter_count(shape)
    too_deep = (ctypes.c_int32 * _hip.MLP_TRAIN_SHAPE_COUNT)(8, 3, 2, 64, _hip.MLP_MAX_HIDDEN + 1, 32, 16, 16, 1, 1)
    assert lib.mdx_mlp_train_record_floats(too_deep) == -1


def test_fused_training_defaults_to_off_and_the_plan_refuses_by_name():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    from diffusion_for_multi_scale_molecular_dynamics_amd.loss import FusedMlpTrainingStep
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.mlp_score_network import MLPScoreNetwork
    network = mc.build_network(mc.D1)
    assert network.fused_training is False and MLPScoreNetwork.fused_training is False
    assert [name for name, _ in kernels.mlp_train_layers(network)][:2] == ["relative_coordinates_embedding_layer", "noise_embedding_layer"]
    used = [name + suffix for name, _ in kernels.mlp_train_layers(network) for suffix in (".weight", ".bias")]
    assert used == [name for name, _ in network.named_parameters() if not name.startswith("condition")]
    with pytest.raises(_hip.MdxError, match="relative_coordinates_embedding_layer.weight lives on cpu"):
        kernels.mlp_train_plan(network)
    assert callable(FusedMlpTrainingStep)
    # with the attribute set, a host forward is still the PyTorch code: the same bits
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION, TIME
    inputs = mc.make_inputs(mc.D1, 3, False)
    batch = {NOISY_AXL_COMPOSITION: AXL(A=torch.from_numpy(inputs.a), X=torch.from_numpy(inputs.x), L=torch.from_numpy(inputs.l)),
             TIME: torch.from_numpy(inputs.time)[:, None], NOISE: torch.from_numpy(inputs.sigma)[:, None],
             CARTESIAN_FORCES: torch.zeros(inputs.x.shape)}
    plain = network(batch, conditional=False)
    twin = copy.deepcopy(network)
    twin.fused_training = True
    same = twin(batch, conditional=False)
    assert all(torch.equal(a, b) for a, b in zip(plain, same))
