"""Generate the MLP-training fixtures tests/golden/mlp_train/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_mlp_train.py

The reference's MLPScoreNetwork on the CPU, filled with tests/formula_weights.py's formula, for mlp_cases.TEMPLATE and ALL_ODD at
B = 5: the parameter gradients of sum(cotangent x output) over its three outputs, by its own float32 autograd and by float64
autograd of a .double() copy on the float64 copies of the same binary32 inputs.

A file holds
  words int32 [10]                                  the shape as include/mdx_hip.h's shape_host
  a int64 [B, N], x f32 [B, N, d], l f32 [B, nl], time f32 [B], sigma f32 [B]       mlp_cases.make_inputs(shape, B, False)
  cot_logits f32 [B, N, C] (MASK column 0), cot_x f32 [B, N, d], cot_l f32 [B, nl]    mlp_train_cases.cotangents(shape, B)
  names [tensors], counts int64 [tensors]           the parameters of the unconditional forward in named_parameters() order
  g32 f32 [total], g64 f64 [total]                  the two gradients, the tensors concatenated flat in that order
  floor f64 [tensors]                               rel-L2 of g32 against g64 per tensor: what float32 autograd itself is off by
"""
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

sys.path.insert(0, os.path.dirname(mg.HERE))
import mlp_cases as mc  # noqa: E402
import mlp_train_cases as tc  # noqa: E402
from formula_weights import fill_with_formula  # noqa: E402

LAYERS = ("relative_coordinates_embedding_layer", "noise_embedding_layer", "time_embedding_layer", "atom_type_embedding_layer",
          "lattice_parameters_embedding_layer", "mlp_layers", "output_A_layer", "output_X_layer", "output_L_layer")


def reference_network(shape):
    parameters = mg.MLPScoreNetworkParameters(
        number_of_atoms=shape.N, num_atom_types=shape.types, spatial_dimension=shape.d, n_hidden_dimensions=shape.layers,
        hidden_dimensions_size=shape.hidden, relative_coordinates_embedding_dimensions_size=shape.ec,
        noise_embedding_dimensions_size=shape.en, time_embedding_dimensions_size=shape.et,
        atom_type_embedding_dimensions_size=shape.ea, lattice_parameters_embedding_dimensions_size=shape.el)
    return fill_with_formula(mg.MLPScoreNetwork(parameters).eval())


def used_parameters(network):
    """[(name, parameter)] of the unconditional forward, in named_parameters() order."""
    return [(name, p) for name, p in network.named_parameters() if name.startswith(LAYERS)]


def gradients(network, inputs, cots, dtype):
    as_float = lambda a: torch.from_numpy(a).to(dtype)
    batch = {mg.NOISY_AXL_COMPOSITION: mg.AXL(A=torch.from_numpy(inputs.a), X=as_float(inputs.x), L=as_float(inputs.l)),
             mg.TIME: as_float(inputs.time)[:, None], mg.NOISE: as_float(inputs.sigma)[:, None],
             mg.CARTESIAN_FORCES: torch.zeros(inputs.x.shape, dtype=dtype)}
    # the reference's one-hot encoding is float32 whatever the module's dtype: the float64 run casts it (the values are 0 and 1)
    from diffusion_for_multi_scale_molecular_dynamics.models.score_networks import mlp_score_network as _mod
    one_hot = _mod.class_index_to_onehot
    _mod.class_index_to_onehot = lambda *a, **k: one_hot(*a, **k).to(dtype)
    try:
        out = network(batch, conditional=False)
    finally:
        _mod.class_index_to_onehot = one_hot
    parameters = [p for _, p in used_parameters(network)]
    got = torch.autograd.grad([out.A, out.X, out.L], parameters, [as_float(c) for c in cots])
    assert all(g.dtype == dtype for g in got)
    return np.concatenate([mg._np(g).reshape(-1) for g in got])


def case(shape):
    B = tc.GOLDEN_BATCH
    inputs, cots = mc.make_inputs(shape, B, False), tc.cotangents(shape, B)
    network = reference_network(shape)
    names = [name for name, _ in used_parameters(network)]
    counts = np.array([p.numel() for _, p in used_parameters(network)], dtype=np.int64)
    g32 = gradients(network, inputs, cots, torch.float32)
    g64 = gradients(copy.deepcopy(network).double(), inputs, cots, torch.float64)
    bounds = np.cumsum([0] + list(counts))
    floor = np.array([tc.rel_l2(g32[lo:hi], g64[lo:hi]) for lo, hi in zip(bounds[:-1], bounds[1:])])
    assert g32.dtype == np.float32 and g64.dtype == np.float64 and np.isfinite(g64).all() and np.all(floor > 0.0)
    return dict(words=np.array(tc.shape_words(shape), dtype=np.int32), a=inputs.a, x=inputs.x, l=inputs.l, time=inputs.time,
                sigma=inputs.sigma, cot_logits=cots[0], cot_x=cots[1], cot_l=cots[2], names=np.array(names), counts=counts,
                g32=g32, g64=g64, floor=floor)


def golden_mlp_train():
    os.makedirs(os.path.join(mg.OUT, tc.GOLDEN_DIRECTORY), exist_ok=True)
    for name, shape in tc.GOLDEN_SHAPES.items():
        mg.save(os.path.join(tc.GOLDEN_DIRECTORY, name + ".npz"), **case(shape))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_mlp_train()
