"""Inputs and a float64 restatement, with a bar per output element, for the fused MLP score network (csrc/mdx_hip.hip):
mdx_mlp_forward and the forwards inside mdx_mlp_pc_sample (generic layer by layer, generic folded, the template's literals, the
register-resident folded family and the padded family).

Everything here is numpy / torch on the CPU.  The restatement is written from models/score_networks/mlp_score_network.py and
include/mdx_hip.h, not from the kernels; tests/test_mlp_cases_cpu.py ties it to the float64 module at 1e-12.

THE NETWORK is a real MLPScoreNetwork whose every nn.Linear is overwritten by a sparse contractive layer in the style of
chain_cases.sparse_layer: r in {1, 2, 4} non-zeros per row (at most the row's length), sum |w| <= 1/2 per row, full binary32
values, biases of order one; the first non-zero of a row sits at a structured column (identity, reversal, rotation by 1, 4, 16,
walking through the layers; hidden layer 0 is always a reversal, so that its row 0 reads the LAST input; hidden layer 0 and the
heads, which have fewer rows than columns, take r = 4 so that few of their inputs go unread).  SiLU has slope <= 1.1,
so the running bar contracts by 0.55 per layer; zeros multiply and add exactly, so a row has (non-zeros) rounded terms; and a
misrouted lane, a wrong zero-pad quad or a head column taken from its neighbour is an O(1) error in the elements it touches.

THE BAR, carried layer by layer (u = 2^-24; every constant below was written down before any GPU run):
  LAYER BY LAYER (mdx_mlp_forward; the sampler with MDX_MLP_SAMPLE_UNFOLDED, SPEC 0 and SPEC 1; global weights)
    cos, sin     the software sincospif_ of 2 x (2 x is exact).  It is bit-exact against the oracle's sequence for arguments in
                 [0, 2] (test_math_sequences_bit_exact), so the bar is the oracle's own distance from float64,
                 |mdxo_sincospif(2 x) - cos / sin(2 pi x)|; for an argument outside [0, 2] (the periodic inputs of
                 mdx_mlp_forward) 2 u more.
    a row        z = W v + b with k non-zeros: bar_z = |W| bar_v + (k + 4) u (|W||v| + |b|) -- k + 1 fused roundings (k fused
                 multiply-adds into four interleaved partial sums, one spare) plus 3 for ((s0 + s1) + (s2 + s3)) + bias.  (The
                 global-weights form adds the at most three tail terms of a row as a rounded product and a rounded addition: the
                 shapes here have at most one non-zero there, which the spare covers.)
    embeddings   noise w sigma + b and time w t + b: one fused multiply-add, 2 u (|w s| + |b|); atom type W[:, a] + b: one
                 addition, 2 u (|W| + |b|); lattice: a row started from the bias, (k + 1) u (|W||l| + |b|).
    SiLU         x' = __fdividef(z, 1 + __expf(-z)): bar_x' = 1.1 bar_z + (8 + 2 |z|) u |x'| -- the slope bound; hardware exp2
                 2 u, the addition u, the reciprocal 2 u, the product u, two spare: 8; and the exponent's argument z log2(e) is a
                 rounded product with a rounded constant: 2 |z| u relative in the exponential.
    the last hidden layer has no activation; the heads are three more rows; the MASK logit is exactly -inf.
  FOLDED (the sampler's default forwards: generic folded, SPEC 1xx, SPEC 2xx)
    W_f = [W0[:, :ec] Wc | W0[:, noise] wn | W0[:, time] wt | W0[:, atoms] | W0[:, lattice]], b_f = b0 + W0 (bc | bn | bt), and
    W_o = W_heads W_last, b_o = W_heads b_last + b_heads: the restatement's own float64 products, rounded ONCE to binary32 by
    the host.  A folded row: the row rule above with k = the non-zeros of the folded row, plus u (|W_f||v| + |b_f|) for that single
    rounding, plus, through |W_f| bar_v, HW_SINCOS_ABS for each cos / sin input (v_cos_f32 / v_sin_f32 with the argument in
    revolutions), the atom-type and lattice embeddings' bars as above, and nothing for sigma and t.  Middle layers and SiLU as
    above.
  HW_SINCOS_ABS = 2 x the largest |v_cos_f32(x) - cos(2 pi x)|, |v_sin_f32(x) - sin(2 pi x)| measured against float64 on an
    MI355X by tests/test_mlp_forward_elements_gpu.py::test_hardware_sincos on sincos_grid() (every k 2^-20 in [0, 1), 64 binary32
    neighbours on either side of 0, 1/4, 1/2, 3/4, 1, and 2^16 random binary32 values): measured maximum 1.237048e-07 (2.08 u)
    for both functions, so HW_SINCOS_ABS = 2.474096e-07.
  THE PREDICTOR STEP (mdx_mlp_pc_sample, one iteration, M = 0, zero z): want = x + (w s) / sigma in float64, error = the torus
    distance, bar = (w / sigma) bar_s + 4 u max(1, |want|); the lattice likewise with sigma_n and + n z_lat.  That step starts at
    index T, where w / sigma >= 1/4.  Its atom types say nothing: there q_bar_tm1 keeps a MASK atom MASK with probability 3/4
    whatever the logits are, and any other type has a 0 / 0 posterior.
  THE ATOM-TYPE STEP is a launch of its own, one predictor step from index 1: q_bar_tm1 is the identity there, so a MASK atom
    unmasks to the arg-max of its real-class logits (zero Gumbel noise, u = 1/2 where greedy) and every other atom keeps its type.
    The types must equal the oracle's update of the float64 logits for every atom whose margin exceeds MARGIN; the margin of a
    MASK atom is the gap between its two largest real-class logits, so the check reads the logits rows of networks with two or
    three atom types.  With ONE atom type there is a single real class and no decision can depend on its logit: the logits row of
    those networks (the template: SPEC 1 has no other shape) is checked by mdx_mlp_forward only, not inside the sampler."""
import collections
import functools

import numpy as np
import torch

import chain_cases as cc

U = 2.0 ** -24
HW_SINCOS_MEASURED = 1.237048e-07   # MI355X, both functions (cos at x = 0x1.fe5p-8, sin a quarter turn further): 2.08 u
HW_SINCOS_ABS = 2.474096e-07        # 2 x HW_SINCOS_MEASURED: the grid is not exhaustive; 4 x the measured figure still fails
SILU_SLOPE = 1.1
SILU_ALLOWANCE = 8.0
ROW_EXTRA = 4                   # one spare fused rounding and the three of ((s0 + s1) + (s2 + s3)) + bias
KINDS = ("identity", "reversal", "rotation1", "rotation4", "rotation16")
NON_ZEROS = (1, 2, 4)
BATCHES = (1, 5, 37)
LDS_LIMIT_BYTES = 128 * 1024    # include/mdx_hip.h, mdx_mlp_forward: image + scratch above it -> weights read from global memory
MARGIN = 1e-3
SMALL_EPSILON = 1e-8
SAMPLER_T = 4                   # time steps of the sampler tests' schedule; the x' step starts at index T
TYPES_INDEX = 1                 # ... and the atom-type step at index 1
SAMPLER_SIGMA_MIN, SAMPLER_SIGMA_MAX = 1e-3, 0.5
RNG_SEED, RNG_CALL = 0x5EED_1234_ABCD, 2

Shape = collections.namedtuple("Shape", "N types d hidden layers ec en et ea el")
TEMPLATE_EMBEDDINGS = (32, 16, 16, 1, 1)


def template(N, types, d, hidden, layers):
    return Shape(N, types, d, hidden, layers, *TEMPLATE_EMBEDDINGS)


TEMPLATE = template(8, 1, 3, 64, 3)
ONE_LANE = Shape(1, 1, 3, 16, 1, 4, 1, 1, 1, 1)
ALL_ODD = Shape(5, 3, 3, 50, 2, 7, 3, 5, 3, 2)
D2 = Shape(5, 2, 2, 48, 3, 8, 4, 4, 3, 2)
D1 = Shape(3, 1, 1, 32, 2, 4, 2, 2, 1, 1)
N20 = template(20, 1, 3, 96, 4)
N24 = template(24, 2, 3, 64, 2)
GLOBAL = template(8, 1, 3, 128, 3)
GLOBAL_TWO_TYPES = template(8, 2, 3, 128, 3)     # the global-weights sampler with a type decision that reads the logits
FORWARD_SHAPES = (TEMPLATE, ONE_LANE, ALL_ODD, D2, D1, N20, N24, GLOBAL)
GENERIC_SHAPES = (TEMPLATE, ALL_ODD, D2, N24)
FAMILY_SHAPES = tuple(template(8, types, 3, 64, layers) for types in (1, 2) for layers in (2, 3, 4))
LATTICE_SHAPES = (TEMPLATE, ALL_ODD)


def shape_id(shape):
    return "N%d_t%d_d%d_h%dx%d_e%d_%d_%d_%d_%d" % tuple(shape)


def n_lattice(d):
    return d * (d + 1) // 2


def folded_inputs(shape):
    return 2 * shape.N * shape.d + 2 + shape.N * shape.ea + shape.el


def outputs(shape):
    return shape.N * (shape.types + 1) + shape.N * shape.d + n_lattice(shape.d)


def first_inputs(shape):
    return shape.ec + shape.en + shape.et + shape.N * shape.ea + shape.el


# ---------------------------------------------------------------------------------------------------------------------------
# the grid of the hardware sin / cos probe
def sincos_grid():
    """binary32: every k 2^-20 in [0, 1); the 64 neighbours on either side of 0, 1/4, 1/2, 3/4 and 1; 2^16 random values."""
    parts = [(np.arange(2 ** 20, dtype=np.float64) * 2.0 ** -20).astype(np.float32)]
    for centre in (0.0, 0.25, 0.5, 0.75, 1.0):
        up = down = np.float32(centre)
        near = [up]
        for _ in range(64):
            up, down = np.nextafter(up, np.float32(2.0)), np.nextafter(down, np.float32(-2.0))
            near += [up, down]
        parts.append(np.array(near, dtype=np.float32))
    parts.append(np.random.default_rng(20).random(2 ** 16, dtype=np.float32))
    grid = np.concatenate(parts)
    assert grid.dtype == np.float32 and np.all(grid.astype(np.float64)[:2 ** 20] * 2.0 ** 20 == np.arange(2 ** 20))
    return grid


# ---------------------------------------------------------------------------------------------------------------------------
# the network
def linears(network):
    """Every nn.Linear of the unconditional forward, by name, in a fixed order."""
    out = [("coordinates", network.relative_coordinates_embedding_layer), ("noise", network.noise_embedding_layer),
           ("time", network.time_embedding_layer), ("atom_type", network.atom_type_embedding_layer),
           ("lattice", network.lattice_parameters_embedding_layer)]
    out += [("hidden%d" % k, layer) for k, layer in enumerate(network.mlp_layers)]
    return out + [("out_a", network.output_A_layer), ("out_x", network.output_X_layer), ("out_l", network.output_L_layer)]


@functools.lru_cache(maxsize=None)
def build_network(shape):
    """The MLPScoreNetwork of `shape` (float32, CPU, eval) with every nn.Linear overwritten by a sparse contractive layer."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.mlp_score_network import (
        MLPScoreNetwork, MLPScoreNetworkParameters)
    network = MLPScoreNetwork(MLPScoreNetworkParameters(
        number_of_atoms=shape.N, num_atom_types=shape.types, spatial_dimension=shape.d, n_hidden_dimensions=shape.layers,
        hidden_dimensions_size=shape.hidden, relative_coordinates_embedding_dimensions_size=shape.ec,
        noise_embedding_dimensions_size=shape.en, time_embedding_dimensions_size=shape.et,
        atom_type_embedding_dimensions_size=shape.ea, lattice_parameters_embedding_dimensions_size=shape.el)).eval()
    seed = sum((k + 1) * v for k, v in enumerate(shape))
    with torch.no_grad():
        for k, (name, linear) in enumerate(linears(network)):
            rows, columns = linear.weight.shape
            kind = "reversal" if name == "hidden0" else KINDS[(seed + k) % len(KINDS)]
            r = 4 if name == "hidden0" or name.startswith("out_") else NON_ZEROS[(seed + k) % 3]
            layer = cc.sparse_layer(columns, min(r, columns), 1000 * seed + k, kind, rows=rows)
            linear.weight.copy_(torch.from_numpy(layer.weight))
            linear.bias.copy_(torch.from_numpy(layer.bias))
    assert network.mlp_layers[0].weight.shape[1] == first_inputs(shape)
    assert float(network.mlp_layers[0].weight.detach()[0, -1]) != 0.0
    return network


class Weights:
    """The float64 copies of a network's parameters: w[name] [out, in], b[name] [out]."""

    def __init__(self, network=None):
        self.w, self.b = {}, {}
        if network is not None:
            for name, linear in linears(network):
                self.w[name] = linear.weight.detach().double().numpy().copy()
                self.b[name] = linear.bias.detach().double().numpy().copy()

    def copy(self):
        out = Weights()
        out.w = {k: v.copy() for k, v in self.w.items()}
        out.b = {k: v.copy() for k, v in self.b.items()}
        return out


@functools.lru_cache(maxsize=None)
def weights_of(shape):
    return Weights(build_network(shape))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
SPECIAL_COORDINATES = (0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -24)
PERIODIC_COORDINATES = (-0.25, 1.5, 3.0)

Inputs = collections.namedtuple("Inputs", "a x l time sigma")


def make_inputs(shape, B, periodic, time=None, sigma=None):
    """a [B, N] int64 with the MASK class (= types) among them, x [B, N, d] float32 with every second element one of 0, 1/4, 1/2,
    3/4, 1 - 2^-24 (periodic: also -0.25, 1.5, 3.0), l [B, nl] with non-zero off-diagonal entries, time [B] with 0, 1 and values
    between, sigma [B] from 1e-3 to 0.5 (log-uniform between); or the given time and sigma for every structure."""
    rng = np.random.default_rng(1000 * B + sum(shape) + (7 if periodic else 0))
    N, d, C, nl = shape.N, shape.d, shape.types + 1, n_lattice(shape.d)
    special = SPECIAL_COORDINATES + (PERIODIC_COORDINATES if periodic else ())
    x = rng.random(B * N * d).astype(np.float32)
    for i in range(0, x.size, 2):
        x[i] = np.float32(special[(i // 2 + B) % len(special)])
    a = rng.integers(0, C, size=(B, N)).astype(np.int64)
    a[0, 0] = C - 1
    if N > 1:
        a[0, 1] = 0
    lattice = rng.uniform(-0.5, 0.5, size=(B, nl))
    lattice[:, :d] = rng.uniform(4.0, 6.0, size=(B, d))
    if time is None:
        t = rng.random(B)
        t[0] = 0.0
        if B > 1:
            t[1] = 1.0
        s = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), size=B))
        s[0] = 1e-3
        if B > 1:
            s[-1] = 0.5
    else:
        t, s = np.full(B, float(time)), np.full(B, float(sigma))
    assert nl == d or np.all(lattice[:, d:] != 0.0)
    return Inputs(a, x.reshape(B, N, d), lattice.astype(np.float32), t.astype(np.float32), s.astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 restatement with its running bar
def silu(z, bar):
    x = z / (1.0 + np.exp(-z))
    return x, SILU_SLOPE * bar + (SILU_ALLOWANCE + 2.0 * np.abs(z)) * U * np.abs(x)


def row(W, b, v, bar_v, extra=ROW_EXTRA, rounded_once=False):
    """z = v W^T + b with the row rule; rounded_once: W and b are float64 products that the host rounds once to binary32."""
    absolute = np.abs(W)
    magnitude = np.abs(v) @ absolute.T + np.abs(b)[None, :]
    non_zeros = (W != 0.0).sum(axis=1)[None, :]
    bar = bar_v @ absolute.T + (non_zeros + extra) * U * magnitude
    if rounded_once:
        bar = bar + U * magnitude
    return v @ W.T + b[None, :], bar


def software_sincos_bar(x32, cos64, sin64):
    """|the oracle's sincospif(2 x) - float64| per element (+ 2 u where 2 x lies outside [0, 2])."""
    from oracle import mdx_oracle
    mdx_oracle.build()
    doubled = (np.float32(2.0) * x32).astype(np.float32)
    sc = mdx_oracle.sincospif(doubled.reshape(-1)).astype(np.float64)
    outside = ((doubled < 0.0) | (doubled > 2.0)).astype(np.float64) * 2.0 * U
    return (np.abs(sc[:, 1].reshape(x32.shape) - cos64) + outside, np.abs(sc[:, 0].reshape(x32.shape) - sin64) + outside)


def embeddings(shape, weights, inputs, atom_shift=False):
    """The pieces both forms share: ((cos|sin), atom-type embeddings [B, N ea] with bar, lattice embedding [B, el] with bar)."""
    B = inputs.x.shape[0]
    x64 = inputs.x.astype(np.float64).reshape(B, -1)
    cos64, sin64 = np.cos(2.0 * np.pi * x64), np.sin(2.0 * np.pi * x64)
    a = np.roll(inputs.a, -1, axis=1) if atom_shift else inputs.a
    wa, ba = weights.w["atom_type"], weights.b["atom_type"]
    emb_a = (wa.T[a] + ba[None, None, :]).reshape(B, -1)                                # Linear(one_hot(a)) = W[:, a] + b
    bar_a = (2.0 * U * (np.abs(wa).T[a] + np.abs(ba)[None, None, :])).reshape(B, -1)
    lattice = inputs.l.astype(np.float64)
    emb_l, bar_l = row(weights.w["lattice"], weights.b["lattice"], lattice, np.zeros_like(lattice), extra=1)
    return (cos64, sin64), (emb_a, bar_a), (emb_l, bar_l)


def heads_and_mask(shape, z, bar):
    """[logits | score_x | score_l] [B, outputs] -> the three outputs and their bars; the MASK logit -inf, its bar 0."""
    B, N, C, d = z.shape[0], shape.N, shape.types + 1, shape.d
    logits, bar_logits = z[:, :N * C].reshape(B, N, C).copy(), bar[:, :N * C].reshape(B, N, C).copy()
    logits[..., C - 1] = -np.inf
    bar_logits[..., C - 1] = 0.0
    return {"logits": logits, "bar_logits": bar_logits,
            "score_x": z[:, N * C:N * C + N * d].reshape(B, N, d), "bar_score_x": bar[:, N * C:N * C + N * d].reshape(B, N, d),
            "score_l": z[:, N * C + N * d:], "bar_score_l": bar[:, N * C + N * d:]}


def forward_layers(shape, weights, inputs, software_bar=True, atom_shift=False):
    """MLPScoreNetwork.forward in float64 with the layer-by-layer bar (software_bar = False: no oracle call, the cos / sin bar
    is 2 u -- the CPU tests of the restatement itself)."""
    w, b = weights.w, weights.b
    (cos64, sin64), (emb_a, bar_a), (emb_l, bar_l) = embeddings(shape, weights, inputs, atom_shift)
    if software_bar:
        bar_cos, bar_sin = software_sincos_bar(inputs.x.reshape(inputs.x.shape[0], -1), cos64, sin64)
    else:
        bar_cos = bar_sin = np.full_like(cos64, 2.0 * U)
    emb_c, bar_c = row(w["coordinates"], b["coordinates"], np.concatenate([cos64, sin64], axis=1),
                       np.concatenate([bar_cos, bar_sin], axis=1))
    sigma, time = inputs.sigma.astype(np.float64)[:, None], inputs.time.astype(np.float64)[:, None]
    emb_n = sigma * w["noise"][:, 0][None, :] + b["noise"][None, :]
    bar_n = 2.0 * U * (np.abs(sigma * w["noise"][:, 0][None, :]) + np.abs(b["noise"])[None, :])
    emb_t = time * w["time"][:, 0][None, :] + b["time"][None, :]
    bar_t = 2.0 * U * (np.abs(time * w["time"][:, 0][None, :]) + np.abs(b["time"])[None, :])
    h = np.concatenate([emb_c, emb_n, emb_t, emb_a, emb_l], axis=1)
    bar = np.concatenate([bar_c, bar_n, bar_t, bar_a, bar_l], axis=1)
    for k in range(shape.layers):
        h, bar = row(w["hidden%d" % k], b["hidden%d" % k], h, bar)
        if k + 1 < shape.layers:
            h, bar = silu(h, bar)
    w_heads = np.concatenate([w["out_a"], w["out_x"], w["out_l"]], axis=0)
    b_heads = np.concatenate([b["out_a"], b["out_x"], b["out_l"]], axis=0)
    return heads_and_mask(shape, *row(w_heads, b_heads, h, bar))


def folded_matrices(shape, weights):
    """(W_f [H, F], b_f), (W_o [outputs, H], b_o): the restatement's own float64 products."""
    w, b = weights.w, weights.b
    w0, o1, o2, o3 = w["hidden0"], shape.ec, shape.ec + shape.en, shape.ec + shape.en + shape.et
    w_f = np.concatenate([w0[:, :o1] @ w["coordinates"], w0[:, o1:o2] @ w["noise"], w0[:, o2:o3] @ w["time"], w0[:, o3:]], axis=1)
    b_f = b["hidden0"] + w0[:, :o1] @ b["coordinates"] + w0[:, o1:o2] @ b["noise"] + w0[:, o2:o3] @ b["time"]
    last = "hidden%d" % (shape.layers - 1)
    w_heads = np.concatenate([w["out_a"], w["out_x"], w["out_l"]], axis=0)
    b_heads = np.concatenate([b["out_a"], b["out_x"], b["out_l"]], axis=0)
    assert w_f.shape == (shape.hidden, folded_inputs(shape))
    return (w_f, b_f), (w_heads @ w[last], w_heads @ b[last] + b_heads)


def forward_folded(shape, weights, inputs, atom_shift=False):
    """The same function through the folded matrices, with the folded bar; needs >= 2 hidden layers."""
    assert shape.layers >= 2
    (cos64, sin64), (emb_a, bar_a), (emb_l, bar_l) = embeddings(shape, weights, inputs, atom_shift)
    (w_f, b_f), (w_o, b_o) = folded_matrices(shape, weights)
    sigma, time = inputs.sigma.astype(np.float64)[:, None], inputs.time.astype(np.float64)[:, None]
    v = np.concatenate([cos64, sin64, sigma, time, emb_a, emb_l], axis=1)
    bar = np.concatenate([np.full_like(cos64, HW_SINCOS_ABS), np.full_like(sin64, HW_SINCOS_ABS), 0.0 * sigma, 0.0 * time,
                          bar_a, bar_l], axis=1)
    h, bar = silu(*row(w_f, b_f, v, bar, rounded_once=True))
    for k in range(1, shape.layers - 1):
        h, bar = silu(*row(weights.w["hidden%d" % k], weights.b["hidden%d" % k], h, bar))
    return heads_and_mask(shape, *row(w_o, b_o, h, bar, rounded_once=True))


def forward(shape, weights, inputs, form, **keywords):
    """form "layers" | "folded": the values are the layer-by-layer restatement's in both; the bars are the form's own."""
    want = forward_layers(shape, weights, inputs, **keywords)
    if form == "folded":
        keywords.pop("software_bar", None)
        folded = forward_folded(shape, weights, inputs, **keywords)
        for name in ("logits", "score_x", "score_l"):
            finite = np.isfinite(want[name])
            assert np.allclose(folded[name][finite], want[name][finite], rtol=1e-12, atol=1e-13), "the folded algebra is not the network"
            want["bar_" + name] = folded["bar_" + name]
    else:
        assert form == "layers"
    return want


def module_forward(shape, inputs):
    """network.double() on the same inputs (the module's own forward, MASK logit included): logits, score_x, score_l."""
    import copy
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION,
                                                                              TIME)
    network = copy.deepcopy(build_network(shape)).double()
    batch = {NOISY_AXL_COMPOSITION: AXL(A=torch.from_numpy(inputs.a), X=torch.from_numpy(inputs.x).double(),
                                        L=torch.from_numpy(inputs.l).double()),
             TIME: torch.from_numpy(inputs.time).double()[:, None], NOISE: torch.from_numpy(inputs.sigma).double()[:, None],
             CARTESIAN_FORCES: torch.zeros(inputs.x.shape, dtype=torch.float64)}
    with torch.no_grad():
        out = network(batch, conditional=False)
    return out.A.numpy(), out.X.numpy(), out.L.numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# negative controls: each returns (weights, keywords of forward) that restate a subtly wrong kernel
CONTROLS = ("weight_scaled", "columns_swapped", "head_column_from_neighbour", "cos_sin_exchanged", "last_input_dropped",
            "atom_embedding_from_next_atom")


def control(shape, weights, inputs, name):
    w = weights.copy()
    keywords = {}
    last = "hidden%d" % (shape.layers - 1)
    if name == "weight_scaled":                       # one weight of the last hidden layer, the one that carries the most
        reference = forward_hidden_input(shape, weights, inputs)
        read = np.max(np.abs(np.concatenate([w.w["out_a"], w.w["out_x"], w.w["out_l"]], axis=0)), axis=0)     # by the heads
        carried = np.abs(w.w[last]) * np.max(np.abs(reference), axis=0)[None, :] * read[:, None]
        i, j = np.unravel_index(np.argmax(carried), carried.shape)
        w.w[last][i, j] *= 1.0 + 2.0 ** -10
    elif name == "columns_swapped":                   # two adjacent columns of the last hidden layer
        j = int(np.argmax(np.abs(w.w[last]).sum(axis=0)[:-1]))
        w.w[last][:, [j, j + 1]] = w.w[last][:, [j + 1, j]]
    elif name == "head_column_from_neighbour":        # score_x output 0 computed with the weights of output 1 (d N >= 2), or the
        if w.w["out_x"].shape[0] >= 2:                # first lattice output with those of the last score_x output
            w.w["out_x"][0], w.b["out_x"][0] = w.w["out_x"][1].copy(), w.b["out_x"][1]
        else:
            w.w["out_l"][0], w.b["out_l"][0] = w.w["out_x"][-1].copy(), w.b["out_x"][-1]
    elif name == "cos_sin_exchanged":
        nd = shape.N * shape.d
        w.w["coordinates"] = np.concatenate([w.w["coordinates"][:, nd:], w.w["coordinates"][:, :nd]], axis=1)
    elif name == "last_input_dropped":                # the non-zero that reads input position in_f - 1 of the first hidden layer
        rows = np.nonzero(w.w["hidden0"][:, -1])[0]
        assert rows.size
        w.w["hidden0"][rows, -1] = 0.0
    elif name == "atom_embedding_from_next_atom":
        keywords["atom_shift"] = True
    else:
        raise KeyError(name)
    return w, keywords


def forward_hidden_input(shape, weights, inputs):
    """The float64 input of the last hidden layer [B, width] (the control that scales one weight picks its column by it)."""
    w, b = weights.w, weights.b
    (cos64, sin64), (emb_a, _), (emb_l, _) = embeddings(shape, weights, inputs)
    sigma, time = inputs.sigma.astype(np.float64)[:, None], inputs.time.astype(np.float64)[:, None]
    h = np.concatenate([np.concatenate([cos64, sin64], axis=1) @ w["coordinates"].T + b["coordinates"],
                        sigma * w["noise"][:, 0] + b["noise"], time * w["time"][:, 0] + b["time"], emb_a, emb_l], axis=1)
    for k in range(shape.layers - 1):
        z = h @ w["hidden%d" % k].T + b["hidden%d" % k]
        h = z / (1.0 + np.exp(-z))
    return h


# ---------------------------------------------------------------------------------------------------------------------------
# the predictor step of the sampler tests
def noise_parameters():
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    return NoiseParameters(total_time_steps=SAMPLER_T, sigma_min=SAMPLER_SIGMA_MIN, sigma_max=SAMPLER_SIGMA_MAX,
                           schedule_type="exponential")


@functools.lru_cache(maxsize=None)
def oracle_schedule(C):
    """The oracle's schedule tables for noise_parameters() and C classes."""
    from oracle import mdx_oracle
    mdx_oracle.build()
    p = noise_parameters()
    return mdx_oracle.noise_schedule(p.total_time_steps, p.schedule_type, p.time_delta, p.sigma_min, p.sigma_max,
                                     p.corrector_step_epsilon, C)


def step_scalars(tables, shape, index=SAMPLER_T):
    """time, sigma, w = g^2, n = g, sigma_n of the predictor step at `index` from tables (a dict of arrays), as binary32."""
    idx = index - 1
    f32 = np.float32
    sigma = f32(tables["sigma"][idx])
    atoms_pow = f32(float(shape.N) ** (1.0 / shape.d))
    return {"idx": idx, "time": f32(tables["time"][idx]), "sigma": sigma, "w": f32(tables["g_squared"][idx]),
            "n": f32(tables["g"][idx]), "sigma_n": f32(sigma / atoms_pow)}


def is_greedy(B):
    return B == 5


def step_inputs(shape, B, scalars):
    """make_inputs(shape, B, False) at the step's time and sigma; for the atom-type step (index 1) two atoms in three are MASK,
    the ones whose new type is read off the logits."""
    inputs = make_inputs(shape, B, False, scalars["time"], scalars["sigma"])
    if scalars["idx"] == 0:
        masked = np.random.default_rng(B + sum(shape)).random(inputs.a.shape) < 2.0 / 3.0
        inputs = inputs._replace(a=np.where(masked, shape.types, inputs.a))
    return inputs


def predictor_step(shape, B, form, scalars, z_lattice=None):
    """One predictor step from make_inputs(shape, B, False, time, sigma) with zero coordinate noise: want x' (unwrapped) and its
    bar, want l' and its bar when z_lattice [B, nl] is given, and the float64 logits."""
    inputs = step_inputs(shape, B, scalars)
    net = forward(shape, weights_of(shape), inputs, form)
    w, sigma = float(scalars["w"]), float(scalars["sigma"])
    want_x = inputs.x.astype(np.float64) + (w * net["score_x"]) / sigma
    out = {"inputs": inputs, "net": net, "x": want_x,
           "bar_x": (w / sigma) * net["bar_score_x"] + 4.0 * U * np.maximum(1.0, np.abs(want_x))}
    if z_lattice is not None:
        sigma_n, n = float(scalars["sigma_n"]), float(scalars["n"])
        want_l = (inputs.l.astype(np.float64) + (w * net["score_l"]) / sigma_n) + n * np.asarray(z_lattice, dtype=np.float64)
        out["l"] = want_l
        out["bar_l"] = (w / sigma_n) * net["bar_score_l"] + 4.0 * U * np.maximum(1.0, np.abs(want_l))
    return out


def torus_distance(got, want):
    diff = np.asarray(got, dtype=np.float64) - want
    return np.abs(diff - np.round(diff))


def type_decisions(logits64, a, tables, idx, greedy):
    """The oracle's atom-type update (zero Gumbel noise, u = 1/2 where greedy, no one-transition rule) on the float64 logits
    rounded to binary32: (types [B, N], qualifies [B, N]) -- an atom qualifies when the best class leads the second by more than
    MARGIN in log(p + eps) and, where greedy, its MASK probability is further than MARGIN from u."""
    from oracle import mdx_oracle
    B, N, C = logits64.shape
    logits32 = logits64.astype(np.float32)
    zero, half = np.zeros((B, N, C), dtype=np.float32), np.full((B, N), 0.5, dtype=np.float32)
    q = [tables[k][idx] for k in ("q_matrix", "q_bar_matrix", "q_bar_tm1_matrix")]
    _, plain, _ = mdx_oracle.atom_types_update(logits32, a, *q, zero, half, SMALL_EPSILON, False, False, return_details=True)
    out, p, g = mdx_oracle.atom_types_update(logits32, a, *q, zero, half, SMALL_EPSILON, greedy, False, return_details=True)
    values = np.sort(np.log(p.astype(np.float64) + SMALL_EPSILON) + g.astype(np.float64), axis=-1)
    qualifies = values[..., -1] - values[..., -2] > MARGIN
    if greedy:
        qualifies &= np.abs(0.5 - plain[..., C - 1].astype(np.float64)) > MARGIN
    return out, qualifies


def records(shape, B, greedy):
    """The caller's noise records of one predictor step: [z N d | gumbel N C | u N | table 8], all zero but u = 1/2 where greedy."""
    N, d, C = shape.N, shape.d, shape.types + 1
    rec = np.zeros((B, N * (d + C + 1) + 8), dtype=np.float32)
    if greedy:
        rec[:, N * d + N * C:N * d + N * C + N] = 0.5
    return rec


# ---------------------------------------------------------------------------------------------------------------------------
# which forward the generic instantiation runs (include/mdx_hip.h, MDX_MLP_SAMPLE_UNFOLDED: the folded one "when the folded first
# layer is smaller than the two it replaces and the matrices fit in LDS")
def fold_pays(shape):
    if shape.layers < 2:
        return False
    plain = 2 * shape.N * shape.d * shape.ec + first_inputs(shape) * shape.hidden + shape.hidden * shape.hidden
    return folded_inputs(shape) * shape.hidden < plain


def wave_floats(shape):
    """The LDS floats of one wavefront of the fused kernels: two scratch vectors, the composition, the outputs, a noise record."""
    N, d, C, nl = shape.N, shape.d, shape.types + 1, n_lattice(shape.d)
    widest = max((folded_inputs(shape) + 63) // 64 * 64, first_inputs(shape), shape.hidden)
    scratch = (widest + 3) // 4 * 4 + 4
    pad4 = (nl + 3) // 4 * 4
    return (2 * scratch + 2 * N + N * d + pad4 + N * C + N * d + pad4 + N * (d + C + 1) + 8 + 3) // 4 * 4


def generic_folds(shape, image_floats):
    """Whether the generic instantiation (no MDX_MLP_SAMPLE_UNFOLDED) runs the folded forward: it pays, and the image, the four
    wavefronts' regions and the two folded matrices fit the LDS limit."""
    H, F, O = shape.hidden, folded_inputs(shape), outputs(shape)
    blobs = ((F + 3) // 4 * 4 * H + H + (H + 3) // 4 * 4 * O + O + 3) // 4 * 4
    return fold_pays(shape) and 4 * (image_floats + 4 * wave_floats(shape) + blobs) <= LDS_LIMIT_BYTES
