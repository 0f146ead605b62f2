"""Cases, a float64 restatement and a bar per gradient element for the MLP score network's training kernels
(csrc/mdx_mlp_train.hip: mdx_mlp_train_forward, mdx_mlp_train_backward).

Everything here is numpy on the CPU.  The shapes, inputs and sparse contractive networks are tests/mlp_cases.py's.  The
restatement is written from models/score_networks/mlp_score_network.py and include/mdx_hip.h, not from the kernels;
tests/test_mlp_train_cases_cpu.py ties it to torch's float64 autograd of the real module.

THE BACKWARD takes the activations the forward fed to every Linear (either restated in float64 from the inputs, or read from the
kernel's own record, which isolates the backward from the forward's binary32 rounding) and the cotangents of the three outputs:
    delta_heads = [cot_logits | cot_x | cot_l]                      dW_head = delta^T a_heads, db_head = sum_b delta
    delta_{NH-1} = delta_heads W_heads                               (no activation follows the last hidden layer)
    delta_{k-1} = (delta_k W_k) silu'(z_{k-1})                       silu'(z) = s (1 + z (1 - s)), s = 1 / (1 + exp(-z))
    delta_features = delta_0 W_0                                     split into the five embedding layers' output deltas
    dW = delta^T a, db = sum_b delta per layer; the atom-type embedding sums over the atoms as well (one weight for N atoms).

THE BAR of a gradient element: the kernel accumulates in binary64 (a binary32 x binary32 product is exact there; delta is never
rounded to binary32) and rounds the element to binary32 once, so
    |got - ref| <= 2^-23 |ref| + (T + 16) 2^-52 S_abs + 2^-149
with S_abs the same backward evaluated on absolute values (|W|, |delta|, |a|, |silu'|): what the terms of every sum that feeds the
element add up to in magnitude; and T the number of terms of the longest of those sums (the batch, for the atom-type embedding the
batch times the atoms, and the widths of the transposed products above the layer).  16 covers the handful of roundings of silu'.
No measured constant."""
import collections

import numpy as np

import mlp_cases as mc

STRUCTURES_PER_SLAB = 8         # MDX_MLP_TRAIN_STRUCTURES_PER_SLAB of include/mdx_hip.h (the CPU test compares)
SHAPES = (mc.TEMPLATE, mc.ONE_LANE, mc.ALL_ODD, mc.D1, mc.N24, mc.GLOBAL)
# 1 and 5; one slab + 1; four slabs, the last one partial: the second launch's loop over the slabs runs four passes per thread
BATCHES = (1, 5, STRUCTURES_PER_SLAB + 1, 3 * STRUCTURES_PER_SLAB + 2)
NULL_PARTS = ("logits", "x", "l")
MISTAKES = ("sigmoid_for_silu_slope", "weight_not_transposed", "bias_misses_last_structure", "atom_embedding_from_neighbour",
            "cos_sin_exchanged")
GOLDEN_DIRECTORY = "mlp_train"
GOLDEN_SHAPES = {"template": mc.TEMPLATE, "all_odd": mc.ALL_ODD}
GOLDEN_BATCH = 5
GOLDEN_FILES = [name + ".npz" for name in GOLDEN_SHAPES]
GOLDEN_FLOOR_FACTOR = 4.0

Activations = collections.namedtuple("Activations", "circle sigma time classes lattice features hidden_in heads_in z")
Gradients = collections.namedtuple("Gradients", "value s_abs terms")      # value, s_abs: {layer: (dW, db)}; terms: {layer: T}


def layer_names(shape):
    """The layers in the order of the address table and of the flat gradient buffer (mlp_cases.linears' names)."""
    return (["coordinates", "noise", "time", "atom_type", "lattice"] + ["hidden%d" % k for k in range(shape.layers)]
            + ["out_a", "out_x", "out_l"])


def shape_words(shape):
    """shape_host of include/mdx_hip.h."""
    return (shape.N, shape.d, shape.types + 1, shape.hidden, shape.layers, shape.ec, shape.en, shape.et, shape.ea, shape.el)


def record_floats(shape):
    nd, nl = shape.N * shape.d, mc.n_lattice(shape.d)
    return 2 * nd + 2 + shape.N + nl + mc.first_inputs(shape) + (2 * shape.layers - 1) * shape.hidden


def parameter_count(shape):
    weights = mc.weights_of(shape)
    return sum(weights.w[name].size + weights.b[name].size for name in layer_names(shape))


def parse_record(shape, record):
    """The kernel's record [B, record_floats] (include/mdx_hip.h) as float64 Activations."""
    record = np.asarray(record, dtype=np.float64)
    assert record.ndim == 2 and record.shape[1] == record_floats(shape)
    nd, nl, H, NH, F0 = shape.N * shape.d, mc.n_lattice(shape.d), shape.hidden, shape.layers, mc.first_inputs(shape)
    at = [0]

    def take(n):
        at[0] += n
        return record[:, at[0] - n:at[0]]

    circle, sigma, time = take(2 * nd), take(1)[:, 0], take(1)[:, 0]
    classes = take(shape.N)
    assert np.array_equal(classes, np.round(classes))
    lattice, features = take(nl), take(F0)
    hidden_in = [take(H) for _ in range(NH - 1)]
    heads_in = take(H)
    z = [take(H) for _ in range(NH - 1)]
    assert at[0] == record.shape[1]
    return Activations(circle, sigma, time, classes.astype(np.int64), lattice, features, hidden_in, heads_in, z)


def activations(shape, weights, inputs):
    """The same Activations restated in float64 from the inputs (the forward of mlp_score_network.py)."""
    w, b = weights.w, weights.b
    B = inputs.x.shape[0]
    x64 = inputs.x.astype(np.float64).reshape(B, -1)
    circle = np.concatenate([np.cos(2.0 * np.pi * x64), np.sin(2.0 * np.pi * x64)], axis=1)
    sigma, time, lattice = inputs.sigma.astype(np.float64), inputs.time.astype(np.float64), inputs.l.astype(np.float64)
    features = np.concatenate([
        circle @ w["coordinates"].T + b["coordinates"], sigma[:, None] * w["noise"][:, 0] + b["noise"],
        time[:, None] * w["time"][:, 0] + b["time"], (w["atom_type"].T[inputs.a] + b["atom_type"]).reshape(B, -1),
        lattice @ w["lattice"].T + b["lattice"]], axis=1)
    h, hidden_in, z = features, [], []
    for k in range(shape.layers):
        h = h @ w["hidden%d" % k].T + b["hidden%d" % k]
        if k + 1 < shape.layers:
            z.append(h)
            h = h / (1.0 + np.exp(-h))
            hidden_in.append(h)
    return Activations(circle, sigma, time, inputs.a.astype(np.int64), lattice, features, hidden_in, h, z)


def outputs(shape, weights, acts):
    """The three raw head outputs of the float64 forward, from its Activations."""
    B, N, C, d = acts.heads_in.shape[0], shape.N, shape.types + 1, shape.d
    head = lambda name: acts.heads_in @ weights.w[name].T + weights.b[name]
    return head("out_a").reshape(B, N, C), head("out_x").reshape(B, N, d), head("out_l")


def cotangents(shape, B, null=None, seed=0):
    """Random float32 cotangents of (logits [B, N, C], score_x [B, N, d], score_l [B, nl]) with an exact 0 in the MASK column (what
    autograd hands back through the -inf fill); the part named by `null` is None."""
    rng = np.random.default_rng(77 + 1000 * B + sum(shape) + seed)
    N, C, d, nl = shape.N, shape.types + 1, shape.d, mc.n_lattice(shape.d)
    logits = rng.standard_normal((B, N, C)).astype(np.float32)
    logits[..., C - 1] = 0.0
    parts = {"logits": logits, "x": rng.standard_normal((B, N, d)).astype(np.float32),
             "l": rng.standard_normal((B, nl)).astype(np.float32)}
    assert null is None or null in parts
    return tuple(None if name == null else parts[name] for name in NULL_PARTS)


def silu_slope(z):
    s = 1.0 / (1.0 + np.exp(-z))
    return s * (1.0 + z * (1.0 - s))


def backward(shape, weights, acts, cots, mistake=None):
    """Gradients(value, s_abs, terms) of every layer's (weight, bias) for Activations and cotangents (None: absent).  `mistake`:
    one of MISTAKES, a restated wrong kernel."""
    assert mistake is None or mistake in MISTAKES
    w = weights.w
    B, N, C, d, H, NH = acts.heads_in.shape[0], shape.N, shape.types + 1, shape.d, shape.hidden, shape.layers
    nd, nl = N * d, mc.n_lattice(d)
    widths = {"logits": N * C, "x": nd, "l": nl}
    delta = np.concatenate([np.zeros((B, widths[name])) if part is None else np.asarray(part, dtype=np.float64).reshape(B, -1)
                            for name, part in zip(NULL_PARTS, cots)], axis=1)
    magnitude = np.abs(delta)
    value, s_abs, terms = {}, {}, {}

    def contract(name, dl, mg, a, longest):
        bias = dl[:-1].sum(axis=0) if mistake == "bias_misses_last_structure" and name == "hidden0" else dl.sum(axis=0)
        value[name] = (dl.T @ a, bias)
        s_abs[name] = (mg.T @ np.abs(a), mg.sum(axis=0))
        terms[name] = max(longest, B)

    longest, at = 1, 0
    for name in ("out_a", "out_x", "out_l"):
        rows = w[name].shape[0]
        contract(name, delta[:, at:at + rows], magnitude[:, at:at + rows], acts.heads_in, longest)
        at += rows
    w_heads = np.concatenate([w["out_a"], w["out_x"], w["out_l"]], axis=0)
    delta, magnitude, longest = delta @ w_heads, magnitude @ np.abs(w_heads), max(longest, w_heads.shape[0])
    for k in range(NH - 1, -1, -1):
        name = "hidden%d" % k
        contract(name, delta, magnitude, acts.hidden_in[k - 1] if k else acts.features, longest)
        matrix = w[name].T if mistake == "weight_not_transposed" and k == NH - 1 and k > 0 else w[name]
        delta, magnitude, longest = delta @ matrix, magnitude @ np.abs(matrix), max(longest, H)
        if k:
            slope = silu_slope(acts.z[k - 1])
            used = 1.0 / (1.0 + np.exp(-acts.z[k - 1])) if mistake == "sigmoid_for_silu_slope" else slope
            delta, magnitude = delta * used, magnitude * np.abs(slope)
    # the concatenated features: [coordinates | noise | time | atom types (N x e_a) | lattice]
    o1, o2, o3, o4 = shape.ec, shape.ec + shape.en, shape.ec + shape.en + shape.et, shape.ec + shape.en + shape.et + N * shape.ea
    circle = acts.circle
    if mistake == "cos_sin_exchanged":
        circle = np.concatenate([circle[:, nd:], circle[:, :nd]], axis=1)
    contract("coordinates", delta[:, :o1], magnitude[:, :o1], circle, longest)
    contract("noise", delta[:, o1:o2], magnitude[:, o1:o2], acts.sigma[:, None], longest)
    contract("time", delta[:, o2:o3], magnitude[:, o2:o3], acts.time[:, None], longest)
    contract("lattice", delta[:, o4:], magnitude[:, o4:], acts.lattice, longest)
    delta_a, magnitude_a = delta[:, o3:o4].reshape(B, N, shape.ea), magnitude[:, o3:o4].reshape(B, N, shape.ea)
    if mistake == "atom_embedding_from_neighbour":
        delta_a = np.roll(delta_a, -1, axis=1)
    one_hot = np.eye(C)[acts.classes]                                            # [B, N, C]
    value["atom_type"] = (np.einsum("bne,bnc->ec", delta_a, one_hot), delta_a.sum(axis=(0, 1)))
    s_abs["atom_type"] = (np.einsum("bne,bnc->ec", magnitude_a, one_hot), magnitude_a.sum(axis=(0, 1)))
    terms["atom_type"] = max(longest, B * N)
    return Gradients(value, s_abs, terms)


def flat(shape, per_layer):
    """{layer: (dW, db)} as the flat gradient buffer: the layers in table order, weight then bias, row-major."""
    return np.concatenate([part.reshape(-1) for name in layer_names(shape) for part in per_layer[name]])


def flat_terms(shape, gradients):
    return np.concatenate([np.full(part.size, gradients.terms[name], dtype=np.float64)
                           for name in layer_names(shape) for part in gradients.value[name]])


def bar(shape, gradients):
    """The bar of every element of the flat gradient buffer."""
    ref, s_abs, terms = flat(shape, gradients.value), flat(shape, gradients.s_abs), flat_terms(shape, gradients)
    return 2.0 ** -23 * np.abs(ref) + (terms + 16.0) * 2.0 ** -52 * s_abs + 2.0 ** -149


def excess(shape, got, gradients):
    """max |got - ref| / bar over the flat buffer, and the index of the worst element."""
    ratio = np.abs(np.asarray(got, dtype=np.float64) - flat(shape, gradients.value)) / bar(shape, gradients)
    worst = int(np.argmax(ratio))
    return float(ratio[worst]), worst


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))
