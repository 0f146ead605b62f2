"""Inputs and float64 restatements, with a bar per output element, for the MFMA chain entry points (csrc/mdx_egnn_chain.hip):
mdx_egnn_edge_chain (rows, piece sums, attention gate), mdx_mlp_chain_rows, mdx_node_mlp_rows(_split), and the integer rules of
mdx_egnn_chain_pack and mdx_egnn_chain_adapt_activation_exponents.

Everything here is numpy / torch on the CPU and states a contract from its documentation (include/mdx_hip.h and the header comment
of the kernel file), not from the kernel that implements it.

SPARSE CONTRACTIVE CHAINS.  A worst-case forward bound through dense random layers grows by ~ 0.5 * 1.7 * sqrt(H) per layer and is
useless after a few of them.  The layers here have r non-zero entries per row (r in 1, 2, 4, 8) with sum |w| <= 1/2 per row, full
binary32 values (both f16 halves of the split are non-zero), and biases of order one.  SiLU has slope <= 1.1, so the running bound
contracts by 0.55 per layer; zeros multiply and add exactly, so a row's sum has r + 1 rounded terms instead of H + 1; and the matrix
cores still run every lane, fragment and chunk, so a misrouted fragment is an O(1) error in exactly the elements it touches.

THE BAR, carried layer by layer (u = 2^-24; every constant below was written down before any GPU run):
  z = W x + b      bar_z = |W| (bar_x + op(x)) + n u (|W||x| + |b|) + 2 u |b| [+ split: 8 u |W||x| + 2^-(25+a) P|x|]
      n            roundings of the sum: r + 1 for exact binary32 (an r-term fused chain started from the bias, one spare);
                   3 r + 1 for the split (three partial products per term: hi.hi, hi.lo, lo.hi);
      2 u |b|      the bias is staged as fl(log2(e) b): the constant's own error and one rounding;
      op(x)        split only, the operand carried with exponent e: 4 u |x| (hi + lo carries 22 bits: 2^-22) + 2^-(25+e) (half the
                   f16 subnormal quantum 2^-24 of the scaled value: the absolute floor); exact binary32: 0;
      8 u |W||x|   split only: 4 u for the dropped lo.lo product (2^-22 of the term), 4 u for the split of the weight;
      2^-(25+a)    split only: the weight's own floor, a = the layer's exponent from mdx_egnn_chain_pack (tied layers: the
                   smaller one), times P|x| = the sum of |x| over the row's non-zero columns.
  x' = SiLU(z)     bar_x' = 1.1 bar_z + 8 u |x'|: the slope bound and the project's own allowance for the hardware exp2, the
                   addition, the reciprocal and the product (tests/test_egnn_helpers_gpu.py::test_message_input, measured there
                   at 0.73 -- inside the chain the exponent's argument is already in units of log2: no |pre| u term).
  x' = z           (the last layer of a row chain)  bar_x' = bar_z + u |z|.
  first edge layer z0 = (a + b) + b0 + radial w_r, elementwise: 4 u (|a| + |b|) [the sum's rounding, log2(e), the last fused
                   multiply-add, one spare] + 4 u |b0| [fl(log2(e) b0): 2, two fused multiply-adds: 2] + (D + 7) u |radial w_r|
                   [radial: D differences at 2 u of their squares, a product and at most D roundings of the running sum of
                   non-negative terms: D + 3; fl(log2(e) w_r): 2; two fused multiply-adds: 2].
  an output        bar + op(x) (the value is read back from the carried halves) + 2 u |x| (ln 2 and its rounding).
  rows in          2 u |x| (log2(e) and its rounding); residual: + u |out| for the addition.
  the head         one more row with r non-zeros and no bias, the layer's bar, + 4 u |w_out||y| (ln 2 on the way out: 2, spare: 2).
  a piece          the sum of its members' bars + 4 u sum |m| (the four steps of the segmented scan).
  the gate         logit = w_att . m + b_att: |w_att| (bar_m + op(m)) + (r + 3) u (|w_att||m| + |b_att|) [r fused multiply-adds, two
                   cross-lane additions, the bias] + 2 u |w_att||m| [fl(ln 2 2^-c w_att)]; g = sigmoid(logit): |g'| <= 1/4 times that
                   + 4 u g [expf, the addition, the division, one spare]; m g: g (bar_m + op(m)) + |m| bar_g + u |m g|.
  node MLP         the wide first layer is two layers whose accumulators continue one another: both halves' bars, every rounding
                   of the second half taken against |W_a||h| + |b| + |W_b||agg|; the projection reads the rows just written:
                   bar_out + u |out| (their rounding to binary32) + 2 u |out| (log2(e)) as the operand's bar, no bias, an output."""
import functools

import numpy as np
import torch

import gather_cases as gc

U = 2.0 ** -24
TILE = 128                                  # rows (edges) of one workgroup tile
WIDTHS = (32, 64, 128, 256)
PRECISIONS = ("f32", "f16x3", "f16x3_32x32")
DEFAULT_ACTIVATION_EXPONENT, MIN_ACTIVATION_EXPONENT = 6, -14       # asserted against the header by the GPU tests
STATUS_F16_RANGE = 4
SILU_SLOPE = 1.1
SILU_ALLOWANCE = 8.0
ROTATIONS = (1, 4, 8, 16, 32)               # across a quad, a half, a k-step, a 32-row chunk (and 1)
GATE_SCALE_LIMIT = 8.0
KINDS = ("random", "identity", "reversal") + tuple("rotation%d" % s for s in ROTATIONS)


def arithmetic(precision):
    """The two arithmetic classes of the three kernels: exact binary32 | split-f16 (either MFMA shape)."""
    assert precision in PRECISIONS
    return "f32" if precision == "f32" else "split"


def silu64(z):
    z = np.asarray(z, dtype=np.float64)
    return z / (1.0 + np.exp(-z))


# ---------------------------------------------------------------------------------------------------------------------------
# generators
class SparseLayer:
    """A layer with r non-zero entries per row: weight [rows, H] float32 (nn.Linear layout), bias [rows] float32 or None."""

    def __init__(self, weight, bias, r, kind):
        self.weight = np.ascontiguousarray(weight, dtype=np.float32)
        self.bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        self.r, self.kind = r, kind
        self.w64 = self.weight.astype(np.float64)
        self.abs64 = np.abs(self.w64)
        self.pattern = (self.w64 != 0.0).astype(np.float64)
        self.b64 = np.zeros(self.weight.shape[0]) if bias is None else self.bias.astype(np.float64)

    def largest(self):
        finite = self.abs64[np.isfinite(self.abs64)]
        return float(finite.max()) if finite.size else 0.0


def first_columns(H, kind, rows=None):
    """The structured column of every row for `kind` (None for "random")."""
    j = np.arange(H if rows is None else rows)
    if kind == "identity":
        return j % H
    if kind == "reversal":
        return (H - 1 - j) % H
    if kind.startswith("rotation"):
        return (j + int(kind[len("rotation"):])) % H
    assert kind == "random"
    return None


def sparse_layer(H, r, seed, kind="random", bias_scale=1.0, rows=None, row_sum=0.5, with_bias=True):
    """r non-zeros per row at distinct columns (the first one at the structured column of `kind`), magnitudes uniform in [0.3, 1]
    times a random sign, scaled so that the row's sum |w| is row_sum times a factor uniform in [0.8, 1] (never a power of two:
    a single non-zero would otherwise be dyadic, with an empty lo half), rounded to binary32; bias uniform in [-1, 1] bias_scale."""
    rows = H if rows is None else rows
    assert 1 <= r <= H
    rng = np.random.default_rng(seed)
    keys = rng.random((rows, H))
    first = first_columns(H, kind, rows)
    if first is not None:
        keys[np.arange(rows), first] = -1.0
    cols = np.argsort(keys, axis=1)[:, :r]
    mags = rng.uniform(0.3, 1.0, size=(rows, r)) * rng.choice([-1.0, 1.0], size=(rows, r))
    mags *= (row_sum * rng.uniform(0.8, 1.0, size=(rows, 1))) / np.abs(mags).sum(axis=1, keepdims=True)
    weight = np.zeros((rows, H))
    weight[np.arange(rows)[:, None], cols] = mags
    bias = rng.uniform(-1.0, 1.0, size=rows) * bias_scale if with_bias else None
    layer = SparseLayer(weight, bias, r, kind)
    assert np.all((layer.weight != 0).sum(axis=1) == r) and np.all(layer.abs64.sum(axis=1) <= row_sum * (1 + 1e-6))
    return layer


def layer_stack(H, n_layers, seed, r=None, bias_scale=1.0):
    """n_layers sparse layers walking through KINDS (layer k: KINDS[(seed + k) % len]) and through r = 1, 2, 4, 8."""
    out = []
    for k in range(n_layers):
        kind = KINDS[(seed + k) % len(KINDS)]
        if kind.startswith("rotation") and int(kind[len("rotation"):]) >= H:
            kind = "rotation16"
        out.append(sparse_layer(H, r if r is not None else (1, 2, 4, 8)[(seed + k) % 4], 1000 * seed + k, kind, bias_scale))
    return out


def pack_exponent(largest):
    """mdx_egnn_chain_pack: a with 2^a max|W| in [2^13, 2^14), clamped to [-40, 40]; 0 for an all-zero layer; infinities and NaNs
    are not magnitudes (SparseLayer.largest skips them)."""
    if largest == 0.0:
        return 0
    mantissa, exponent = np.frexp(np.float32(largest))          # largest = mantissa 2^exponent, mantissa in [1/2, 1)
    floor_log2 = max(int(exponent) - 1, -126)
    return int(min(max(13 - floor_log2, -40), 40))


def pack_exponents(layers, tied=0, head=None):
    """[len(layers) + 1] as mdx_egnn_chain_pack writes them: per layer, tied runs (bit l: layer l shares layer l - 1's power of two)
    take the smallest exponent of the run; last: the head row's (0 without one)."""
    exps = [pack_exponent(layer.largest()) for layer in layers]
    l = 1
    while l < len(layers):
        if tied >> l & 1:
            lo = l - 1
            hi = l
            while hi + 1 < len(layers) and (tied >> (hi + 1) & 1):
                hi += 1
            exps[lo:hi + 1] = [min(exps[lo:hi + 1])] * (hi + 1 - lo)
            l = hi + 1
        else:
            l += 1
    return exps + [0 if head is None else pack_exponent(head.largest())]


def adapted_exponent(current, maximum_bits):
    """mdx_egnn_chain_adapt_activation_exponents for one position: min(current, clamp(12 - floor(log2 m), -14, 6)) -- 2^e m in
    [2^12, 2^13) -- for a recorded maximum m (its float bits; an infinity or a NaN counts as the largest float, a subnormal as
    below every normal number); a zero maximum keeps the exponent."""
    bits = int(maximum_bits) & 0x7fffffff
    if bits == 0:
        return current
    floor_log2 = 127 if bits >= 0x7f800000 else (bits >> 23) - 127
    return min(current, min(max(12 - floor_log2, MIN_ACTIVATION_EXPONENT), DEFAULT_ACTIVATION_EXPONENT))


def workgroup_tiles(n_rows, n_cus):
    """The tiles each workgroup of a launch over n_rows rows runs, in order: a persistent grid of min(tiles, CUs) workgroups;
    workgroup b runs on XCD b mod 8 (one XCD with fewer than 8 workgroups); every XCD takes one contiguous eighth of the tiles
    (ceil(tiles / 8) of them, the last XCDs what is left) and its workgroups walk it side by side."""
    n_tiles = (n_rows + TILE - 1) // TILE
    grid = min(n_tiles, n_cus)
    n_xcd = 8 if grid >= 8 else 1
    per_xcd = (n_tiles + n_xcd - 1) // n_xcd
    out = []
    for b in range(grid):
        xcd, slot = b % n_xcd, b // n_xcd
        wgs = (grid - xcd + n_xcd - 1) // n_xcd
        lo, hi = xcd * per_xcd, min(xcd * per_xcd + per_xcd, n_tiles)
        out.append(list(range(lo + slot, hi, wgs)))
    assert sorted(t for tiles in out for t in tiles) == list(range(n_tiles)), "the order does not cover every tile once"
    return out


def most_tiles(n_rows, n_cus):
    return max(len(tiles) for tiles in workgroup_tiles(n_rows, n_cus))


def graph_with_poison(degrees, seed, capacity_extra=0):
    """gather_cases.ragged_graph over len(degrees) nodes plus ONE POISON NODE behind them (index len(degrees), no edges): its
    node_proj and coord rows are NaN and no live edge names it; the capacity_extra edge rows behind the live ones name it on both
    sides.  -> (edges [E + capacity_extra, 2], offsets, degree (both with the poison node), E)."""
    n = len(degrees)
    edges, offsets, degree = gc.ragged_graph(list(degrees), n, seed)
    E = edges.shape[0]
    edges = np.concatenate([edges, np.full((capacity_extra, 2), n, dtype=np.int64)], axis=0)
    return edges, np.append(offsets, E), np.append(degree, 0), E


def long_degrees(n_edges):
    """gather_cases.DEGREES repeated (every second time in the shuffled order) until they hold n_edges edges, the last node cut."""
    out, total, k = [], 0, 0
    while total < n_edges:
        for d in (gc.DEGREES if k % 2 == 0 else gc.DEGREES_SHUFFLED):
            d = min(d, n_edges - total)
            out.append(d)
            total += d
            if total == n_edges:
                break
        k += 1
    assert out[0] == 0 and out[-1] > 0 and sum(out) == n_edges
    return out


class EdgeCase:
    """One edge-chain problem: graph, node rows, layers."""

    def __init__(self, H, n_message, n_coord, D, degrees, seed, r=None, capacity_extra=0, attention=False, widths=None):
        self.H, self.n_message, self.n_coord, self.D, self.seed = H, n_message, n_coord, D, seed
        rng = np.random.default_rng(seed)
        self.edges, self.offsets, self.degree, self.E = graph_with_poison(degrees, seed + 1, capacity_extra)
        self.n_nodes = len(self.degree)
        self.node_proj = rng.uniform(-1.0, 1.0, size=(self.n_nodes, 2 * H)).astype(np.float32)
        self.coord = rng.uniform(-0.5, 0.5, size=(self.n_nodes, D)).astype(np.float32)
        self.node_proj[-1] = np.nan
        self.coord[-1] = np.nan
        self.bias_in = rng.uniform(-1.0, 1.0, size=H).astype(np.float32)
        self.w_radial = rng.uniform(-1.0, 1.0, size=H).astype(np.float32)
        self.layers = layer_stack(H, n_message + n_coord, seed, r)
        self.message_width, self.coord_width = widths if widths is not None else (H, H)
        if widths is not None:
            self._pad(*widths)
        self._gate_and_head(attention)

    def _gate_and_head(self, attention):
        """The two single rows, drawn against the float64 activations they meet (a condition on the inputs: nothing here is
        measured on a kernel).  The contraction that keeps the bar flat also makes every edge's activations alike, so
          * the gate row (8 non-zeros, sum |w| = 1) is scaled until the logits of the live edges spread over 1.5 -- by
            GATE_SCALE_LIMIT at the most: the gate's bar grows with the row, and behind more than one message layer the spread
            stays below 1.5 -- and its bias puts their middle within 0.3 of zero;
          * the head row (16 non-zeros, sum |w| = 1) takes the signs of the activations of edge 0, so that the scalar is a sum
            without cancellation and its bar stays a few u of its value."""
        H, L, seed = self.H, self.n_message + self.n_coord, self.seed
        m, c = self.message_width, self.coord_width

        def row(width, r, row_seed, **keywords):
            narrow = sparse_layer(width, min(r, width), row_seed, rows=1, **keywords)
            weight = np.zeros((1, H), dtype=np.float32)
            weight[:, :width] = narrow.weight
            return weight, narrow
        ar = Bars("f32", L + 2)
        x, _ = ar.first_edge_layer(self, self.edges[:self.E])
        self.att = None
        for l in range(L):
            x = ar.silu(ar.linear(self.layers[l], l, x, l))
            if l + 1 == self.n_message and attention:
                weight, narrow = row(m, 8, seed + 9, row_sum=1.0, bias_scale=0.3)
                logits = x[0] @ weight.astype(np.float64).T
                scale = np.float32(min(1.5 / float(logits.max() - logits.min()), GATE_SCALE_LIMIT))
                logits = x[0] @ (weight * scale).astype(np.float64).T
                centre = np.float32(0.5 * (logits.max() + logits.min()))
                self.att = SparseLayer(weight * scale, narrow.bias - centre, narrow.r, narrow.kind)
                x, _ = ar.gate(self.att, x, l + 1)
        weight, narrow = row(c, 16, seed + 7, with_bias=False, row_sum=1.0)
        signs = np.where(x[0][0] < 0.0, -1.0, 1.0).astype(np.float32)
        self.w_out = SparseLayer(np.abs(weight) * signs[None, :], None, narrow.r, narrow.kind)

    def _pad(self, m, c):
        """Unequal widths m (messages) and c (coordinate MLP) inside the chain width H: every weight, bias and vector outside
        them is zero (what EdgeChainPack does); the generators are re-drawn at the narrow widths and embedded."""
        H, seed = self.H, self.seed

        def embed(layer, rows, cols):
            w = np.zeros((H, H) if layer.weight.shape[0] > 1 else (1, H), dtype=np.float32)
            w[:layer.weight.shape[0], :cols] = layer.weight[:, :cols]
            b = None
            if layer.bias is not None:
                b = np.zeros(w.shape[0], dtype=np.float32)
                b[:rows] = layer.bias[:rows]
            w[rows:] = 0.0
            return SparseLayer(w, b, layer.r, layer.kind)
        self.bias_in[m:] = 0.0
        self.w_radial[m:] = 0.0
        self.node_proj[:-1, m:H] = 0.0
        self.node_proj[:-1, H + m:] = 0.0
        layers = []
        for k in range(self.n_message + self.n_coord):
            cols = m if k <= self.n_message else c
            rows = m if k < self.n_message else c
            narrow = sparse_layer(cols, min(4, cols), 1000 * seed + 50 + k, rows=rows)
            layers.append(embed(narrow, rows, cols))
        self.layers = layers


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 restatement with its running bar
class Bars:
    """State = (value, bar) float64 arrays.  act_exps: one exponent per position (None: the default everywhere); weight_exps: as
    pack_exponents gives them."""

    def __init__(self, precision, n_positions, act_exps=None, weight_exps=None):
        self.split = arithmetic(precision) == "split"
        self.act_exps = [DEFAULT_ACTIVATION_EXPONENT] * n_positions if act_exps is None else [int(e) for e in act_exps]
        self.weight_exps = weight_exps
        self.positions = {}                  # q -> (largest |value| - bar, largest |value| + bar) of the carried values there

    def op(self, v, q):
        return 4.0 * U * np.abs(v) + 2.0 ** -(25 + self.act_exps[q]) if self.split else 0.0

    def note(self, q, state):
        v, bar = state
        lo, hi = float(np.max(np.abs(v) - bar)), float(np.max(np.abs(v) + bar))
        if q in self.positions:
            lo, hi = max(lo, self.positions[q][0]), max(hi, self.positions[q][1])
        self.positions[q] = (lo, hi)

    def rows_in(self, x32):
        v = np.asarray(x32, dtype=np.float32).astype(np.float64)
        return v, 2.0 * U * np.abs(v)

    def first_edge_layer(self, case, edges):
        H, D = case.H, case.D
        src, dst = edges[:, 0], edges[:, 1]
        a = case.node_proj[src, :H].astype(np.float64)
        b = case.node_proj[dst, H:].astype(np.float64)
        diff = case.coord[src].astype(np.float64) - case.coord[dst].astype(np.float64)
        radial = (diff * diff).sum(axis=1)
        b0, wr = case.bias_in.astype(np.float64), case.w_radial.astype(np.float64)
        rw = radial[:, None] * wr[None, :]
        z = a + b + b0[None, :] + rw
        bar = U * (4.0 * (np.abs(a) + np.abs(b)) + 4.0 * np.abs(b0)[None, :] + (D + 7.0) * np.abs(rw))
        return self.silu((z, bar)), radial

    def linear(self, layer, l, state, q, start=None):
        """(z, bar_z, magnitude) of layer `layer` (index l in the image, for its exponent) on the operand `state` carried at
        position q; start: the (z, bar, magnitude) this layer's accumulators continue from."""
        v, bar = state
        av = np.abs(v)
        wav = av @ layer.abs64.T
        ab = np.abs(layer.b64)[None, :]
        mag = wav + ab + (0.0 if start is None else start[2])
        z = v @ layer.w64.T + layer.b64[None, :]
        n = 3 * layer.r + 1 if self.split else layer.r + 1
        bz = (bar + self.op(v, q)) @ layer.abs64.T + n * U * mag + 2.0 * U * ab
        if self.split:
            bz = bz + 8.0 * U * wav + 2.0 ** -(25 + self.weight_exps[l]) * (av @ layer.pattern.T)
        if start is not None:
            z, bz = z + start[0], bz + start[1]
        return z, bz, mag

    @staticmethod
    def silu(state):
        z, bz = state[0], state[1]
        x = silu64(z)
        return x, SILU_SLOPE * bz + SILU_ALLOWANCE * U * np.abs(x)

    @staticmethod
    def identity(state):
        return state[0], state[1] + U * np.abs(state[0])

    def output(self, state, q):
        v, bar = state
        return v, bar + self.op(v, q) + 2.0 * U * np.abs(v)

    def head(self, row, l, state, q):
        z, bz, mag = self.linear(row, l, state, q)
        return z[:, 0], (bz + 4.0 * U * mag)[:, 0]

    def gate(self, att, state, q):
        v, bar = state
        w, b = att.abs64, float(att.b64[0])
        wm = np.abs(v) @ w.T
        logit = v @ att.w64.T + b
        bar_logit = (bar + self.op(v, q)) @ w.T + (att.r + 3.0) * U * (wm + abs(b)) + 2.0 * U * wm
        g = 1.0 / (1.0 + np.exp(-logit))
        bar_g = 0.25 * bar_logit + 4.0 * U * g
        out = v * g
        return (out, g * (bar + self.op(v, q)) + np.abs(v) * bar_g + U * np.abs(out)), logit[:, 0]


def edge_chain(case, precision, act_exps=None, n_live=None):
    """The contract of mdx_egnn_edge_chain on the first n_live edge rows (default: all live ones): dict with `messages`, `scalar`
    and their bars [n_live, H] / [n_live], the logits of the gate, and `positions` (Bars.positions)."""
    L = case.n_message + case.n_coord
    n_live = case.E if n_live is None else n_live
    edges = case.edges[:n_live]
    ar = Bars(precision, L + 2, act_exps, pack_exponents(case.layers, 0, case.w_out))
    x, _ = ar.first_edge_layer(case, edges)
    ar.note(0, x)
    logits = None
    messages = None
    for l in range(L):
        x = ar.silu(ar.linear(case.layers[l], l, x, l))
        ar.note(l + 1, x)
        if l + 1 == case.n_message:
            if case.att is not None:
                x, logits = ar.gate(case.att, x, l + 1)
            messages = ar.output(x, l + 1)
    scalar = ar.head(case.w_out, L, x, L)
    return {"messages": messages[0], "bar_messages": messages[1], "scalar": scalar[0], "bar_scalar": scalar[1],
            "logits": logits, "positions": ar.positions}


def piece_buffer(values64, bars, offsets, degree, capacity):
    """The compact piece buffer of a launch with `capacity` edge rows of which the first len(values64) are live: (pieces, bars)
    float64 [ceil(capacity / 16) + n_nodes, H]; rows no node owns are NaN.  A piece's bar: its members' bars + 4 u sum |m|."""
    n_nodes = len(degree)
    rows = ((capacity + 15) >> 4) + n_nodes
    pieces = np.full((rows, values64.shape[1]), np.nan)
    piece_bars = np.full_like(pieces, np.nan)
    for node in range(n_nodes):
        e0 = int(offsets[node])
        for row, first, end in gc.piece_rows(node, e0, e0 + int(degree[node]), capacity):
            assert np.all(np.isnan(pieces[row])), "two pieces claim one row"
            pieces[row] = values64[first:end].sum(axis=0)
            piece_bars[row] = bars[first:end].sum(axis=0) + 4.0 * U * np.abs(values64[first:end]).sum(axis=0)
    return pieces, piece_bars


def row_chain(x32, layers, precision, residual32=None, act_exps=None):
    """The contract of mdx_mlp_chain_rows: (out, bar, positions)."""
    L = len(layers)
    ar = Bars(precision, L + 2, act_exps, pack_exponents(layers))
    x = ar.rows_in(x32)
    ar.note(0, x)
    for l, layer in enumerate(layers):
        z = ar.linear(layer, l, x, l)
        x = ar.silu(z) if l + 1 < L else ar.identity(z)
        ar.note(l + 1, x)
    out, bar = ar.output(x, L)
    if residual32 is not None:
        out = out + np.asarray(residual32, dtype=np.float32).astype(np.float64)
        bar = bar + U * np.abs(out)
    return out, bar, ar.positions


def node_mlp(h32, agg32, wide, inner, precision, residual, projection=None, act_exps=None):
    """The contract of mdx_node_mlp_rows: wide = (W[:, :H] with the bias, W[:, H:] without), inner = the H -> H layers behind it
    (the last one linear), projection = (W_src, W_dst) without biases or None.  -> (out, bar, proj or None, bar, positions)."""
    image = list(wide) + list(inner) + (list(projection) if projection is not None else [])
    L = 2 + len(inner)
    tied = (1 << 1) | ((1 << (L + 1)) if projection is not None else 0)
    ar = Bars(precision, L + 2, act_exps, pack_exponents(image, tied))
    h, agg = ar.rows_in(h32), ar.rows_in(agg32)
    ar.note(0, h)
    ar.note(0, agg)
    x = ar.silu(ar.linear(wide[1], 1, agg, 0, start=ar.linear(wide[0], 0, h, 0)))
    ar.note(2, x)
    for k, layer in enumerate(inner):
        z = ar.linear(layer, 2 + k, x, 2 + k)
        x = ar.silu(z) if k + 1 < len(inner) else ar.identity(z)
        ar.note(3 + k, x)
    out, bar = ar.output(x, L)
    if residual:
        out = out + h[0]
        bar = bar + U * np.abs(out)
    proj = proj_bar = None
    if projection is not None:
        operand = (out, bar + 3.0 * U * np.abs(out))
        ar.note(L + 1, operand)
        halves = []
        for k, layer in enumerate(projection):
            z, bz, _ = ar.linear(layer, L + k, operand, L + 1)
            halves.append((z, bz + 2.0 * U * np.abs(z)))
        proj = np.concatenate([halves[0][0], halves[1][0]], axis=1)
        proj_bar = np.concatenate([halves[0][1], halves[1][1]], axis=1)
    return out, bar, proj, proj_bar, ar.positions


# ---------------------------------------------------------------------------------------------------------------------------
# binary32 evaluations of the same contracts (the CPU tests hold the bars to them): torch's float32 on the CPU, and a numpy
# emulation of the split -- hi = f16(2^e v), lo = f16(2^e v - hi), three products, binary32 sums
class Torch32:
    def __init__(self, *unused, **unused_too):
        pass

    @staticmethod
    def linear(layer, l, x, q, start=None):
        z = torch.from_numpy(x) @ torch.from_numpy(layer.weight).t()
        if layer.bias is not None:
            z = z + torch.from_numpy(layer.bias)
        z = z.numpy()
        return z if start is None else start + z

    @staticmethod
    def silu(z):
        return torch.nn.functional.silu(torch.from_numpy(np.ascontiguousarray(z))).numpy()

    @staticmethod
    def carried(x, q):
        return x


class Split32:
    """drop = (layer index, "lo_hi"): that layer's (weight lo) x (operand hi) product is left out -- the emulated mutation."""

    def __init__(self, act_exps, weight_exps, drop=None):
        self.act_exps, self.weight_exps, self.drop = act_exps, weight_exps, drop

    @staticmethod
    def halves(scaled):
        hi = scaled.astype(np.float16)
        lo = (scaled - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float32), lo.astype(np.float32)

    def linear(self, layer, l, x, q, start=None):
        a, e = self.weight_exps[l], self.act_exps[q]
        xh, xl = self.halves(x * np.float32(2.0 ** e))
        wh, wl = self.halves(layer.weight * np.float32(2.0 ** a))
        acc = np.zeros((x.shape[0], layer.weight.shape[0]), dtype=np.float32) if start is None else start
        if layer.bias is not None:
            acc = acc + layer.bias * np.float32(2.0 ** (a + e))
        acc = acc + xh @ wh.T
        acc = acc + xl @ wh.T
        if self.drop != (l, "lo_hi"):
            acc = acc + xh @ wl.T
        assert acc.dtype == np.float32
        return acc

    def unscale(self, acc, l, q):
        return acc * np.float32(2.0 ** -(self.weight_exps[l] + self.act_exps[q]))

    @staticmethod
    def silu(z):
        z = z.astype(np.float32)
        return (z / (np.float32(1.0) + np.exp(-z))).astype(np.float32)

    def carried(self, x, q):
        scale = np.float32(2.0 ** self.act_exps[q])
        hi, lo = self.halves(x * scale)
        return (hi + lo) / scale


def row_chain32(x32, layers, residual32=None, split=None):
    """mdx_mlp_chain_rows in binary32: torch's float32 (split=None) or the emulated split (a Split32)."""
    ar = split if split is not None else Torch32()
    L = len(layers)
    x = np.asarray(x32, dtype=np.float32)
    for l, layer in enumerate(layers):
        z = ar.linear(layer, l, x, l)
        if split is not None:
            z = split.unscale(z, l, l)
        x = ar.silu(z) if l + 1 < L else z
    out = ar.carried(x, L)
    return out if residual32 is None else np.asarray(residual32, dtype=np.float32) + out


def edge_chain32(case, split=None):
    """mdx_egnn_edge_chain in binary32 on the live edges: (messages, scalar)."""
    ar = split if split is not None else Torch32()
    H, L = case.H, case.n_message + case.n_coord
    edges = case.edges[:case.E]
    src, dst = edges[:, 0], edges[:, 1]
    diff = case.coord[src] - case.coord[dst]
    radial = np.zeros(case.E, dtype=np.float32)
    for k in range(case.D):
        radial = radial + diff[:, k] * diff[:, k]
    z = ((case.node_proj[src, :H] + case.node_proj[dst, H:]) + case.bias_in[None, :]) + radial[:, None] * case.w_radial[None, :]
    x = ar.silu(z)
    messages = None
    for l in range(L):
        z = ar.linear(case.layers[l], l, x, l)
        if split is not None:
            z = split.unscale(z, l, l)
        x = ar.silu(z)
        if l + 1 == case.n_message:
            if case.att is not None:
                m = ar.carried(x, l + 1)
                logit = m @ case.att.weight.T + case.att.bias
                x = (m * (np.float32(1.0) / (np.float32(1.0) + np.exp(-logit)))).astype(np.float32)
            messages = ar.carried(x, l + 1)
    s = ar.linear(case.w_out, L, x, L)
    if split is not None:
        s = split.unscale(s, L, L)
    assert messages.dtype == np.float32 and s.dtype == np.float32
    return messages, s[:, 0]


def node_mlp32(h32, agg32, wide, inner, residual, projection=None, split=None):
    ar = split if split is not None else Torch32()
    L = 2 + len(inner)
    h, agg = np.asarray(h32, dtype=np.float32), np.asarray(agg32, dtype=np.float32)
    z = ar.linear(wide[1], 1, agg, 0, start=ar.linear(wide[0], 0, h, 0))
    if split is not None:
        z = split.unscale(z, 0, 0)
    x = ar.silu(z)
    for k, layer in enumerate(inner):
        z = ar.linear(layer, 2 + k, x, 2 + k)
        if split is not None:
            z = split.unscale(z, 2 + k, 2 + k)
        x = ar.silu(z) if k + 1 < len(inner) else z
    out = ar.carried(x, L)
    if residual:
        out = h + out
    proj = None
    if projection is not None:
        halves = []
        for k, layer in enumerate(projection):
            z = ar.linear(layer, L + k, out, L + 1)
            halves.append(split.unscale(z, L + k, L + 1) if split is not None else z)
        proj = np.concatenate(halves, axis=1)
    return out, proj


# ---------------------------------------------------------------------------------------------------------------------------
# the cases both test files walk
ROW_WIDTHS = WIDTHS
ROW_LAYERS = (1, 2, 3, 16)
ROW_COUNTS = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129)
PARITIES = [(m, c) for m in (1, 2, 3) for c in (1, 2, 3)] + [(8, 8)]
DIMENSIONS = (1, 2, 3, 4, 6, 8)
EDGE_WIDTHS = (32, 256)
PADDED_WIDTHS = [(16, 32), (48, 80), (160, 256), (32, 16)]
NODE_INNER = (0, 1, 4)


def row_inputs(H, M, seed):
    """x [M, H] and a residual [M, H] of order one; row M - 1 is like no other row (the ragged lanes are clamped to it)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-2.0, 2.0, size=(M, H)).astype(np.float32)
    res = rng.uniform(-2.0, 2.0, size=(M, H)).astype(np.float32)
    assert M == 1 or not np.any(np.all(x[:-1] == x[-1], axis=1))
    return x, res


@functools.lru_cache(maxsize=None)
def row_layers(H, n_layers):
    return tuple(layer_stack(H, n_layers, 3 * H + n_layers))


def dimension_of(H, n_message, n_coord):
    """Every coordinate dimension of DIMENSIONS appears among the parity classes of either width."""
    return DIMENSIONS[(PARITIES.index((n_message, n_coord)) + (0 if H == 32 else 3)) % len(DIMENSIONS)]


@functools.lru_cache(maxsize=None)
def edge_case(H, n_message, n_coord, ordering, capacity_extra=0, attention=False, widths=None):
    seed = 100 * H + 10 * n_message + n_coord + (5000 if ordering == "shuffled" else 0)
    width = H if widths is None else next(w for w in WIDTHS if w >= max(widths))
    return EdgeCase(width, n_message, n_coord, dimension_of(H, n_message, n_coord), gc.ORDERINGS[ordering], seed,
                    capacity_extra=capacity_extra, attention=attention, widths=widths)


@functools.lru_cache(maxsize=None)
def node_case(H, n_inner, projection, uneven=False):
    """wide = two halves, inner = n_inner SiLU layers and the linear last one, projection = two layers or None; uneven: the second
    half's weights are 2^-10 of the first's (the tied exponent then costs it its low bits: the floor term must cover that)."""
    seed = 7 * H + n_inner
    a = sparse_layer(H, 4, seed, "rotation8", row_sum=0.25)
    b = sparse_layer(H, 4, seed + 1, "reversal", row_sum=0.25, with_bias=False)
    if uneven:
        b = SparseLayer(b.weight * np.float32(2.0 ** -10), None, b.r, b.kind)
    inner = tuple(layer_stack(H, n_inner + 1, seed + 2))
    proj = (sparse_layer(H, 2, seed + 3, "rotation4", with_bias=False),
            sparse_layer(H, 4, seed + 4, "identity", with_bias=False)) if projection else None
    return (a, b), inner, proj


def node_inputs(H, M, seed, agg_scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-2.0, 2.0, size=(M, H)).astype(np.float32),
            (rng.uniform(-2.0, 2.0, size=(M, H)) * agg_scale).astype(np.float32))


def multi_tile_rows(n_cus, multiple=2):
    """multiple x CUs + 8 full tiles and a ragged one of 37 rows."""
    return TILE * (multiple * n_cus + 8) + 37


def sharpness(values, bars):
    """The median of bar / |value| over the non-zero outputs."""
    values, bars = np.asarray(values).reshape(-1), np.asarray(bars).reshape(-1)
    keep = np.isfinite(values) & (values != 0.0)
    return float(np.median(bars[keep] / np.abs(values[keep])))
