"""E(n)-equivariant graph network used as a score network backbone (PyTorch forward).

Same architecture and parameter names (state_dict keys) as the reference's EGNN / E_GCL
(src/.../models/egnn.py:20-385; Satorras et al., arXiv:2102.09844), so reference checkpoints load unchanged.
Written for sorted edge lists (edges grouped by source node, which is what the HIP radius-graph kernel and
get_edges_batch produce):
  * segment sums over sorted edges use torch.segment_reduce -- no atomics, run-to-run deterministic;
  * the first message layer is applied per NODE and gathered per edge (W [h_i | h_j | r] = W_i h_i + W_j h_j + w_r r),
    which removes the [E, 2H+1] concatenation and 2/5 of the message-MLP FLOPs;
  * on device tensors the two per-node reductions run as one-wavefront-per-node HIP kernels over the sorted segments
    (kernels.segment_rows for the messages; kernels.egnn_coord_head = last coordinate layer H -> 1, product with
    coord_diff and segment mean in one pass over the [E, H] activations);
  * on device tensors, without autograd, the whole per-edge part of a layer -- first message layer, the message MLP,
    the attention gate, the coordinate MLP and its H -> 1 head -- is ONE hand-written MFMA kernel (kernels.egnn_edge_chain,
    csrc/mdx_egnn_chain.hip) that keeps the [E, H] activations in registers between layers; `tanh` and `normalize` act in
    the per-node kernel that adds the coordinate updates up; `edge_chain_precision` selects exact binary32 MFMA ("f32") or
    the split-f16 three-product form ("f16x3"); None keeps the per-layer PyTorch path (also taken for shapes the kernel does
    not cover: widths above 256, other activations).  Narrow and unequal message / coordinate widths (the reference's defaults
    are 16 / 32) run on the chain zero-padded to its next width.

The HIP calls are invisible to autograd, so they are used only when no gradient can be requested (torch.no_grad(), or
nothing requires grad); with autograd on, the module runs as plain PyTorch.  Callers that pass their own edge list
(no `degree`) get it sorted by source here first: the segment kernels need that order, the reference's
unsorted_segment_sum accepted any.

What a layer launches is decided once per forward, by E_GCL.route() -> Route, and executed by E_GCL.run(): no other part of a
forward asks for a pack or looks at a shape (inside route(), _node_mlp_pack asks for the next layer's edge pack, whose
projection it appends).  `fused`: device tensors and no gradient can be requested; H: the chain's width; E: edge rows.
The first row whose condition holds is taken:

  edge part (RoutePath.edge)
    "table"          the caller asks for it, and the chain applies, without attention, with in-kernel sums, at full message
                     width, feature width == H <= 256, D <= 8, a status word, n_nodes < 2^31:
                     [the grid's egnn_node_inputs, by the score network], egnn_edge_chain (keyed, on the grid),
                     egnn_table_check, egnn_table_gather
    "chain"          fused, offsets, E > 0, edge_chain_precision set, Linear / SiLU stacks of a width the kernel has (narrow or
                     unequal widths zero-padded; attention only with in-kernel sums): [linear: the per-node projections, unless
                     the previous layer's node kernel made them], egnn_edge_chain, then the reduction below
    "torch"          otherwise: PyTorch -- with fused, message width % 4 == 0 and SiLU first, the first message layer is
                     linear (per node) + egnn_message_input (RoutePath.message_input)
  message sums (RoutePath.sums)
    "table" / "pieces" / "rows"  by the table gather / inside the chain kernel as piece sums (the pack's LDS allows them,
                     n_nodes < 2^31) / by segment_rows afterwards (chain without piece sums; PyTorch edge part with fused,
                     offsets and message width % 4 == 0);   "torch": segment_reduce
  per-node reductions (RoutePath.reduce)
    "gather"         table, or chain with piece sums at full message width, feature width == H, D <= 8:
                     ONE launch (egnn_table_gather / egnn_node_gather)
    "aggregate"      any other chain: egnn_coord_aggregate, segment_combine (piece sums) or segment_rows, cat
                     (RoutePath.sliced, a padded chain: the cat takes the sums' first message_width columns)
    "coord_head"     PyTorch edge part with segment_rows and a plain H -> 1 head behind SiLU: egnn_coord_head;   "torch"
  node part (RoutePath.node)
    "none"           RoutePath.coords_only (asked for, chain + gather, no attention): the gather runs without its message half,
                     h comes back None
    "pack"           after a gather, a node MLP NodeMlpPack covers at the feature width: node_mlp_rows -- with the next
                     layer's projections (RoutePath.projects_next) when that layer has a chain pack of the same width, and h
                     read through the nodes' classes (RoutePath.class_rows) when asked for on the table
    "rows"           RowChainPack covers the MLP after its first layer: linear + silu, mlp_chain_rows
    "torch"          otherwise (always behind a PyTorch edge part)
"""
from typing import Callable, List, NamedTuple, Optional, Tuple

import torch
from torch import nn

from .. import kernels
from ..namespace import AXL


def run_mlp(layers, x: torch.Tensor) -> torch.Tensor:
    """Apply a Sequential of Linear / SiLU / ... modules as plain PyTorch ops (layer shapes the MFMA chains do not cover)."""
    for layer in layers:
        x = layer(x)
    return x


class RoutePath(NamedTuple):
    """What one E_GCL forward launches, in plain words (the table in the module docstring)."""
    edge: str                       # "torch" | "chain" | "table"
    sums: str                       # "torch" | "rows" | "pieces" | "table"
    reduce: str                     # "torch" | "coord_head" | "aggregate" | "gather"
    sliced: bool = False
    node: str = "torch"             # "torch" | "rows" | "pack" | "none"
    coords_only: bool = False
    class_rows: bool = False
    projects_next: bool = False
    message_input: bool = False


class Route(NamedTuple):
    """E_GCL.route()'s answer: the path and the packs it selected (node_pack: the NodeMlpPack of node == "pack", the
    RowChainPack of "rows").  Good for the forward it was made for: the packs follow the parameters."""
    path: RoutePath
    edge_pack: Optional[kernels.EdgeChainPack] = None
    node_pack: Optional[kernels.ChainPack] = None


def segment_sum_sorted(data: torch.Tensor, degree: torch.Tensor) -> torch.Tensor:
    """Sum rows of `data` over consecutive segments of lengths `degree` (edges sorted by source node).

    Replaces unsorted_segment_sum (src/.../models/egnn_utils.py:11-38) for sorted edge lists."""
    return torch.segment_reduce(data, "sum", lengths=degree, axis=0, unsafe=True)


class LayerDeviceState:
    """Everything an E_GCL owns on the device for the fused path; plain Python, one object per layer, never copied or
    pickled with it (the packs hold raw pointers: a copy of the layer starts with an empty one and rebuilds on first use).
      packs      kind ("edge", "rows", "node") -> precision -> (stamp, pack): one kernels.EdgeChainPack / RowChainPack /
                 NodeMlpPack per precision
      in_use     kind -> (stamp, pack): what the last request of that kind selected
      scales     (kind, n_layers, device) -> kernels.ActivationScales, shared by the kind's packs of every precision
      memos      the kernels.EgnnTableMemo of the layer as a first graph layer, by shape, device and precision;
                 memo_used: the one the last table forward ran on; table_worst: its midpoint-check result (device)"""
    KINDS = ("edge", "rows", "node")

    def __init__(self):
        self.packs = {kind: {} for kind in self.KINDS}
        self.in_use = {kind: (None, None) for kind in self.KINDS}
        self.scales, self.memos = {}, {}
        self.memo_used = self.table_worst = None

    def pack(self, kind: str, precision: str, stamp, build):
        """The pack of `kind` for `precision` and `stamp`, from build() when none is kept.  A pack a captured iteration may
        point at is never freed by a precision switch: the generator's one-iteration switch to "f32" and back selects among
        the kept entries and repacks nothing, and only a new stamp replaces an entry -- that of its own precision."""
        if self.in_use[kind][0] != stamp:
            kept = self.packs[kind]
            if kept.get(precision, (None, None))[0] != stamp:
                kept[precision] = (stamp, build())
            self.in_use[kind] = kept[precision]
        return self.in_use[kind][1]


class E_GCL(nn.Module):
    """One equivariant convolution layer (egnn.py:20-289)."""

    def __init__(self, input_size: int, output_size: int, message_n_hidden_dimensions: int,
                 message_hidden_dimensions_size: int, node_n_hidden_dimensions: int, node_hidden_dimensions_size: int,
                 coordinate_n_hidden_dimensions: int, coordinate_hidden_dimensions_size: int,
                 act_fn: Callable = nn.SiLU(), residual: bool = True, attention: bool = False,
                 normalize: bool = False, coords_agg: str = "mean", message_agg: str = "mean", tanh: bool = False):
        super().__init__()
        if coords_agg not in ("mean", "sum"):
            raise ValueError(f"coords_agg should be mean or sum. Got {coords_agg}")
        if message_agg not in ("mean", "sum"):
            raise ValueError(f"message_agg should be mean or sum. Got {message_agg}")
        self.residual, self.attention, self.normalize, self.tanh = residual, attention, normalize, tanh
        self.coords_mean = coords_agg == "mean"
        self.message_mean = message_agg == "mean"
        self.epsilon = 1e-8
        self.input_size = input_size
        self.use_fused_ops = True        # device tensors only; the CPU path is plain PyTorch
        # "f16x3" (default: split-f16 MFMA, binary32-level accuracy -- measured against fp64 in tests/test_egnn_chain_gpu.py --
        # at 2.7x the speed; a value beyond the f16 range is reported and the generator recomputes with "f32"),
        # "f32" (exact binary32 MFMA) or None (per-layer library GEMMs)
        self.edge_chain_precision = "f16x3"
        self.status_word = None          # device int32 word for MDX_STATUS_EGNN_F16_RANGE (set by the score network)
        self._device_state = LayerDeviceState()

        mh, nh, ch = message_hidden_dimensions_size, node_hidden_dimensions_size, coordinate_hidden_dimensions_size
        layers = [nn.Linear(2 * input_size + 1, mh), act_fn]
        for _ in range(message_n_hidden_dimensions):
            layers += [nn.Linear(mh, mh), act_fn]
        self.message_mlp = nn.Sequential(*layers)

        layers = [nn.Linear(input_size + mh, nh), act_fn]
        for _ in range(node_n_hidden_dimensions):
            layers += [nn.Linear(nh, nh), act_fn]
        layers.append(nn.Linear(nh, output_size))
        self.node_mlp = nn.Sequential(*layers)

        layers = [nn.Linear(mh, ch), act_fn]
        for _ in range(coordinate_n_hidden_dimensions):
            layers += [nn.Linear(ch, ch), act_fn]
        layers.append(nn.Linear(ch, 1, bias=False))
        if tanh:
            layers.append(nn.Tanh())
        self.coord_mlp = nn.Sequential(*layers)

        if attention:
            self.att_mlp = nn.Sequential(nn.Linear(mh, 1), nn.Sigmoid())

    def __getstate__(self):
        """Copies and pickles of the module (copy.deepcopy, torch.save of a whole model) carry no device state."""
        return {**self.__dict__, "_device_state": LayerDeviceState(), "status_word": None}

    @property
    def device_state(self) -> LayerDeviceState:
        """(created here for a module unpickled without one: an older pickle, or the reference's)"""
        state = self.__dict__.get("_device_state")
        if state is None:
            state = self.__dict__["_device_state"] = LayerDeviceState()
        return state

    # (stamp, pack) of the kernels.EdgeChainPack, the RowChainPack (the node MLP after its first layer) and the NodeMlpPack (the
    # whole node MLP) the last forward selected; (None, None) before the first
    _chain = property(lambda self: self.device_state.in_use["edge"])
    _node_chain = property(lambda self: self.device_state.in_use["rows"])
    _node_mlp = property(lambda self: self.device_state.in_use["node"])
    _node_chain_kept = property(lambda self: self.device_state.packs["rows"])
    _activation_scales = property(lambda self: self.device_state.scales)
    _table_memos = property(lambda self: self.device_state.memos)
    table_worst = property(lambda self: self.device_state.table_worst)

    def _scales(self, kind: str, n_layers: int, device):
        """kernels.ActivationScales of one of the layer's chains ("edge", "node", "rows"): the per-position powers of two of
        the split-f16 kernels and the maxima the exact-f32 kernels collect, shared by the chain's packs of every precision
        and kept across repacks (an exponent only ever goes down)."""
        kept = self.device_state.scales
        key = (kind, n_layers, str(device))
        if key not in kept:
            kept[key] = kernels.ActivationScales(n_layers, device)
        return kept[key]

    def adapt_f16_range(self):
        """After an exact-f32 pass (the generator's answer to an f16-range report): turn the maxima that pass collected into
        activation exponents for the split-f16 kernels (device-side, no host read)."""
        for scales in self.device_state.scales.values():
            scales.adapt()
        self.reset_table_memos()

    def begin_f16_range_fallback(self):
        """Before the exact-f32 pass of a fallback: forget the maxima earlier f32 launches have left."""
        for scales in self.device_state.scales.values():
            scales.maxima.zero_()
        self.reset_table_memos()       # (a skipped build would also skip its share of the maxima)

    def reset_f16_range(self):
        """Back to the default activation exponents (and no collected maxima): what a freshly built layer has."""
        for scales in self.device_state.scales.values():
            scales.reset()
        self.reset_table_memos()

    def table_memo(self, pack, n_classes: int, n_even: int, embedding_width: int, coord_dimension: int, device, stamp):
        """The kernels.EgnnTableMemo of this layer as a first graph layer: one per device, precision and grid shape, kept (a
        captured iteration holds its pointers).  `stamp`: whatever the table's arithmetic depends on besides sigma and the
        activation exponents -- this layer's pack is added here; when it differs from the stamp of the last call, the key is
        reset (a fill on the stream)."""
        state = self.device_state
        key = (pack.precision, n_classes, n_even, pack.hidden, embedding_width, coord_dimension, str(device))
        memo = state.memos.get(key)
        if memo is None:
            memo = state.memos[key] = kernels.EgnnTableMemo(n_classes, n_even, pack.hidden, embedding_width, coord_dimension, device)
        stamp = (self._chain[0], stamp)
        if memo.stamp != stamp or state.memo_used is not memo:
            # (also after a forward of another precision: the switch to "f32" and back around a range report)
            if memo.stamp is not None:
                memo.reset()
            memo.stamp = stamp
            state.memo_used = memo
        return memo

    def table_builds(self) -> int:
        """Distance tables built so far by this layer, over all its memos (host reads: tests and evidence)."""
        return sum(memo.builds() for memo in self.device_state.memos.values())

    def reset_table_memos(self):
        """Forget every kept distance table (the activation exponents or maxima changed, or the caller wants a fresh build)."""
        for memo in self.device_state.memos.values():
            memo.reset()

    def _messages(self, h: torch.Tensor, edge_index: torch.Tensor, radial: torch.Tensor, message_input: bool) -> torch.Tensor:
        """The message MLP in PyTorch; message_input (RoutePath's): its first layer and SiLU as kernels.egnn_message_input."""
        first = self.message_mlp[0]
        n_in = self.input_size
        w = first.weight
        mh = w.shape[0]
        # node-level projections h W_src^T | h W_dst^T, combined per edge
        proj = torch.nn.functional.linear(h, torch.cat([w[:, :n_in], w[:, n_in:2 * n_in]], dim=0))
        rest = list(self.message_mlp)[1:]
        if message_input:
            out = kernels.egnn_message_input(proj.contiguous(), edge_index, radial.reshape(-1).contiguous(), first.bias,
                                             w[:, 2 * n_in].contiguous(), silu=True)
            rest = rest[1:]
        else:
            row, col = edge_index[:, 0], edge_index[:, 1]
            pre = proj[:, :mh].index_select(0, row) + proj[:, mh:].index_select(0, col)
            out = torch.addcmul(pre + first.bias, radial, w[:, 2 * n_in].unsqueeze(0))
        out = run_mlp(rest, out)
        if self.attention:
            out = out * self.att_mlp(out)
        return out

    # ---- the layer's public pieces under the reference's names (src/models/egnn.py:136-262): plain PyTorch, any edge order.
    # forward() below does not come through them on the GPU (one MFMA kernel per layer); composed as the reference's forward
    # composes them they give the same function (tests/test_host_cpu.py::test_e_gcl_public_pieces_compose_to_forward).
    def message_model(self, source: torch.Tensor, target: torch.Tensor, radial: torch.Tensor) -> torch.Tensor:
        """m_ij = phi_e(h_i, h_j, |x_i - x_j|^2), gated by its own attention value when `attention`."""
        out = self.message_mlp(torch.cat([source, target, radial], dim=1))
        return out * self.att_mlp(out) if self.attention else out

    def node_model(self, x: torch.Tensor, edge_index: torch.Tensor, messages: torch.Tensor) -> torch.Tensor:
        """h_i' = phi_h(h_i, sum or mean over the edges of source i of m_ij) (+ h_i when `residual`)."""
        from .egnn_utils import unsorted_segment_mean, unsorted_segment_sum
        reduce = unsorted_segment_mean if self.message_mean else unsorted_segment_sum
        out = self.node_mlp(torch.cat([x, reduce(messages, edge_index[:, 0], num_segments=x.size(0))], dim=1))
        return x + out if self.residual else out

    def coord_model(self, coord: torch.Tensor, edge_index: torch.Tensor, coord_diff: torch.Tensor,
                    messages: torch.Tensor) -> torch.Tensor:
        """x_i += sum or mean over the edges of source i of (x_i - x_j) phi_x(m_ij) -- IN PLACE, as the reference."""
        from .egnn_utils import unsorted_segment_mean, unsorted_segment_sum
        reduce = unsorted_segment_mean if self.coords_mean else unsorted_segment_sum
        coord += reduce(coord_diff * self.coord_mlp(messages), edge_index[:, 0], num_segments=coord.size(0))
        return coord

    def coord2radial(self, edge_index: torch.Tensor, coord: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(|x_i - x_j|^2 [E, 1], x_i - x_j [E, d]); with `normalize` the difference is scaled by normalize_radial_norm."""
        coord_diff = coord[edge_index[:, 0]] - coord[edge_index[:, 1]]
        radial = torch.sum(coord_diff ** 2, 1).unsqueeze(1)
        if self.normalize:
            coord_diff = self.normalize_radial_norm(radial) * coord_diff
        return radial, coord_diff

    def normalize_radial_norm(self, radial_norm_squared: torch.Tensor) -> torch.Tensor:
        """tanh(r^2) / sqrt(r^2 + epsilon^2): the scaled difference goes to 0 like r^2 at contact and to unit length far away."""
        return torch.tanh(radial_norm_squared) / torch.sqrt(radial_norm_squared + self.epsilon ** 2)

    def _chain_modules(self):
        """(first message layer, message H->H layers, coordinate H->H layers, coordinate head) if the per-edge MLPs have
        the Linear / SiLU alternation the fused kernel implements, else None.  The layer's options ride along: `tanh` is the
        nn.Tanh behind the head (applied where the head's scalar is consumed), `normalize` a per-edge factor there too,
        `attention` the gate inside the kernel (_attention_layer)."""
        message, coordinate = list(self.message_mlp), list(self.coord_mlp)
        if self.tanh:
            if not coordinate or not isinstance(coordinate[-1], nn.Tanh):
                return None
            coordinate = coordinate[:-1]
        if self.attention and self._attention_layer() is None:
            return None
        if len(message) % 2 or len(coordinate) % 2 == 0:
            return None
        pairs = list(zip(message[0::2], message[1::2])) + list(zip(coordinate[0:-1:2], coordinate[1:-1:2]))
        if not all(isinstance(lin, nn.Linear) and isinstance(act, nn.SiLU) for lin, act in pairs):
            return None
        if not isinstance(coordinate[-1], nn.Linear):
            return None
        return message[0], message[2::2], coordinate[0:-1:2], coordinate[-1]

    def _attention_layer(self):
        """att_mlp's nn.Linear(H, 1) when the gate has the reference's form Linear + Sigmoid, else None."""
        att = list(getattr(self, "att_mlp", []))
        if len(att) == 2 and isinstance(att[0], nn.Linear) and isinstance(att[1], nn.Sigmoid) and att[0].out_features == 1 \
                and att[0].bias is not None:
            return att[0]
        return None

    def _coord_flags(self) -> int:
        return kernels.coord_flags(self.normalize, self.tanh)

    def _edge_chain_pack(self):
        """The layer's kernels.EdgeChainPack, rebuilt when a parameter, the device or the precision changed; None when
        the fused kernel does not apply."""
        precision = self.edge_chain_precision
        modules = self._chain_modules() if precision is not None else None
        if modules is None:
            return None
        if not kernels.EdgeChainPack.supported(*modules):
            return None
        attention = self._attention_layer() if self.attention else None
        if attention is not None and attention.in_features != modules[0].out_features:
            return None
        linears = [modules[0], *modules[1], *modules[2], modules[3]] + ([attention] if attention is not None else [])
        stamp = (precision,) + kernels.parameter_stamp(*(t for lin in linears for t in (lin.weight, lin.bias)))
        pack = self.device_state.pack("edge", precision, stamp, lambda: kernels.EdgeChainPack(
            *modules, input_size=self.input_size, precision=precision, attention_layer=attention,
            scales=self._scales("edge", len(modules[1]) + len(modules[2]), modules[0].weight.device)))
        if attention is not None and not pack.piece_sums_ok:
            return None          # (the gate is instantiated for the in-kernel message sums only: mdx_egnn_edge_chain)
        return pack

    def _node_linears(self):
        """The node MLP's nn.Linear layers when the fused path is on and the stack is Linear / SiLU alternation ending in a
        Linear (two Linears at least), else None."""
        node = list(self.node_mlp)
        if self.edge_chain_precision is None or len(node) < 3 or len(node) % 2 == 0:
            return None
        linears, acts = node[0::2], node[1::2]
        if not all(isinstance(lin, nn.Linear) for lin in linears) or not all(isinstance(a, nn.SiLU) for a in acts):
            return None
        return linears

    def _node_chain_pack(self):
        """kernels.RowChainPack of the node MLP's H -> H layers (all but its first, 2H -> H, layer), or None when the stack
        is not Linear / SiLU alternation of equal widths ending in a Linear."""
        linears = self._node_linears()
        if linears is None:
            return None
        rest = linears[1:]
        if linears[0].out_features != rest[0].in_features or not kernels.RowChainPack.supported(rest):
            return None
        precision = self.edge_chain_precision
        stamp = (precision,) + kernels.parameter_stamp(*(t for lin in rest for t in (lin.weight, lin.bias)))
        return self.device_state.pack("rows", precision, stamp, lambda: kernels.RowChainPack(
            rest, precision, scales=self._scales("rows", len(rest), rest[0].weight.device)))

    def _node_mlp_pack(self, next_layer=None):
        """kernels.NodeMlpPack of the WHOLE node MLP (Linear(2H, H) first), or None when it does not have that shape; with
        the per-node projections of `next_layer` appended when that layer runs the fused edge chain on the same width."""
        linears = self._node_linears()
        if linears is None or not kernels.NodeMlpPack.supported(linears):
            return None
        next_pack = next_layer._edge_chain_pack() if next_layer is not None and next_layer.use_fused_ops else None
        projection = None
        if next_pack is not None and tuple(next_pack.proj_weight.shape) == (2 * linears[0].out_features, linears[0].out_features) \
                and next_pack.hidden == linears[0].out_features and next_pack.message_width == next_pack.hidden:
            projection = next_pack.proj_weight
        first_next = next_layer.message_mlp[0].weight if projection is not None else None
        precision = self.edge_chain_precision
        stamp = (precision,) + kernels.parameter_stamp(*(t for lin in linears for t in (lin.weight, lin.bias)), first_next)
        return self.device_state.pack("node", precision, stamp, lambda: kernels.NodeMlpPack(
            linears, precision, next_projection=projection,
            scales=self._scales("node", kernels.NodeMlpPack.n_chain_layers(linears), linears[0].weight.device)))

    def _coord_head_is_plain(self) -> bool:
        last = self.coord_mlp[-1]
        return isinstance(last, nn.Linear) and last.out_features == 1 and last.bias is None and \
            last.in_features % 4 == 0 and len(self.coord_mlp) >= 2 and isinstance(self.coord_mlp[-2], nn.SiLU)

    def forward(self, h: torch.Tensor, edge_index: torch.Tensor, coord: torch.Tensor,
                degree: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None,
                n_edges: Optional[torch.Tensor] = None, node_proj: Optional[torch.Tensor] = None,
                next_layer: Optional["E_GCL"] = None, table=None, coords_only: bool = False,
                row_class: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """h [n_nodes, F]; edge_index [E, 2] sorted by column 0; coord [n_nodes, D]; degree [n_nodes] edge counts;
        offsets [n_nodes] = exclusive scan of degree (enables the segment kernels on device tensors); n_edges: int64 [1]
        on the device when edge_index is a capacity-sized list whose first n_edges rows are the edges (fused chain only);
        node_proj: this layer's per-node projections [n_nodes, 2H], when the previous layer's node kernel has already
        computed them; next_layer: the graph layer that follows (run() returns its projections when this layer's node
        kernel computes them; they are dropped here).
        table, coords_only, row_class: what the caller would like (route()); a table or a coords_only that the layer cannot
        honour is ignored, class rows it cannot honour are an error (there is no h per node to fall back to):
        table: kernels.EgnnTable when the caller guarantees what the layer's per-edge output on a distance grid needs (one
        value of h per class, the coordinates a torus uplift): the edge chain then runs on the grid and the edges are
        interpolated from it (_table_gather).
        coords_only: the caller reads the coordinates alone (the last graph layer of a forward whose atom-type logits nobody
        reads: its h feeds the classification head only): (None, coord_out), the same bits in coord_out.
        row_class: int64 [n_nodes], with h = ONE row per class [n_classes, F] -- node i's features are h[row_class[i]], and the
        [n_nodes, F] matrix does not exist: the layer reads h in its node kernel alone, through the index."""
        if degree is None:
            degree = torch.bincount(edge_index[:, 0], minlength=h.shape[0])
        # the HIP calls are invisible to autograd: only when no gradient can be requested
        needs_grad = torch.is_grad_enabled() and (h.requires_grad or coord.requires_grad or
                                                  any(t.requires_grad for t in self.parameters()))
        route = self.route(degree.shape[0], h.shape[1], coord.shape[1], edge_index.shape[0], h.is_cuda and not needs_grad,
                           offsets is not None, next_layer, table is not None, coords_only, row_class is not None)
        out, coord, _ = self.run(route, h, edge_index, coord, degree, offsets, n_edges, node_proj, table, row_class)
        return out, coord

    def route(self, n_nodes: int, width: int, coord_dimension: int, n_edge_rows: int, fused: bool, has_offsets: bool,
              next_layer: Optional["E_GCL"] = None, table: bool = False, coords_only: bool = False,
              class_rows: bool = False) -> Route:
        """What a forward of this shape runs (the table in the module docstring), from shapes and attributes alone: the one
        place that asks for the layer's packs and evaluates what they and the kernels cover.
        width: h's; fused: device tensors and no gradient can be requested; has_offsets: forward's `offsets` are there;
        table, coords_only, class_rows: the caller's wishes -- granted where the table says so, else dropped: read the answer
        in the path (a caller with class rows asks BEFORE it decides not to make h per node)."""
        fused = fused and self.use_fused_ops
        pack = self._edge_chain_pack() if fused and has_offsets and n_edge_rows > 0 else None
        if pack is None:
            linears = [m for m in self.message_mlp if isinstance(m, nn.Linear)]
            message_input = fused and linears[0].out_features % 4 == 0 and isinstance(self.message_mlp[1], nn.SiLU)
            segments = fused and has_offsets and linears[-1].out_features % 4 == 0
            return Route(RoutePath("torch", "rows" if segments else "torch",
                              "coord_head" if segments and self._coord_head_is_plain() else "torch", message_input=message_input))
        pieces = pack.piece_sums_ok and n_nodes < (1 << 31)     # the messages are added up per node inside the kernel
        full = pack.message_width == pack.hidden                # (else a narrow / unequal-width layer run zero-padded)
        gather_covers = pieces and full and width == pack.hidden and coord_dimension <= 8
        # the chain's ROWS mode has no attention gate; the table gather has the node gather's output contract and reports
        # to the status word
        on_table = table and gather_covers and not self.attention and pack.hidden <= 256 and self.status_word is not None
        edge, sums = ("table", "table") if on_table else ("chain", "pieces" if pieces else "rows")
        if gather_covers and coords_only and not on_table and not self.attention:
            return Route(RoutePath(edge, sums, "gather", node="none", coords_only=True), pack)
        whole = self._node_mlp_pack(next_layer) if gather_covers else None
        if whole is not None and whole.hidden == width:
            return Route(RoutePath(edge, sums, "gather", node="pack", class_rows=class_rows and on_table,
                              projects_next=whole.projects), pack, whole)
        # the node MLP on [h | agg] as one matrix: its first layer in PyTorch, the rest as one launch where a pack covers it
        rows = self._node_chain_pack()
        if rows is not None and self.residual and width != rows.hidden:
            rows = None
        return Route(RoutePath(edge, sums, "gather" if gather_covers else "aggregate", not full,
                          node="torch" if rows is None else "rows"), pack, rows)

    def _table_gather(self, pack, table, left, coord, edge_index, offsets, degree):
        """egnn_node_gather's ([left | message sums] or the sums, coord_out) with the per-edge chain replaced by the chain on the
        distance grid (kernels.egnn_table_grid), its midpoint check (MDX_STATUS_EGNN_TABLE into the status word when it fails
        or sigma is not uniform) and the interpolating gather.  Fixed sizes, no host read: capture-safe."""
        _, grid_coord, grid_edges = kernels.egnn_table_grid(table.n_classes, table.n_even, coord.shape[1], coord.device)
        memo = table.memo
        # the table kept on the device: the chain and the midpoint check return at once while the memo's key holds this forward's
        # sigma; the uniform-sigma check runs regardless (kernels.EgnnTableMemo)
        values, scalars = kernels.egnn_edge_chain(pack, memo.grid_proj, grid_coord, grid_edges, status=self.status_word,
                                                  memo=memo, sigma=table.sigma)
        self.device_state.table_worst = memo.worst
        kernels.egnn_table_check(values, scalars, table.n_classes, table.n_even, table.sigma, memo.workspace,
                                 worst=memo.worst, status=self.status_word, key=memo.key)
        return kernels.egnn_table_gather(values, scalars, table.n_classes, table.n_even, table.atom_types, offsets, degree,
                                         self.message_mean, left, coord, edge_index, self.coords_mean,
                                         flags=self._coord_flags(), status=self.status_word)

    def run(self, route: Route, h, edge_index, coord, degree, offsets=None, n_edges=None, node_proj=None, table=None,
            row_class=None):
        """forward() on `route` (this layer's, for these shapes) -> (h_out, or None with coords_only; coord_out; the next
        layer's per-node projections, or None).  The arguments are forward()'s."""
        path, pack = route.path, route.edge_pack
        assert (row_class is not None) == path.class_rows, "class rows go to a layer whose route reads them, and only there"
        if pack is None:
            return self._run_torch(path, h, edge_index, coord, degree, offsets, n_edges) + (None,)
        coord = coord.contiguous()
        n_rows, flags = edge_index.shape[0], self._coord_flags()
        if path.edge == "table":
            def gather(left):
                return self._table_gather(pack, table, left, coord, edge_index, offsets, degree)
        else:
            # node projections (a PyTorch matmul per node) -> the per-edge work in one MFMA kernel; with piece sums the
            # messages are added up per node inside the kernel and never written out as [E, H]
            proj = node_proj if node_proj is not None else torch.nn.functional.linear(h, pack.proj_weight)
            pieces = path.sums == "pieces"
            messages, edge_scalar = kernels.egnn_edge_chain(pack, proj.contiguous(), coord, edge_index, status=self.status_word,
                                                            n_edges_dev=n_edges, piece_sums=pieces)
            if path.coords_only:
                # the coordinate half of the node gather alone (the same launch with the message half switched off: the same
                # butterfly, the same bits); no node MLP
                return kernels.egnn_node_gather(None, n_rows, offsets, degree, self.message_mean, None, edge_scalar, coord,
                                                edge_index, self.coords_mean, flags=flags) + (None,)

            def gather(left):
                if path.reduce == "gather":
                    return kernels.egnn_node_gather(messages, n_rows, offsets, degree, self.message_mean, left, edge_scalar,
                                                    coord, edge_index, self.coords_mean, flags=flags)
                coord_out = kernels.egnn_coord_aggregate(edge_scalar, coord, edge_index, offsets, degree, self.coords_mean,
                                                         flags=flags)
                agg = (kernels.segment_combine(messages, n_rows, offsets, degree, self.message_mean) if pieces
                       else kernels.segment_rows(messages, offsets, degree, self.message_mean))
                if path.sliced:     # [n_nodes, H] with columns message_width .. H-1 zero: the node MLP takes the real ones
                    agg = agg[:, :pack.message_width]
                return torch.cat([left, agg], dim=1), coord_out
        if path.node == "pack":
            # everything per node between the edge chain and the node MLP in one pass (the message sums and the updated
            # coordinates), then the whole node MLP (its 2H -> H layer included, reading h and the sums as the two halves of
            # its input row: [h | agg] is never formed), the residual and -- when a graph layer follows -- that layer's
            # per-node projections: one launch on the matrix cores
            h = h.contiguous()
            agg, coord_out = gather(None)
            out = kernels.node_mlp_rows(route.node_pack, h, self.residual, status=self.status_word, agg=agg, row_class=row_class)
            out, next_proj = out if path.projects_next else (out, None)
            return out, coord_out, next_proj
        node_in, coord_out = gather(h.contiguous())
        if path.node == "rows":
            # first node layer (2H -> H, + SiLU): a PyTorch matmul per node; the other layers and the residual: one MFMA launch
            first = self.node_mlp[0]
            hidden = torch.nn.functional.silu(torch.nn.functional.linear(node_in, first.weight, first.bias))
            out = kernels.mlp_chain_rows(route.node_pack, hidden, residual=h.contiguous() if self.residual else None,
                                         status=self.status_word)
            return out, coord_out, None
        out = run_mlp(self.node_mlp, node_in)
        return (h + out if self.residual else out), coord_out, None

    def _run_torch(self, path: RoutePath, h, edge_index, coord, degree, offsets, n_edges):
        """run() without an edge chain: PyTorch, any shape, differentiable -- but for the three helper kernels the path names
        (only ever where no gradient can be requested)."""
        assert n_edges is None, "a capacity-sized edge list needs the fused edge chain in every layer"
        row, col = edge_index[:, 0], edge_index[:, 1]
        count = degree.clamp(min=1).to(h.dtype).unsqueeze(1)      # (the reference DIVIDES by the count: egnn_utils.py:66-68)

        coord_diff = coord.index_select(0, row) - coord.index_select(0, col)
        radial = (coord_diff ** 2).sum(dim=1, keepdim=True)
        if self.normalize:
            coord_diff = torch.tanh(radial) / torch.sqrt(radial + self.epsilon ** 2) * coord_diff

        messages = self._messages(h, edge_index, radial, path.message_input)

        if path.reduce == "coord_head":
            hidden = run_mlp(list(self.coord_mlp)[:-1], messages)
            coord = coord + kernels.egnn_coord_head(hidden.contiguous(), self.coord_mlp[-1].weight.reshape(-1),
                                                    coord_diff.contiguous(), offsets, degree, self.coords_mean)
        else:
            trans = segment_sum_sorted(coord_diff * run_mlp(self.coord_mlp, messages), degree)
            coord = coord + (trans / count if self.coords_mean else trans)

        if path.sums == "rows":
            agg = kernels.segment_rows(messages.contiguous(), offsets, degree, self.message_mean)
        else:
            agg = segment_sum_sorted(messages, degree)
            if self.message_mean:
                agg = agg / count
        out = run_mlp(self.node_mlp, torch.cat([h, agg], dim=1))
        return (h + out if self.residual else out), coord


class EGNN(nn.Module):
    """Stack of E_GCL layers with input embedding and node-classification head (egnn.py:292-385)."""

    def __init__(self, input_size: int, num_classes: int, message_n_hidden_dimensions: int,
                 message_hidden_dimensions_size: int, node_n_hidden_dimensions: int, node_hidden_dimensions_size: int,
                 coordinate_n_hidden_dimensions: int, coordinate_hidden_dimensions_size: int,
                 act_fn: Callable = nn.SiLU(), residual: bool = True, attention: bool = False,
                 normalize: bool = False, tanh: bool = False, coords_agg: str = "mean", message_agg: str = "mean",
                 n_layers: int = 4):
        super().__init__()
        self.n_layers = n_layers
        self.embedding_in = nn.Linear(input_size, node_hidden_dimensions_size)
        self.graph_layers = nn.ModuleList([])
        self.node_classification_layer = nn.Linear(node_hidden_dimensions_size, num_classes)
        for _ in range(n_layers):
            self.graph_layers.append(E_GCL(
                input_size=node_hidden_dimensions_size, output_size=node_hidden_dimensions_size,
                message_n_hidden_dimensions=message_n_hidden_dimensions,
                message_hidden_dimensions_size=message_hidden_dimensions_size,
                node_n_hidden_dimensions=node_n_hidden_dimensions,
                node_hidden_dimensions_size=node_hidden_dimensions_size,
                coordinate_n_hidden_dimensions=coordinate_n_hidden_dimensions,
                coordinate_hidden_dimensions_size=coordinate_hidden_dimensions_size,
                act_fn=act_fn, residual=residual, attention=attention, normalize=normalize, coords_agg=coords_agg,
                message_agg=message_agg, tanh=tanh))

    def routes(self, n_nodes: int, coord_dimension: int, n_edge_rows: int, fused, has_offsets: bool, table: bool = False,
               coords_only: bool = False, class_rows: bool = False) -> List[Route]:
        """Every graph layer's E_GCL.route() for a forward of these shapes, each with the layer behind it as its next_layer.
        fused: device tensors and no gradient can be requested -- one answer, or one per layer; table, class_rows: wishes for
        the FIRST layer (it runs on a distance table; h is one row per class); coords_only: for the LAST (nobody reads h)."""
        layers = list(self.graph_layers)
        fused = list(fused) if isinstance(fused, (list, tuple)) else [fused] * len(layers)
        return [layer.route(n_nodes, self.embedding_in.out_features, coord_dimension, n_edge_rows, fused[k], has_offsets,
                            following, table and k == 0, coords_only and following is None, class_rows and k == 0)
                for k, (layer, following) in enumerate(zip(layers, layers[1:] + [None]))]

    def run(self, routes: List[Route], h: torch.Tensor, edges: torch.Tensor, x: torch.Tensor, degree, first_proj=None,
            first_table=None, first_row_class=None) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
        """The graph layers on `routes` (routes() for these shapes) -> (h, or None when the last route is coords_only; x).
        h: embedding_in(node features) already (kernels.egnn_node_inputs); degree: the edge count per node [n_nodes] of a list
        sorted by source, or the triple (degree, offsets, n_edges) of a capacity-sized list (utils/neighbors.get_edges_static).
        For the first layer, where the caller has them: first_proj, its per-node projections [n_nodes, 2H] of h; first_table,
        the kernels.EgnnTable of a "table" route; first_row_class, the nodes' classes of a class_rows route, h then being one
        embedded row per class (E_GCL.forward's node_proj, table and row_class)."""
        n_edges = None
        if isinstance(degree, tuple):
            degree, offsets, n_edges = degree
        else:
            offsets = (torch.cumsum(degree, 0) - degree) if x.is_cuda else None
        proj, table, row_class = first_proj, first_table, first_row_class
        for layer, route in zip(self.graph_layers, routes):
            h, x, proj = layer.run(route, h, edges, x, degree, offsets, n_edges, proj, table, row_class)
            table = row_class = None
        return h, x

    def no_gradient_reaches(self, h: torch.Tensor, x: torch.Tensor) -> List[bool]:
        """Per graph layer: can no gradient be requested through it?  None comes in with h or x, and neither it nor a layer
        before it has a parameter that asks for one (the HIP calls are invisible to autograd)."""
        grad, free = torch.is_grad_enabled(), []
        reached = grad and (h.requires_grad or x.requires_grad)
        for layer in self.graph_layers:
            reached = reached or (grad and any(t.requires_grad for t in layer.parameters()))
            free.append(not reached)
        return free

    def forward(self, h: torch.Tensor, edges: torch.Tensor, x: torch.Tensor, degree=None, routes: Optional[List[Route]] = None,
                first_proj=None, first_table=None, first_row_class=None) -> AXL:
        """degree: None (a caller's own edge list, any order), the edge count per node [n_nodes] of a list sorted by source,
        or the triple (degree, offsets, n_edges) of a capacity-sized list (utils/neighbors.get_edges_static).
        routes: the score network's entrance (a module call, so that forward hooks see it) -- run() with these arguments, on
        inputs it has prepared: A is the last layer's h (the caller applies node_classification_layer: kernels.egnn_outputs),
        L is None."""
        if routes is not None:
            h, x = self.run(routes, h, edges, x, degree, first_proj, first_table, first_row_class)
            return AXL(A=h, X=x, L=None)
        assert first_proj is None and first_table is None and first_row_class is None, "prepared inputs come with routes"
        emb = self.embedding_in
        if h.is_cuda and emb.in_features <= 8:
            # [sigma | one-hot type] -> hidden: with 2-4 input features the library GEMM spends 0.45 ms on a K = 3
            # problem; as rank-1 updates it is a few elementwise passes over [n_nodes, hidden]
            out = emb.bias.unsqueeze(0) + h[:, :1] * emb.weight[:, 0].unsqueeze(0)
            for k in range(1, emb.in_features):
                out = torch.addcmul(out, h[:, k:k + 1], emb.weight[:, k].unsqueeze(0))
            h = out
        else:
            h = emb(h)
        if degree is None:
            # a caller's own edge list: any order is accepted (as by the reference's unsorted_segment_sum); the segment
            # kernels need the edges grouped by source, so sort them (stable: the order within a node is kept)
            edges = edges[torch.argsort(edges[:, 0], stable=True)]
            degree = torch.bincount(edges[:, 0], minlength=h.shape[0])
        fused = [h.is_cuda and free for free in self.no_gradient_reaches(h, x)]
        h, x = self.run(self.routes(h.shape[0], x.shape[1], edges.shape[0], fused, x.is_cuda), h, edges, x, degree)
        return AXL(A=self.node_classification_layer(h), X=x, L=torch.zeros_like(x))
