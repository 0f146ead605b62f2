"""The MFMA chain kernels (csrc/mdx_egnn_chain.hip: mdx_egnn_edge_chain in rows, piece-sums and attention form,
mdx_mlp_chain_rows, mdx_node_mlp_rows(_split), mdx_egnn_chain_pack, mdx_egnn_chain_adapt_activation_exponents), each called through
the C ABI, PER ELEMENT against the float64 restatements of tests/chain_cases.py on sparse contractive chains -- see that module's
docstring for the construction and for the bar, every constant of which was written down before any GPU run
(tests/test_chain_cases_cpu.py holds the restatements and the bars without a GPU).

Every output is a view inside a NaN-filled buffer with 64 guard floats on either side; every comparison is |got - want| <= bar for
every element; each family prints its worst error / bar.  tests/test_egnn_chain_gpu.py keeps the dense random layers: the check of
the arithmetic at full density."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_cases as cc
import gather_cases as gc

pytestmark = pytest.mark.gpu

PAD = 64
LOG2E = 1.4426950408889634
MEASURED = {}
SPLIT_MODES = [p for p in cc.PRECISIONS if p != "f32"]


def _hip():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    return _hip


def _kernels():
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    return kernels


def _dev(array, device):
    return torch.as_tensor(np.ascontiguousarray(array)).to(device)


def _guarded(rows, columns, device):
    """A [rows, columns] output inside a larger NaN-filled buffer: (buffer, view)."""
    buffer = torch.full((rows * columns + 2 * PAD,), float("nan"), dtype=torch.float32, device=device)
    return buffer, buffer[PAD:PAD + rows * columns].view(rows, columns)


def _untouched(buffer, rows, columns):
    return bool(torch.isnan(buffer[:PAD]).all()) and bool(torch.isnan(buffer[PAD + rows * columns:]).all())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _report(family, ratio):
    MEASURED[family] = max(MEASURED.get(family, 0.0), ratio)
    print(f"{family}: worst error / bar {ratio:.3f}")


def _check(family, got, want, bar, where=None):
    """|got - want| <= bar for every element (bar 0: equal), no NaN; reports the worst ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == bar.shape, (got.shape, want.shape, bar.shape)
    assert np.all(np.isfinite(got)), (family, where, np.argwhere(~np.isfinite(got))[:4])
    error = np.abs(got - want)
    exact = bar == 0.0
    assert np.all(error[exact] == 0.0), (family, where)
    ratio = float(np.max(error[~exact] / bar[~exact])) if np.any(~exact) else 0.0
    _report(family, ratio)
    assert ratio <= 1.0, (family, where, ratio, np.argwhere(error > bar)[:4])


def _linear(weight, bias, device):
    module = torch.nn.Linear(weight.shape[1], weight.shape[0], bias=bias is not None)
    with torch.no_grad():
        module.weight.copy_(torch.from_numpy(np.ascontiguousarray(weight)))
        if bias is not None:
            module.bias.copy_(torch.from_numpy(np.ascontiguousarray(bias)))
    return module.to(device)


def _modules(layers, device):
    return [_linear(layer.weight, layer.bias, device) for layer in layers]


def _status(device):
    return torch.zeros(1, dtype=torch.int32, device=device)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. mdx_mlp_chain_rows
def _row_chain(device, pack, x, residual):
    M, H = x.shape
    buffer, out = _guarded(M, H, device)
    status = _status(device)
    _hip().call("mdx_mlp_chain_rows", C.byref(pack.c_struct), _dev(x, device), None if residual is None else _dev(residual, device),
                M, None, out, status)
    got = out.cpu().numpy()
    assert _untouched(buffer, M, H)
    return got, int(status.item())


@pytest.mark.parametrize("precision", cc.PRECISIONS)
@pytest.mark.parametrize("n_layers", cc.ROW_LAYERS)
@pytest.mark.parametrize("H", cc.ROW_WIDTHS)
def test_row_chain_elements(cuda, H, n_layers, precision):
    """mdx_mlp_chain_rows per element: 1 (the purely linear path), 2, 3 and 16 layers of every kind (identity, reversal, rotations
    across a quad, a half, a k-step and a chunk, random columns); M = 1 (one lane), 15 / 16 / 17 (the two column groups of the
    16x16 shape), 31 / 32 / 33 (a wavefront), 127 / 128 / 129 (a tile); with and without residual; nothing past row M is written.
    Measured on an MI355X: at most 0.76 of the bar."""
    layers = cc.row_layers(H, n_layers)
    pack = _kernels().RowChainPack(_modules(layers, cuda), precision)
    for M in cc.ROW_COUNTS:
        x, res = cc.row_inputs(H, M, 17 * H + M)
        for residual in (None, res):
            want, bar, _ = cc.row_chain(x, layers, precision, residual)
            got, status = _row_chain(cuda, pack, x, residual)
            assert status == 0
            _check("row chain", got, want, bar, (M, residual is not None))


# ---------------------------------------------------------------------------------------------------------------------------
# 2 - 5. mdx_egnn_edge_chain
def _edge_pack(case, precision, device, scales=None):
    m, c, n = case.message_width, case.coord_width, case.n_message
    first = np.zeros((m, 3), dtype=np.float32)
    first[:, 2] = case.w_radial[:m]
    message = [_linear(layer.weight[:m, :m], layer.bias[:m], device) for layer in case.layers[:n]]
    coord = [_linear(layer.weight[:c, :(m if k == 0 else c)], layer.bias[:c], device) for k, layer in enumerate(case.layers[n:])]
    attention = None if case.att is None else _linear(case.att.weight[:, :m], case.att.bias, device)
    pack = _kernels().EdgeChainPack(_linear(first, case.bias_in[:m], device), message, coord,
                                    _linear(case.w_out.weight[:, :c], None, device), input_size=1, precision=precision,
                                    scales=scales, attention_layer=attention)
    assert pack.hidden == case.H and pack.piece_sums_ok
    return pack


def _edge_chain(device, pack, case, piece_sums, n_live=None):
    """One launch over all of case.edges as the capacity (the live count on the device when it is smaller) into guarded buffers:
    (messages or pieces, scalar [capacity], status)."""
    capacity, H = case.edges.shape[0], case.H
    n_live = case.E if n_live is None else n_live
    rows = ((capacity + 15) >> 4) + case.n_nodes if piece_sums else capacity
    assert not piece_sums or rows == _hip().lib().mdx_egnn_piece_rows(capacity, case.n_nodes)
    m_buffer, messages = _guarded(rows, H, device)
    s_buffer, scalar = _guarded(capacity, 1, device)
    status = _status(device)
    count = None if n_live == capacity else torch.tensor([n_live], dtype=torch.int64, device=device)
    pack.c_struct.message_mode = 1 if piece_sums else 0
    _hip().call("mdx_egnn_edge_chain", C.byref(pack.c_struct), _dev(case.node_proj, device), _dev(case.coord, device), case.D,
                _dev(case.edges, device), capacity, count, messages, scalar, status)
    got = messages.cpu().numpy(), scalar.cpu().numpy().reshape(-1), int(status.item())
    assert _untouched(m_buffer, rows, H) and _untouched(s_buffer, capacity, 1)
    return got


def _check_pieces(family, got, want, case, where):
    pieces, bars = cc.piece_buffer(want["messages"], want["bar_messages"], case.offsets, case.degree, case.edges.shape[0])
    owned = ~np.isnan(pieces[:, 0])
    assert np.all(np.isnan(got[~owned])), (family, where, "a row no node owns was written")
    _check(family, got[owned], pieces[owned], bars[owned], where)


@pytest.mark.parametrize("precision", cc.PRECISIONS)
@pytest.mark.parametrize("n_message,n_coord", cc.PARITIES)
@pytest.mark.parametrize("H", cc.EDGE_WIDTHS)
def test_edge_chain_elements(cuda, H, n_message, n_coord, precision):
    """mdx_egnn_edge_chain per element, every parity class of (message layers, coordinate layers) -- which operand set the message
    store, the aggregation and the head read -- and coordinate dimensions 1, 2, 3, 4, 6 (the unrolled form), 8 across them; ragged
    sorted graphs (degrees 0 ... 200 in two orders) with self-loops (radial 0) and repeated destinations, one poison node with NaN
    rows that no live edge names.
    Rows mode: messages and the head scalar of every edge; with the live count on the device and 40 more edge rows that name the
    poison node: the same bits inside the count, NaN fill behind it, status 0.
    Piece sums, both orderings: every owned row of the compact buffer against the float64 piece sums, every other row still NaN;
    the head scalars bit-equal to rows mode; with the count below the capacity the last live edge closes its piece in the row the
    CAPACITY's layout gives it, and nothing behind is touched.
    Measured on an MI355X: messages at most 0.22, head scalars 0.08, pieces 0.19 of the bar."""
    scalars = {}
    for ordering in gc.ORDERINGS:
        case = cc.edge_case(H, n_message, n_coord, ordering)
        pack = _edge_pack(case, precision, cuda)
        want = cc.edge_chain(case, precision)
        if ordering == "listed":
            messages, scalar, status = _edge_chain(cuda, pack, case, False)
            assert status == 0
            _check("edge chain messages", messages, want["messages"], want["bar_messages"], ordering)
        pieces, scalar_p, status = _edge_chain(cuda, pack, case, True)
        assert status == 0
        if ordering == "listed":
            assert np.array_equal(_bits(scalar_p), _bits(scalar)), "the head scalar depends on the message mode"
        _check("edge chain head scalar", scalar_p, want["scalar"], want["bar_scalar"], ordering)
        _check_pieces("edge chain pieces", pieces, want, case, ordering)
        scalars[ordering] = scalar_p
        # the live count on the device, below the capacity
        longer = cc.edge_case(H, n_message, n_coord, ordering, capacity_extra=40)
        assert longer.E == case.E and np.array_equal(longer.edges[:case.E], case.edges) and np.all(longer.edges[case.E:] == case.n_nodes - 1)
        if ordering == "listed":
            messages_c, scalar_c, status = _edge_chain(cuda, pack, longer, False)
            assert status == 0
            assert np.array_equal(_bits(messages_c[:case.E]), _bits(messages)) and np.array_equal(_bits(scalar_c[:case.E]), _bits(scalar))
            assert np.all(np.isnan(messages_c[case.E:])) and np.all(np.isnan(scalar_c[case.E:]))
        pieces_c, scalar_c, status = _edge_chain(cuda, pack, longer, True)
        assert status == 0 and np.array_equal(_bits(scalar_c[:case.E]), _bits(scalar_p)) and np.all(np.isnan(scalar_c[case.E:]))
        _check_pieces("edge chain pieces", pieces_c, want, longer, (ordering, "count below capacity"))


@pytest.mark.parametrize("precision", cc.PRECISIONS)
@pytest.mark.parametrize("widths", cc.PADDED_WIDTHS)
def test_padded_widths_elements(cuda, widths, precision):
    """Zero-padded unequal widths through EdgeChainPack (the reference's defaults 16 / 32 among them): message columns m .. H-1
    are exactly 0.0 in rows mode and in every owned piece row; everything else within the bar.
    Measured on an MI355X: at most 0.21 of the bar."""
    m, c = widths
    case = cc.edge_case(0, 2, 2, "listed", widths=widths)
    pack = _edge_pack(case, precision, cuda)
    assert pack.message_width == m and pack.hidden == case.H
    want = cc.edge_chain(case, precision)
    messages, scalar, status = _edge_chain(cuda, pack, case, False)
    assert status == 0 and np.all(_bits(messages[:, m:]) == 0), "a padded message column is not +0.0"
    _check("padded widths", messages[:, :m], want["messages"][:, :m], want["bar_messages"][:, :m])
    _check("padded widths", scalar, want["scalar"], want["bar_scalar"])
    pieces, scalar_p, status = _edge_chain(cuda, pack, case, True)
    owned = ~np.isnan(cc.piece_buffer(want["messages"], want["bar_messages"], case.offsets, case.degree, case.E)[0][:, 0])
    assert status == 0 and np.all(pieces[owned][:, m:] == 0.0) and np.array_equal(_bits(scalar_p), _bits(scalar))
    _check_pieces("padded widths", pieces, want, case, "pieces")


@pytest.mark.parametrize("precision", cc.PRECISIONS)
@pytest.mark.parametrize("n_message,n_coord", cc.PARITIES)
@pytest.mark.parametrize("H", cc.EDGE_WIDTHS)
def test_attention_gate_elements(cuda, H, n_message, n_coord, precision):
    """The attention instantiations per element, every parity class: the gated piece sums and the head scalars (which see the
    gated messages).  A second run with another b_att changes every gated value: the gate's bias is read.  (The spread of the
    logits is what tests/test_chain_cases_cpu.py asserts: about 1.5 is reachable behind one message layer only.)
    Measured on an MI355X: pieces at most 0.07, head scalars 0.07 of the bar."""
    case = cc.edge_case(H, n_message, n_coord, "shuffled", attention=True)
    pack = _edge_pack(case, precision, cuda)
    want = cc.edge_chain(case, precision)
    pieces, scalar, status = _edge_chain(cuda, pack, case, True)
    assert status == 0
    _check("attention head scalar", scalar, want["scalar"], want["bar_scalar"])
    _check_pieces("attention pieces", pieces, want, case, None)
    pack.att_b.add_(0.75)
    pieces_b, scalar_b, status = _edge_chain(cuda, pack, case, True)
    owned = ~np.isnan(pieces[:, 0])
    assert status == 0 and np.all(pieces_b[owned] != pieces[owned])
    # (the head scalars follow, but behind several contracting coordinate layers not in every edge's last bit)
    assert n_coord > 3 or np.any(scalar_b != scalar)


# ---------------------------------------------------------------------------------------------------------------------------
# 6. mdx_node_mlp_rows(_split)
def _node_pack(wide, inner, projection, precision, device, scales=None):
    first = _linear(np.concatenate([wide[0].weight, wide[1].weight], axis=1), wide[0].bias, device)
    proj = None if projection is None else _dev(np.concatenate([projection[0].weight, projection[1].weight], axis=0), device)
    pack = _kernels().NodeMlpPack([first] + _modules(inner, device), precision, next_projection=proj, scales=scales)
    assert pack.projects == (projection is not None)
    return pack


def _node_mlp(device, pack, h, agg, residual, split):
    M, H = h.shape
    o_buffer, out = _guarded(M, H, device)
    p_buffer, proj = _guarded(M, 2 * H, device) if pack.projects else (None, None)
    status = _status(device)
    if split:
        _hip().call("mdx_node_mlp_rows_split", C.byref(pack.c_struct), _dev(h, device), _dev(agg, device), int(residual), M, None,
                    out, proj, status)
    else:
        _hip().call("mdx_node_mlp_rows", C.byref(pack.c_struct), _dev(np.concatenate([h, agg], axis=1), device), int(residual), M,
                    None, out, proj, status)
    assert _untouched(o_buffer, M, H) and (proj is None or _untouched(p_buffer, M, 2 * H))
    return out.cpu().numpy(), None if proj is None else proj.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("precision", cc.PRECISIONS)
@pytest.mark.parametrize("uneven", [False, True])
@pytest.mark.parametrize("n_inner", cc.NODE_INNER)
@pytest.mark.parametrize("H", cc.EDGE_WIDTHS)
def test_node_mlp_elements(cuda, H, n_inner, uneven, precision):
    """mdx_node_mlp_rows per element: `out` and both halves of `proj` (a second pair of sparse layers), 0, 1 and 4 inner layers,
    with and without the residual and the projection, 129 rows; mdx_node_mlp_rows_split gives the same bits.  uneven: the second
    half of the wide first layer has weights 2^-10 of the first half's, so the tied exponent costs it its low bits -- the floor
    term of the bar covers that.
    Measured on an MI355X: out at most 0.37, proj 0.24 of the bar."""
    wide, inner, projection = cc.node_case(H, n_inner, True, uneven)
    h, agg = cc.node_inputs(H, 129, 9 * H + n_inner, agg_scale=32.0 if uneven else 1.0)
    for with_projection in (True, False):
        pack = _node_pack(wide, inner, projection if with_projection else None, precision, cuda)
        for residual in (False, True):
            out, bar, proj, proj_bar, _ = cc.node_mlp(h, agg, wide, inner, precision, residual, projection if with_projection else None)
            got, got_p, status = _node_mlp(cuda, pack, h, agg, residual, False)
            assert status == 0
            _check("node MLP out", got, out, bar, (with_projection, residual))
            if with_projection:
                _check("node MLP proj", got_p, proj, proj_bar, residual)
            got_s, got_ps, status = _node_mlp(cuda, pack, h, agg, residual, True)
            assert status == 0 and np.array_equal(_bits(got_s), _bits(got))
            assert not with_projection or np.array_equal(_bits(got_ps), _bits(got_p))


# ---------------------------------------------------------------------------------------------------------------------------
# 7. more than one tile per workgroup
def _cus(device):
    return int(torch.cuda.get_device_properties(device).multi_processor_count)


@functools.lru_cache(maxsize=None)
def _long_edge_case(H, n_rows, attention):
    return cc.EdgeCase(H, 2, 1, 6 if H == 256 else 3, cc.long_degrees(n_rows), 31 * H + 1, r=2, attention=attention)


@functools.lru_cache(maxsize=None)
def _long_edge_want(H, n_rows, attention, arithmetic):
    return cc.edge_chain(_long_edge_case(H, n_rows, attention), "f32" if arithmetic == "f32" else "f16x3")


@functools.lru_cache(maxsize=None)
def _long_row_want(H, n_rows, arithmetic):
    layers = tuple(cc.layer_stack(H, 3, 5 * H, r=2))
    x, res = cc.row_inputs(H, n_rows, 23)
    return layers, x, res, cc.row_chain(x, layers, "f32" if arithmetic == "f32" else "f16x3", res)[:2]


@functools.lru_cache(maxsize=None)
def _long_node_want(H, n_rows, arithmetic):
    wide, inner, projection = cc.node_case(H, 1, True)
    h, agg = cc.node_inputs(H, n_rows, 29)
    return wide, inner, projection, h, agg, cc.node_mlp(h, agg, wide, inner, "f32" if arithmetic == "f32" else "f16x3", True, projection)[:4]


MULTI_TILE = ([("pieces", H, precision, 2) for H in (256, 32) for precision in cc.PRECISIONS] +
              [("pieces", 32, "f16x3", 3), ("rows", 256, "f16x3", 2), ("row chain", 128, "f16x3", 2), ("row chain", 128, "f32", 2),
               ("node MLP", 256, "f16x3", 2), ("attention", 64, "f16x3", 2)])


@pytest.mark.parametrize("kind,H,precision,multiple", MULTI_TILE)
def test_workgroups_that_run_several_tiles(cuda, kind, H, precision, multiple):
    """What flows from one 128-row tile of a workgroup into its next -- the prefetched fragments, the initial accumulator (layer
    0's bias), the ring slots, the count of pending stores -- per element: multiple x CUs + 8 full tiles and a ragged one of 37
    rows, so that (asserted with chain_cases.workgroup_tiles) some workgroup runs at least `multiple` tiles; piece sums at H = 256
    and 32 in all three precisions, rows mode, the row chain, the node MLP with its projection tail, the attention form.
    Measured on an MI355X: at most 0.46 of the bar (the row chain; pieces 0.17, rows 0.22, node MLP 0.27, attention 0.08)."""
    n_cus = _cus(cuda)
    n_rows = cc.multi_tile_rows(n_cus, multiple)
    assert cc.most_tiles(n_rows, n_cus) >= multiple
    arithmetic = cc.arithmetic(precision)
    family = "several tiles, " + kind
    if kind in ("pieces", "rows", "attention"):
        case = _long_edge_case(H, n_rows, kind == "attention")
        assert case.E == n_rows
        want = _long_edge_want(H, n_rows, kind == "attention", arithmetic)
        pack = _edge_pack(case, precision, cuda)
        got, scalar, status = _edge_chain(cuda, pack, case, kind != "rows")
        assert status == 0
        _check(family, scalar, want["scalar"], want["bar_scalar"], "head scalar")
        if kind == "rows":
            _check(family, got, want["messages"], want["bar_messages"], "messages")
        else:
            _check_pieces(family, got, want, case, "pieces")
    elif kind == "row chain":
        layers, x, res, (want, bar) = _long_row_want(H, n_rows, arithmetic)
        got, status = _row_chain(cuda, _kernels().RowChainPack(_modules(layers, cuda), precision), x, res)
        assert status == 0
        _check(family, got, want, bar)
    else:
        wide, inner, projection, h, agg, (out, bar, proj, proj_bar) = _long_node_want(H, n_rows, arithmetic)
        got, got_p, status = _node_mlp(cuda, _node_pack(wide, inner, projection, precision, cuda), h, agg, True, True)
        assert status == 0
        _check(family, got, out, bar, "out")
        _check(family, got_p, proj, proj_bar, "proj")


# ---------------------------------------------------------------------------------------------------------------------------
# 8. caller-supplied activation exponents
def _exponent_sets(n_positions):
    return {"zero": [0] * n_positions, "lowest": [cc.MIN_ACTIVATION_EXPONENT] * n_positions,
            "mixed": [(6, 3, 0, -3, -6, 2, -9, 5)[q % 8] for q in range(n_positions)]}


@pytest.mark.parametrize("precision", SPLIT_MODES)
@pytest.mark.parametrize("which", ["zero", "lowest", "mixed"])
def test_caller_supplied_activation_exponents(cuda, which, precision):
    """ActivationScales.exponents written by the test -- every position at 0, every position at -14, another value per position --
    in row mode, edge mode and node-MLP mode: the results stay within the bar computed for THOSE exponents (whose floor
    2^-(25 + e) is the term that moves).
    Measured on an MI355X: at most 0.58 of the bar."""
    assert _hip().EGNN_F16_ACTIVATION_EXPONENT == cc.DEFAULT_ACTIVATION_EXPONENT
    kernels = _kernels()
    H, M = 64, 129
    layers = cc.row_layers(H, 3)
    exps = _exponent_sets(5)[which]
    scales = kernels.ActivationScales(3, cuda)
    scales.exponents.copy_(torch.tensor(exps, dtype=torch.int32))
    x, res = cc.row_inputs(H, M, 41)
    want, bar, _ = cc.row_chain(x, layers, precision, res, act_exps=exps)
    got, status = _row_chain(cuda, kernels.RowChainPack(_modules(layers, cuda), precision, scales=scales), x, res)
    assert status == 0
    _check("exponents, row chain", got, want, bar, which)
    case = cc.edge_case(32, 2, 1, "listed")
    scales = kernels.ActivationScales(3, cuda)
    scales.exponents.copy_(torch.tensor(exps, dtype=torch.int32))
    want = cc.edge_chain(case, precision, act_exps=exps)
    messages, scalar, status = _edge_chain(cuda, _edge_pack(case, precision, cuda, scales), case, False)
    assert status == 0
    _check("exponents, edge chain", messages, want["messages"], want["bar_messages"], which)
    _check("exponents, edge chain", scalar, want["scalar"], want["bar_scalar"], which)
    wide, inner, projection = cc.node_case(32, 1, True)
    exps = _exponent_sets(6)[which]
    scales = kernels.ActivationScales(4, cuda)
    scales.exponents.copy_(torch.tensor(exps, dtype=torch.int32))
    h, agg = cc.node_inputs(32, M, 43)
    out, bar, proj, proj_bar, _ = cc.node_mlp(h, agg, wide, inner, precision, True, projection, act_exps=exps)
    got, got_p, status = _node_mlp(cuda, _node_pack(wide, inner, projection, precision, cuda, scales), h, agg, True, False)
    assert status == 0
    _check("exponents, node MLP", got, out, bar, which)
    _check("exponents, node MLP", got_p, proj, proj_bar, which)


@pytest.mark.parametrize("precision", SPLIT_MODES)
def test_node_mlp_uses_position_0_for_both_halves(cuda, precision):
    """mdx_node_mlp_rows treats positions 0 and 1 as one (position 0's exponent): with position 1 at -14 -- a floor of 2^-11 if it
    were used for agg -- the result stays within the bar of position 0's exponent, 6.
    Measured on an MI355X: at most 0.20 of the bar."""
    kernels = _kernels()
    wide, inner, projection = cc.node_case(32, 1, True)
    exps = [6, cc.MIN_ACTIVATION_EXPONENT, 6, 6, 6, 6]
    scales = kernels.ActivationScales(4, cuda)
    scales.exponents.copy_(torch.tensor(exps, dtype=torch.int32))
    h, agg = cc.node_inputs(32, 129, 47)
    out, bar, proj, proj_bar, _ = cc.node_mlp(h, agg, wide, inner, precision, True, projection, act_exps=[6] * 6)
    got, got_p, status = _node_mlp(cuda, _node_pack(wide, inner, projection, precision, cuda, scales), h, agg, True, False)
    assert status == 0
    _check("exponents, position 0 twice", got, out, bar)
    _check("exponents, position 0 twice", got_p, proj, proj_bar)


@pytest.mark.parametrize("precision", SPLIT_MODES)
def test_f16_range_is_reported_per_position(cuda, precision):
    """One input element of 1300: 2^6 log2(e) 1300 is beyond 65504 at position 0 only (behind the first layer |value| <= 0.5 x
    1300 + 1 < 709) -> MDX_STATUS_EGNN_F16_RANGE; the same data with position 0's exponent lowered to 5 is inside the range at
    every position: status 0 and every element within the bar.
    Measured on an MI355X: at most 0.16 of the bar."""
    kernels = _kernels()
    assert _hip().STATUS_EGNN_F16_RANGE == cc.STATUS_F16_RANGE
    H, M = 64, 33
    layers = cc.row_layers(H, 3)
    x, res = cc.row_inputs(H, M, 53)
    x[5, 7] = 1300.0
    scales = kernels.ActivationScales(3, cuda)
    pack = kernels.RowChainPack(_modules(layers, cuda), precision, scales=scales)
    _, status = _row_chain(cuda, pack, x, res)
    assert status == cc.STATUS_F16_RANGE
    exps = [5, 6, 6, 6, 6]
    scales.exponents.copy_(torch.tensor(exps, dtype=torch.int32))
    got, status = _row_chain(cuda, pack, x, res)
    assert status == 0
    want, bar, _ = cc.row_chain(x, layers, precision, res, act_exps=exps)
    _check("exponents, range", got, want, bar)


# ---------------------------------------------------------------------------------------------------------------------------
# 9. recorded maxima
def _check_maxima(family, scales, positions, n_positions):
    words = scales.maxima.cpu().numpy().astype(np.int32).view(np.uint32)
    got = words.view(np.float32).astype(np.float64)
    worst = 0.0
    for q in range(n_positions):
        if q not in positions:
            assert words[q] == 0, (family, q, "a position this mode does not use was written")
            continue
        lo, hi = positions[q]
        lo, hi = LOG2E * lo * (1 - 4 * cc.U), LOG2E * hi * (1 + 4 * cc.U)       # log2(e) and its rounding, as for rows in
        assert lo <= got[q] <= hi, (family, q, lo, got[q], hi)
        worst = max(worst, abs(got[q] - 0.5 * (lo + hi)) / (0.5 * (hi - lo)))
    _report(family, worst)
    return words


def test_recorded_maxima(cuda):
    """activation_maxima (exact-f32 kernels, zero-filled): after one launch each position's word decodes to the float64 maximum of
    log2(e) |value| at that position, within that position's bar; positions the mode does not use stay 0; a second launch on
    smaller data (some of the same rows) leaves every word unchanged.  Edge mode (positions 0 .. L), row mode (0 .. L), node-MLP mode with projection
    (0, 2 .. L, L + 1).
    Measured on an MI355X: at most 0.11 of the interval's half width away from its middle."""
    kernels = _kernels()
    case = cc.edge_case(32, 2, 3, "listed")
    scales = kernels.ActivationScales(5, cuda)
    pack = _edge_pack(case, "f32", cuda, scales)
    want = cc.edge_chain(case, "f32")
    _edge_chain(cuda, pack, case, False)
    words = _check_maxima("maxima, edge chain", scales, want["positions"], 7)
    assert set(want["positions"]) == set(range(6))
    _edge_chain(cuda, pack, case, False, n_live=case.E // 2)
    assert np.array_equal(scales.maxima.cpu().numpy().astype(np.int32).view(np.uint32), words)

    H, M = 64, 129
    layers = cc.row_layers(H, 3)
    x, res = cc.row_inputs(H, M, 59)
    scales = kernels.ActivationScales(3, cuda)
    pack = kernels.RowChainPack(_modules(layers, cuda), "f32", scales=scales)
    positions = cc.row_chain(x, layers, "f32", res)[2]
    assert set(positions) == {0, 1, 2, 3}
    _row_chain(cuda, pack, x, res)
    words = _check_maxima("maxima, row chain", scales, positions, 5)
    _row_chain(cuda, pack, x[:64], res[:64])
    assert np.array_equal(scales.maxima.cpu().numpy().astype(np.int32).view(np.uint32), words)

    wide, inner, projection = cc.node_case(32, 1, True)
    h, agg = cc.node_inputs(32, M, 61)
    scales = kernels.ActivationScales(4, cuda)
    pack = _node_pack(wide, inner, projection, "f32", cuda, scales)
    positions = cc.node_mlp(h, agg, wide, inner, "f32", True, projection)[4]
    assert set(positions) == {0, 2, 3, 4, 5}
    _node_mlp(cuda, pack, h, agg, True, False)
    words = _check_maxima("maxima, node MLP", scales, positions, 6)
    _node_mlp(cuda, pack, h[:64], agg[:64], True, False)
    assert np.array_equal(scales.maxima.cpu().numpy().astype(np.int32).view(np.uint32), words) and words[1] == 0


# ---------------------------------------------------------------------------------------------------------------------------
# 10, 11. the integer rules
def _float_bits(value):
    return int(np.float32(value).view(np.uint32))


MAXIMA_BITS = [0, 1, 0x007fffff, _float_bits(1.0), _float_bits(np.nextafter(np.float32(2.0 ** 12), np.float32(0))),
               _float_bits(2.0 ** 12), _float_bits(np.nextafter(np.float32(2.0 ** 13), np.float32(0))), _float_bits(2.0 ** 13),
               _float_bits(65504.0), _float_bits(np.finfo(np.float32).max), 0x7f800000, 0x7fc00000, _float_bits(2.0 ** 6),
               _float_bits(2.0 ** 7), _float_bits(3.0e-3)]


@pytest.mark.parametrize("start", [6, -3])
def test_adapt_activation_exponents_exactly(cuda, start):
    """mdx_egnn_chain_adapt_activation_exponents on a table of maxima bits -- 0, subnormals, 1.0, just below and at 2^12 and 2^13,
    65504, the largest float, infinity, NaN: every exponent is min(current, clamp(12 - floor(log2 m), -14, 6)), a zero maximum
    keeps its exponent, every maximum is cleared; a count of 0 or of 19 is refused and nothing is written."""
    hip = _hip()
    count = len(MAXIMA_BITS)
    assert count <= hip.EGNN_CHAIN_MAX_LAYERS + 2
    maxima = torch.tensor(np.array(MAXIMA_BITS, dtype=np.uint32).view(np.int32), device=cuda)
    exponents = torch.full((count,), start, dtype=torch.int32, device=cuda)
    hip.call("mdx_egnn_chain_adapt_activation_exponents", maxima, count, exponents)
    want = [cc.adapted_exponent(start, bits) for bits in MAXIMA_BITS]
    assert exponents.cpu().tolist() == want and want[0] == start
    assert not maxima.cpu().any()
    for refused in (0, hip.EGNN_CHAIN_MAX_LAYERS + 3):
        maxima = torch.full((32,), _float_bits(2.0 ** 12), dtype=torch.int32, device=cuda)
        exponents = torch.full((32,), start, dtype=torch.int32, device=cuda)
        code = hip.lib().mdx_egnn_chain_adapt_activation_exponents(hip.ptr(maxima, torch.int32, "maxima"), refused,
                                                                   hip.ptr(exponents, torch.int32, "exponents"), hip.stream_handle())
        torch.cuda.synchronize()
        assert code != 0 and bool((exponents == start).all()) and bool((maxima == _float_bits(2.0 ** 12)).all())


@pytest.mark.parametrize("precision", SPLIT_MODES)
def test_pack_exponents_exactly(cuda, precision):
    """mdx_egnn_chain_pack's weight_exponents: layers whose largest |W| is 1, 2^-20, 2^-60 (the clamp at 40), an all-zero layer
    (0), a layer with one infinite entry (ignored: the largest finite one counts), and the head row; tied runs take the smallest
    exponent of the run."""
    kernels = _kernels()
    H = 32
    rng = np.random.default_rng(3)
    shape = rng.uniform(0.25, 1.0, size=(H, H)).astype(np.float32)
    shape[3, 5] = 1.0

    def layer(largest):
        return cc.SparseLayer(shape * np.float32(largest), None, H, "random")
    with_inf = shape * np.float32(0.125)
    with_inf[7, 9] = np.inf
    layers = [layer(1.0), layer(2.0 ** -20), layer(2.0 ** -60), cc.SparseLayer(np.zeros((H, H)), None, H, "random"),
              cc.SparseLayer(with_inf, None, H, "random"), layer(1.999)]
    head = cc.SparseLayer(shape[:1] * np.float32(3.0), None, H, "random")
    assert cc.pack_exponents(layers, 0, head) == [13, 33, 40, 0, 16, 13, 12]
    weights = [_dev(l.weight, cuda) for l in layers]
    for tied in (0, 1 << 1, (1 << 1) | (1 << 2), (1 << 2) | (1 << 4) | (1 << 5), 1 << 3):
        _, exponents = kernels._pack_chain_image(weights, _dev(head.weight, cuda), H, precision, tied)
        assert exponents.cpu().tolist() == cc.pack_exponents(layers, tied, head), tied
    _, exponents = kernels._pack_chain_image(weights, None, H, "f32", 0)
    assert exponents.cpu().tolist() == [0] * 7
