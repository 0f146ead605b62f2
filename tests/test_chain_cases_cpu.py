"""tests/chain_cases.py without a GPU: the float64 restatements of the chain entry points against the package's own modules, the
bars against two binary32 evaluations of the same chains (torch's float32 on the CPU; a numpy emulation of the split-f16 form),
against the emulation with one lo x hi product left out (which must fall outside), the sharpness condition on the inputs, and
every structural precondition the GPU tests (tests/test_egnn_chain_elements_gpu.py) rely on."""
import numpy as np
import pytest
import torch

import chain_cases as cc
import gather_cases as gc

SHARP = 2.0 ** -15          # the median of bar / |value| over the non-zero outputs, in every case
CUS = 256                   # compute units of an MI355X (the GPU tests read the count from the device)


def _inside(got, want, bar):
    return bool(np.all(np.isfinite(got))) and bool(np.all(np.abs(got.astype(np.float64) - want) <= bar))


def _worst(got, want, bar):
    return float(np.max(np.abs(got.astype(np.float64) - want) / bar))


def _split(layers, n_positions, drop=None, tied=0, head=None, act_exps=None):
    exps = [cc.DEFAULT_ACTIVATION_EXPONENT] * n_positions if act_exps is None else act_exps
    return cc.Split32(exps, cc.pack_exponents(layers, tied, head), drop)


# ---------------------------------------------------------------------------------------------------------------------------
# generators and integer rules
def test_layer_generators():
    """r non-zeros per row at distinct columns, sum |w| <= 1/2, every non-zero with BOTH f16 halves non-zero at the pack's scale,
    the structured column where the kind says, and the permutation set: identity, reversal, rotations by 1, 4, 8, 16 and 32 columns."""
    assert cc.ROTATIONS == (1, 4, 8, 16, 32)
    assert set(cc.KINDS) == {"random", "identity", "reversal"} | {"rotation%d" % s for s in cc.ROTATIONS}
    for H in cc.WIDTHS:
        for r in (1, 2, 4, 8):
            for kind in cc.KINDS:
                layer = cc.sparse_layer(H, r, 11 * H + r, kind)
                assert np.all((layer.weight != 0).sum(axis=1) == r)
                assert np.all(layer.abs64.sum(axis=1) <= 0.5) and np.all(layer.abs64.sum(axis=1) >= 0.39)
                first = cc.first_columns(H, kind)
                if first is not None:
                    assert np.all(layer.weight[np.arange(H), first] != 0)
                scaled = layer.weight * np.float32(2.0 ** cc.pack_exponent(layer.largest()))
                assert 2.0 ** 13 <= np.abs(scaled).max() < 2.0 ** 14
                hi, lo = cc.Split32.halves(scaled)
                assert np.all((hi != 0) == (layer.weight != 0)) and np.mean(lo[layer.weight != 0] != 0) > 0.95
    assert np.array_equal(cc.first_columns(8, "identity"), np.arange(8))
    assert np.array_equal(cc.first_columns(8, "reversal"), np.arange(8)[::-1])
    assert np.array_equal(cc.first_columns(8, "rotation4"), (np.arange(8) + 4) % 8)
    # a 16-layer stack walks through every kind and every r
    stack = cc.row_layers(256, 16)
    assert {layer.kind for layer in stack} == set(cc.KINDS) and {layer.r for layer in stack} == {1, 2, 4, 8}


def test_pack_and_adapt_rules():
    assert [cc.pack_exponent(m) for m in (1.0, 2.0 ** -20, 2.0 ** -60, 0.0, 1.5, 0.99)] == [13, 33, 40, 0, 13, 14]
    layers = [cc.SparseLayer(np.full((4, 4), m, dtype=np.float32), None, 4, "random") for m in (1.0, 2.0 ** -20, 4.0, 0.25)]
    assert cc.pack_exponents(layers) == [13, 33, 11, 15, 0]
    assert cc.pack_exponents(layers, tied=1 << 1) == [13, 13, 11, 15, 0]
    assert cc.pack_exponents(layers, tied=(1 << 1) | (1 << 3)) == [13, 13, 11, 11, 0]
    assert cc.pack_exponents(layers, tied=(1 << 2) | (1 << 3)) == [13, 11, 11, 11, 0]
    with_inf = np.full((4, 4), 0.5, dtype=np.float32)
    with_inf[1, 2] = np.inf
    assert cc.pack_exponents([cc.SparseLayer(with_inf, None, 4, "random")]) == [14, 0]
    bits = lambda v: int(np.float32(v).view(np.uint32))
    for current in (6, -3):
        assert cc.adapted_exponent(current, 0) == current
        assert cc.adapted_exponent(current, 1) == current                                   # a subnormal: the default at most
        assert cc.adapted_exponent(current, bits(1.0)) == current
        assert cc.adapted_exponent(current, bits(2.0 ** 6)) == min(current, 6)
        assert cc.adapted_exponent(current, bits(2.0 ** 7)) == min(current, 5)
        assert cc.adapted_exponent(current, bits(np.nextafter(np.float32(2.0 ** 12), np.float32(0)))) == min(current, 1)
        assert cc.adapted_exponent(current, bits(2.0 ** 12)) == min(current, 0)
        assert cc.adapted_exponent(current, bits(2.0 ** 13)) == min(current, -1)
        assert cc.adapted_exponent(current, bits(65504.0)) == -3
        for huge in (bits(np.finfo(np.float32).max), 0x7f800000, 0x7fc00000, 0xffc00000):
            assert cc.adapted_exponent(current, huge) == -14


def test_workgroup_tiles():
    """The helper covers every tile once (asserted inside it) for every relation of the tile count to 8, to the number of CUs and
    to their multiples; the multi-tile cases of the GPU tests make some workgroup run two tiles, the long one three."""
    for n_cus in (8, 64, 256, 304):
        for n_tiles in (1, 7, 8, 9, 15, 17, n_cus - 1, n_cus, n_cus + 1, 2 * n_cus + 8, 3 * n_cus + 9):
            tiles = cc.workgroup_tiles(cc.TILE * (n_tiles - 1) + 37, n_cus)
            assert len(tiles) == min(n_tiles, n_cus)
            if n_tiles % 8 == 0 and n_tiles <= n_cus:
                assert max(len(t) for t in tiles) == 1
        assert cc.most_tiles(cc.multi_tile_rows(n_cus, 2), n_cus) >= 2
        assert cc.most_tiles(cc.multi_tile_rows(n_cus, 3), n_cus) >= 3
    # (a tile count that is no multiple of 8 leaves some XCD with fewer workgroups than tiles: nine tiles on nine workgroups
    # are two each for the workgroups of XCDs 1 to 3 and none for those of the last three)
    assert [len(t) for t in cc.workgroup_tiles(9 * cc.TILE, CUS)] == [1, 2, 2, 2, 1, 0, 0, 0, 1]


def test_graphs_and_parity_classes():
    for name, degrees in gc.ORDERINGS.items():
        gc._check_ordering(degrees)
        edges, offsets, degree, E = cc.graph_with_poison(degrees, 3, capacity_extra=40)
        poison = len(degrees)
        assert E == sum(degrees) and edges.shape[0] == E + 40 and degree[poison] == 0
        assert not np.any(edges[:E] == poison) and np.all(edges[E:] == poison)
        assert np.any(edges[:E, 0] == edges[:E, 1])
        assert np.max(np.bincount(edges[:E, 1])) >= 2
    degrees = cc.long_degrees(cc.multi_tile_rows(8, 2))
    assert sum(degrees) == cc.multi_tile_rows(8, 2)
    classes = {(m % 2, c % 2) for m, c in cc.PARITIES}
    assert classes == {(0, 0), (0, 1), (1, 0), (1, 1)} and (8, 8) in cc.PARITIES
    for H in cc.EDGE_WIDTHS:
        assert {cc.dimension_of(H, m, c) for m, c in cc.PARITIES} == set(cc.DIMENSIONS)
    case = cc.edge_case(32, 2, 1, "listed")
    assert np.all(np.isnan(case.node_proj[-1])) and np.all(np.isnan(case.coord[-1]))
    assert np.all(np.isfinite(case.node_proj[:-1])) and np.all(np.isfinite(case.coord[:-1]))


# ---------------------------------------------------------------------------------------------------------------------------
# the restatements against the package's own modules, float64, CPU path
def _set(linear, layer):
    with torch.no_grad():
        linear.weight.copy_(torch.from_numpy(layer.w64))
        if linear.bias is not None:
            linear.bias.copy_(torch.from_numpy(layer.b64))


@pytest.mark.parametrize("n_message,n_coord,attention", [(1, 1, False), (2, 3, False), (3, 2, True), (8, 8, False)])
def test_edge_restatement_against_e_gcl(n_message, n_coord, attention):
    """E_GCL.message_model and coord_mlp in float64 with the first layer's weight [I 0 | 0 I | w_r] on the node rows themselves
    (input_size = 2 H): the contract's x0 = SiLU(P[src, :H] + P[dst, H:] + b0 + radial w_r) and everything behind it."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.egnn import E_GCL
    H = 32
    case = cc.edge_case(H, n_message, n_coord, "listed", attention=attention)
    module = E_GCL(2 * H, H, n_message, H, 0, H, n_coord - 1, H, attention=attention).double()
    first = np.zeros((H, 4 * H + 1))
    first[:, :H] = np.eye(H)
    first[:, 3 * H:4 * H] = np.eye(H)
    first[:, 4 * H] = case.w_radial
    _set(module.message_mlp[0], cc.SparseLayer(first, case.bias_in, 1, "random"))
    for k in range(n_message):
        _set(module.message_mlp[2 * (k + 1)], case.layers[k])
    for k in range(n_coord):
        _set(module.coord_mlp[2 * k], case.layers[n_message + k])
    _set(module.coord_mlp[2 * n_coord], case.w_out)
    if attention:
        _set(module.att_mlp[0], case.att)
    edges = torch.from_numpy(case.edges[:case.E])
    h = torch.from_numpy(case.node_proj.astype(np.float64))
    radial, _ = module.coord2radial(edges, torch.from_numpy(case.coord.astype(np.float64)))
    with torch.no_grad():
        messages = module.message_model(h[edges[:, 0]], h[edges[:, 1]], radial)
        scalar = module.coord_mlp(messages).reshape(-1)
    want = cc.edge_chain(case, "f32")
    assert np.all(np.abs(want["messages"] - messages.numpy()) <= 1e-12 * np.abs(messages.numpy()) + 1e-300)
    assert np.all(np.abs(want["scalar"] - scalar.numpy()) <= 1e-12 * np.abs(scalar.numpy()) + 1e-300)


@pytest.mark.parametrize("n_inner,residual", [(0, True), (1, False), (4, True)])
def test_node_restatement_against_e_gcl(n_inner, residual):
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.egnn import E_GCL, run_mlp
    H, M = 32, 33
    wide, inner, proj = cc.node_case(H, n_inner, True)
    module = E_GCL(H, H, 0, H, n_inner, H, 0, H, residual=residual).double()
    both = cc.SparseLayer(np.concatenate([wide[0].w64, wide[1].w64], axis=1), wide[0].bias, 8, "random")
    _set(module.node_mlp[0], both)
    for k, layer in enumerate(inner):
        _set(module.node_mlp[2 * (k + 1)], layer)
    h, agg = cc.node_inputs(H, M, 5)
    with torch.no_grad():
        got = run_mlp(module.node_mlp, torch.from_numpy(np.concatenate([h, agg], axis=1).astype(np.float64))).numpy()
    if residual:
        got = got + h
    out, _, projected, _, _ = cc.node_mlp(h, agg, wide, inner, "f32", residual, proj)
    assert np.all(np.abs(out - got) <= 1e-12 * np.abs(got))
    want_p = got @ np.concatenate([proj[0].w64, proj[1].w64], axis=0).T
    assert np.all(np.abs(projected - want_p) <= 1e-12 * np.abs(want_p) + 1e-300)
    # the row chain is the same module stack behind its first layer
    x, res = cc.row_inputs(H, M, 6)
    with torch.no_grad():
        tail = run_mlp(list(module.node_mlp)[2:], torch.from_numpy(x.astype(np.float64))).numpy()
    rows, _, _ = cc.row_chain(x, inner, "f32", res)
    assert np.all(np.abs(rows - (tail + res)) <= 1e-12 * np.abs(tail + res))


# ---------------------------------------------------------------------------------------------------------------------------
# the bars against binary32 evaluations, and the sharpness condition
@pytest.mark.parametrize("n_layers", cc.ROW_LAYERS)
@pytest.mark.parametrize("H", cc.ROW_WIDTHS)
def test_row_chain_bars(H, n_layers):
    layers = cc.row_layers(H, n_layers)
    for M in cc.ROW_COUNTS:
        x, res = cc.row_inputs(H, M, 17 * H + M)
        for residual in (None, res):
            want, bar, _ = cc.row_chain(x, layers, "f32", residual)
            assert _inside(cc.row_chain32(x, layers, residual), want, bar)
            want, bar, _ = cc.row_chain(x, layers, "f16x3", residual)
            assert _inside(cc.row_chain32(x, layers, residual, _split(layers, n_layers + 2)), want, bar)
            assert cc.sharpness(want, bar) <= SHARP, (M, cc.sharpness(want, bar))
            if M >= 127:
                # (the contraction that keeps the bar flat also shrinks an early layer's error by 0.55 per layer behind it: the
                # last layers are where one missing product is still an error of the output)
                for l in {max(n_layers - 2, 0), n_layers - 1}:
                    mutant = cc.row_chain32(x, layers, residual, _split(layers, n_layers + 2, drop=(l, "lo_hi")))
                    assert not _inside(mutant, want, bar), (M, l)


@pytest.mark.parametrize("attention", [False, True])
@pytest.mark.parametrize("n_message,n_coord", cc.PARITIES)
@pytest.mark.parametrize("H", cc.EDGE_WIDTHS)
def test_edge_chain_bars(H, n_message, n_coord, attention):
    L = n_message + n_coord
    for ordering in gc.ORDERINGS:
        case = cc.edge_case(H, n_message, n_coord, ordering, attention=attention)
        for precision in ("f32", "f16x3"):
            want = cc.edge_chain(case, precision)
            split = None if precision == "f32" else _split(case.layers, L + 2, head=case.w_out)
            messages, scalar = cc.edge_chain32(case, split)
            assert _inside(messages, want["messages"], want["bar_messages"]), _worst(messages, want["messages"], want["bar_messages"])
            assert _inside(scalar, want["scalar"], want["bar_scalar"]), _worst(scalar, want["scalar"], want["bar_scalar"])
            assert cc.sharpness(want["messages"], want["bar_messages"]) <= SHARP
            assert cc.sharpness(want["scalar"], want["bar_scalar"]) <= SHARP
            pieces, piece_bars = cc.piece_buffer(want["messages"], want["bar_messages"], case.offsets, case.degree, case.E)
            summed = gc.pieces_from_messages(messages.astype(np.float64), case.offsets, case.degree, rounded=False)
            owned = ~np.isnan(pieces[:, 0])
            assert np.array_equal(owned, ~np.isnan(summed[:, 0])) and _inside(summed[owned], pieces[owned], piece_bars[owned])
            assert cc.sharpness(pieces[owned], piece_bars[owned]) <= SHARP
        if attention:
            logits = want["logits"]
            # The aim is a spread of about 1.5.  The contraction that keeps the bar flat makes the edges' messages alike
            # (by 0.55 per message layer), and the gate's bar grows with its row: at GATE_SCALE_LIMIT, the largest row that
            # keeps the sharpness condition below, the logits spread over 0.25 to 1.5 behind one message layer and over less
            # behind more of them; they still differ from edge to edge, and the gate sits between 0.3 and 0.7
            spread = float(logits.max() - logits.min())
            assert spread <= 1.5 * (1 + 1e-6) and (spread >= 0.25 if n_message == 1 else spread > 0.0), spread
            assert abs(0.5 * float(logits.max() + logits.min())) <= 0.31
        # the emulated mutation: one lo x hi product gone from the last message layer
        mutant = cc.edge_chain32(case, _split(case.layers, L + 2, drop=(n_message - 1, "lo_hi"), head=case.w_out))
        assert not _inside(mutant[0], want["messages"], want["bar_messages"]), ordering


@pytest.mark.parametrize("widths", cc.PADDED_WIDTHS)
def test_padded_width_bars(widths):
    m, c = widths
    case = cc.edge_case(0, 2, 2, "listed", widths=widths)
    assert case.H == {(16, 32): 32, (48, 80): 128, (160, 256): 256, (32, 16): 32}[widths]
    want = cc.edge_chain(case, "f16x3")
    assert np.all(want["messages"][:, m:] == 0.0) and np.all(want["messages"][:, :m] != 0.0)
    messages, scalar = cc.edge_chain32(case, _split(case.layers, 6, head=case.w_out))
    assert np.all(messages[:, m:] == 0.0)
    assert _inside(messages, want["messages"], want["bar_messages"]) and _inside(scalar, want["scalar"], want["bar_scalar"])
    messages, scalar = cc.edge_chain32(case)
    want = cc.edge_chain(case, "f32")
    assert _inside(messages, want["messages"], want["bar_messages"]) and _inside(scalar, want["scalar"], want["bar_scalar"])
    assert cc.sharpness(want["messages"], want["bar_messages"]) <= SHARP and cc.sharpness(want["scalar"], want["bar_scalar"]) <= SHARP


@pytest.mark.parametrize("uneven", [False, True])
@pytest.mark.parametrize("n_inner", cc.NODE_INNER)
@pytest.mark.parametrize("H", cc.EDGE_WIDTHS)
def test_node_mlp_bars(H, n_inner, uneven):
    wide, inner, proj = cc.node_case(H, n_inner, True, uneven)
    image = list(wide) + list(inner) + list(proj)
    L = 2 + len(inner)
    tied = (1 << 1) | (1 << (L + 1))
    h, agg = cc.node_inputs(H, 129, 9 * H + n_inner, agg_scale=32.0 if uneven else 1.0)
    for residual in (False, True):
        out, bar, projected, proj_bar, _ = cc.node_mlp(h, agg, wide, inner, "f32", residual, proj)
        got, got_p = cc.node_mlp32(h, agg, wide, inner, residual, proj)
        assert _inside(got, out, bar) and _inside(got_p, projected, proj_bar)
        out, bar, projected, proj_bar, _ = cc.node_mlp(h, agg, wide, inner, "f16x3", residual, proj)
        got, got_p = cc.node_mlp32(h, agg, wide, inner, residual, proj, _split(image, L + 2, tied=tied))
        assert _inside(got, out, bar) and _inside(got_p, projected, proj_bar), (_worst(got, out, bar), _worst(got_p, projected, proj_bar))
        assert cc.sharpness(out, bar) <= SHARP and cc.sharpness(projected, proj_bar) <= SHARP
        mutant, _ = cc.node_mlp32(h, agg, wide, inner, residual, proj, _split(image, L + 2, drop=(L - 1, "lo_hi"), tied=tied))
        assert not _inside(mutant, out, bar)
        _, mutant_p = cc.node_mlp32(h, agg, wide, inner, residual, proj, _split(image, L + 2, drop=(L + 1, "lo_hi"), tied=tied))
        assert not _inside(mutant_p, projected, proj_bar)
    if uneven:
        # the tied exponent is the large half's: the small half's weights sit 2^10 lower in the f16 range
        exps = cc.pack_exponents(image, tied)
        assert exps[0] == exps[1] == cc.pack_exponent(wide[0].largest()) == cc.pack_exponent(wide[1].largest()) - 10


def test_multi_tile_case_bars():
    """The multi-tile family at a small CU count: a long graph, few layers, all three modes of the chain."""
    n_cus = 8
    n = cc.multi_tile_rows(n_cus, 2)
    assert cc.most_tiles(n, n_cus) >= 2
    case = cc.EdgeCase(32, 2, 1, 6, cc.long_degrees(n), 77, r=2)
    assert case.E == n
    for precision in ("f32", "f16x3"):
        want = cc.edge_chain(case, precision)
        got = cc.edge_chain32(case, None if precision == "f32" else _split(case.layers, 5, head=case.w_out))
        assert _inside(got[0], want["messages"], want["bar_messages"]) and _inside(got[1], want["scalar"], want["bar_scalar"])
