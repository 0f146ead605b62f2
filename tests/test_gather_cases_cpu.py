"""The float64 restatements of tests/gather_cases.py against plainer statements of the same things: they are the yardsticks of
tests/test_egnn_node_gather_gpu.py and tests/test_egnn_table_kernels_gpu.py, so they are checked here, without a GPU."""
import numpy as np
import pytest
import torch

import gather_cases as gc

INV_SPACING = 256.0
N_EVEN = 40


@pytest.mark.parametrize("ordering", sorted(gc.ORDERINGS))
def test_pieces_add_up_to_index_add(ordering):
    """A node's pieces added in edge order are index_add_ of the messages (1e-12: float64 pieces, only the association
    differs); with dyadic messages, whose sums are exact, the binary32 pieces give it exactly.  No NaN row is read, every
    owned row is read once, and every row that is not NaN is owned."""
    degrees = gc.ORDERINGS[ordering]
    edges, offsets, degree = gc.ragged_graph(degrees, len(degrees), seed=11)
    E, H = edges.shape[0], 12
    rng = np.random.default_rng(5)
    messages = rng.standard_normal((E, H))
    want = torch.zeros(len(degrees), H, dtype=torch.float64).index_add_(0, torch.as_tensor(edges[:, 0]),
                                                                        torch.as_tensor(messages)).numpy()
    pieces = gc.pieces_from_messages(messages, offsets, degree, rounded=False)
    got, read = gc.combine_pieces(pieces, offsets, degree, np.float64)
    assert np.all(np.isfinite(got)) and np.max(np.abs(got - want)) <= 1e-12
    assert len(set(read)) == len(read) and sorted(read) == [r for r in range(pieces.shape[0]) if not np.isnan(pieces[r, 0])]
    assert pieces.shape[0] == ((E + 15) >> 4) + len(degrees) and len(read) < pieces.shape[0]         # some rows ARE unowned
    assert np.array_equal(gc.piece_counts(offsets, degree) == 0, degree == 0)
    dyadic = rng.integers(-512, 513, size=(E, H)) / 64.0
    want = torch.zeros(len(degrees), H, dtype=torch.float64).index_add_(0, torch.as_tensor(edges[:, 0]),
                                                                        torch.as_tensor(dyadic)).numpy()
    pieces32 = gc.pieces_from_messages(dyadic, offsets, degree)
    assert pieces32.dtype == np.float32
    got32, _ = gc.combine_pieces(pieces32, offsets, degree, np.float32)
    assert got32.dtype == np.float32 and np.array_equal(got32.astype(np.float64), want)


def test_piece_rows_follow_the_documented_layout():
    """Hand-made cases of include/mdx_hip.h's rule, E = 40 (3 boundary rows), node 7."""
    own = 3 + 7
    assert gc.piece_rows(7, 5, 5, 40) == []
    assert gc.piece_rows(7, 0, 16, 40) == [(0, 0, 16)]                               # exactly one group
    assert gc.piece_rows(7, 15, 16, 40) == [(0, 15, 16)]                             # one edge, the boundary edge
    assert gc.piece_rows(7, 3, 9, 40) == [(own, 3, 9)]                               # inside a group
    assert gc.piece_rows(7, 14, 18, 40) == [(0, 14, 16), (own, 16, 18)]
    assert gc.piece_rows(7, 15, 40, 40) == [(0, 15, 16), (1, 16, 32), (own, 32, 40)]
    assert gc.piece_rows(7, 2, 32, 40) == [(0, 2, 16), (1, 16, 32)]


def _points(seed, low, high, count=4000):
    rng = np.random.default_rng(seed)
    u = rng.uniform(low, high, size=count)
    return np.concatenate([u, np.arange(np.ceil(low), np.floor(high) + 1.0), [low, high]])


@pytest.mark.parametrize("n_classes", [1, 3])
def test_table_reference_reproduces_a_cubic(n_classes):
    """4-point Lagrange interpolation is exact on cubics, so the float64 interpolation of the binary32-rounded table differs
    from the polynomial by the table's rounding alone: at most u |v| per point, u S in all (measured here: 0.97 u S).  Generic cubics
    on u >= 1, where no reflection enters, up to u = n_even - 2 exactly (the last cell, t = 1); even ones, a + b rho^2, on all
    of [0, n_even - 2], where the reflected left neighbour of cell 0 is the polynomial's own value."""
    columns = 5
    worst = {}
    for even, low in ((False, 1.0), (True, 0.0)):
        coefficients, table = gc.cubic_table(n_classes, N_EVEN, columns, INV_SPACING, seed=3, even=even)
        assert table.dtype == np.float32 and table.shape == (n_classes ** 2 * (2 * N_EVEN - 1), columns)
        u = _points(17, low, N_EVEN - 2.0)
        E = u.shape[0]
        rng = np.random.default_rng(23)
        classes = rng.integers(0, n_classes, size=2 * E)
        edges = np.stack([np.arange(E), E + np.arange(E)], axis=1)
        got, magnitude = gc.table_edge_values(table, n_classes, N_EVEN, classes, edges, u)
        pair = classes[edges[:, 0]] * n_classes + classes[edges[:, 1]]
        want, _ = gc.cubic_value(coefficients, pair, u / INV_SPACING)
        ratio = np.abs(got - want) / (gc.U * magnitude)
        worst[even] = float(ratio.max())
        assert ratio.max() <= 1.0 + 1e-6, (even, ratio.max())
    print(f"n_classes {n_classes}: |interpolation - cubic| / (u S) = {worst[False]:.3f} (cubic), {worst[True]:.3f} (even)")


def test_table_reference_sums_per_node_and_tells_the_pairs_apart():
    """table_reference is the per-node sum of table_edge_values; the table of pair (a, b) is not that of (b, a), and swapping
    the classes of an edge's ends changes the value."""
    n_classes = 3
    degrees = gc.DEGREES
    edges, offsets, degree = gc.ragged_graph(degrees, len(degrees), seed=4)
    coefficients, table = gc.cubic_table(n_classes, N_EVEN, 4, INV_SPACING, seed=9)
    K = 2 * N_EVEN - 1
    blocks = table.reshape(n_classes, n_classes, K, 4)
    for a in range(n_classes):
        for b in range(a):
            assert not np.any(blocks[a, b] == blocks[b, a])
    classes = np.arange(len(degrees)) % n_classes
    u = np.random.default_rng(2).uniform(0.0, N_EVEN - 2.0, size=edges.shape[0])
    total, S = gc.table_reference(table, n_classes, N_EVEN, classes, edges, offsets, degree, u)
    values, magnitudes = gc.table_edge_values(table, n_classes, N_EVEN, classes, edges, u)
    for node in range(len(degrees)):
        span = slice(int(offsets[node]), int(offsets[node] + degree[node]))
        assert np.allclose(total[node], values[span].sum(axis=0), rtol=0, atol=1e-12 * (1.0 + S[node].max()))
        assert np.allclose(S[node], magnitudes[span].sum(axis=0), rtol=1e-14, atol=0)
    assert np.all(total[degree == 0] == 0.0) and np.all(S[degree > 0] > 0.0)
    swapped, _ = gc.table_edge_values(table, n_classes, N_EVEN, classes, edges[:, ::-1], u)
    mixed = classes[edges[:, 0]] != classes[edges[:, 1]]
    assert mixed.any() and np.all(swapped[mixed] != values[mixed]) and np.array_equal(swapped[~mixed], values[~mixed])


def test_midpoint_rows_are_the_cubic_midpoints():
    """The check's formula at t = 1/2 reproduces a cubic's midpoints to binary32 rounding (and those of cell 0 for an even one)."""
    coefficients, table = gc.cubic_table(1, N_EVEN, 6, INV_SPACING, seed=8, even=True)
    even = table[:N_EVEN]
    mid = gc.midpoint_rows(even, N_EVEN)
    assert mid.shape == (N_EVEN - 1, 6) and mid.dtype == np.float32
    scale = np.abs(table).max(axis=0)
    assert np.max(np.abs(mid[:-1].astype(np.float64) - table[N_EVEN:-1]) / scale) <= 8 * gc.U       # (the last one is not read)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_coordinate_reference_against_torch_float64(flags):
    """coord_reference against the update written with torch float64 ops and index_add_ (models/egnn.py's form), both means; an
    edge between two nodes at the same place and a self-loop contribute exactly zero, also under COORD_NORMALIZE (0 / 1e-8);
    the float32 evaluation of transcendental_allowance on the CPU stays within a few u of it."""
    degrees = gc.DEGREES
    n, D = len(degrees), 3
    edges, offsets, degree = gc.ragged_graph(degrees, n, seed=6)
    rng = np.random.default_rng(1)
    coord = rng.standard_normal((n, D)).astype(np.float32)
    a, b = edges[int(offsets[2])]
    assert a != b
    coord[b] = coord[a]
    s = rng.standard_normal(edges.shape[0]).astype(np.float32)
    c, sd = torch.as_tensor(coord).double(), torch.as_tensor(s).double()
    diff = c[edges[:, 0]] - c[edges[:, 1]]
    if flags & gc.COORD_NORMALIZE:
        r2 = (diff ** 2).sum(1, keepdim=True)
        diff = torch.tanh(r2) / torch.sqrt(r2 + 1e-16) * diff
    trans = diff * (torch.tanh(sd) if flags & gc.COORD_TANH else sd)[:, None]
    agg = torch.zeros(n, D, dtype=torch.float64).index_add_(0, torch.as_tensor(edges[:, 0]), trans)
    for mean in (False, True):
        want = c + (agg / torch.as_tensor(degree).clamp(min=1)[:, None] if mean else agg)
        got, magnitude, terms = gc.coord_reference(coord, edges, offsets, degree, s.astype(np.float64), flags, mean)
        assert np.max(np.abs(got - want.numpy())) <= 1e-12
        assert np.array_equal(got[degree == 0], coord[degree == 0].astype(np.float64))
        assert np.all(magnitude >= np.abs(got - coord) - 1e-12)
    loops = edges[:, 0] == edges[:, 1]
    assert loops.any() and np.all(terms[loops] == 0.0) and np.all(terms[int(offsets[2])] == 0.0)
    allowance = gc.transcendental_allowance(coord, edges, s, flags, torch.device("cpu"))
    assert 0.0 < allowance <= 2 * 16 * gc.U
