"""kernels.egnn_table_gather (csrc/mdx_egnn_node.hip) and kernels.egnn_table_check (csrc/mdx_egnn_table.hip) called directly on
synthetic tables: every
(class pair, column) of the table is a random cubic in rho, so the 4-point interpolation is exact up to rounding and a float64
interpolation of the same binary32 table (gather_cases.table_reference) is a reference with a bar per node and column."""
import functools

import numpy as np
import pytest
import torch

import gather_cases as gc

pytestmark = pytest.mark.gpu

U = gc.U
N_EVEN = 40
K = 2 * N_EVEN - 1
STEP = 2.0 ** -12                          # exact points: coordinates are multiples of it, distances k STEP, u = k / 16
LAST = 16 * (N_EVEN - 2)                   # k of u = n_even - 2, the end of the grid
# distances from the first entry, in STEP: inside cell 0 (k < 16), cell 1, the middle, the last cell (k >= LAST - 16), its end
AXIS_K = [0, 3, 7, 12, 15, 16, 100, 250, 333, 480, 590, 596, 600, 604, 607, LAST, 5]
# the same for points a (3, 4) STEP on a line, distances 5 a STEP (5 * 121 = 605 is inside the last cell)
LINE_A = [0, 1, 2, 3, 20, 50, 66, 96, 118, 119, 120, 121, 117, 60, 30, 10, 90]
MEASURED = {}


def _pkg():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    assert kernels.TABLE_INV_SPACING * STEP * 16 == 1.0
    assert (_hip.EGNN_COORD_NORMALIZE, _hip.EGNN_COORD_TANH) == (gc.COORD_NORMALIZE, gc.COORD_TANH)
    return _hip, kernels


def _dev(array, device):
    return torch.as_tensor(np.ascontiguousarray(array)).to(device)


@functools.lru_cache(maxsize=None)
def _graph(ordering):
    """ragged_graph with 17 destinations pinned: the node with the most edges points at every node once (edges 2 .. 18 of its
    range), so every distance class of AXIS_K / LINE_A occurs whatever the random destinations are.  Returns also the order in
    which the nodes take the entries of those lists (that node first)."""
    degrees = gc.ORDERINGS[ordering]
    n = len(degrees)
    edges, offsets, degree = gc.ragged_graph(degrees, n, seed=40 + len(ordering))
    hub = int(np.argmax(degree))
    order = np.array([hub] + [i for i in range(n) if i != hub])
    edges = edges.copy()
    edges[offsets[hub] + 2:offsets[hub] + 2 + n, 1] = order
    return edges, offsets, degree, order


@functools.lru_cache(maxsize=None)
def _table(n_classes, H, even):
    """(coefficients [n_pairs, H + 1, 4], table float32 [n_pairs K, H], table_scalar float32 [n_pairs K]): column H is the scalar."""
    coefficients, table = gc.cubic_table(n_classes, N_EVEN, H + 1, 256.0, seed=1000 * n_classes + H, even=even)
    blocks = table.reshape(n_classes, n_classes, K, H + 1)
    for a in range(n_classes):
        for b in range(a):
            assert not np.any(blocks[a, b] == blocks[b, a])          # F_ab is visibly not F_ba
    return coefficients, np.ascontiguousarray(table[:, :H]), np.ascontiguousarray(table[:, H])


def _classes(n, n_classes, seed=7):
    classes = np.random.default_rng(seed).integers(0, n_classes, size=n)
    assert len(set(classes.tolist())) == n_classes
    return classes.astype(np.int64)


def _exact_coordinates(layout, D, order):
    """float32 [n, D] on a line, every pairwise distance an exact multiple of STEP: along the last axis ("axis"), or along
    (3, 4, 0, ...) ("line").  The other components hold a constant, so the differences there are exact zeros."""
    n = len(order)
    coord = np.full((n, D), 0.25, dtype=np.float64)
    if layout == "axis":
        coord[order, D - 1] = np.asarray(AXIS_K) * STEP
    else:
        coord[order, 0] = 3 * np.asarray(LINE_A) * STEP
        coord[order, 1] = 0.125 + 4 * np.asarray(LINE_A) * STEP
    assert np.array_equal(coord.astype(np.float32).astype(np.float64), coord)
    return coord.astype(np.float32)


def _generic_coordinates(D, n, seed):
    """Random binary32 points of a box whose diagonal stays inside the grid."""
    side = 0.97 * ((N_EVEN - 2) / 256.0) / np.sqrt(D)
    return (np.random.default_rng(seed).uniform(0.0, side, size=(n, D))).astype(np.float32)


def _gather(kernels, cuda, tables, n_classes, classes, graph, coord, mean_messages, mean_coords, flags, left=None):
    _, table, scalar = tables
    edges, offsets, degree = graph[:3]
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    out, coord_out = kernels.egnn_table_gather(_dev(table, cuda), _dev(scalar, cuda), n_classes, N_EVEN, _dev(classes, cuda),
                                               _dev(offsets, cuda), _dev(degree, cuda), mean_messages,
                                               None if left is None else _dev(left, cuda), _dev(coord, cuda), _dev(edges, cuda),
                                               mean_coords, flags=flags, status=status)
    return out.cpu().numpy(), coord_out.cpu().numpy(), int(status.item())


def _bars(tables, n_classes, classes, graph, coord, u, generic):
    """What the message half is compared with, and the per-edge scalar with its error bound.

    Messages, per node and column: table_reference and (deg + 12) u S -- the weights carry 3 roundings each (two products and a
    division; t and t +- 1, t - 2 are exact at the exact points), the interpolation 4 (a product and up to three additions),
    the sum over the edges deg, the mean 1: deg + 8, within the deg + 12 of the issue that asked for this test.  Generic points add
    |dF/du| (D + 2) u |u| per edge: r^2 carries (D + 2) u ((c_i - c_j)^2: 3, D - 1 additions), its root half of that and
    one more, the product with the spacing none.
    The scalar of an edge (no sum): 12 u S_e, plus the same term for generic points."""
    coefficients, table, scalar = tables
    edges, offsets, degree = graph[:3]
    D = coord.shape[1]
    want, S = gc.table_reference(table, n_classes, N_EVEN, classes, edges, offsets, degree, u)
    bar = (degree + 12)[:, None] * U * S
    s_edge, S_edge = gc.table_edge_values(scalar[:, None], n_classes, N_EVEN, classes, edges, u)
    s_edge, s_error = s_edge[:, 0], 12 * U * S_edge[:, 0]
    if generic:
        pair = classes[edges[:, 0]] * n_classes + classes[edges[:, 1]]
        _, slope = gc.cubic_value(coefficients, pair, u / 256.0)
        slope = np.abs(slope) / 256.0 * ((D + 2) * U * np.abs(u))[:, None]               # [E, H + 1]
        bar = bar + gc.segment_sum(slope[:, :-1], offsets, degree)
        s_error = s_error + slope[:, -1]
    return want, bar, s_edge, s_error


def _check_messages(got, want, bar, degree, mean, label):
    scale = (1.0 / np.maximum(degree, 1))[:, None] if mean else 1.0
    error = np.abs(got.astype(np.float64) - want * scale)
    assert np.all(np.isfinite(got)) and np.all(error <= bar * scale), (label, np.argwhere(~(error <= bar * scale))[:4])
    assert np.all(got[degree == 0] == 0.0)
    full = degree > 0
    ratio = float(np.max(error[full] / (bar * scale)[full]))
    MEASURED[label] = ratio
    return ratio


def _check_coordinates(cuda, got, coord, graph, s_edge, s_error, flags, mean, label, skip=()):
    """gather_cases.coord_bar with s_e the interpolated scalar, plus the scalar's own error through |d term / d s|."""
    edges, offsets, degree = graph[:3]
    s32 = s_edge.astype(np.float32)
    allowance = gc.transcendental_allowance(coord, edges, s32, flags, cuda) if flags else 0.0
    want, magnitude, _ = gc.coord_reference(coord, edges, offsets, degree, s_edge, flags, mean)
    _, sensitivity = gc.coord_terms(coord, edges, s_edge, flags)
    scale = (1.0 / np.maximum(degree, 1))[:, None] if mean else 1.0
    bar = gc.coord_bar(coord, degree, magnitude, flags, allowance) + gc.segment_sum(sensitivity * s_error[:, None], offsets,
                                                                                   degree) * scale
    error = np.abs(got.astype(np.float64) - want)
    keep = np.ones(len(degree), dtype=bool)
    keep[list(skip)] = False
    assert got.shape == coord.shape and np.all(np.isfinite(got))
    assert np.all(error[keep] <= bar[keep]), (label, np.argwhere(~(error <= bar) & keep[:, None])[:4])
    assert np.array_equal(got[degree == 0], coord[degree == 0])
    ratio = float(np.max(error[keep] / bar[keep]))
    MEASURED[label] = ratio
    return ratio, allowance


EXACT_CASES = [("axis", False, "listed"), ("axis", True, "shuffled"), ("line", False, "shuffled"), ("line", True, "listed")]


@pytest.mark.parametrize("D", [1, 3, 6])
@pytest.mark.parametrize("n_classes", [1, 3])
@pytest.mark.parametrize("H", [4, 32, 128, 256])
def test_gather_at_exact_points(cuda, H, n_classes, D):
    """Distances that are exact in binary32 (r^2, its root, u = k / 16 and t): the only errors are the weights' and the sums'.
    Per node and column against table_reference within (deg + 12) u S (_bars), both means, with and without `left`; the
    coordinate half per node and component within its bar, flags 0 and all flags.  The points cover cell 0 (u < 1, u = 0
    included), the last cell and u = n_even - 2 exactly ("axis"), and the status stays 0.  With the even tables a + b rho^2 the
    reference itself is within u S of the polynomial in cell 0 too (the reflection is exact), which is checked first.
    Measured on an MI355X: messages at most 0.23 of the bar, coordinates 0.68 (flags 0) and 0.74 (all flags, allowance at most
    6.65 u; where the sum is small against c_i the final addition's rounding is most of the bar)."""
    _hip, kernels = _pkg()
    classes = _classes(17, n_classes)
    for layout, even, ordering in EXACT_CASES:
        if layout == "line" and D < 2:
            continue
        graph = _graph(ordering)
        edges, offsets, degree, order = graph
        tables = _table(n_classes, H, even)
        coord = _exact_coordinates(layout, D, order)
        u = gc.edge_u(coord, edges, 256.0)
        assert np.array_equal(u * 16, np.round(u * 16)) and u.max() <= N_EVEN - 2
        assert np.any((u > 0) & (u < 1)) and np.any(u == 0) and np.any((u > N_EVEN - 3) & (u < N_EVEN - 2))
        assert layout != "axis" or np.any(u == N_EVEN - 2)
        want, bar, s_edge, s_error = _bars(tables, n_classes, classes, graph, coord, u, generic=False)
        if even:
            pair = classes[edges[:, 0]] * n_classes + classes[edges[:, 1]]
            values, magnitudes = gc.table_edge_values(tables[1], n_classes, N_EVEN, classes, edges, u)
            truth, _ = gc.cubic_value(tables[0], pair, u / 256.0)
            assert np.all(np.abs(values - truth[:, :H]) <= (1 + 1e-6) * U * magnitudes)
        for mean in (False, True):
            label = (H, n_classes, D, layout, even, mean)
            got, coord_got, word = _gather(kernels, cuda, tables, n_classes, classes, graph, coord, mean, mean, 0)
            assert word == 0 and got.shape == (17, H)
            ratio = _check_messages(got, want, bar, degree, mean, ("exact",) + label)
            left = np.random.default_rng(H).standard_normal((17, H)).astype(np.float32)
            wide, coord_all, word = _gather(kernels, cuda, tables, n_classes, classes, graph, coord, mean, mean, 3, left=left)
            assert word == 0 and np.array_equal(wide.view(np.uint32), np.concatenate([left, got], axis=1).view(np.uint32))
            ratio_c, _ = _check_coordinates(cuda, coord_got, coord, graph, s_edge, s_error, 0, mean, ("exact coord 0",) + label)
            ratio_f, allowance = _check_coordinates(cuda, coord_all, coord, graph, s_edge, s_error, 3, mean,
                                                    ("exact coord 3",) + label)
            print(f"exact H {H} classes {n_classes} D {D} {layout} even {even} mean {mean}: messages {ratio:.3f} of the bar, "
                  f"coordinates {ratio_c:.3f} (flags 0), {ratio_f:.3f} (flags 3, allowance {allowance / U:.2f} u)")


@pytest.mark.parametrize("D", [1, 3, 6])
@pytest.mark.parametrize("n_classes", [1, 3])
@pytest.mark.parametrize("H", [4, 32, 128, 256])
def test_gather_at_generic_points(cuda, H, n_classes, D):
    """Random binary32 coordinates inside the grid, the reference at the float64 u of the same coordinates: the bar of the exact
    points plus |dF/du| (D + 2) u |u| per edge for the kernel's binary32 u (_bars); the coordinate half with the scalar's error
    carried through.  Both means, flags 0 and all flags, both orderings.
    Measured on an MI355X: messages at most 0.19 of the bar, coordinates 0.43 (flags 0) and 0.88 (all flags, allowance at most
    10.06 u)."""
    _hip, kernels = _pkg()
    classes = _classes(17, n_classes, seed=8)
    tables = _table(n_classes, H, False)
    for ordering in sorted(gc.ORDERINGS):
        graph = _graph(ordering)
        edges, offsets, degree, _ = graph
        coord = _generic_coordinates(D, 17, seed=D + len(ordering))
        u = gc.edge_u(coord, edges, 256.0)
        assert u.max() < N_EVEN - 2 - 0.5 and np.any(u > 0)
        want, bar, s_edge, s_error = _bars(tables, n_classes, classes, graph, coord, u, generic=True)
        for mean in (False, True):
            label = (H, n_classes, D, ordering, mean)
            got, coord_got, word = _gather(kernels, cuda, tables, n_classes, classes, graph, coord, mean, mean, 0)
            _, coord_all, word_all = _gather(kernels, cuda, tables, n_classes, classes, graph, coord, mean, not mean, 3)
            assert word == 0 and word_all == 0
            ratio = _check_messages(got, want, bar, degree, mean, ("generic",) + label)
            ratio_c, _ = _check_coordinates(cuda, coord_got, coord, graph, s_edge, s_error, 0, mean, ("generic coord 0",) + label)
            ratio_f, allowance = _check_coordinates(cuda, coord_all, coord, graph, s_edge, s_error, 3, not mean,
                                                    ("generic coord 3",) + label)
            print(f"generic H {H} classes {n_classes} D {D} {ordering} mean {mean}: messages {ratio:.3f} of the bar, "
                  f"coordinates {ratio_c:.3f} (flags 0), {ratio_f:.3f} (flags 3, allowance {allowance / U:.2f} u)")


@pytest.mark.parametrize("H,n_classes,D", [(32, 3, 3), (256, 1, 1)])
def test_gather_reports_a_distance_beyond_the_grid(cuda, H, n_classes, D):
    """One edge with u = n_even - 2 + 1/16 raises MDX_STATUS_EGNN_TABLE; every node but that edge's is still within its bar."""
    _hip, kernels = _pkg()
    classes = _classes(17, n_classes)
    edges, offsets, degree, order = _graph("listed")
    hub, far = int(order[0]), int(order[AXIS_K.index(LAST)])
    coord = _exact_coordinates("axis", D, order)
    coord[far, D - 1] = np.float32((LAST + 1) * STEP)
    edges = edges.copy()
    pinned = offsets[hub] + 2 + AXIS_K.index(LAST)
    assert edges[pinned, 0] == hub and edges[pinned, 1] == far
    again = np.flatnonzero(((edges[:, 0] == hub) & (edges[:, 1] == far)) | ((edges[:, 0] == far) & (edges[:, 1] == hub)))
    edges[again[again != pinned], 1] = edges[again[again != pinned], 0]
    u = gc.edge_u(coord, edges, 256.0)
    assert np.sum(u > N_EVEN - 2) == 1 and u[pinned] == N_EVEN - 2 + 1.0 / 16
    graph = (edges, offsets, degree, order)
    tables = _table(n_classes, H, False)
    got, coord_got, word = _gather(kernels, cuda, tables, n_classes, classes, graph, coord, False, False, 0)
    assert word & _hip.STATUS_EGNN_TABLE
    want, bar, s_edge, s_error = _bars(tables, n_classes, classes, graph, coord, u, generic=False)
    others = np.arange(17) != hub
    _check_messages(got[others], want[others], bar[others], degree[others], False, ("beyond", H))
    _check_coordinates(cuda, coord_got, coord, graph, s_edge, s_error, 0, False, ("beyond coord", H), skip=(hub,))
    # the same problem without that edge's excess: no report
    coord[far, D - 1] = np.float32(LAST * STEP)
    assert _gather(kernels, cuda, tables, n_classes, classes, graph, coord, False, False, 0)[2] == 0


@pytest.mark.parametrize("n_classes", [1, 3])
def test_gather_reports_a_class_outside_the_table(cuda, n_classes):
    """A node of class -1 or n_classes raises the bit; so does a node that is only ever a DESTINATION (the launch covers the
    first 16 nodes, node 16 is reached through edges alone); valid classes leave the word at 0."""
    _hip, kernels = _pkg()
    H, D = 32, 3
    edges, offsets, degree, order = _graph("listed")
    graph = (edges, offsets, degree, order)
    tables = _table(n_classes, H, False)
    coord = _exact_coordinates("axis", D, order)
    classes = _classes(17, n_classes)
    for node in (0, 9):                    # node 0 has no edges: a source is checked whatever its degree
        for bad in (-1, n_classes):
            wrong = classes.copy()
            wrong[node] = bad
            assert _gather(kernels, cuda, tables, n_classes, wrong, graph, coord, False, False, 0)[2] & _hip.STATUS_EGNN_TABLE
    assert _gather(kernels, cuda, tables, n_classes, classes, graph, coord, False, False, 0)[2] == 0
    n = 16
    assert np.any(edges[:offsets[n], 1] == n)
    _, table, scalar = tables
    for bad, expected in ((classes[n], False), (-1, True), (n_classes, True)):
        wrong = classes.copy()
        wrong[n] = bad
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        out, coord_out = torch.empty(n, H, device=cuda), torch.empty(n, D, device=cuda)
        _hip.call("mdx_egnn_table_gather", _dev(table, cuda), _dev(scalar, cuda), H, n_classes, N_EVEN, kernels.TABLE_INV_SPACING,
                  _dev(wrong, cuda), _dev(offsets[:n], cuda), _dev(degree[:n], cuda), n, 0, None, out, _dev(coord, cuda), D,
                  _dev(edges, cuda), 0, 0, coord_out, status)
        assert bool(int(status.item()) & _hip.STATUS_EGNN_TABLE) == expected


def test_gather_refuses_a_width_above_256(cuda):
    _hip, kernels = _pkg()
    edges, offsets, degree, order = _graph("listed")
    with pytest.raises(_hip.MdxError, match="unsupported"):
        kernels.egnn_table_gather(torch.zeros(K, 260, device=cuda), torch.zeros(K, device=cuda), 1, N_EVEN,
                                  torch.zeros(17, dtype=torch.int64, device=cuda), _dev(offsets, cuda), _dev(degree, cuda), False, None,
                                  torch.zeros(17, 3, device=cuda), _dev(edges, cuda), False)


# ---- mdx_egnn_table_check
def _check_table(n_classes, H):
    """[n_pairs, K, H + 1] float32: even rows a cubic, midpoint rows the check's own formula in binary32 -- a table whose every
    midpoint error is exactly zero."""
    _, table = gc.cubic_table(n_classes, N_EVEN, H + 1, 256.0, seed=77 + H)
    blocks = table.reshape(n_classes * n_classes, K, H + 1).copy()
    for p in range(blocks.shape[0]):
        blocks[p, N_EVEN:] = gc.midpoint_rows(blocks[p, :N_EVEN], N_EVEN)
    return blocks


def _run_check(kernels, cuda, blocks, n_classes, sigma=(0.05, 0.05, 0.05)):
    """(worst, status word) of one check; the workspace must come back zeroed."""
    H = blocks.shape[2] - 1
    flat = blocks.reshape(-1, H + 1)
    workspace = torch.zeros(n_classes ** 2 * (H + 2), dtype=torch.int32, device=cuda)
    worst = torch.full((1,), -1.0, dtype=torch.float32, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    kernels.egnn_table_check(_dev(flat[:, :H], cuda), _dev(flat[:, H], cuda), n_classes, N_EVEN,
                             torch.tensor(sigma, dtype=torch.float32, device=cuda), workspace, worst=worst, status=status)
    assert not bool(workspace.any()), "the check left its workspace dirty"
    return float(worst.item()), int(status.item())


def _largest(blocks, p):
    """The pair's largest |value| over what the check reads: every even row and the midpoints j <= n_even - 3."""
    return float(np.abs(blocks[p, :K - 1]).max())


@pytest.mark.parametrize("n_classes", [1, 3])
@pytest.mark.parametrize("H", [4, 32, 256])
def test_check_measures_one_wrong_midpoint(cuda, H, n_classes):
    """A table made by the check's formula: worst == 0, status 0.  Then delta on ONE midpoint j of one (pair, column), at the
    first and last midpoint of each chunk of 32 (j = 0 reads the reflected row): worst == delta / big to 2 u (the kernel's
    subtraction and division; delta is what the perturbed binary32 value really differs by, big the pair's largest |value|),
    the bit raised at delta / big = 2 TABLE_TOLERANCE and not at TABLE_TOLERANCE / 2.  The midpoint n_even - 2, which no cell
    of the gather uses, changes nothing.  The workspace is zero after every call (_run_check)."""
    _hip, kernels = _pkg()
    perfect = _check_table(n_classes, H)
    n_pairs = n_classes * n_classes
    assert _run_check(kernels, cuda, perfect, n_classes) == (0.0, 0)
    columns = [0, H - 1, H, H // 2]                         # column H is the scalar (H = 256: a thread's second column)
    for index, j in enumerate([0, 31, 32, N_EVEN - 3]):
        p, c = (index * 5 + 2) % n_pairs, columns[index]
        for ratio, raised in ((2.0 * kernels.TABLE_TOLERANCE, True), (0.5 * kernels.TABLE_TOLERANCE, False)):
            blocks = perfect.copy()
            blocks[p, N_EVEN + j, c] = np.float32(np.float64(perfect[p, N_EVEN + j, c]) + ratio * _largest(perfect, p))
            delta = abs(np.float64(blocks[p, N_EVEN + j, c]) - np.float64(perfect[p, N_EVEN + j, c]))
            expected = delta / _largest(blocks, p)
            assert 0.9 * ratio < expected < 1.1 * ratio
            worst, word = _run_check(kernels, cuda, blocks, n_classes)
            assert abs(worst - expected) <= 2 * U * expected, (j, p, c, worst, expected)
            assert bool(word & _hip.STATUS_EGNN_TABLE) == raised
            MEASURED[("check", H, n_classes, j, raised)] = abs(worst - expected) / (U * expected)
            # the unused midpoint on top, far beyond every value of the table: the same answer
            blocks[p, N_EVEN + N_EVEN - 2, :] = 1.0e6
            assert _run_check(kernels, cuda, blocks, n_classes) == (worst, word)
    unused = perfect.copy()
    unused[:, N_EVEN + N_EVEN - 2, :] += 1000.0
    assert _run_check(kernels, cuda, unused, n_classes) == (0.0, 0)


@pytest.mark.parametrize("n_classes", [1, 3])
def test_check_reports_nan_and_unequal_sigma(cuda, n_classes):
    """A NaN anywhere the check reads -- an even row, a midpoint, the scalar -- raises the bit; so does a sigma that is not
    uniform over the batch, with a perfect table (worst stays 0).  One sigma alone is uniform."""
    _hip, kernels = _pkg()
    H = 32
    perfect = _check_table(n_classes, H)
    last = n_classes * n_classes - 1
    for row, column in ((0, 3), (N_EVEN - 1, 0), (17, H), (N_EVEN + 35, H - 1), (N_EVEN + 3, H)):
        blocks = perfect.copy()
        blocks[last, row, column] = np.nan
        assert _run_check(kernels, cuda, blocks, n_classes)[1] & _hip.STATUS_EGNN_TABLE, (row, column)
    for sigma in ((0.05, 0.05, 0.06), (0.06, 0.05, 0.05), (0.05, float("nan"), 0.05)):
        worst, word = _run_check(kernels, cuda, perfect, n_classes, sigma=sigma)
        assert worst == 0.0 and word & _hip.STATUS_EGNN_TABLE
    assert _run_check(kernels, cuda, perfect, n_classes, sigma=(0.05,)) == (0.0, 0)
