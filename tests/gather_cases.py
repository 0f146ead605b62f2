"""Inputs and float64 restatements for the per-node end of an EGNN layer (segment_combine_kernel, egnn_node_gather_kernel,
egnn_coord_aggregate_kernel, egnn_table_gather_kernel: csrc/mdx_egnn_node.hip; egnn_table_check_kernel: csrc/mdx_egnn_table.hip).

Everything here is numpy / torch on the CPU and states a contract from its documentation (include/mdx_hip.h), not from the
kernel that implements it: the compact piece layout, the coordinate update, the cubic interpolation on the distance grid."""
import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of binary32
WAVE = 64               # edges of a node per pass of egnn_node_gather_kernel / egnn_table_gather_kernel (one per lane)
BUTTERFLY = 6           # additions on the way from 64 lane sums to one
COORD_NORMALIZE, COORD_TANH = 1, 2          # MDX_EGNN_COORD_* (asserted against the header by the GPU tests)

# every length class of a node's edge range against the 16-edge groups of the piece layout and the 64-lane passes: empty
# (node 0 and an interior node), one edge, 15 / 16 / 17, 31 / 32 / 33, 63 / 64 / 65, 127 / 128 / 129, 200, and a non-empty last
DEGREES = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200, 0, 3]
# the same list in another order: other residues of the nodes' first and last edges modulo 16 (see _check_ordering)
DEGREES_SHUFFLED = [0, 64, 15, 31, 65, 0, 127, 129, 1, 17, 200, 32, 16, 63, 3, 33, 128]
ORDERINGS = {"listed": DEGREES, "shuffled": DEGREES_SHUFFLED}


def _check_ordering(degrees):
    """What both orderings must hold for the piece layout's branches to run: some node's last edge at 15 mod 16 (its last
    piece is a boundary row), some non-empty node's first edge at 0 mod 16, some node's at neither; a node inside one 16-edge
    group and a node across several; node 0 and an interior node empty, the last one not."""
    degree = np.asarray(degrees, dtype=np.int64)
    first = np.cumsum(degree) - degree
    last = first + degree - 1
    full = degree > 0
    assert np.any(last[full] % 16 == 15), "no node ends on a boundary edge"
    assert np.any(first[full] % 16 == 0), "no node starts a 16-edge group"
    assert np.any((last[full] % 16 != 15) & (first[full] % 16 != 0))
    assert np.any(full & (first // 16 == last // 16)) and np.any(last // 16 - first // 16 >= 2)
    assert degree[0] == 0 and np.any(degree[1:-1] == 0) and degree[-1] > 0
    assert sorted(degrees) == sorted(DEGREES)


for _degrees in ORDERINGS.values():
    _check_ordering(_degrees)
# the shuffled list adds what the listed one lacks: a node that BEGINS on a boundary edge (a piece of one edge) ...
_first = np.cumsum(DEGREES_SHUFFLED) - np.asarray(DEGREES_SHUFFLED)
assert np.any((_first % 16 == 15) & (np.asarray(DEGREES_SHUFFLED) > 1))
# ... and the two disagree on where the groups fall
assert not np.array_equal(_first % 16, (np.cumsum(DEGREES) - np.asarray(DEGREES)) % 16)


def ragged_graph(degrees, n_nodes, seed):
    """(edges [E, 2] int64 sorted by source, offsets [n_nodes], degree [n_nodes]) of a graph whose node i has degrees[i] edges.
    Destinations are random over all nodes; every node with two edges or more has a self-loop as its second edge."""
    assert len(degrees) == n_nodes
    degree = np.asarray(degrees, dtype=np.int64)
    offsets = np.cumsum(degree) - degree
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(n_nodes, dtype=np.int64), degree)
    dst = rng.integers(0, n_nodes, size=src.shape[0], dtype=np.int64)
    loops = offsets[degree >= 2] + 1
    dst[loops] = src[loops]
    assert np.all(np.diff(src) >= 0) and np.any(dst == src) and np.any(dst != src)
    return np.stack([src, dst], axis=1), offsets, degree


def piece_rows(node, e0, e1, n_edges):
    """The rows of the compact piece buffer that belong to node `node` with the edges [e0, e1), in edge order, each with the
    edge range it sums: [(row, first edge, last edge + 1), ...].  include/mdx_hip.h, MDX_EGNN_MESSAGES_PIECE_SUMS: the edges of
    the node inside the group [16 k, 16 k + 16) land in row k when the group's last edge is the node's, otherwise -- the node's
    last edge is inside the group -- in the node's own row ceil(n_edges / 16) + node."""
    rows = []
    start = e0
    while start < e1:
        group_end = (start | 15) + 1                      # one past the boundary edge of start's group
        if group_end <= e1:
            rows.append((start >> 4, start, group_end))
        else:
            rows.append((((n_edges + 15) >> 4) + node, start, e1))
        start = min(group_end, e1)
    return rows


def pieces_from_messages(messages64, offsets, degree, rounded=True):
    """The compact piece buffer [ceil(E / 16) + n_nodes, H] that holds the per-group sums of messages64 [E, H]: float64 sums,
    rounded to binary32 once at the end (rounded=False: left in float64).  Rows that no node owns are NaN."""
    messages64 = np.asarray(messages64, dtype=np.float64)
    n_edges, n_nodes = messages64.shape[0], len(degree)
    assert n_edges == int(np.sum(degree))
    pieces = np.full((((n_edges + 15) >> 4) + n_nodes, messages64.shape[1]), np.nan)
    for node in range(n_nodes):
        e0 = int(offsets[node])
        for row, first, end in piece_rows(node, e0, e0 + int(degree[node]), n_edges):
            assert np.all(np.isnan(pieces[row])), "two pieces claim one row"
            pieces[row] = messages64[first:end].sum(axis=0)
    return pieces.astype(np.float32) if rounded else pieces


def combine_pieces(pieces, offsets, degree, dtype):
    """"Add a node's pieces in edge order", starting from zero, in `dtype` arithmetic: ([n_nodes, H] sums, the rows read in
    order).  In np.float32 this is the summation order mdx_segment_combine promises, bit for bit."""
    n_nodes = len(degree)
    n_edges = int(np.sum(degree))
    out = np.zeros((n_nodes, pieces.shape[1]), dtype=dtype)
    read = []
    for node in range(n_nodes):
        e0 = int(offsets[node])
        for row, _, _ in piece_rows(node, e0, e0 + int(degree[node]), n_edges):
            out[node] = out[node] + pieces[row].astype(dtype)
            read.append(row)
    return out, read


def piece_counts(offsets, degree):
    """P_i: the number of pieces of each node."""
    n_edges = int(np.sum(degree))
    return np.array([len(piece_rows(i, int(offsets[i]), int(offsets[i] + degree[i]), n_edges)) for i in range(len(degree))])


def segment_sum(values, offsets, degree):
    """[n_nodes, ...] float64 sums of values [E, ...] over each node's edge range."""
    values = np.asarray(values, dtype=np.float64)
    out = np.zeros((len(degree),) + values.shape[1:])
    for node in range(len(degree)):
        out[node] = values[int(offsets[node]):int(offsets[node] + degree[node])].sum(axis=0)
    return out


# ---- the coordinate update: coord_out[i] = coord[i] + (1 / degree_i if mean) sum_e (f_e (coord[i] - coord[dst_e])) s'_e
def coord_terms(coord32, edges, s64, flags):
    """The per-edge, per-component terms [E, D] in float64 from binary32 coordinates: (c_i - c_j) s, with s <- tanh(s) under
    COORD_TANH and the difference scaled by tanh(r^2) / sqrt(r^2 + 1e-16) under COORD_NORMALIZE, r^2 summed in component order.
    Also returns |d term / d s| [E, D], what an error of s is multiplied by (tanh' <= 1)."""
    coord = np.asarray(coord32, dtype=np.float32).astype(np.float64)
    diff = coord[edges[:, 0]] - coord[edges[:, 1]]
    s = np.asarray(s64, dtype=np.float64)
    if flags & COORD_TANH:
        s = np.tanh(s)
    if flags & COORD_NORMALIZE:
        r2 = np.zeros(diff.shape[0])
        for k in range(diff.shape[1]):
            r2 = r2 + diff[:, k] * diff[:, k]
        diff = (np.tanh(r2) / np.sqrt(r2 + 1e-16))[:, None] * diff
    return diff * s[:, None], np.abs(diff)


def coord_reference(coord32, edges, offsets, degree, s64, flags, mean):
    """(coord_out [n_nodes, D] float64, sum over the node's edges of |term| (divided like the sum), the terms [E, D])."""
    terms, _ = coord_terms(coord32, edges, s64, flags)
    scale = (1.0 / np.maximum(degree, 1))[:, None] if mean else 1.0
    total = segment_sum(terms, offsets, degree) * scale
    return np.asarray(coord32, dtype=np.float64) + total, segment_sum(np.abs(terms), offsets, degree) * scale, terms


def torch_float32_terms(coord32, edges, s32, flags, device):
    """The same terms from plain torch float32 operations on `device` -- a second binary32 evaluation, independent of the
    kernels under test, to size what tanhf, sqrtf and the division may cost (transcendental_allowance)."""
    coord = torch.as_tensor(np.asarray(coord32, dtype=np.float32)).to(device)
    index = torch.as_tensor(edges).to(device)
    s = torch.as_tensor(np.asarray(s32, dtype=np.float32)).to(device)
    diff = coord[index[:, 0]] - coord[index[:, 1]]
    if flags & COORD_TANH:
        s = torch.tanh(s)
    if flags & COORD_NORMALIZE:
        r2 = torch.zeros_like(s)
        for k in range(diff.shape[1]):
            r2 = r2 + diff[:, k] * diff[:, k]
        diff = (torch.tanh(r2) / torch.sqrt(r2 + 1e-16))[:, None] * diff
    return (diff * s[:, None]).double().cpu().numpy()


def transcendental_allowance(coord32, edges, s32, flags, device):
    """Twice the worst relative distance, over the non-zero terms of these very inputs, between torch's float32 evaluation on
    `device` and float64 (twice: two independent binary32 evaluations may err in opposite directions).  A term that is zero in
    float64 (c_i == c_j) must be zero in float32 too."""
    want, _ = coord_terms(coord32, edges, np.asarray(s32, dtype=np.float32).astype(np.float64), flags)
    got = torch_float32_terms(coord32, edges, s32, flags, device)
    zero = want == 0.0
    assert np.all(got[zero] == 0.0) and np.all(np.isfinite(got))
    return 2.0 * float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])))


def coord_bar(coord32, degree, magnitude, flags, allowance, sequential=False):
    """The bar on coord_out[i, k], from the kernels' own sequence of operations (written down before any measurement).

    egnn_node_gather_kernel and egnn_table_gather_kernel, per component k, with T = sum_e |term_e| over the node's exact terms:
      * a term is fl(fl(c_i - c_j) s): 2 roundings (difference, product); under COORD_NORMALIZE fl(fl(f fl(c_i - c_j)) s), one
        more, with f's own error in the allowance below;
      * lane l adds its terms e0 + l, e0 + l + 64, ...: ceil(deg / 64) of them onto zero, ceil(deg / 64) - 1 roundings;
      * the butterfly over the 64 lanes: 6 additions on the path of every term;
      * the mean's division: 1;
      * the final c_i + total: 1 rounding of the result, u (|c_i| + |total|): 1 on T and the separate u |c_i|.
    Sum: (ceil(deg / 64) - 1 + 6 + 2 + 1 + 1) u T = (ceil(deg / 64) + 6 + 3) u T, to first order; without the mean one of them
    is spare, and the largest second-order part, (1 + u)^14 - 1 = 14 u (1 + 4e-7), is far inside what a worst case leaves unused.
    egnn_coord_aggregate_kernel (sequential=True) adds the node's terms one after the other: the chain is deg instead of
    ceil(deg / 64) + 6.
    allowance: the relative error granted per term to tanhf, sqrtf and the division of the flags (0 without flags), measured
    against a second binary32 evaluation and not against the kernel (transcendental_allowance).
    magnitude is T [n_nodes, D], already divided by deg under the mean."""
    degree = np.asarray(degree, dtype=np.float64)
    chain = degree if sequential else np.ceil(degree / WAVE) + BUTTERFLY
    roundings = chain + 3 + (1 if flags & COORD_NORMALIZE else 0)
    return (roundings[:, None] * U + allowance) * magnitude + U * np.abs(np.asarray(coord32, dtype=np.float64))


# ---- the distance grid: rows p K + m at rho = m h (m < n_even), p K + n_even + j at (j + 1/2) h; K = 2 n_even - 1
COEFFICIENT_SCALE = (1.0, 20.0, 400.0, 8000.0)       # all four terms of a cubic matter on rho <= 0.15


def grid_rho(n_even, inv_spacing):
    r = np.arange(2 * n_even - 1, dtype=np.float64)
    return np.where(r < n_even, r, r - n_even + 0.5) / inv_spacing


def cubic_table(n_classes, n_even, columns, inv_spacing, seed, even=False):
    """(coefficients [n_pairs, columns, 4], table [n_pairs K, columns] float32): an independent random cubic in rho per class
    pair and column, evaluated in float64 at the grid's points and rounded to binary32.  even=True: a + b rho^2 (what the
    reflection at rho = 0 reproduces exactly)."""
    rng = np.random.default_rng(seed)
    n_pairs = n_classes * n_classes
    coefficients = rng.standard_normal((n_pairs, columns, 4)) * np.asarray(COEFFICIENT_SCALE)
    if even:
        coefficients[..., 1] = 0.0
        coefficients[..., 3] = 0.0
    rho = grid_rho(n_even, inv_spacing)
    powers = np.stack([rho ** 0, rho, rho ** 2, rho ** 3], axis=1)               # [K, 4]
    values = np.einsum("kq,pcq->pkc", powers, coefficients)
    return coefficients, values.reshape(n_pairs * rho.shape[0], columns).astype(np.float32)


def cubic_value(coefficients, pair, rho):
    """F [E, columns] and dF/drho [E, columns] of the cubics of `pair` [E] at rho [E]."""
    c = coefficients[pair]                                                      # [E, columns, 4]
    r = rho[:, None]
    return (c[..., 0] + r * (c[..., 1] + r * (c[..., 2] + r * c[..., 3])),
            c[..., 1] + r * (2.0 * c[..., 2] + r * 3.0 * c[..., 3]))


def lagrange_weights(t):
    """4-point Lagrange weights [E, 4] on the nodes -1, 0, 1, 2 at t, float64."""
    t = np.asarray(t, dtype=np.float64)
    return np.stack([-(t * (t - 1.0) * (t - 2.0)) / 6.0, ((t + 1.0) * (t - 1.0) * (t - 2.0)) / 2.0,
                     -((t + 1.0) * t * (t - 2.0)) / 2.0, ((t + 1.0) * t * (t - 1.0)) / 6.0], axis=1)


def table_edge_values(table32, n_classes, n_even, classes, edges, u):
    """Per edge: the float64 Lagrange interpolation [E, columns] of the binary32 table at float64 u [E] (u = rho inv_spacing),
    and the sum over its four points of |w v| [E, columns].  The cell is the documented one: m = min(floor(u), n_even - 3), and
    the left neighbour of cell 0 is the point right of it (F is even in rho)."""
    table = np.asarray(table32, dtype=np.float32).astype(np.float64)
    K = 2 * n_even - 1
    assert table.shape[0] == n_classes * n_classes * K
    u = np.asarray(u, dtype=np.float64)
    m = np.minimum(np.floor(u).astype(np.int64), n_even - 3)
    w = lagrange_weights(u - m)
    pair = classes[edges[:, 0]] * n_classes + classes[edges[:, 1]]
    row = pair * K + m
    rows = np.stack([np.where(m > 0, row - 1, row + 1), row, row + 1, row + 2], axis=1)        # [E, 4]
    products = w[:, :, None] * table[rows]                                                     # [E, 4, columns]
    return products.sum(axis=1), np.abs(products).sum(axis=1)


def table_reference(table32, n_classes, n_even, classes, edges, offsets, degree, u):
    """Per node: the sum over its edges of the interpolated table values [n_nodes, columns], and S = the sum over its edges and
    over the four points of |w v|."""
    values, magnitudes = table_edge_values(table32, n_classes, n_even, classes, edges, u)
    return segment_sum(values, offsets, degree), segment_sum(magnitudes, offsets, degree)


def edge_u(coord32, edges, inv_spacing):
    """float64 u = |c_i - c_j| inv_spacing [E] from binary32 coordinates."""
    coord = np.asarray(coord32, dtype=np.float32).astype(np.float64)
    diff = coord[edges[:, 0]] - coord[edges[:, 1]]
    return np.sqrt((diff * diff).sum(axis=1)) * inv_spacing


def midpoint_rows(even32, n_even):
    """The midpoint rows j < n_even - 1 from even rows [n_even, columns] by mdx_egnn_table_check's own formula in binary32:
    ((w0 v0 + w1 v1) + w2 v2) + w3 v3 with w = (-1, 9, 9, -1) / 16 and v0 of j = 0 the row right of it.  The last midpoint
    j = n_even - 2 (which the check does not read: it has no row j + 2) takes the plain mean of its neighbours."""
    even = np.asarray(even32, dtype=np.float32)
    w0, w1 = np.float32(-0.0625), np.float32(0.5625)
    j = np.arange(n_even - 2)
    v0, v1, v2, v3 = even[np.where(j > 0, j - 1, 1)], even[j], even[j + 1], even[j + 2]
    mid = ((w0 * v0 + w1 * v1) + w1 * v2) + w0 * v3
    assert mid.dtype == np.float32
    return np.concatenate([mid, (np.float32(0.5) * (even[-2] + even[-1]))[None]], axis=0)
