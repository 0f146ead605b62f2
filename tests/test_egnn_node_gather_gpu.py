"""mdx_segment_combine, mdx_egnn_node_gather and mdx_egnn_coord_aggregate (csrc/mdx_egnn_node.hip), each called directly, against
float64 restatements of their contracts (tests/gather_cases.py) with a bar per node and per column / component.

The pieces are NOT the edge chain's: gather_cases.pieces_from_messages writes the documented compact layout on its own, with NaN
in every row that no node owns, so a kernel that reads a row it should not read shows up as a NaN."""
import functools

import numpy as np
import pytest
import torch

import gather_cases as gc

pytestmark = pytest.mark.gpu

U = gc.U
WIDTHS = [4, 32, 64, 128, 256, 260]          # 260: 65 quads, the second pass of a wavefront over the columns
DIMENSIONS = [1, 2, 3, 4, 6, 8]
PAD = 64                                     # guard floats on either side of an output (a multiple of 4: 16-byte stores)
MEASURED = {}


def _pkg():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    assert (_hip.EGNN_COORD_NORMALIZE, _hip.EGNN_COORD_TANH) == (gc.COORD_NORMALIZE, gc.COORD_TANH)
    return _hip, kernels


@functools.lru_cache(maxsize=None)
def _graph(ordering):
    degrees = gc.ORDERINGS[ordering]
    return gc.ragged_graph(degrees, len(degrees), seed=20 + len(ordering))


@functools.lru_cache(maxsize=None)
def _message_case(H, ordering):
    """(pieces float32 with NaN in the unowned rows, left float32) -- computed once, never modified."""
    edges, offsets, degree = _graph(ordering)
    rng = np.random.default_rng(100 + H)
    pieces = gc.pieces_from_messages(rng.standard_normal((edges.shape[0], H)), offsets, degree)
    assert np.isnan(pieces).any()
    return pieces, rng.standard_normal((len(degree), H)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _coord_case(D, ordering):
    """(coord float32 [n, D], edge scalar float32 [E]); two distinct nodes joined by an edge sit at the same place."""
    edges, offsets, degree = _graph(ordering)
    rng = np.random.default_rng(200 + D)
    coord = (0.5 * rng.standard_normal((len(degree), D))).astype(np.float32)
    a, b = edges[np.flatnonzero(edges[:, 0] != edges[:, 1])[0]]
    coord[b] = coord[a]
    return coord, rng.standard_normal(edges.shape[0]).astype(np.float32)


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


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("ordering", sorted(gc.ORDERINGS))
@pytest.mark.parametrize("H", WIDTHS)
def test_message_sums(cuda, H, ordering, mean):
    """out[i, :] = (1 / degree_i if mean) x the sum of node i's pieces.

    Against the float64 sum of the binary32 pieces, per node and column, within (P_i + 1) u sum |piece| (P_i pieces: P_i - 1
    rounded additions -- the first one adds to zero -- and the mean's division; one u to spare for the second order).  In sum mode
    also the very bits of the binary32 sum taken in increasing edge order, which is what include/mdx_hip.h promises.  Nodes without
    edges give exact zeros; with `left` the row is [left | sums] bit for bit; mdx_segment_combine and the message half of
    mdx_egnn_node_gather give the same bits, and the latter's coordinates do not depend on the message half being there.
    Nothing is written outside [n_nodes, H].  Measured on an MI355X: at most 0.66 of the bar."""
    _hip, kernels = _pkg()
    edges, offsets, degree = _graph(ordering)
    n, E = len(degree), edges.shape[0]
    pieces, left = _message_case(H, ordering)
    coord, scalar = _coord_case(3, ordering)
    d_pieces, d_left, d_off, d_deg, d_edges = (_dev(x, cuda) for x in (pieces, left, offsets, degree, edges))
    d_coord, d_scalar = _dev(coord, cuda), _dev(scalar, cuda)

    buffer, out = _guarded(n, H, cuda)
    _hip.call("mdx_segment_combine", d_pieces, E, d_off, d_deg, n, H, int(mean), None, out)
    got = out.cpu().numpy()
    assert _untouched(buffer, n, H)
    buffer2, out2 = _guarded(n, H, cuda)
    coord_buffer, coord_out = _guarded(n, 3, cuda)
    _hip.call("mdx_egnn_node_gather", d_pieces, E, d_off, d_deg, n, H, int(mean), None, out2, d_scalar, d_coord, 3, d_edges, 0, 0,
              coord_out)
    assert _untouched(buffer2, n, H) and _untouched(coord_buffer, n, 3)
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(got))
    _, coord_alone = kernels.egnn_node_gather(None, E, d_off, d_deg, mean, None, d_scalar, d_coord, d_edges, False)
    assert torch.equal(coord_alone, coord_out)

    scale = (1.0 / np.maximum(degree, 1))[:, None] if mean else 1.0
    want, _ = gc.combine_pieces(pieces, offsets, degree, np.float64)
    magnitude, _ = gc.combine_pieces(np.abs(pieces), offsets, degree, np.float64)
    bar = (gc.piece_counts(offsets, degree) + 1)[:, None] * U * magnitude * scale
    error = np.abs(got.astype(np.float64) - want * scale)
    assert np.all(np.isfinite(got)) and np.all(error <= bar), np.argwhere(~(error <= bar))[:4]
    assert np.all(_bits(got[degree == 0]) == 0)
    ratio = float(np.max(error[degree > 0] / bar[degree > 0]))
    MEASURED[("messages", H, ordering, mean)] = ratio
    print(f"messages H {H} {ordering} mean {mean}: worst error / bar {ratio:.3f}")
    if not mean:
        ordered, _ = gc.combine_pieces(pieces, offsets, degree, np.float32)
        assert np.array_equal(_bits(got), _bits(ordered))

    wide = kernels.segment_combine(d_pieces, E, d_off, d_deg, mean, left=d_left).cpu().numpy()
    wide2, _ = kernels.egnn_node_gather(d_pieces, E, d_off, d_deg, mean, d_left, d_scalar, d_coord, d_edges, False)
    assert wide.shape == (n, 2 * H)
    assert np.array_equal(_bits(wide), _bits(np.concatenate([left, got], axis=1)))
    assert np.array_equal(_bits(wide2.cpu().numpy()), _bits(wide))


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("ordering", sorted(gc.ORDERINGS))
@pytest.mark.parametrize("D", DIMENSIONS)
def test_coordinate_update(cuda, D, ordering, mean, flags):
    """coord_out = coord + (1 / degree if mean) sum_e f_e (c_i - c_j) s_e of mdx_egnn_node_gather (the coordinate half alone) and
    of mdx_egnn_coord_aggregate against float64 from the same binary32 inputs, per node and component within
    gather_cases.coord_bar (derived there); nodes without edges keep their coordinates bit for bit; coord_out has D columns and
    nothing around it is written.  The graph has self-loops and an edge between two nodes at the same place (r^2 = 0: the factor
    is 0 / 1e-8 = 0, not NaN).

    The flags' allowance is twice the worst per-term relative distance between torch's float32 evaluation of the same formula on
    the GPU and float64, over these inputs.  Measured on an MI355X, the largest over D and the orderings: 7.99 u (NORMALIZE),
    6.61 u (TANH), 8.96 u (both).  The kernels' worst error / bar there: node_gather 0.48 (flags 0), 0.22, 0.35, 0.28 (flags 1, 2,
    3); coord_aggregate 0.63, 0.26, 0.43, 0.30."""
    _hip, kernels = _pkg()
    edges, offsets, degree = _graph(ordering)
    n, E = len(degree), edges.shape[0]
    coord, scalar = _coord_case(D, ordering)
    d_off, d_deg, d_edges, d_coord, d_scalar = (_dev(x, cuda) for x in (offsets, degree, edges, coord, scalar))
    allowance = gc.transcendental_allowance(coord, edges, scalar, flags, cuda) if flags else 0.0
    want, magnitude, terms = gc.coord_reference(coord, edges, offsets, degree, scalar.astype(np.float64), flags, mean)
    assert np.any(np.all(terms == 0.0, axis=1) & (edges[:, 0] != edges[:, 1])) and np.any(edges[:, 0] == edges[:, 1])

    results = {}
    buffer, out = _guarded(n, D, cuda)
    _hip.call("mdx_egnn_node_gather", None, E, d_off, d_deg, n, 4, 0, None, None, d_scalar, d_coord, D, d_edges, int(mean), flags, out)
    assert _untouched(buffer, n, D)
    results["node_gather"] = out.cpu().numpy()
    buffer, out = _guarded(n, D, cuda)
    _hip.call("mdx_egnn_coord_aggregate", d_scalar, d_coord, D, d_edges, d_off, d_deg, n, int(mean), flags, out)
    assert _untouched(buffer, n, D)
    results["coord_aggregate"] = out.cpu().numpy()
    wrapped = kernels.egnn_coord_aggregate(d_scalar, d_coord, d_edges, d_off, d_deg, mean, flags=flags)
    assert tuple(wrapped.shape) == (n, D) and np.array_equal(_bits(wrapped.cpu().numpy()), _bits(results["coord_aggregate"]))

    for name, got in results.items():
        bar = gc.coord_bar(coord, degree, magnitude, flags, allowance, sequential=name == "coord_aggregate")
        error = np.abs(got.astype(np.float64) - want)
        assert np.all(np.isfinite(got)) and np.all(error <= bar), (name, np.argwhere(~(error <= bar))[:4])
        assert np.array_equal(_bits(got[degree == 0]), _bits(coord[degree == 0]))
        ratio = float(np.max(error / bar))
        MEASURED[(name, D, ordering, mean, flags)] = ratio
        print(f"{name} D {D} {ordering} mean {mean} flags {flags}: worst error / bar {ratio:.3f}"
              + (f", allowance {allowance / U:.2f} u" if flags else ""))
    if flags:
        MEASURED[("allowance", D, ordering, flags)] = allowance / U


def test_refusals_and_the_empty_problem(cuda):
    """coord_dimension = 9 and H = 6 are "unsupported", an unknown flag bit is an "invalid argument"; n_nodes = 0 launches nothing
    and writes nothing."""
    _hip, kernels = _pkg()
    edges, offsets, degree = _graph("listed")
    n, E = len(degree), edges.shape[0]
    d_off, d_deg, d_edges = (_dev(x, cuda) for x in (offsets, degree, edges))
    d_scalar = torch.zeros(E, device=cuda)
    rows = kernels.lib().mdx_egnn_piece_rows(E, n)
    assert rows == ((E + 15) >> 4) + n
    pieces = torch.zeros(rows, 8, device=cuda)
    with pytest.raises(_hip.MdxError, match="unsupported"):
        kernels.egnn_node_gather(pieces, E, d_off, d_deg, False, None, d_scalar, torch.zeros(n, 9, device=cuda), d_edges, False)
    with pytest.raises(_hip.MdxError, match="unsupported"):
        kernels.egnn_node_gather(torch.zeros(rows, 6, device=cuda), E, d_off, d_deg, False, None, d_scalar,
                                 torch.zeros(n, 3, device=cuda), d_edges, False)
    with pytest.raises(_hip.MdxError, match="unsupported"):
        kernels.segment_combine(torch.zeros(rows, 6, device=cuda), E, d_off, d_deg, False)
    for bad in (4, 7, 1 << 30):
        with pytest.raises(_hip.MdxError, match="invalid argument"):
            kernels.egnn_node_gather(pieces, E, d_off, d_deg, False, None, d_scalar, torch.zeros(n, 3, device=cuda), d_edges, False,
                                     flags=bad)
        with pytest.raises(_hip.MdxError, match="invalid argument"):
            kernels.egnn_coord_aggregate(d_scalar, torch.zeros(n, 3, device=cuda), d_edges, d_off, d_deg, False, flags=bad)
    buffer, out = _guarded(n, 8, cuda)
    coord_buffer, coord_out = _guarded(n, 3, cuda)
    coord = torch.zeros(n, 3, device=cuda)
    _hip.call("mdx_egnn_node_gather", pieces, E, d_off, d_deg, 0, 8, 0, None, out, d_scalar, coord, 3, d_edges, 0, 0, coord_out)
    _hip.call("mdx_segment_combine", pieces, E, d_off, d_deg, 0, 8, 0, None, out)
    _hip.call("mdx_egnn_coord_aggregate", d_scalar, coord, 3, d_edges, d_off, d_deg, 0, 0, 0, coord_out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buffer).all()) and bool(torch.isnan(coord_buffer).all())
    empty = torch.zeros(0, dtype=torch.int64, device=cuda)
    none, nothing = kernels.egnn_node_gather(None, 0, empty, empty, False, None, torch.zeros(0, device=cuda),
                                             torch.zeros(0, 3, device=cuda), torch.zeros(0, 2, dtype=torch.int64, device=cuda), False)
    assert none is None and tuple(nothing.shape) == (0, 3)
