"""The kernels around the EGNN edge chain (csrc/mdx_egnn.hip) -- mdx_egnn_node_inputs(_keyed), mdx_egnn_message_input, mdx_egnn_scores,
mdx_egnn_outputs, mdx_egnn_coord_head, mdx_segment_rows -- each called directly, against the restatements of their contracts
(tests/egnn_helper_cases.py, checked without a GPU by tests/test_egnn_helper_cases_cpu.py).

Where the contract fixes the binary32 operations the test asks for the restatement's bits; elsewhere for a bar per element,
derived from the operation counts in each docstring and written down before any measurement.  Outputs are views of larger
NaN-filled buffers (64 guard floats on either side), inputs that must not be read are NaN."""
import functools

import numpy as np
import pytest
import torch

import egnn_helper_cases as hc

pytestmark = pytest.mark.gpu

U = hc.U
PAD = 64
MEASURED = {}


def _hip():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    return _hip


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


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _report(family, ratio):
    MEASURED[family] = max(MEASURED.get(family, 0.0), ratio)
    print(f"{family}: worst error / bar {ratio:.3f}")


@functools.lru_cache(maxsize=None)
def _wave_vector_sets():
    return hc.wave_vector_sets()


# ---------------------------------------------------------------------------------------------------------------------------
# mdx_egnn_node_inputs
def _embedding(H, F, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((H, F)).astype(np.float32), rng.standard_normal(H).astype(np.float32)


def _sigmas(B, seed):
    sigma = np.random.default_rng(seed).uniform(0.01, 0.51, size=B).astype(np.float32)
    assert len(set(sigma.tolist())) == B
    return sigma


def _node_inputs(device, x, k, sigma, N, a, first, second=None, key=None):
    """mdx_egnn_node_inputs_keyed into guarded outputs: (z, h, second_out or None) as numpy arrays."""
    n, n_k = x.shape[0], k.shape[0]
    (w, b), (H, F) = first, first[0].shape
    z_buffer, z = _guarded(n, 2 * n_k, device)
    h_buffer, h = _guarded(n, H, device)
    w2 = b2 = h2 = None
    H2 = 0
    if second is not None:
        assert second[0].shape[1] == F
        H2 = second[0].shape[0]
        w2, b2 = _dev(second[0], device), _dev(second[1], device)
        h2_buffer, h2 = _guarded(n, H2, device)
    _hip().call("mdx_egnn_node_inputs_keyed", _dev(x, device), _dev(k, device), n_k, _dev(sigma, device), N, _dev(a, device),
                _dev(w, device), _dev(b, device), F, H, n, z, h, w2, b2, H2, h2, key)
    assert _untouched(z_buffer, n, 2 * n_k) and _untouched(h_buffer, n, H)
    assert second is None or _untouched(h2_buffer, n, H2)
    return z.cpu().numpy(), h.cpu().numpy(), None if second is None else h2.cpu().numpy()


@pytest.mark.parametrize("name", ["synthetic%d" % n_k for n_k in hc.N_K] + ["bloch5"])
def test_uplift_bits(cuda, name):
    """z is the correctly rounded binary32 of the binary64 cos / sin of the binary32 angle: the bits of egnn_helper_cases.uplift
    (the midpoint condition of the CPU test is what makes "correctly rounded" decidable), at every number of nodes per pass of the
    wavefront-per-node kernel (n_k up to 64: 4, 3, 2, 1; above: a lane-strided loop), for node counts that do not fill a pass, and
    from the element-wise kernel (H = 6) as well."""
    k = _wave_vector_sets()[name]
    for B, N in hc.NODE_SHAPES:
        x = hc.node_coordinates(B, N)
        want = hc.uplift(x, k)
        a = hc.atom_types(B * N, 3, 1)
        for H in (8, 6):
            z, _, _ = _node_inputs(cuda, x, k, _sigmas(B, 2), N, a, _embedding(H, 3, 3))
            assert _same_bits(z, want), (name, B, N, H, np.argwhere(_bits(z) != _bits(want))[:4])


# (H, second_width): one wavefront per node for H = 4, 96, 256 with a second map of 8 or 512 columns; element-wise for H = 30,
# for a second map whose width is no multiple of 4, and for tables beyond 48 KiB (F = 10: 11 x 1536 floats = 67.6 KB)
SELECTION = [(4, 8), (96, 512), (256, 8), (256, 512), (30, None), (30, 8), (64, 6), (512, 1024)]


@pytest.mark.parametrize("C", [1, 2, 8])
@pytest.mark.parametrize("H,H2", SELECTION)
def test_embedding_bits(cuda, H, H2, C):
    """h and second_out are fl(fl(b + fl(sigma W[:, 0])) + W[:, 1 + a]) bit for bit in every branch of the kernel selection, with
    sigma distinct per structure; atom types -1 and F - 1 have no column and get b + sigma W[:, 0]; z alongside."""
    F = C + 2
    k = _wave_vector_sets()["synthetic13"]
    for B, N in hc.NODE_SHAPES:
        n = B * N
        x, sigma, a = hc.node_coordinates(B, N), _sigmas(B, 10 + B), hc.atom_types(n, F, 20 + n)
        assert n < 5 or ({-1, F - 1, F - 2, 0} <= set(a.tolist()))
        first = _embedding(H, F, 30 + H)
        second = None if H2 is None else _embedding(H2, F, 40 + H2)
        z, h, h2 = _node_inputs(cuda, x, k, sigma, N, a, first, second)
        assert _same_bits(h, hc.embed32(sigma, a, first[0], first[1], N)), (B, N)
        assert second is None or _same_bits(h2, hc.embed32(sigma, a, second[0], second[1], N)), (B, N)
        assert _same_bits(z, hc.uplift(x, k)), (B, N)


def test_both_node_input_kernels_give_the_same_bits(cuda):
    """The wavefront-per-node kernel (no second map) and the element-wise kernel (the same inputs plus a second map of odd width)
    give the same z and h bit for bit."""
    B, N, H, F = 7, 13, 64, 4
    k = _wave_vector_sets()["synthetic13"]
    x, sigma, a = hc.node_coordinates(B, N), _sigmas(B, 5), hc.atom_types(B * N, F, 6)
    first = _embedding(H, F, 7)
    z_rows, h_rows, _ = _node_inputs(cuda, x, k, sigma, N, a, first)
    z_elements, h_elements, _ = _node_inputs(cuda, x, k, sigma, N, a, first, _embedding(7, F, 8))
    assert _same_bits(z_rows, z_elements) and _same_bits(h_rows, h_elements)


@pytest.mark.parametrize("H", [8, 130])
def test_node_inputs_grid_stride(cuda, H):
    """33 410 nodes: more than the 2048 blocks x 16 nodes of the wavefront-per-node kernel (H = 8) and, at H = 130, more elements
    than the element-wise kernel's 16384 blocks x 256 threads; every node's z and h still the restatement's bits."""
    B, N = hc.GRID_STRIDE_SHAPE
    F = 4
    assert B * N > 2048 * 16 and B * N * 130 > 16384 * 256
    k = _wave_vector_sets()["synthetic3"]
    x, sigma, a = hc.node_coordinates(B, N), _sigmas(B, 50), hc.atom_types(B * N, F, 51)
    first = _embedding(H, F, 52)
    z, h, _ = _node_inputs(cuda, x, k, sigma, N, a, first)
    assert _same_bits(z, hc.uplift(x, k))
    assert _same_bits(h, hc.embed32(sigma, a, first[0], first[1], N))


@pytest.mark.parametrize("H,H2", [(8, 8), (30, 7)])
def test_keyed_early_return(cuda, H, H2):
    """mdx_egnn_node_inputs_keyed without a memo object: while table_key[0] holds the bits of sigma[0] none of the three outputs
    is written (both kernels); with MDX_EGNN_TABLE_NO_KEY they are."""
    B, N, F = 3, 5, 4
    k = _wave_vector_sets()["synthetic3"]
    x, sigma, a = hc.node_coordinates(B, N), _sigmas(B, 60), hc.atom_types(B * N, F, 61)
    first, second = _embedding(H, F, 62), _embedding(H2, F, 63)
    current = torch.tensor([int(sigma[:1].view(np.int32)[0]), 0], dtype=torch.int32, device=cuda)
    for outputs in _node_inputs(cuda, x, k, sigma, N, a, first, second, key=current):
        assert np.all(np.isnan(outputs))
    assert _hip().EGNN_TABLE_NO_KEY == 0x7fc00000
    none = torch.tensor([_hip().EGNN_TABLE_NO_KEY, 0], dtype=torch.int32, device=cuda)
    z, h, h2 = _node_inputs(cuda, x, k, sigma, N, a, first, second, key=none)
    assert _same_bits(z, hc.uplift(x, k)) and _same_bits(h, hc.embed32(sigma, a, first[0], first[1], N))
    assert _same_bits(h2, hc.embed32(sigma, a, second[0], second[1], N))


# ---------------------------------------------------------------------------------------------------------------------------
# mdx_egnn_message_input
def _message_case(E, H, n_nodes, seed):
    """Inputs with |pre| <= 24 by construction (four terms of at most 6); node_proj rows that no edge names are NaN."""
    rng = np.random.default_rng(seed)
    edges = hc.message_edges(E, n_nodes, seed + 1)
    proj = rng.uniform(-6.0, 6.0, size=(n_nodes, 2 * H)).astype(np.float32)
    unused = np.setdiff1d(np.arange(n_nodes), edges)
    assert len(unused) >= 1
    proj[unused] = np.nan
    bias = rng.uniform(-6.0, 6.0, size=H).astype(np.float32)
    w_radial = rng.uniform(-3.0, 3.0, size=H).astype(np.float32)
    radial = rng.uniform(0.0, 2.0, size=E).astype(np.float32)
    return proj, edges, radial, bias, w_radial


def _message_input(device, case, H, silu):
    proj, edges, radial, bias, w_radial = case
    E = edges.shape[0]
    buffer, out = _guarded(E, H, device)
    _hip().call("mdx_egnn_message_input", _dev(proj, device), _dev(edges, device), _dev(radial, device), _dev(bias, device),
                _dev(w_radial, device), E, H, silu, out)
    got = out.cpu().numpy()
    assert _untouched(buffer, E, H)
    return got


@pytest.mark.parametrize("E", [1, 77])
@pytest.mark.parametrize("H", [4, 64, 260])
def test_message_input(cuda, H, E):
    """silu = 0: the bits of fl(fl(fl(P[src, :H] + P[dst, H:]) + bias) + fl(r w_r)).  silu = 1: within
    (|pre| + 8) u |silu(pre)| + 2^-126 of the float64 SiLU of that binary32 sum -- the fast exponential is a hardware exp2 of
    a rounded product, whose rounding alone is |pre| u of the exponential; the hardware exp2, the addition of 1 and the
    division are a few more.  The edges name one node twice (src == dst), the last node on either side, and leave nodes out
    whose rows are NaN: a wrong row or the two halves swapped give a NaN or another number.
    Measured on an MI355X: at most 0.73 of the bar."""
    n_nodes = 9
    case = _message_case(E, H, n_nodes, 70 + H + E)
    edges = case[1]
    if E > 1:
        assert np.any(edges[:, 0] == edges[:, 1]) and np.any(edges[:, 0] == n_nodes - 1) and np.any(edges[:, 1] == n_nodes - 1)
    pre = hc.message_pre32(*case)
    assert np.all(np.isfinite(pre)) and np.max(np.abs(pre)) <= 30.0
    assert _same_bits(_message_input(cuda, case, H, 0), pre)
    got = _message_input(cuda, case, H, 1).astype(np.float64)
    want = hc.silu64(pre)
    bar = (np.abs(pre.astype(np.float64)) + 8.0) * U * np.abs(want) + 2.0 ** -126
    ratio = float(np.max(np.abs(got - want) / bar))
    _report("message_input silu", ratio)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bar), np.argwhere(~(np.abs(got - want) <= bar))[:4]


def test_message_input_grid_stride(cuda):
    """16 400 edges x 1024 columns = 4 198 400 quads, more than 16384 blocks x 256 threads: every element still the bits."""
    E, H = 16400, 1024
    assert E * (H // 4) > 16384 * 256
    case = _message_case(E, H, 50, 80)
    assert _same_bits(_message_input(cuda, case, H, 0), hc.message_pre32(*case))


def test_message_input_refusals_and_no_edges(cuda):
    """H = 6 is "unsupported", H = 0 an "invalid argument"; without edges nothing is written."""
    hip = _hip()
    proj, edges, radial, bias, w_radial = (_dev(t, cuda) for t in _message_case(5, 8, 9, 90))
    out = torch.full((5 * 8,), float("nan"), device=cuda)
    with pytest.raises(hip.MdxError, match="unsupported"):
        hip.call("mdx_egnn_message_input", proj, edges, radial, bias, w_radial, 5, 6, 1, out)
    with pytest.raises(hip.MdxError, match="invalid argument"):
        hip.call("mdx_egnn_message_input", proj, edges, radial, bias, w_radial, 5, 0, 1, out)
    hip.call("mdx_egnn_message_input", proj, edges, radial, bias, w_radial, 0, 8, 1, out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------------------------------
# mdx_egnn_scores and mdx_egnn_outputs
def _score_case(n_nodes, n_k, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n_nodes, 2 * n_k)).astype(np.float32), rng.standard_normal((n_nodes, 2 * n_k)).astype(np.float32),
            hc.wave_vectors(n_k, seed + 1))


def _scores(device, z, x_hat, k):
    n = z.shape[0]
    buffer, out = _guarded(n, 3, device)
    _hip().call("mdx_egnn_scores", _dev(z, device), _dev(x_hat, device), _dev(k, device), k.shape[0], n, out)
    got = out.cpu().numpy()
    assert _untouched(buffer, n, 3)
    return got


def _outputs(device, z, x_hat, k, h, weight, bias, mask_class, n_zero=0):
    """(scores, logits, zeros) of mdx_egnn_outputs as numpy arrays, all three in guarded buffers."""
    n, (C, H) = z.shape[0], weight.shape
    s_buffer, scores = _guarded(n, 3, device)
    l_buffer, logits = _guarded(n, C, device)
    z_buffer, zeros = _guarded(1, n_zero, device)
    _hip().call("mdx_egnn_outputs", _dev(z, device), _dev(x_hat, device), _dev(k, device), k.shape[0], _dev(h, device),
                _dev(weight, device), _dev(bias, device), H, C, mask_class, n, scores, logits,
                zeros.view(-1) if n_zero else None, n_zero)
    got = scores.cpu().numpy(), logits.cpu().numpy(), zeros.view(-1).cpu().numpy()
    assert _untouched(s_buffer, n, 3) and _untouched(l_buffer, n, C) and _untouched(z_buffer, 1, n_zero)
    return got


@pytest.mark.parametrize("n_k", [1, 3, 13, 65])
def test_scores(cuda, n_k):
    """S[i, alpha] per element within (2 n_k + 2) u sum_k |terms| of float64: a term is two rounded products, the pair's sum one
    more, and the accumulator takes n_k additions -- n_k + 3 roundings on the path of a term, never more than 2 n_k + 2.  The
    scores of mdx_egnn_outputs are the same bits.  Measured on an MI355X: at most 0.42 of the bar."""
    worst = 0.0
    for n_nodes in (1, 2, 3, 5, 77):
        z, x_hat, k = _score_case(n_nodes, n_k, 100 + n_k + n_nodes)
        want, size = hc.scores64(z, x_hat, k)
        got = _scores(cuda, z, x_hat, k)
        bar = (2 * n_k + 2) * U * size
        error = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float(np.max(error / bar)))
        assert np.all(np.isfinite(got)) and np.all(error <= bar), (n_nodes, np.argwhere(~(error <= bar))[:4])
        h, weight, bias = np.ones((n_nodes, 4), np.float32), np.ones((1, 4), np.float32), np.zeros(1, np.float32)
        fused, _, _ = _outputs(cuda, z, x_hat, k, h, weight, bias, -1)
        assert _same_bits(fused, got), n_nodes
    _report("scores", worst)


def _mask_classes(C):
    return sorted({-1, 0, C // 2, C - 1})


@pytest.mark.parametrize("C", [1, 2, 3, 8])
@pytest.mark.parametrize("H", [4, 252, 256, 260, 1024])
def test_logits(cuda, H, C):
    """logits[i, c] = h_i . W_c + b_c per element within (H / 4 + 10) u (sum_j |h_j w_j| + |b|) of float64 (a lane's partial sums,
    a 6-step tree, the bias), for every place of the MASK class -- none, 0, a middle one, the last -- whose logit is exactly
    -inf and whose weight row, NaN here, must not reach any other sum; C = 1 with mask_class = 0 gives -inf alone.  Node counts
    below, at and off the four nodes of a wavefront's pass.  Measured on an MI355X: at most 0.23 of the bar."""
    worst = 0.0
    rng = np.random.default_rng(200 + H + C)
    for n_nodes in (1, 3, 6, 77):
        z, x_hat, k = _score_case(n_nodes, 3, 300 + n_nodes)
        h = rng.standard_normal((n_nodes, H)).astype(np.float32)
        weight, bias = rng.standard_normal((C, H)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
        want, size = hc.logits64(h, weight, bias)
        for mask_class in _mask_classes(C):
            poisoned = weight.copy()
            if mask_class >= 0:
                poisoned[mask_class] = np.nan
            scores, logits, _ = _outputs(cuda, z, x_hat, k, h, poisoned, bias, mask_class)
            kept = np.array([c != mask_class for c in range(C)])
            assert np.all(logits[:, ~kept] == -np.inf) and np.all(np.isfinite(logits[:, kept])), (n_nodes, mask_class)
            if kept.any():
                error = np.abs(logits.astype(np.float64) - want)[:, kept]
                bar = ((H / 4 + 10) * U * size)[:, kept]
                worst = max(worst, float(np.max(error / bar)))
                assert np.all(error <= bar), (n_nodes, mask_class, np.argwhere(~(error <= bar))[:4])
            assert _same_bits(scores, _scores(cuda, z, x_hat, k))
    _report("logits", worst)


@pytest.mark.parametrize("H", [256, 260])
def test_every_lane_and_component_enters_the_logit_once(cuda, H):
    """Row i of h is one-hot at column i, W holds distinct dyadic numbers and b = 0: logits[i, c] == W[c, i] exactly says that
    lane i / 4 mod 64's component i mod 4 of quad i / 4 reaches the wavefront's total, and only once (H = 260: the second pass
    over the columns too)."""
    C = 8
    h = np.eye(H, dtype=np.float32)
    weight = ((np.arange(C * H, dtype=np.float64).reshape(C, H) + 1.0) / 64.0).astype(np.float32)
    assert len(np.unique(weight)) == C * H
    z, x_hat, k = _score_case(H, 1, 400)
    _, logits, _ = _outputs(cuda, z, x_hat, k, h, weight, np.zeros(C, np.float32), -1)
    assert _same_bits(logits, weight.T), np.argwhere(logits != weight.T)[:4]


@pytest.mark.parametrize("n_zero", [0, 1, 42])
def test_zero_out(cuda, n_zero):
    """zero_out [n_zero] is written as zeros and nothing beside it, with nodes and -- for n_zero > 0 -- without any."""
    z, x_hat, k = _score_case(5, 3, 500)
    h, weight, bias = np.ones((5, 8), np.float32), np.ones((2, 8), np.float32), np.zeros(2, np.float32)
    _, _, zeros = _outputs(cuda, z, x_hat, k, h, weight, bias, 1, n_zero)
    assert zeros.shape == (n_zero,) and np.all(_bits(zeros) == 0)
    if n_zero:
        buffer, zeros = _guarded(1, n_zero, cuda)
        _hip().call("mdx_egnn_outputs", None, None, None, 3, None, None, None, 8, 2, 1, 0, None, None, zeros.view(-1), n_zero)
        assert np.all(_bits(zeros.cpu().numpy()) == 0) and _untouched(buffer, 1, n_zero)


def test_outputs_and_scores_grid_stride(cuda):
    """mdx_egnn_outputs at 262 149 nodes (more than 16384 blocks x 4 wavefronts x 4 nodes) and mdx_egnn_scores at 1 398 102
    (3 n_nodes beyond 16384 x 256 threads), n_k = 1: scores against the vectorised binary32 restatement and float64, logits
    within their bar.  Measured on an MI355X: 0.71 (scores, whose bar at n_k = 1 is 4 u) and 0.27 (logits) of the bars."""
    n_outputs, n_scores = 262149, 1398102
    assert n_outputs > 16384 * 16 and 3 * n_scores > 16384 * 256
    z, x_hat, k = _score_case(n_scores, 1, 600)
    want, size = hc.scores64(z, x_hat, k)
    got = _scores(cuda, z, x_hat, k)
    error, bar = np.abs(got.astype(np.float64) - want), 4 * U * size
    assert np.all(error <= bar)
    assert np.all(np.abs(got.astype(np.float64) - hc.scores32(z, x_hat, k)) <= bar)
    _report("scores grid stride", float(np.max(error[bar > 0] / bar[bar > 0])))
    rng = np.random.default_rng(601)
    H, C = 4, 2
    h = rng.standard_normal((n_outputs, H)).astype(np.float32)
    weight, bias = rng.standard_normal((C, H)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    scores, logits, _ = _outputs(cuda, z[:n_outputs], x_hat[:n_outputs], k, h, weight, bias, -1)
    assert _same_bits(scores, got[:n_outputs])
    want, size = hc.logits64(h, weight, bias)
    error, bar = np.abs(logits.astype(np.float64) - want), (H / 4 + 10) * U * size
    assert np.all(error <= bar)
    _report("logits grid stride", float(np.max(error / bar)))


# ---------------------------------------------------------------------------------------------------------------------------
# mdx_egnn_coord_head and mdx_segment_rows
DIMENSIONS = [1, 2, 3, 6, 64]


def _segment_case(H, d, seed):
    """(hidden [E + 3, H], w [H], coord_diff [E + 3, d]) on the DEGREES segments; the rows behind the last segment are NaN."""
    rng = np.random.default_rng(seed)
    E = int(np.sum(hc.DEGREES))
    hidden = np.concatenate([rng.standard_normal((E, H)), np.full((3, H), np.nan)]).astype(np.float32)
    coord_diff = np.concatenate([rng.standard_normal((E, d)), np.full((3, d), np.nan)]).astype(np.float32)
    return hidden, (rng.standard_normal(H) / H ** 0.5).astype(np.float32), coord_diff


def _segment_rows(device, data, offsets, degree, mean):
    n, H = len(degree), data.shape[1]
    buffer, out = _guarded(n, H, device)
    _hip().call("mdx_segment_rows", _dev(data, device), _dev(offsets, device), _dev(degree, device), n, H, int(mean), out)
    got = out.cpu().numpy()
    assert _untouched(buffer, n, H)
    return got


def _coord_head(device, hidden, w, coord_diff, offsets, degree, mean):
    n, H, d = len(degree), hidden.shape[1], coord_diff.shape[1]
    buffer, trans = _guarded(n, d, device)
    _hip().call("mdx_egnn_coord_head", _dev(hidden, device), _dev(w, device), _dev(coord_diff, device), _dev(offsets, device),
                _dev(degree, device), n, H, d, int(mean), trans)
    got = trans.cpu().numpy()
    assert _untouched(buffer, n, d)
    return got


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("H", [4, 64, 256, 260])
def test_segment_kernels(cuda, H, mean):
    """On segments of every length class against the four rows in flight (egnn_helper_cases.DEGREES), per element:
    mdx_segment_rows within (deg + 1) u sum_e |v| (deg - 1 rounded additions, the mean's division, one to spare) and
    mdx_egnn_coord_head, for d = 1, 2, 3, 6, 64, within (H / 4 + deg + 10) u sum_e |c_e| sum_j |h_ej w_j| (a lane's partial dot
    product, the butterfly, the product with c_e, deg additions, the division); both magnitudes divided like the sum under the
    mean.  Empty segments are exact zeros, the NaN rows behind the last segment are not read, nothing outside the output is
    written.  Measured on an MI355X: at most 0.54 (rows) and 0.15 (coordinate head) of the bars."""
    offsets, degree = hc.segments()
    empty = degree == 0
    for d in DIMENSIONS:
        hidden, w, coord_diff = _segment_case(H, d, 700 + H + d)
        if d == DIMENSIONS[0]:
            got = _segment_rows(cuda, hidden, offsets, degree, mean)
            want, size = hc.segment_rows64(hidden, offsets, degree, mean)
            error, bar = np.abs(got.astype(np.float64) - want), (degree + 1)[:, None] * U * size
            assert np.all(np.isfinite(got)) and np.all(error <= bar), np.argwhere(~(error <= bar))[:4]
            assert np.all(_bits(got[empty]) == 0)
            _report("segment_rows", float(np.max(error[~empty] / bar[~empty])))
        got = _coord_head(cuda, hidden, w, coord_diff, offsets, degree, mean)
        want, size = hc.coord_head64(hidden, w, coord_diff, offsets, degree, mean)
        error, bar = np.abs(got.astype(np.float64) - want), (H / 4 + degree + 10)[:, None] * U * size
        assert np.all(np.isfinite(got)) and np.all(error <= bar), (d, np.argwhere(~(error <= bar))[:4])
        assert np.all(_bits(got[empty]) == 0)
        _report("coord_head", float(np.max(error[~empty] / bar[~empty])))


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("H", [4, 64, 256, 260])
def test_segment_kernels_on_dyadic_data(cuda, H, mean):
    """Data whose every partial sum is exact in binary32 (egnn_helper_cases.dyadic_segment_case): the sums are the exact ones,
    and under the mean float32(sum) / float32(deg) in true division -- not a product with a rounded reciprocal."""
    offsets, degree = hc.segments()
    count = np.maximum(degree, 1).astype(np.float64)[:, None] if mean else 1.0
    for d in DIMENSIONS:
        hidden, w, coord_diff, data = hc.dyadic_segment_case(H, d, 800 + H + d)
        if d == DIMENSIONS[0]:
            exact, _ = hc.segment_rows64(data, offsets, degree, False)
            assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
            assert _same_bits(_segment_rows(cuda, data, offsets, degree, mean), (exact / count).astype(np.float32))
        exact, _ = hc.coord_head64(hidden, w, coord_diff, offsets, degree, False)
        assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
        # (float64 quotient of two binary32 numbers, rounded once: the correctly rounded binary32 quotient; + 0.0: a sum that
        # starts from +0 is never -0, which numpy's sum of the single term 0 x negative is)
        assert _same_bits(_coord_head(cuda, hidden, w, coord_diff, offsets, degree, mean),
                          (exact / count + 0.0).astype(np.float32)), d


def test_segment_refusals(cuda):
    """H % 4 != 0 is "unsupported" for both kernels, and so is d = 65 (one lane per component)."""
    hip = _hip()
    offsets, degree = (_dev(t, cuda) for t in hc.segments())
    n, E = len(hc.DEGREES), int(np.sum(hc.DEGREES))
    data, w = torch.zeros(E, 8, device=cuda), torch.zeros(8, device=cuda)
    out = torch.zeros(n, 65, device=cuda)
    with pytest.raises(hip.MdxError, match="unsupported"):
        hip.call("mdx_segment_rows", data, offsets, degree, n, 6, 0, out)
    with pytest.raises(hip.MdxError, match="unsupported"):
        hip.call("mdx_egnn_coord_head", data, w, torch.zeros(E, 3, device=cuda), offsets, degree, n, 6, 3, 0, out)
    with pytest.raises(hip.MdxError, match="unsupported"):
        hip.call("mdx_egnn_coord_head", data, w, torch.zeros(E, 65, device=cuda), offsets, degree, n, 8, 65, 0, out)
