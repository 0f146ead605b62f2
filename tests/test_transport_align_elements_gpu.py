"""The transport alignment kernel (csrc/mdx_transport.hip: transport_align_kernel<1>, <2> and <4>, one, two and four columns per
lane) called through the C ABI -- mdx_transport_align and mdx_equivariant_analytical_score -- PER ELEMENT against the float64
restatement of tests/transport_cases.py, at 1 ... 256 atoms, 1, 2 and 3 dimensions, 1 ... 48 operations (ragged round-robin tails
among them), shared and per-structure mu.  See that module's docstring for the restatement, the cases and the bars, every
constant of which was written down before any GPU run (tests/test_transport_cases_cpu.py holds the restatement to the reference's
binary64 records and checks the conditions on the cases without a GPU).

Every output is a view inside a larger buffer with 64 guard elements on either side -- NaN for the binary32 and binary64 outputs,
a sentinel for the int32 ones -- and the guards are checked after every launch.  Each family prints its worst error / bar.
tests/test_transport_gpu.py and tests/test_equivariant_analytical_gpu.py keep the reference-made fixtures (N <= 65)."""
import functools

import numpy as np
import pytest
import torch

import transport_cases as tc

pytestmark = pytest.mark.gpu

PAD = 64
SENTINEL = -77777
MEASURED = {}


def _hip():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    return _hip


def _dev(array, device):
    return torch.from_numpy(np.array(array, order="C")).to(device)        # a copy: the cases are read-only


def _guarded(shape, dtype, device):
    """An output of `shape` inside a larger buffer of NaNs (floats) or sentinels (int32): (buffer, view)."""
    count = int(np.prod(shape))
    fill = SENTINEL if dtype == torch.int32 else float("nan")
    buffer = torch.full((count + 2 * PAD,), fill, dtype=dtype, device=device)
    return buffer, buffer[PAD:PAD + count].view(*shape)


def _untouched(buffer, view):
    count = view.numel()
    guards = torch.cat([buffer[:PAD], buffer[PAD + count:]])
    assert guards.numel() == 2 * PAD
    return bool((guards == SENTINEL).all()) if buffer.dtype == torch.int32 else bool(torch.isnan(guards).all())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _report(family, ratio):
    MEASURED[family] = max(MEASURED.get(family, 0.0), ratio)
    print(f"{family}: worst error / bar {ratio:.3f}")


def _check(family, error, bar, where):
    """error <= bar for every element (no NaN); reports the worst ratio."""
    error, bar = np.asarray(error, dtype=np.float64), np.broadcast_to(np.asarray(bar, dtype=np.float64), np.shape(error))
    assert np.all(np.isfinite(error)), (family, where, np.argwhere(~np.isfinite(error))[:4])
    exact = bar == 0.0
    assert np.all(error[exact] == 0.0), (family, where)
    ratio = float(np.max(error[~exact] / bar[~exact])) if np.any(~exact) else 0.0
    _report(family, ratio)
    assert ratio <= 1.0, (family, where, ratio, np.argwhere(error > bar)[:4])


def _align(device, x, mu, operations, details=True, with_status=True):
    """One mdx_transport_align launch into guarded buffers: (image f32 [B, N, D], operation [B], col_idx [B, N], costs [B, O],
    status) on the host, the three details None when their pointers are null."""
    B, N, D = x.shape
    O = operations.shape[0]
    stride = 0 if mu.ndim == 2 else N * D
    outputs = [_guarded((B, N, D), torch.float32, device)]
    if details:
        outputs += [_guarded((B,), torch.int32, device), _guarded((B, N), torch.int32, device), _guarded((B, O), torch.float64, device)]
    views = [view for _, view in outputs] + [None] * (4 - len(outputs))
    status = torch.zeros(1, dtype=torch.int32, device=device) if with_status else None
    _hip().call("mdx_transport_align", _dev(x, device), _dev(mu, device), stride, _dev(operations, device), O, B, N, D, *views, status)
    torch.cuda.synchronize()
    for buffer, view in outputs:
        assert _untouched(buffer, view), "a guard element was written"
    got = [None if view is None else view.cpu().numpy() for view in views]
    return (*got, None if status is None else int(status.item()))


def _score(device, x, sigmas, mu, operations, sigma_d_square, kmax):
    """One mdx_equivariant_analytical_score launch into a guarded buffer: (score f32 [B, N, D], status)."""
    B, N, D = x.shape
    buffer, view = _guarded((B, N, D), torch.float32, device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    _hip().call("mdx_equivariant_analytical_score", _dev(x, device), _dev(sigmas, device), _dev(mu, device), _dev(operations, device),
                operations.shape[0], float(sigma_d_square), int(kmax), B, N, D, view, status)
    torch.cuda.synchronize()
    assert _untouched(buffer, view), "a guard element was written"
    return view.cpu().numpy(), int(status.item())


def _cost_bar(case, optimum):
    """1e-12 of the optimum; at N = 1, where the optimum is the square of rounding noise, the absolute bar of the cases module."""
    return tc.COST_BAR * np.abs(optimum) + (tc.single_atom_cost_bar(case.D) if case.N == 1 else 0.0)


@pytest.mark.parametrize("name", tc.NAMES)
def test_alignment_elements(cuda, name):
    """mdx_transport_align with details, every structure of every case:
      costs[b, o] of ALL operations within 1e-12 relative of scipy's optimum; col_idx[b] a permutation; the restatement's cost of
      the reported (operation, col_idx) within 1e-12 relative of the lowest optimum; every element of the image in [0, 1) and
      within 2^-24 on the torus of the restatement's image of the kernel's OWN reported choice; on the generic cases (N >= 63)
      operation and col_idx equal the restatement's.  (At N = 1 the costs are rounding noise squared: an absolute bar, see
      tests/transport_cases.py.)
    The same bits from a launch with the three detail pointers (and the status) null, from B copies of a shared mu, and for a
    structure moved from b = 0 to b = B - 1.
    Measured on an MI355X: costs at most 0.008 of the bar, the cost of the reported choice below 0.001, the image 0.500 (the one
    rounding to binary32)."""
    case, want = tc.case(name), tc.solution(name)
    B, N, O = case.B, case.N, case.O
    image, operation, col_idx, costs, status = _align(cuda, case.x, case.mu, case.operations)
    assert status == 0
    _check("alignment costs", np.abs(costs - want.costs), _cost_bar(case, want.costs), name)
    assert np.array_equal(np.sort(col_idx, axis=1), np.broadcast_to(np.arange(N), (B, N))), (name, "col_idx is no permutation")
    assert ((operation >= 0) & (operation < O)).all()
    assert (image >= 0.0).all() and (image < 1.0).all()
    composed = np.empty_like(want.image)
    reported_cost = np.empty(B)
    for b in range(B):
        composed[b], reported_cost[b] = tc.chosen(want.xt[b], want.mt[b], case.operations, operation[b], col_idx[b])
    lowest = want.costs.min(axis=1)
    _check("alignment cost of the reported choice", np.abs(reported_cost - lowest), _cost_bar(case, lowest), name)
    _check("alignment image", tc.torus(image, composed), np.full(image.shape, tc.IMAGE_BAR), name)
    if case.generic:
        assert np.array_equal(operation, want.operation), (name, operation, want.operation)
        assert np.array_equal(col_idx, want.col_idx[np.arange(B), want.operation]), name
    # null detail pointers
    bare = _align(cuda, case.x, case.mu, case.operations, details=False, with_status=False)
    assert bare[1] is None and bare[2] is None and bare[3] is None and np.array_equal(_bits(bare[0]), _bits(image))
    # a shared mu is its B copies
    if case.shared:
        copies = _align(cuda, case.x, np.broadcast_to(case.mu, case.x.shape), case.operations)
        assert np.array_equal(_bits(copies[0]), _bits(image)) and np.array_equal(copies[1], operation)
        assert np.array_equal(copies[2], col_idx) and copies[3].tobytes() == costs.tobytes()
    # a structure does not depend on its place in the batch
    if B > 1:
        x = case.x.copy()
        x[B - 1] = x[0]
        mu = case.mu
        if not case.shared:
            mu = case.mu.copy()
            mu[B - 1] = mu[0]
        moved = _align(cuda, x, mu, case.operations)
        for got, first in zip(moved[:4], (image, operation, col_idx, costs)):
            assert got[B - 1].tobytes() == first[0].tobytes() and got[:B - 1].tobytes() == first[:B - 1].tobytes(), name


@pytest.mark.parametrize("name", tc.SHARED_MU)
def test_fused_score_elements(cuda, name):
    """mdx_equivariant_analytical_score on the shared-mu cases, one sigma per structure cycling through 0.01, 0.2, the two binary32
    either side of 0x1.988454p-2, 0.5 and the two binary32 whose s_eff lie either side of the threshold (so both branches run
    inside one launch), kmax 2 and 4: every element within 2^-24 |want| (1 + 2^-10) + SCORE_F max_structure |want| of the
    restatement's score.  (At N = 1 the score is a multiple of rounding noise: the absolute term of tests/transport_cases.py.)
    Measured on an MI355X: at most 0.997 of the bar (the one rounding to binary32, which reaches 2^-24 |want| just above a power
    of two: the bar is sharp)."""
    case, want = tc.case(name), tc.solution(name)
    sigmas = tc.sigmas_of(name)
    for kmax in tc.KMAX:
        expected = tc.score(want.xt, want.image, sigmas, case.sigma_d_square, kmax)
        got, status = _score(cuda, case.x, sigmas, case.mu, case.operations, case.sigma_d_square, kmax)
        assert status == 0
        _check("fused score", np.abs(got.astype(np.float64) - expected), tc.score_bar(expected, sigmas, case.sigma_d_square), (name, kmax))


@functools.lru_cache(maxsize=None)
def _three_of_256():
    case, want = tc.case("d3_n256"), tc.solution("d3_n256")
    x = np.ascontiguousarray(case.x[[0, 2, 3]])         # a uniform structure and two near the sites
    x.setflags(write=False)
    return case, want, x, [0, 2, 3]


def test_status_path_with_four_columns_per_lane(cuda):
    """N = 256, B = 3, O = 48: a NaN in the LAST atom of structure 1 gives, in that structure only, an all-NaN image, operation
    -1, col_idx -1 and NaN costs, and sets STATUS_ANALYTICAL_COORDINATES; the other two structures have the bits of the clean
    launch, which has those of the same structures inside the case's own launch of four."""
    case, want, x, rows = _three_of_256()
    clean = _align(cuda, x, case.mu, case.operations)
    assert clean[4] == 0
    assert np.array_equal(clean[1], want.operation[rows]) and np.array_equal(clean[2], want.col_idx[rows, want.operation[rows]])
    bad = x.copy()
    bad[1, 255, 2] = np.nan
    image, operation, col_idx, costs, status = _align(cuda, bad, case.mu, case.operations)
    assert status == _hip().STATUS_ANALYTICAL_COORDINATES
    assert np.isnan(image[1]).all() and operation[1] == -1 and (col_idx[1] == -1).all() and np.isnan(costs[1]).all()
    for b in (0, 2):
        for got, first in zip((image, operation, col_idx, costs), clean[:4]):
            assert got[b].tobytes() == first[b].tobytes(), b
    # the fused score takes the same path
    sigmas = tc.SIGMAS[[1, 4, 0]]
    scores, status = _score(cuda, bad, sigmas, case.mu, case.operations, case.sigma_d_square, 2)
    clean_scores, clean_status = _score(cuda, x, sigmas, case.mu, case.operations, case.sigma_d_square, 2)
    assert status == _hip().STATUS_ANALYTICAL_COORDINATES and clean_status == 0
    assert np.isnan(scores[1]).all() and np.array_equal(_bits(scores[[0, 2]]), _bits(clean_scores[[0, 2]]))


def test_public_modules_at_256_atoms(cuda):
    """EquivariantAnalyticalScoreNetwork with number_of_atoms = 256 (the limit its constructor advertises): a forward satisfies
    the score bar against the restatement made with the network's own symmetries (the package's order of the 48 operations, not
    this suite's); Transporter.get_optimal_transport at N = 256 gives the kernel's bits.
    Measured on an MI355X: the forward at most 0.986 of the bar, the image 0.415."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.equivariant_analytical_score_network import (
        EquivariantAnalyticalScoreNetwork, EquivariantAnalyticalScoreNetworkParameters)
    from diffusion_for_multi_scale_molecular_dynamics_amd.transport.transporter import Transporter
    from test_analytical_score_gpu import _batch
    case, _, x, _ = _three_of_256()
    kmax = 4
    net = EquivariantAnalyticalScoreNetwork(EquivariantAnalyticalScoreNetworkParameters(
        spatial_dimension=3, number_of_atoms=256, num_atom_types=1, kmax=kmax, sigma_d=case.sigma_d,
        equilibrium_relative_coordinates=case.mu.tolist())).eval().to(cuda)
    symmetries = net.symmetries.detach().cpu().numpy()
    assert symmetries.shape == (48, 3, 3) and tc.as_set(symmetries) == tc.as_set(case.operations)
    assert np.array_equal(net.equilibrium_relative_coordinates.detach().cpu().numpy(), case.mu)
    sigmas = tc.SIGMAS[[0, 5, 6]]
    want = tc.align(x, case.mu, symmetries)
    assert (tc.operation_gaps(want.costs) > tc.OPERATION_GAP).all()
    expected = tc.score(want.xt, want.image, sigmas, case.sigma_d_square, kmax)
    with torch.no_grad():
        out = net(_batch(_dev(x, cuda), _dev(sigmas, cuda)), conditional=False)
    net.check_status()
    got = out.X.cpu().numpy()
    assert got.shape == x.shape and got.dtype == np.float32
    _check("public forward", np.abs(got.astype(np.float64) - expected), tc.score_bar(expected, sigmas, case.sigma_d_square), "N = 256")
    direct, status = _score(cuda, x, sigmas, case.mu, symmetries, case.sigma_d_square, kmax)
    assert status == 0 and np.array_equal(_bits(got), _bits(direct))
    # the transporter: shared mu expanded to [B, N, D], as the reference's method takes it
    transporter = Transporter(net.symmetries)
    image = transporter.get_optimal_transport(_dev(x, cuda), _dev(np.broadcast_to(case.mu, x.shape), cuda))
    kernel_image = _align(cuda, x, case.mu, symmetries)[0]
    assert image.dtype == torch.float32 and np.array_equal(_bits(image.cpu().numpy()), _bits(kernel_image))
    _check("public transport", tc.torus(kernel_image, want.image), np.full(x.shape, tc.IMAGE_BAR), "N = 256")


def test_two_launches_give_the_same_bits(cuda):
    """N = 256, O = 48, B = 4: the alignment with its details and the fused score, twice."""
    case = tc.case("d3_n256")
    first, second = (_align(cuda, case.x, case.mu, case.operations) for _ in range(2))
    for a, b in zip(first[:4], second[:4]):
        assert a.tobytes() == b.tobytes()
    sigmas = tc.sigmas_of("d3_n256")
    first, second = (_score(cuda, case.x, sigmas, case.mu, case.operations, case.sigma_d_square, 4)[0] for _ in range(2))
    assert first.tobytes() == second.tobytes()


def test_the_first_minimum_in_operation_order(cuda):
    """Six operations each listed twice (O = 12, a ragged round-robin over 8 wavefronts) tie exactly: the two costs of a pair have
    the same bits whichever wavefront solved them, and the chosen operation is the first of its pair -- twice the restatement's
    choice among the six."""
    case = tc.case("d3_n63")
    once = tc.align(case.x, case.mu, case.operations[:6])
    assert (tc.operation_gaps(once.costs) > tc.OPERATION_GAP).all()
    image, operation, col_idx, costs, status = _align(cuda, case.x, case.mu, np.repeat(case.operations[:6], 2, axis=0))
    assert status == 0 and costs[:, 0::2].tobytes() == costs[:, 1::2].tobytes()
    assert np.array_equal(operation, 2 * once.operation)
    assert np.array_equal(col_idx, once.col_idx[np.arange(case.B), once.operation])
    _check("first minimum", tc.torus(image, once.image), np.full(image.shape, tc.IMAGE_BAR), "d3_n63")
