"""The optimal torus translation on the GPU (kernels.optimal_translation, csrc/mdx_optimal_translation.hip) against the reference's
own transport/optimal_translation.py (tests/golden/optimal_translation/, made by tests/golden/make_golden_optimal_translation.py
from the reference in binary32 and in binary64).

The kernel is binary64 inside, so the reference's binary64 result is what it is held to.  The bar on tau is derived, not measured:
tau lies in [-1/2, 1/2], it is ONE rounding to binary32 (spacing 2^-25 below 1/2, so at most 2^-26) of a binary64 value whose own
error is of order N 2^-53, and the fixtures' maker asserts that the candidate a binary64 evaluation picks is the reference's (the
two best costs of every (b, alpha) are more than 1e-6 apart): |tau - reference64| <= 2^-24 with margin.  The squared distance is
held to 1e-12 relative of the binary64 cost of the reference's tau, evaluated with the exact form of the displacement
(d - round(d)); the reference's own atan2 form keeps only eight digits where d is 1e-8 away from an integer (recorded in the
fixtures as atan2_cost_error).  The largest distances seen are printed (run with -s) and recorded in
profiles/r13_optimal_translation.md.

Not here: the reference's three helper functions.  They belong to its public module, which this package does not hold (see
tests/test_optimal_translation_cpu.py)."""
import numpy as np
import pytest
import torch

from test_optimal_translation_cpu import CASES, fixture

pytestmark = pytest.mark.gpu

TAU_BAR = 2.0 ** -24
COST_BAR = 1e-12


def _call(cuda, x, y, **kw):
    """(tau, squared_distance, number_of_candidates, status word) on the device, as numpy where it is compared as numbers."""
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    tau, squared_distance, count = kernels.optimal_translation(torch.as_tensor(x).to(cuda), torch.as_tensor(y).to(cuda),
                                                               with_details=True, status=status, **kw)
    assert tau.dtype == torch.float32 and squared_distance.dtype == torch.float64 and count.dtype == torch.int32
    assert tau.shape == squared_distance.shape == count.shape == (y.shape[0], y.shape[2]) and tau.is_cuda
    return tau, squared_distance, count, int(status.item())


def _bits(*tensors):
    return [t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).cpu() for t in tensors]


def _same_bits(a, b):
    return all(torch.equal(p, q) for p, q in zip(_bits(*a), _bits(*b)))


@pytest.mark.parametrize("name", CASES)
def test_parity_with_the_reference(cuda, name):
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    case = fixture(name)
    for D in case["dimensions"]:
        x, y, tau64, cost64 = (case[f"d{D}_{key}"] for key in ("x", "y", "tau64", "cost64"))
        tau, squared_distance, count, status = _call(cuda, x, y)
        tau, squared_distance, count = tau.cpu().numpy(), squared_distance.cpu().numpy(), count.cpu().numpy()
        infinite = np.isinf(tau64)
        assert np.array_equal(np.isinf(tau), infinite) and (tau[infinite] > 0).all() and not np.isnan(tau).any()
        distance = np.abs(tau.astype(np.float64)[~infinite] - tau64[~infinite])
        relative = np.abs(squared_distance[~infinite] - cost64[~infinite])
        print(f"{name} D {D}: |tau - reference64| max {distance.max():.2e}; squared distance, largest relative difference "
              f"{(relative[cost64[~infinite] > 0] / cost64[~infinite][cost64[~infinite] > 0]).max(initial=0.0):.2e}")
        assert distance.size + infinite.sum() == tau64.size and (distance <= TAU_BAR).all(), distance.max()
        assert np.array_equal(count, case[f"d{D}_count64"])
        assert np.array_equal(np.isinf(squared_distance), infinite) and (squared_distance[infinite] > 0).all()
        assert (relative <= COST_BAR * cost64[~infinite]).all(), (squared_distance, cost64)
        assert status == (_hip.STATUS_TRANSLATION_NO_CANDIDATE if infinite.any() else 0)


@pytest.mark.parametrize("N", [8, 64])
def test_minimal_on_a_grid_without_the_reference(cuda, N):
    """D^2(x, y + t) in binary64 torch on 4001 values of t per dimension: the kernel's minimum is not above the grid's, and its tau
    is within one grid step of the grid's arg-min."""
    case = fixture(f"uniform_n{N}")
    steps = 4001
    grid = torch.linspace(-0.5, 0.5, steps, dtype=torch.float64)
    for D in case["dimensions"]:
        x, y = torch.from_numpy(case[f"d{D}_x"]), torch.from_numpy(case[f"d{D}_y"])
        tau, squared_distance, _, status = _call(cuda, x, y)
        d = (y.double()[None] + grid[:, None, None, None]) - x.double()[None]             # [steps, B, N, D]
        on_grid = ((d - d.round())**2).sum(dim=2)
        lowest, where = on_grid.min(dim=0)
        assert status == 0 and bool((squared_distance.cpu() <= lowest + 1e-12).all())
        assert bool(((tau.cpu().double() - grid[where]).abs() <= 1.0 / (steps - 1)).all())


def test_a_coordinate_that_is_not_finite_voids_its_structure_only(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    case = fixture("uniform_n65")
    x, y = case["d3_x"].copy(), case["d3_y"].copy()
    clean = _call(cuda, x, y)
    assert clean[3] == 0
    y[1, 64, 2] = np.nan
    x[3, 0, 0] = np.inf
    tau, squared_distance, count, status = _call(cuda, x, y)
    assert status == _hip.STATUS_ANALYTICAL_COORDINATES
    bad, good = [1, 3], [0, 2, 4]
    assert bool(torch.isnan(tau[bad]).all()) and bool(torch.isnan(squared_distance[bad]).all()) and bool((count[bad] == -1).all())
    assert _same_bits([t[good] for t in (tau, squared_distance, count)], [t[good] for t in clean[:3]])


@pytest.mark.parametrize("name", ["shared_n8", "shared_n64"])
def test_a_shared_x_gives_the_bits_of_its_copies(cuda, name):
    case = fixture(name)
    for D in case["dimensions"]:
        x, y = case[f"d{D}_x"], case[f"d{D}_y"]
        assert x.ndim == 2
        shared = _call(cuda, x, y)
        expanded = _call(cuda, np.ascontiguousarray(np.broadcast_to(x, y.shape)), y)
        assert shared[3] == expanded[3] == 0 and _same_bits(shared[:3], expanded[:3])


def test_shapes_are_checked(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
    y = torch.rand(2, 5, 3, device=cuda)
    for bad in (torch.rand(3, 5, 3, device=cuda), torch.rand(5, 2, device=cuda), torch.rand(2, 5, device=cuda)):
        with pytest.raises(ValueError, match="expected"):
            kernels.optimal_translation(bad, y)
    with pytest.raises(ValueError, match="expected"):
        kernels.optimal_translation(y[0], y[0])
    with pytest.raises(MdxError, match="unsupported size or option"):
        kernels.optimal_translation(torch.rand(257, 3, device=cuda), torch.rand(2, 257, 3, device=cuda))
    with pytest.raises(MdxError, match="unsupported size or option"):
        kernels.optimal_translation(torch.rand(2, 8, 4, device=cuda), torch.rand(2, 8, 4, device=cuda))
    with pytest.raises(TypeError):
        kernels.optimal_translation(y.double(), y)
    assert kernels.optimal_translation(y[:0], y[:0]).shape == (0, 3)


def test_a_captured_call_replays_the_eager_bits(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    case = fixture("uniform_n64")
    x, y = torch.from_numpy(case["d3_x"]).to(cuda), torch.from_numpy(case["d3_y"]).to(cuda)
    assert y.shape == (5, 64, 3)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    eager = kernels.optimal_translation(x, y, with_details=True, status=status)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = kernels.optimal_translation(x, y, with_details=True, status=status)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(captured, eager)
    assert int(status.item()) == 0


def test_two_calls_give_the_same_bits(cuda):
    case = fixture("uniform_n256")
    first, second = _call(cuda, case["d3_x"], case["d3_y"]), _call(cuda, case["d3_x"], case["d3_y"])
    assert first[3] == second[3] == 0 and _same_bits(first[:3], second[:3])
