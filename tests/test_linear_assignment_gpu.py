"""The device linear-assignment solver (csrc/mdx_transport.hip, kernels.linear_assignment) against
scipy.optimize.linear_sum_assignment on the same binary64 matrices.  The sizes cover one, two and four columns per lane and the
ragged tails (a lane owns columns lane, lane + 64, ..).  scipy is the tests' alone: the package never imports it."""
import functools

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 63, 64, 65, 130, 256, 127, 128, 129, 192, 193, 255]      # appended to: a size's seed is its index
PER_SIZE = 3


def _kernels():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    return _hip, kernels


@functools.lru_cache(maxsize=None)
def _matrices(kind, n):
    """(matrices f64 [3, n, n], scipy's col_idx [3, n], scipy's optimum [3]): made once, shared, never written to."""
    rng = np.random.default_rng(1000 * SIZES.index(n) + len(kind))
    if kind == "uniform":
        costs = rng.random((PER_SIZE, n, n))
    elif kind == "integers":
        costs = rng.integers(0, 4, (PER_SIZE, n, n)).astype(np.float64)
    elif kind == "equal":
        costs = np.full((PER_SIZE, n, n), 0.7)
    else:
        costs = 10.0 ** rng.uniform(-12.0, 3.0, (PER_SIZE, n, n))
    cols = np.stack([linear_sum_assignment(c)[1] for c in costs])
    optimum = np.array([c[np.arange(n), col].sum() for c, col in zip(costs, cols)])
    for a in (costs, cols, optimum):
        a.setflags(write=False)
    return costs, cols, optimum


def _solve(costs, cuda, status=None):
    _, kernels = _kernels()
    col_idx, total = kernels.linear_assignment(torch.from_numpy(np.array(costs)).to(cuda), status=status)
    assert col_idx.dtype == torch.int32 and total.dtype == torch.float64 and col_idx.is_cuda
    return col_idx.cpu().numpy(), total.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
def test_unique_optimum_is_scipys(cuda, n):
    costs, cols, optimum = _matrices("uniform", n)
    got_cols, got_total = _solve(costs, cuda)
    assert np.array_equal(got_cols, cols)
    assert (np.abs(got_total - optimum) <= 1e-12 * np.abs(optimum)).all(), (got_total, optimum)


@pytest.mark.parametrize("kind", ["integers", "equal", "range"])
@pytest.mark.parametrize("n", SIZES)
def test_ties_and_a_wide_range_reach_scipys_optimum(cuda, n, kind):
    """Integer costs in 0..3 and an all-equal matrix have many optimal assignments, costs spread over 1e-12 .. 1e3 make the
    duals lose the small entries: the answer is a permutation whose cost, summed again on the host, is scipy's optimum -- exactly
    for the integer and all-equal matrices, to 1e-12 of the optimum otherwise.  The kernel's own cost is the same terms summed
    in row order, where numpy sums pairwise: equal for integers, within 1e-12 otherwise."""
    costs, _, optimum = _matrices(kind, n)
    got_cols, got_total = _solve(costs, cuda)
    for m in range(PER_SIZE):
        assert sorted(got_cols[m].tolist()) == list(range(n)), (kind, n, m)
        again = costs[m][np.arange(n), got_cols[m]].sum()
        if kind == "range":
            assert abs(again - optimum[m]) <= 1e-12 * abs(optimum[m]), (again, optimum[m])
        else:
            assert again == optimum[m], (kind, n, m, again, optimum[m])
        if kind == "integers":
            assert got_total[m] == optimum[m], (n, m, got_total[m], optimum[m])
        assert abs(got_total[m] - optimum[m]) <= 1e-12 * abs(optimum[m]), (kind, n, m, got_total[m], optimum[m])


@pytest.mark.parametrize("n", [5, 65, 256])
def test_binary32_input_is_its_binary64_promotion(cuda, n):
    costs32 = _matrices("uniform", n)[0].astype(np.float32)
    cols32, total32 = _solve(costs32, cuda)
    cols64, total64 = _solve(costs32.astype(np.float64), cuda)
    assert np.array_equal(cols32, cols64) and total32.tobytes() == total64.tobytes()
    assert np.array_equal(cols32, np.stack([linear_sum_assignment(c.astype(np.float64))[1] for c in costs32]))


@pytest.mark.parametrize("n", [3, 130])
def test_a_cost_that_is_not_finite_is_reported_not_a_fault(cuda, n):
    """One launch: a NaN in one matrix, an infinity in another, one clean.  The first two come back as -1 with a NaN cost and the
    status bit; the clean one is solved.  (The kernel checks the matrix first and dereferences nothing that depends on it.)"""
    _hip, _ = _kernels()
    costs, cols, optimum = _matrices("uniform", n)
    bad = costs.copy()
    bad[0, n - 1, n // 2] = np.nan
    bad[1, 0, 0] = np.inf
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    got_cols, got_total = _solve(bad, cuda, status)
    assert int(status.item()) == _hip.STATUS_LAP_COST
    assert (got_cols[:2] == -1).all() and np.isnan(got_total[:2]).all()
    assert np.array_equal(got_cols[2], cols[2]) and abs(got_total[2] - optimum[2]) <= 1e-12 * optimum[2]
    clean = torch.zeros(1, dtype=torch.int32, device=cuda)
    _solve(costs, cuda, clean)
    assert int(clean.item()) == 0


@pytest.mark.parametrize("n", [64, 256])
def test_two_launches_give_the_same_bits(cuda, n):
    for kind in ("uniform", "integers"):
        costs = _matrices(kind, n)[0]
        first, second = _solve(costs, cuda), _solve(costs, cuda)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()


def test_sizes_beyond_the_kernel_are_refused(cuda):
    _hip, kernels = _kernels()
    with pytest.raises(_hip.MdxError, match="unsupported size or option"):
        kernels.linear_assignment(torch.zeros(1, 257, 257, device=cuda))
    with pytest.raises(ValueError):
        kernels.linear_assignment(torch.zeros(1, 3, 4, device=cuda))
    empty_cols, empty_costs = kernels.linear_assignment(torch.zeros(0, 4, 4, device=cuda))
    assert empty_cols.shape == (0, 4) and empty_costs.shape == (0,)
