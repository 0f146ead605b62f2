"""The optimal-transport modules on the GPU (transport/, csrc/mdx_transport.hip) against the reference's own outputs
(tests/golden/transport/, made by tests/golden/make_golden_transport.py from the reference in binary32 and in binary64).

The alignment kernel is binary64 inside, so the reference's binary64 image is what it is held to: 1e-6 per structure on the torus
(one rounding of the output to binary32, 6e-8, with margin -- the bar of tests/test_analytical_score_gpu.py).  The discrete
choices (operation, permutation) and the costs are compared on the cases whose structures are stable between the reference's two
precisions; where operations tie exactly (two atoms; the toy sites) only the image is.

Not here: NoisingTransform(use_optimal_transport=True).  tests/test_generator_gpu.py pins that the constructor refuses it; the
per-structure-mu path it would run is held to the `noising_d3_n8` fixture through Transporter.get_optimal_transport instead."""
import numpy as np
import pytest
import torch

from test_transport_cpu import fixture

pytestmark = pytest.mark.gpu

CASES = ["d1_n3", "d2_n3", "d3_n5", "d3_n8", "d3_n8_identity", "d3_n2_ties", "toy1d", "d3_n64", "d3_n65", "noising_d3_n8"]
BAR = 1e-6
EPS32 = 2.0 ** -24


def _transporter(case, cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd.transport.transporter import Transporter
    return Transporter(torch.from_numpy(case["operations"]).to(cuda))


def _torus(a, b):
    """The largest coordinate difference on the torus, per structure."""
    diff = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.abs(diff - np.round(diff)).reshape(diff.shape[0], -1).max(axis=1)


def _mu(case, cuda):
    """mu as the reference's method takes it: [B, N, D]."""
    x = case["X"]
    mu = case["MU"] if "MU" in case.files else np.broadcast_to(case["sites"], x.shape)
    return torch.from_numpy(np.ascontiguousarray(mu)).to(cuda)


def _centre_bar(x):
    """What a binary32 evaluation of the atan2 centre may differ by from the binary64 one, per structure and dimension: every sine
    and cosine of 2 pi x carries the rounding of its argument (2 pi 2^-24) and its own (2^-24), the mean no more than that, and
    atan2 turns an error e of a mean of length |m| into e / |m| radians: (2 pi + 1) 2^-24 / (2 pi |m|), doubled for the two
    means, plus two roundings of the result."""
    m = np.abs(np.exp(2j * np.pi * x.astype(np.float64)).mean(axis=1))
    return 2.0 * (2.0 * np.pi + 1.0) * EPS32 / (2.0 * np.pi * m) + 2.0 * EPS32


@pytest.mark.parametrize("name", CASES)
def test_aligned_image_and_discrete_choices(cuda, name):
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    case = fixture(name)
    transporter = _transporter(case, cuda)
    x, mu = torch.from_numpy(case["X"]).to(cuda), _mu(case, cuda)
    image = transporter.get_optimal_transport(x, mu)
    assert image.shape == x.shape and image.dtype == torch.float32 and image.is_cuda
    got = image.cpu().numpy()
    assert (got >= 0.0).all() and (got < 1.0).all()
    distance = _torus(got, case["image64"])
    held = np.ones(len(distance), bool) if bool(case["compare_discrete"]) else case["agree"]
    print(f"{name}: image vs binary64 on the torus, max over {int(held.sum())} structures {distance[held].max():.2e}")
    assert held.any() and (distance[held] <= BAR).all(), distance
    operations = transporter._operations(x.device)
    aligned, operation, col_idx, costs = kernels.transport_align(x, mu, operations, with_details=True)
    assert torch.equal(aligned, image)
    if "MU" not in case.files:      # one shared [N, D] mu gives the bits of its B copies
        shared = kernels.transport_align(x, torch.from_numpy(case["sites"]).to(cuda), operations)
        assert torch.equal(shared, image)
    if not bool(case["compare_discrete"]):
        return
    assert case["stable"].all()
    operation, col_idx, costs = operation.cpu().numpy(), col_idx.cpu().numpy(), costs.cpu().numpy()
    assert np.array_equal(operation, case["operation64"])
    assert np.array_equal(col_idx, case["col_idx64"][np.arange(len(operation)), operation])
    assert (np.abs(costs - case["costs64"]) <= 1e-12 * np.abs(case["costs64"])).all(), np.abs(costs / case["costs64"] - 1).max()


@pytest.mark.parametrize("name", ["d3_n5", "d3_n8"])
def test_transporter_methods_one_by_one(cuda, name):
    case = fixture(name)
    transporter = _transporter(case, cuda)
    x = torch.from_numpy(case["X"]).to(cuda)
    bar = _centre_bar(case["X"])
    centre = transporter.get_atan2_translation(x).cpu().numpy().astype(np.float64)
    diff = centre - case["centre64"]
    assert centre.shape == case["centre64"].shape and (np.abs(diff - np.round(diff)) <= bar).all()
    invariant = transporter.get_translation_invariant(x).cpu().numpy()
    assert (_torus(invariant, case["x_invariant64"]) <= bar.max(axis=1) + 2 * EPS32).all()
    # the cost matrices in binary32 from the binary64 invariants: each geodesic displacement g (|g| <= 1/2) carries the rounding
    # of the inputs, of 2 pi delta, of sin / cos / atan2 -- a few 2^-24 of a turn, 8 here -- and d/dg of g^2 is 2 |g| <= 1
    O, N, D = case["operations"].shape[0], int(case["N"]), int(case["D"])
    x_inv = torch.from_numpy(case["x_invariant64"][:2]).float().to(cuda)
    mu_inv = torch.from_numpy(np.broadcast_to(case["mu_invariant64"], (2, N, D)).copy()).float().to(cuda)
    matrices = transporter._get_all_cost_matrices(x_inv, mu_inv)
    assert matrices.shape == (2, O, N, N)
    assert (np.abs(matrices.cpu().numpy() - case["cost_matrices64"]) <= 8 * EPS32 * D).all()
    # the two assignment methods on the fixture's own binary64 matrices
    stored = torch.from_numpy(case["cost_matrices64"]).to(cuda)
    identity = np.eye(N, dtype=np.float32)
    for b, o in ((0, 0), (1, O - 1), (1, O // 2)):
        permutation, cost = transporter._find_permutation_and_cost(stored[b, o])
        assert np.array_equal(permutation.cpu().numpy(), identity[:, case["col_idx64"][b, o]])
        assert abs(float(cost) - case["costs64"][b, o]) <= 1e-12 * case["costs64"][b, o]
    permutations, chosen = transporter._solve_linear_assigment_problem(stored)
    assert permutations.shape == (2, N, N) and chosen.shape == (2, D, D)
    for b in range(2):
        o = int(case["operation64"][b])
        assert np.array_equal(permutations[b].cpu().numpy(), identity[:, case["col_idx64"][b, o]])
        assert np.array_equal(chosen[b].cpu().numpy(), case["operations"][o])
    # ... and composed as the reference composes them they give the kernel's image
    rotated = torch.einsum("bij,bnj->bni", chosen.double(), torch.from_numpy(case["mu_invariant64"]).to(cuda).expand(2, N, D))
    composed = torch.einsum("bmn,bmd->bnd", permutations.double(), rotated).cpu().numpy()
    assert (_torus(composed, case["image64"][:2]) <= 1e-12).all()


def test_translation_invariant_has_the_references_three_properties(cuda):
    """Invariant under a global translation, equivariant under a permutation of the atoms and under a point-group operation (the
    reference's own tests of get_translation_invariant), within the binary32 bar of the centre."""
    case = fixture("d3_n5")
    transporter = _transporter(case, cuda)
    x = torch.from_numpy(case["X"][:8]).to(cuda)
    want = transporter.get_translation_invariant(x).cpu().numpy()
    bar = (2 * _centre_bar(case["X"][:8]).max(axis=1) + 4 * EPS32)
    shift = torch.tensor([0.3, 0.55, 0.8], device=cuda)
    shifted = torch.remainder(x + shift, 1.0)
    assert (_torus(transporter.get_translation_invariant(shifted).cpu().numpy(), want) <= bar).all()
    permutation = torch.tensor([3, 0, 4, 2, 1], device=cuda)
    assert (_torus(transporter.get_translation_invariant(x[:, permutation]).cpu().numpy(), want[:, permutation.cpu().numpy()]) <= bar).all()
    for o in (7, 20, 41):
        operation = torch.from_numpy(case["operations"][o]).to(cuda)
        rotated = torch.remainder(torch.einsum("ij,bnj->bni", operation, x), 1.0)
        expected = np.einsum("ij,bnj->bni", case["operations"][o].astype(np.float64), want.astype(np.float64))
        assert (_torus(transporter.get_translation_invariant(rotated).cpu().numpy(), expected) <= bar).all(), o


def test_optimal_permutation(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd.transport.optimal_permutation import get_optimal_permutation
    g = torch.Generator().manual_seed(3)
    for n, d in ((1, 3), (6, 2), (70, 3)):
        x = torch.rand(n, d, generator=g)
        shuffle = torch.randperm(n, generator=g)
        y = torch.remainder(x[shuffle] + 1e-4 * torch.randn(n, d, generator=g), 1.0)       # y[k] is x[shuffle[k]], nearly
        permutation = get_optimal_permutation(x.to(cuda), y.to(cuda))
        assert permutation.shape == (n, n) and permutation.is_cuda
        assert torch.equal(permutation.cpu(), torch.eye(n)[torch.argsort(shuffle), :])
        assert (_torus((permutation.cpu() @ y).numpy()[None], x.numpy()[None]) <= 1e-3).all()


def test_a_coordinate_that_is_not_finite_is_reported(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    case = fixture("d3_n5")
    transporter = _transporter(case, cuda)
    x, mu = torch.from_numpy(case["X"]).to(cuda), _mu(case, cuda)
    clean = transporter.get_optimal_transport(x, mu)
    bad = x.clone()
    bad[3, 2, 1] = float("inf")
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    out, operation, col_idx, costs = kernels.transport_align(bad, mu, transporter._operations(x.device), with_details=True, status=status)
    others = [b for b in range(x.shape[0]) if b != 3]
    assert torch.isnan(out[3]).all() and torch.equal(out[others], clean[others])
    assert int(operation[3]) == -1 and (col_idx[3] == -1).all() and torch.isnan(costs[3]).all()
    assert int(status.item()) == _hip.STATUS_ANALYTICAL_COORDINATES
    # any finite coordinate is accepted: a structure moved by whole cells has the same image
    moved = transporter.get_optimal_transport(x + 2.0, mu)
    assert (_torus(moved.cpu().numpy(), clean.cpu().numpy()) <= 4 * EPS32 * 3).all()
