"""The equivariant analytical score network on the GPU (csrc/mdx_transport.hip) against the reference's own outputs
(tests/golden/transport/, made by tests/golden/make_golden_transport.py from the reference in binary32 and in binary64).

The kernel is binary64 inside, so the binary64 output is what it is held to (1e-6 per (case, noise level), 2e-6 per structure:
one rounding of the output to binary32, 6e-8, with margin); against the reference's binary32 output the bar is the fixture's own
floor |out32 - out64| / |out64| plus the same 1e-6 (the triangle inequality) -- the bars of tests/test_analytical_score_gpu.py."""
import warnings

import numpy as np
import pytest
import torch

from test_analytical_score_gpu import _batch, _rel
from test_transport_cpu import NETWORK_CASES, fixture, network_of

pytestmark = pytest.mark.gpu

BAR_CASE, BAR_STRUCTURE = 1e-6, 2e-6


def _per_structure(got, want):
    B = got.shape[0]
    return np.linalg.norm((got - want).reshape(B, -1), axis=1) / np.linalg.norm(want.reshape(B, -1), axis=1)


@pytest.mark.parametrize("name", NETWORK_CASES)
def test_score_against_the_reference(cuda, name):
    case = fixture(name)
    net = network_of(case).to(cuda)
    x = torch.from_numpy(case["X"]).to(cuda)
    failed = []
    for level, sigma_value in enumerate(case["sigma"]):
        sigma = torch.full((x.shape[0],), float(sigma_value), device=cuda)
        with torch.no_grad():
            out = net(_batch(x, sigma), conditional=False)
        assert out.X.is_cuda and out.A.is_cuda and out.L.is_cuda and out.L.shape == x.shape and not out.L.any()
        assert np.array_equal(out.A.cpu().numpy(), np.broadcast_to(np.array([0.0, -np.inf], np.float32), x.shape[:2] + (2,)))
        got = out.X.cpu().numpy().astype(np.float64)
        s64, s32 = case["score64"][level], case["score32"][level].astype(np.float64)
        rel64, per64 = _rel(got, s64), _per_structure(got, s64)
        per32, floor = _per_structure(got, s32), case["floor_structure"][level]
        print(f"{name} sigma {float(sigma_value):g}: vs binary64 {rel64:.2e} (structure max {per64.max():.2e}); vs binary32 beyond "
              f"its floor by {np.max(per32 - floor):.2e}")
        if not rel64 <= BAR_CASE:
            failed.append(f"level {level}: rel-L2 vs binary64 {rel64:.3e} > {BAR_CASE}")
        if not (per64 <= BAR_STRUCTURE).all():
            failed.append(f"level {level}: a structure vs binary64 {per64.max():.3e} > {BAR_STRUCTURE}")
        # (the binary32 norm in the denominator differs from the binary64 one by the floor itself: second order)
        if not (per32 <= floor * (1 + floor) + BAR_CASE).all():
            failed.append(f"level {level}: a structure vs binary32 beyond its floor + {BAR_CASE}: {np.max(per32 - floor):.3e}")
        # the public method (two kernels and plain torch in binary32 between them) agrees with the forward to binary32 rounding
        # of the residual u: d score / d u = sigma / sigma_eff^2 at most, times a few 2^-24
        public = net.get_normalized_scores(x, sigma.view(-1, 1, 1).expand(x.shape).contiguous()).cpu().numpy().astype(np.float64)
        slope = float(sigma_value) / (float(case["sigma_d"]) ** 2 + float(sigma_value) ** 2)
        if bool(case["compare_discrete"]) and not (np.abs(public - got) <= 2e-6 * slope + 2e-6 * np.abs(got)).all():
            failed.append(f"level {level}: get_normalized_scores differs from the forward by {np.abs(public - got).max():.3e}")
    assert not failed, failed


def _score(net, x, sigma_value=0.2):
    sigma = torch.full((x.shape[0],), sigma_value, device=x.device)
    with torch.no_grad():
        return net(_batch(x, sigma), conditional=False).X.cpu().numpy().astype(np.float64)


def test_forward_is_equivariant(cuda):
    """Under a permutation of the atoms, a global translation and a point-group operation of the input, on the generic
    (uniformly drawn) structures of the (3, 5) case: 1e-5."""
    case = fixture("d3_n5")
    net = network_of(case).to(cuda)
    x = torch.from_numpy(case["X"][:8]).to(cuda)
    want = _score(net, x)
    permutation = [3, 0, 4, 2, 1]
    assert _rel(_score(net, x[:, permutation].contiguous()), want[:, permutation]) <= 1e-5
    shift = torch.tensor([0.25, 0.5, 0.125], device=cuda)
    assert _rel(_score(net, torch.remainder(x + shift, 1.0)), want) <= 1e-5
    for o in (7, 20, 41):
        operation = torch.from_numpy(case["operations"][o]).to(cuda)
        rotated = torch.remainder(torch.einsum("ij,bnj->bni", operation, x), 1.0).contiguous()
        expected = np.einsum("ij,bnj->bni", case["operations"][o].astype(np.float64), want)
        assert _rel(_score(net, rotated), expected) <= 1e-5, o


def test_negative_controls(cuda):
    """What the symmetries and the permutation are for: each of the two wrong answers differs from the right one by far more
    than 1e-3."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.score.wrapped_gaussian_score import get_coordinates_sigma_normalized_score
    from diffusion_for_multi_scale_molecular_dynamics_amd.utils.basis_transformations import map_relative_coordinates_to_unit_cell
    case = fixture("d3_n5")
    net = network_of(case).to(cuda)
    identity_only = network_of(case, use_point_group_symmetries=False).to(cuda)
    sites = torch.from_numpy(case["sites"]).to(cuda)
    g = torch.Generator().manual_seed(11)
    operation = torch.from_numpy(case["operations"][13]).to(cuda)       # not the identity
    assert not torch.equal(operation, torch.eye(3, device=cuda))
    noise = (0.01 * torch.randn(4, 5, 3, generator=g)).to(cuda)
    rotated = torch.remainder(torch.einsum("ij,nj->ni", operation, sites)[None] + noise + 0.3, 1.0).contiguous()
    with_symmetries, without = _score(net, rotated), _score(identity_only, rotated)
    assert _rel(without, with_symmetries) > 1e-3
    # the same score composed from the public pieces, with the aligned sites in the right and in a wrong order
    sigma, sigma_d = 0.2, float(case["sigma_d"])
    effective = float(np.sqrt(sigma_d**2 + sigma**2))
    x_invariant = net.transporter.get_translation_invariant(rotated)
    aligned = net.get_nearest_equilibrium_coordinates(rotated)
    composed = {}
    for key, order in (("right", [0, 1, 2, 3, 4]), ("wrong", [1, 2, 3, 4, 0])):
        u = map_relative_coordinates_to_unit_cell(x_invariant - aligned[:, order])
        score = get_coordinates_sigma_normalized_score(u, torch.full_like(u, effective), int(case["kmax"]))
        composed[key] = (sigma * score / effective).cpu().numpy().astype(np.float64)
    assert _rel(composed["right"], with_symmetries) <= 1e-4
    assert _rel(composed["wrong"], with_symmetries) > 1e-3


def test_state_dict_on_the_device(cuda):
    case = fixture("d3_n8")
    state = network_of(case).to(cuda).state_dict()
    assert list(state) == list(case["state_keys"])
    assert [str(tuple(v.shape)) for v in state.values()] == list(case["state_shapes"])
    assert [str(v.dtype) for v in state.values()] == list(case["state_dtypes"])
    assert all(v.is_cuda for v in state.values())


def test_invalid_sigma_is_reported_not_a_fault(cuda):
    case = fixture("d3_n5")
    net = network_of(case).to(cuda)
    x = torch.from_numpy(case["X"]).to(cuda)
    sigma = torch.full((x.shape[0],), 0.2, device=cuda)
    clean = net(_batch(x, sigma), conditional=False).X
    net.check_status()
    bad_sigma = sigma.clone()
    bad_sigma[1] = 0.0
    nan_x = x.clone()
    nan_x[5, 2, 1] = float("nan")
    for kwargs, rows, message in ((dict(x=x, sigma=bad_sigma), [1], "All values of sigma should be larger than zero."),
                                  (dict(x=nan_x, sigma=sigma), [5], "relative coordinates"),
                                  (dict(x=nan_x, sigma=bad_sigma), [1, 5], "All values of sigma should be larger than zero.")):
        out = net(_batch(kwargs["x"], kwargs["sigma"]), conditional=False).X
        others = [b for b in range(x.shape[0]) if b not in rows]
        assert torch.isnan(out[rows]).all() and torch.equal(out[others], clean[others])
        with pytest.raises(AssertionError, match=message):
            net.check_status()
        assert int(net.graph_status.item()) == 0
        net.check_status()
    # any finite coordinate is accepted (the reference wraps everything here)
    assert _rel(net(_batch(x + 1.0, sigma), conditional=False).X.cpu().numpy(), clean.cpu().numpy()) <= 1e-5
    net.check_status()


def test_sampler_runs_the_network_in_the_captured_loop(cuda):
    """LangevinGenerator at T 8, B 4, N 5: eager launches and the hipGraph replay give the same bits, and nothing falls back to
    eager launches (the forward reads nothing on the host)."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators import network_hooks
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.langevin_generator import LangevinGenerator
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import (
        PredictorCorrectorSamplingParameters)
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    case = fixture("d3_n5")
    net = network_of(case).to(cuda)
    assert net.capture_safe(4, 5, cuda) is True and network_hooks.capture_safe(net, 4, 5, cuda)
    noise = NoiseParameters(total_time_steps=8, sigma_min=1e-4, sigma_max=0.25)
    samples = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for use_graph in (False, True):
            spar = PredictorCorrectorSamplingParameters(number_of_atoms=5, num_atom_types=1, number_of_samples=4,
                                                        number_of_corrector_steps=1, use_fixed_lattice_parameters=True,
                                                        cell_dimensions=[5.43, 5.43, 5.43], rng_mode="device", seed=20251019,
                                                        use_hip_graph=use_graph)
            generator = LangevinGenerator(noise, spar, net)
            with torch.no_grad():
                samples.append(generator.sample(4, cuda))
            assert ("graph_loop" in generator._buffers) == use_graph
    assert not [str(w.message) for w in caught if "eagerly" in str(w.message)]
    eager, graphed = samples
    assert torch.equal(eager.X, graphed.X) and torch.equal(eager.A, graphed.A) and torch.isfinite(graphed.X).all()
    net.check_status()
