"""ForceFieldAugmentedScoreNetwork inside the sampler: the iteration around it is captured into a hipGraph, replays give the eager
launches' bits, the EGNN behind it runs with the sampler's uniform-sigma hint (its first-layer table), and a change of the
force-field parameters recaptures."""
import warnings

import pytest
import torch

import cases
import nets
from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.langevin_generator import LangevinGenerator
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
    PredictorCorrectorSamplingParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.force_field_augmented_score_network import (
    ForceFieldAugmentedScoreNetwork, ForceFieldParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION,
                                                                          TIME)
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters

pytestmark = pytest.mark.gpu

B, N = 8, 64


def _inner(kind, device):
    if kind == "mlp":
        return nets.mlp_net(N, 1, hidden=64, n_hidden=2, seed=5).to(device)
    net = nets.egnn_net(1, "radial_cutoff", 7.5, hidden=32, n_layers=2, n_hidden=2, seed=7).to(device)
    return net


def _generator(net, use_graph, strength=5.0, seed=20250815):
    noise = NoiseParameters(total_time_steps=3, sigma_min=1e-4, sigma_max=0.2, schedule_type="linear",
                            corrector_step_epsilon=2.5e-8)
    sampling = PredictorCorrectorSamplingParameters(
        number_of_atoms=N, num_atom_types=1, number_of_samples=B, number_of_corrector_steps=2, atom_type_greedy_sampling=False,
        one_atom_type_transition_per_step=False, use_fixed_lattice_parameters=True, cell_dimensions=[10.86] * 3,
        rng_mode="device", seed=seed, use_hip_graph=use_graph)
    ff = ForceFieldAugmentedScoreNetwork(net, ForceFieldParameters(radial_cutoff=2.5, strength=strength))
    return LangevinGenerator(noise, sampling, ff)


def _two_calls(gen, device):
    outs = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            for _ in range(2):
                outs.append(gen.sample(B, device))
    return outs, [str(w.message) for w in caught]


def _equal(a, b):
    return torch.equal(a.A, b.A) and torch.equal(a.X, b.X) and torch.equal(a.L, b.L)


@pytest.mark.parametrize("kind", ["mlp", "egnn"])
def test_captured_loop_matches_eager_launches(cuda, kind):
    net = _inner(kind, cuda)
    hints = []
    if kind == "egnn":
        net.register_forward_pre_hook(lambda module, args: hints.append(module.sigma_uniform_hint))
    graph_gen = _generator(net, True)
    got, messages = _two_calls(graph_gen, cuda)
    assert not [m for m in messages if "launched eagerly" in m], messages
    assert graph_gen._buffers["graph_loop"].graph is not None
    want, _ = _two_calls(_generator(net, False), cuda)
    assert _equal(got[0], want[0]) and _equal(got[1], want[1])
    assert not torch.equal(got[0].X, got[1].X)           # (the second call is another trajectory)
    if kind == "egnn":
        assert hints and all(hints), hints               # the sampler's forwards reach the EGNN with the hint
        assert net.egnn.graph_layers[0]._chain[1] is not None, "the fused edge chain did not run"


def test_wrapped_egnn_forward_is_the_bare_forward_plus_the_kernel(cuda):
    net = _inner("egnn", cuda)
    ff = ForceFieldAugmentedScoreNetwork(net, ForceFieldParameters(radial_cutoff=2.5, strength=5.0))
    g = torch.Generator().manual_seed(3)
    X = ((cases.diamond_sites(2)[None] + 0.02 * torch.randn(B, N, 3, generator=g)) % 1.0).to(cuda)
    L = torch.tensor([10.86, 10.86, 10.86, 0.0, 0.0, 0.0], device=cuda).repeat(B, 1)
    batch = {NOISY_AXL_COMPOSITION: AXL(A=torch.zeros(B, N, dtype=torch.long, device=cuda), X=X, L=L),
             TIME: torch.full((B, 1), 0.5, device=cuda), NOISE: torch.full((B, 1), 0.05, device=cuda),
             CARTESIAN_FORCES: torch.zeros(B, N, 3, device=cuda)}
    with torch.no_grad():
        ff.sigma_uniform_hint = True
        assert net.sigma_uniform_hint is True
        wrapped = ff(batch, conditional=False)
        bare = net(batch, conditional=False)
        ff.sigma_uniform_hint = False
        forces = kernels.force_field_pseudo_force(X, L, 1.0, 2.5, 5.0)
    ff.check_status()
    assert torch.equal(wrapped.X, bare.X + forces)
    assert torch.equal(wrapped.A, bare.A) and torch.equal(wrapped.L, bare.L)


def test_strength_change_recaptures(cuda):
    net = _inner("mlp", cuda)
    gen = _generator(net, True)
    with torch.no_grad():
        gen.sample(B, cuda)
        first = gen._buffers["graph_loop"]
        gen.axl_network.force_field_parameters.strength = 9.0
        got = gen.sample(B, cuda)
    assert gen._buffers["graph_loop"] is not first and gen._buffers["graph_loop"].graph is not None
    fresh = _generator(net, True, strength=9.0)
    with torch.no_grad():
        fresh.sample(B, cuda)
        want = fresh.sample(B, cuda)
    assert _equal(got, want)


def test_cli_force_field_graph_matches_eager(cuda, tmp_path):
    import yaml
    from diffusion_for_multi_scale_molecular_dynamics_amd import sample_diffusion
    base = dict(noise=dict(total_time_steps=6, sigma_min=1e-4, sigma_max=0.25),
                sampling=dict(algorithm="predictor_corrector", spatial_dimension=3, number_of_atoms=8, number_of_samples=12,
                              sample_batchsize=6, num_atom_types=1, number_of_corrector_steps=1,
                              use_fixed_lattice_parameters=True, cell_dimensions=[5.43, 5.43, 5.43], rng_mode="device"),
                elements=["Si"], force_field=dict(radial_cutoff=2.5, strength=5.0),
                model=dict(score_network=dict(architecture="mlp", number_of_atoms=8, num_atom_types=1,
                                              n_hidden_dimensions=2, hidden_dimensions_size=16,
                                              relative_coordinates_embedding_dimensions_size=8,
                                              noise_embedding_dimensions_size=4, time_embedding_dimensions_size=4,
                                              atom_type_embedding_dimensions_size=1,
                                              lattice_parameters_embedding_dimensions_size=1)))
    samples = {}
    for graph in (True, False):
        cfg = dict(base, sampling=dict(base["sampling"], use_hip_graph=graph))
        path = tmp_path / f"graph_{graph}.yaml"
        path.write_text(yaml.safe_dump(cfg))
        out = tmp_path / f"out_{graph}"
        sample_diffusion.main(["--config", str(path), "--output", str(out), "--device", "cuda", "--random_init_seed", "3"])
        samples[graph] = torch.load(out / "samples.pt", weights_only=False)["original_axl"]
    assert _equal(samples[True], samples[False])
