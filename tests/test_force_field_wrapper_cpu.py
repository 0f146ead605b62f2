"""ForceFieldAugmentedScoreNetwork on the host: what the generator reads through the wrapper, and the captured graph's key."""
import warnings

import pytest
import torch

import nets
from diffusion_for_multi_scale_molecular_dynamics_amd.generators import network_hooks as hooks
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.langevin_generator import LangevinGenerator
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
    PredictorCorrectorSamplingParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.force_field_augmented_score_network import (
    ForceFieldAugmentedScoreNetwork, ForceFieldParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters


class _Inner(torch.nn.Module):
    """What the generator looks for on an EGNN, as plain attributes."""

    def __init__(self, safe):
        super().__init__()
        self.sigma_uniform_hint = False
        self.first_layer_table = "auto"
        self.safe = safe
        self.asked = None

    def capture_safe(self, batch_size, number_of_atoms, device):
        self.asked = (batch_size, number_of_atoms, device)
        return self.safe


def _wrap(inner, strength=5.0):
    return ForceFieldAugmentedScoreNetwork(inner, ForceFieldParameters(radial_cutoff=2.5, strength=strength))


def test_hint_and_table_pass_through():
    inner = _Inner(True)
    ff = _wrap(inner)
    assert ff.sigma_uniform_hint is False and ff.first_layer_table == "auto"
    ff.sigma_uniform_hint = True
    ff.first_layer_table = "off"
    assert inner.sigma_uniform_hint is True and inner.first_layer_table == "off"
    inner.first_layer_table = "on"
    assert ff.first_layer_table == "on"
    # an inner network without them: the wrapper has none either (the generator's hasattr / getattr defaults apply)
    bare = _wrap(nets.fake_net(1))
    assert not hasattr(bare, "sigma_uniform_hint") and getattr(bare, "first_layer_table", "off") == "off"


@pytest.mark.parametrize("safe", [True, False])
def test_capture_safe_is_the_inner_networks_answer(safe):
    inner = _Inner(safe)
    assert _wrap(inner).capture_safe(512, 64, "cpu") is safe
    assert inner.asked == (512, 64, "cpu")
    assert _wrap(nets.fake_net(1)).capture_safe(512, 64, "cpu") is True


def _generator(net):
    noise = NoiseParameters(total_time_steps=4, sigma_min=1e-4, sigma_max=0.25)
    sampling = PredictorCorrectorSamplingParameters(number_of_atoms=8, num_atom_types=1, number_of_samples=4,
                                                    number_of_corrector_steps=1, use_fixed_lattice_parameters=True,
                                                    cell_dimensions=[5.43] * 3, rng_mode="device", seed=1, use_hip_graph=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LangevinGenerator(noise, sampling, net)


def test_graph_key_follows_the_force_field_values():
    start = AXL(A=torch.zeros(4, 8, dtype=torch.long), X=torch.zeros(4, 8, 3), L=torch.zeros(4, 6))
    inner = nets.fake_net(1)
    gen_a, gen_b = _generator(_wrap(inner, 5.0)), _generator(_wrap(inner, 6.0))
    assert gen_a._graph_key(start) != gen_b._graph_key(start)
    assert _generator(_wrap(inner, 5.0))._graph_key(start) == gen_a._graph_key(start)
    # the same parameter object mutated: the key kept by a loop must not follow it
    key = gen_a._graph_key(start)
    gen_a.axl_network.force_field_parameters.strength = 7.0
    assert gen_a._graph_key(start) != key
    gen_a.axl_network.force_field_parameters.strength = 5.0
    assert gen_a._graph_key(start) == key
    gen_a.axl_network.force_field_parameters.radial_cutoff = 2.0
    assert gen_a._graph_key(start) != key


def test_forwarded_methods_reach_the_inner_network_and_are_absent_without_it():
    inner = _Inner(True)
    inner.calls = []
    inner.adapt_f16_range = lambda: inner.calls.append("adapt")
    inner.begin_f16_range_fallback = lambda: inner.calls.append("begin")
    inner.edge_chain_precision = "f16x3"
    ff = _wrap(inner)
    with hooks.exact_f32(ff):
        assert inner.edge_chain_precision == "f32" and inner.calls == ["begin"]
    assert inner.edge_chain_precision == "f16x3" and inner.calls == ["begin", "adapt"]
    bare = _wrap(nets.fake_net(1))
    for name in ForceFieldAugmentedScoreNetwork.FORWARDED:
        assert not hasattr(bare, name)
        setattr(bare, name, "dropped")
        assert not hasattr(bare, name) and not hasattr(bare._score_network, name)


def test_hooks_on_a_bare_module():
    """A caller's plain torch.nn.Module is a legal network: every hook has a meaning without the attribute."""
    net = torch.nn.Linear(2, 2)
    before = set(vars(net))
    assert hooks.status_word(net) is None and hooks.take_reports(net) == 0
    assert not hooks.reports_watched(net)
    hooks.clear_reports(net)
    assert hooks.capture_safe(net, 4, 8, "cpu") is True
    with hooks.uniform_sigma(net):
        assert not hasattr(net, "sigma_uniform_hint")
    assert hooks.capture_key(net) == (None, None, None)
    assert set(vars(net)) == before


def test_hooks_read_the_live_network():
    inner = _Inner(True)
    assert hooks.reports_watched(inner)                  # first_layer_table "auto"
    inner.first_layer_table = "off"
    assert not hooks.reports_watched(inner)
    inner.edge_chain_precision = "f16x3"
    assert hooks.reports_watched(inner) and hooks.reports_watched(_wrap(inner))
    inner.graph_status = torch.tensor([hooks.REPORTS | 1], dtype=torch.int32)
    assert hooks.take_reports(inner) == hooks.REPORTS and int(inner.graph_status) == 1 and hooks.take_reports(inner) == 0
    with hooks.uniform_sigma(inner):
        assert inner.sigma_uniform_hint is True
    assert inner.sigma_uniform_hint is False
