"""The contract of network_hooks.logits_unread (generators/network_hooks.py): a hint around one forward, nothing more."""
import pytest
import torch

from diffusion_for_multi_scale_molecular_dynamics_amd.generators import network_hooks as hooks
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.force_field_augmented_score_network import (
    ForceFieldAugmentedScoreNetwork, ForceFieldParameters)


class _Hinted(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.sigma_uniform_hint = False
        self.logits_unread_hint = False


def test_a_network_without_the_attribute_is_left_alone():
    bare = torch.nn.Linear(2, 2)
    with hooks.logits_unread(bare):
        assert not hasattr(bare, "logits_unread_hint")
    assert not hasattr(bare, "logits_unread_hint")


def test_it_nests_with_uniform_sigma_either_way_round():
    net = _Hinted()
    with hooks.uniform_sigma(net):
        with hooks.logits_unread(net):
            assert net.sigma_uniform_hint is True and net.logits_unread_hint is True
        assert net.sigma_uniform_hint is True and net.logits_unread_hint is False
    with hooks.logits_unread(net):
        with hooks.uniform_sigma(net):
            assert net.sigma_uniform_hint is True and net.logits_unread_hint is True
        assert net.sigma_uniform_hint is False and net.logits_unread_hint is True
    assert net.sigma_uniform_hint is False and net.logits_unread_hint is False


def test_it_is_restored_when_the_forward_raises():
    net = _Hinted()
    with pytest.raises(RuntimeError, match="inside"):
        with hooks.logits_unread(net):
            assert net.logits_unread_hint is True
            raise RuntimeError("inside")
    assert net.logits_unread_hint is False


def test_the_force_field_wrapper_passes_it_through():
    inner = _Hinted()
    ff = ForceFieldAugmentedScoreNetwork(inner, ForceFieldParameters(radial_cutoff=2.5, strength=5.0))
    with hooks.logits_unread(ff):
        assert inner.logits_unread_hint is True
    assert inner.logits_unread_hint is False
    bare = ForceFieldAugmentedScoreNetwork(torch.nn.Linear(2, 2), ForceFieldParameters(radial_cutoff=2.5, strength=5.0))
    with hooks.logits_unread(bare):                       # the wrapped network lacks the name: so does the wrapper
        assert not hasattr(bare, "logits_unread_hint")
