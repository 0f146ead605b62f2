"""What AnalyticalScoreNetwork and EquivariantAnalyticalScoreNetwork share through _ExactScoreOutputs, on the host: the constant
A and L outputs, the status-word protocol of check_status(), and the one reader of status bits in kernels.py."""
import pytest
import torch

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks._exact_score_outputs import _ExactScoreOutputs
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.analytical_score_network import (
    AnalyticalScoreNetwork, AnalyticalScoreNetworkParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.equivariant_analytical_score_network import (
    EquivariantAnalyticalScoreNetwork, EquivariantAnalyticalScoreNetworkParameters)

BLOCK = dict(spatial_dimension=1, number_of_atoms=2, num_atom_types=1, kmax=5, equilibrium_relative_coordinates=[[0.25], [0.75]],
             sigma_d=0.01)
CPU = torch.device("cpu")


@pytest.fixture(params=["analytical", "equivariant_analytical"])
def network(request):
    if request.param == "analytical":
        return AnalyticalScoreNetwork(AnalyticalScoreNetworkParameters(**BLOCK))
    return EquivariantAnalyticalScoreNetwork(EquivariantAnalyticalScoreNetworkParameters(**BLOCK))


def test_both_classes_take_the_shared_methods_from_the_mixin(network):
    for name in ("capture_safe", "check_status", "_status_on", "_constant_outputs", "_check_batch", "_as_axl"):
        assert name not in vars(type(network)) and getattr(type(network), name) is getattr(_ExactScoreOutputs, name)


def test_constant_outputs_are_made_once_per_batch_size(network):
    logits, zeros = network._constant_outputs(3, CPU)
    classes = network.number_of_atomic_classes
    assert logits.shape == (3, 2, classes) and zeros.shape == (3, 2, 1)
    assert torch.equal(logits[..., :-1], torch.zeros(3, 2, classes - 1)) and torch.all(logits[..., -1] == -torch.inf)
    assert torch.equal(zeros, torch.zeros(3, 2, 1))
    again = network._constant_outputs(3, CPU)
    assert again[0] is logits and again[1] is zeros
    other = network._constant_outputs(4, CPU)
    assert other[0] is not logits and other[1] is not zeros and other[0].shape == (4, 2, classes) and other[1].shape == (4, 2, 1)


def test_check_status_raises_the_references_assertions_and_clears_its_own_bits(network):
    network.check_status()                  # no status word yet: nothing to read
    network.graph_status = torch.tensor([_hip.STATUS_ANALYTICAL_SIGMA | 16], dtype=torch.int32)
    with pytest.raises(AssertionError) as raised:
        network.check_status()
    assert str(raised.value) == "All values of sigma should be larger than zero."
    assert network.graph_status.tolist() == [16]
    network.check_status()                  # another kernel's bit is not this class's to raise
    network.graph_status = torch.tensor([_hip.STATUS_ANALYTICAL_COORDINATES | 16], dtype=torch.int32)
    with pytest.raises(AssertionError) as raised:
        network.check_status()
    assert str(raised.value) == "the relative coordinates should all be in [0, 1)"
    assert network.graph_status.tolist() == [16]


def test_raise_loss_status_raises_the_index_error_and_clears_every_bit_of_its_own():
    status = torch.tensor([_hip.STATUS_LOSS_INDEX | _hip.STATUS_ANALYTICAL_SIGMA], dtype=torch.int32)
    with pytest.raises(IndexError):
        kernels.raise_loss_status(status)
    assert status.tolist() == [0]
