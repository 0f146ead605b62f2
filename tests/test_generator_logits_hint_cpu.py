"""When LangevinGenerator tells its network that a step's atom-type logits are unread (LangevinGenerator._logits_unread, the
condition around network_hooks.logits_unread): a step that leaves the types alone, or any step with ONE atom type -- and only
when the caller drops the predictions and nothing records, overrides or hooks the forward."""
import warnings

import pytest
import torch

import cases
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.langevin_generator import LangevinGenerator
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
    PredictorCorrectorSamplingParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.inner = torch.nn.Linear(2, 2)
        self.sigma_uniform_hint = self.logits_unread_hint = False


def _generator(num_atom_types, net=None, cls=LangevinGenerator, **record):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        npar = NoiseParameters(**cases.noise_ns(4))
        spar = PredictorCorrectorSamplingParameters(**cases.sampling_ns(8, num_atom_types, M=2, greedy=False, one=False),
                                                    rng_mode="device", seed=1, **record)
    return cls(npar, spar, net if net is not None else _Net())


def test_one_atom_type_hints_in_predictor_and_corrector():
    gen = _generator(1)
    assert gen._logits_unread(update_types=True, predictions_unread=True)          # the predictor
    assert gen._logits_unread(update_types=False, predictions_unread=True)         # a corrector
    assert not gen._logits_unread(update_types=True, predictions_unread=False)     # (a caller that reads the predictions)
    assert not gen._logits_unread(update_types=False, predictions_unread=False)


@pytest.mark.parametrize("num_atom_types", [2, 4])
def test_more_atom_types_hint_only_where_the_types_stay(num_atom_types):
    gen = _generator(num_atom_types)
    assert not gen._logits_unread(update_types=True, predictions_unread=True)
    assert gen._logits_unread(update_types=False, predictions_unread=True)


class _OwnPredictions(LangevinGenerator):
    def _get_model_predictions(self, *args, **kwargs):
        return super()._get_model_predictions(*args, **kwargs)


@pytest.mark.parametrize("update_types", [True, False])
def test_any_watcher_keeps_the_forward_whole(update_types):
    ask = dict(update_types=update_types, predictions_unread=True)
    assert _generator(1)._logits_unread(**ask)
    assert not _generator(1, record_samples=True)._logits_unread(**ask)
    assert not _generator(1, record_samples=True, record_atom_type_update=True)._logits_unread(**ask)
    assert not _generator(1, cls=_OwnPredictions)._logits_unread(**ask)
    gen = _generator(1)
    gen._get_model_predictions = lambda *a, **k: None                              # a replacement on the instance
    assert not gen._logits_unread(**ask)
    for target in ("net", "inner"):
        net = _Net()
        handle = (net if target == "net" else net.inner).register_forward_hook(lambda module, args, out: None)
        gen = _generator(1, net=net)
        assert not gen._logits_unread(**ask)
        handle.remove()
        assert gen._logits_unread(**ask)                                           # (looked up at every step, never cached)
