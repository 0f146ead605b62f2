"""Hyper-parameters of the denoising loss, one object per modality in an AXL (src/.../loss/loss_parameters.py:9-86)."""
from dataclasses import dataclass
from typing import Any, Dict

from ..namespace import AXL


@dataclass(kw_only=True)
class LossParameters:
    """Hyper-parameters for the loss function for a single modality (A, X xor L)."""

    lambda_weight: float = 1.0
    algorithm: str


@dataclass(kw_only=True)
class MSELossParameters(LossParameters):
    algorithm: str = "mse"


@dataclass(kw_only=True)
class WeightedMSELossParameters(LossParameters):
    """weights(sigma) = exp(exponent (sigma - sigma0)) + 1; the defaults give weights(0.5) ~ 10^3."""

    algorithm: str = "weighted_mse"
    sigma0: float = 0.2
    exponent: float = 23.0259  # ~ 10 ln(10)


@dataclass(kw_only=True)
class AtomTypeLossParameters(LossParameters):
    algorithm: str = "d3pm"
    ce_weight: float = 0.001
    eps: float = 1e-8  # avoid divisions by zero


def _parameters_from_dictionary(configuration: Dict[str, Any], identifier: str, options: Dict[str, type]):
    """options[configuration[identifier]](**configuration), with the reference's two assertions
    (utils/configuration_parsing.py:24-35)."""
    assert identifier in configuration.keys(), \
        f"The identifier field '{identifier}' is missing from the configuration dictionary."
    option_id = configuration[identifier]
    assert option_id in options.keys(), f"The option field '{option_id}' is missing from the options dictionary."
    return options[option_id](**configuration)


def create_loss_parameters(model_dictionary: Dict[str, Any]) -> AXL:
    """The `loss:` block of a model configuration as an AXL of parameter objects; a missing block or modality gets mse
    (d3pm for the atom types)  (:45-79)."""
    default_mse_dict = dict(algorithm="mse")
    default_d3pm_dict = dict(algorithm="d3pm")
    default_axl_dict = dict(coordinates=default_mse_dict, atom_types=default_d3pm_dict, lattice_parameters=default_mse_dict)
    loss_config_dictionary = model_dictionary.get("loss", default_axl_dict)
    loss_parameters = {}
    for var in ["coordinates", "atom_types", "lattice_parameters"]:
        default_params = default_d3pm_dict if var == "atom_types" else default_mse_dict
        loss_parameters[var] = _parameters_from_dictionary(configuration=loss_config_dictionary.get(var, default_params),
                                                           identifier="algorithm", options=LOSS_PARAMETERS_BY_ALGO)
    return AXL(A=loss_parameters["atom_types"], X=loss_parameters["coordinates"], L=loss_parameters["lattice_parameters"])


LOSS_PARAMETERS_BY_ALGO = dict(mse=MSELossParameters, weighted_mse=WeightedMSELossParameters, d3pm=AtomTypeLossParameters)
