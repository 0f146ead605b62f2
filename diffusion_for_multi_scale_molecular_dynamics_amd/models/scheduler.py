"""The reference's models/scheduler.py: the `scheduler:` block of a training configuration and torch's two schedulers.

torch's CosineAnnealingLR and ReduceLROnPlateau are used as they are: they write `param_groups[i]["lr"]`, which
models/optimizer.py::FusedAdam.step() compares with what it last wrote to its device buffer."""
from dataclasses import asdict, dataclass
from typing import Any, AnyStr, Dict, Union

from torch import optim

from ..utils.configuration_parsing import create_parameters_from_configuration_dictionary


@dataclass(kw_only=True)
class SchedulerParameters:
    """Base data class for scheduler parameters."""

    name: str


@dataclass(kw_only=True)
class ReduceLROnPlateauSchedulerParameters(SchedulerParameters):
    """Parameters for the reduce LR on plateau scheduler."""

    name: str = "ReduceLROnPlateau"
    factor: float = 0.1
    patience: int = 10
    # what the scheduler monitors: not a parameter of the scheduler itself, but needed when optimizers and schedulers are configured
    monitor: str = "validation_epoch_loss"


@dataclass(kw_only=True)
class CosineAnnealingLRSchedulerParameters(SchedulerParameters):
    """Parameters for the cosine annealing scheduler."""

    name: str = "CosineAnnealingLR"
    T_max: int
    eta_min: float = 0.0


SCHEDULER_PARAMETERS_BY_NAME = dict(CosineAnnealingLR=CosineAnnealingLRSchedulerParameters,
                                    ReduceLROnPlateau=ReduceLROnPlateauSchedulerParameters)

SCHEDULERS_BY_NAME = dict(CosineAnnealingLR=optim.lr_scheduler.CosineAnnealingLR,
                          ReduceLROnPlateau=optim.lr_scheduler.ReduceLROnPlateau)


def create_scheduler_parameters(hyper_params: Dict[str, Any]) -> Union[SchedulerParameters, None]:
    """The parameters of the `scheduler` block of a configuration dictionary, None without one  (:49-72)."""
    if "scheduler" not in hyper_params:
        return None
    return create_parameters_from_configuration_dictionary(configuration=dict(hyper_params["scheduler"]), identifier="name",
                                                           options=SCHEDULER_PARAMETERS_BY_NAME)


def load_scheduler_dictionary(scheduler_parameters: SchedulerParameters, optimizer: optim.Optimizer) -> Dict[AnyStr, Any]:
    """dict(lr_scheduler=the scheduler on `optimizer`, [monitor=what it watches])  (:75-106)."""
    name = scheduler_parameters.name
    assert name in SCHEDULERS_BY_NAME.keys(), \
        f"Scheduler '{name}' is not implemented. Possible choices are {SCHEDULERS_BY_NAME.keys()}"
    scheduler_dict = dict()
    scheduler_parameters_dict = asdict(scheduler_parameters)
    scheduler_parameters_dict.pop("name")
    if "monitor" in scheduler_parameters_dict:
        scheduler_dict["monitor"] = scheduler_parameters_dict.pop("monitor")
    scheduler_dict["lr_scheduler"] = SCHEDULERS_BY_NAME[name](optimizer, **scheduler_parameters_dict)
    return scheduler_dict
