"""Excisors by name (src/.../active_learning_loop/excisor/excisor_factory.py:12-59)."""
from typing import Any, AnyStr, Dict

from .base_excisor import BaseEnvironmentExcision, BaseEnvironmentExcisionArguments
from .nearest_neighbors_excisor import NearestNeighborsExcision, NearestNeighborsExcisionArguments
from .no_op_excisor import NoOpExcision, NoOpExcisionArguments
from .spherical_excisor import SphericalExcision, SphericalExcisionArguments

EXCISOR_PARAMETERS_BY_NAME = dict(noop=NoOpExcisionArguments, nearest_neighbors=NearestNeighborsExcisionArguments,
                                  spherical_cutoff=SphericalExcisionArguments)
EXCISOR_BY_NAME = dict(noop=NoOpExcision, nearest_neighbors=NearestNeighborsExcision, spherical_cutoff=SphericalExcision)


def create_excisor_parameters(excisor_dictionary: Dict[AnyStr, Any]) -> BaseEnvironmentExcisionArguments:
    algorithm = excisor_dictionary["algorithm"]
    assert algorithm in EXCISOR_PARAMETERS_BY_NAME.keys(), \
        f"Excision method {algorithm} is not implemented. Possible choices are {EXCISOR_PARAMETERS_BY_NAME.keys()}"
    return EXCISOR_PARAMETERS_BY_NAME[algorithm](**excisor_dictionary)


def create_excisor(excisor_parameters: BaseEnvironmentExcisionArguments) -> BaseEnvironmentExcision:
    algorithm = excisor_parameters.algorithm
    assert algorithm in EXCISOR_BY_NAME.keys(), \
        f"Excision method {algorithm} is not implemented. Possible choices are {EXCISOR_BY_NAME.keys()}"
    return EXCISOR_BY_NAME[algorithm](excisor_parameters)
