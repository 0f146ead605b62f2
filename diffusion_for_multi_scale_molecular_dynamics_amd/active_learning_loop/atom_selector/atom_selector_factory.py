"""Atom selectors by name (src/.../active_learning_loop/atom_selector/atom_selector_factory.py:10-57)."""
from typing import Any, AnyStr, Dict

from .base_atom_selector import BaseAtomSelector, BaseAtomSelectorParameters
from .threshold_atom_selector import ThresholdAtomSelector, ThresholdAtomSelectorParameters
from .top_k_atom_selector import TopKAtomSelector, TopKAtomSelectorParameters

ATOM_SELECTOR_PARAMETERS_BY_NAME = dict(threshold=ThresholdAtomSelectorParameters, top_k=TopKAtomSelectorParameters)
ATOM_SELECTOR_BY_NAME = dict(threshold=ThresholdAtomSelector, top_k=TopKAtomSelector)


def create_atom_selector_parameters(atom_selector_parameter_dictionary: Dict[AnyStr, Any]) -> BaseAtomSelectorParameters:
    assert "algorithm" in atom_selector_parameter_dictionary, "The algorithm is missing."
    algorithm = atom_selector_parameter_dictionary["algorithm"]
    assert algorithm in ATOM_SELECTOR_PARAMETERS_BY_NAME.keys(), \
        (f"Atom selector method {algorithm} is not implemented. "
         f"Possible choices are {ATOM_SELECTOR_PARAMETERS_BY_NAME.keys()}")
    return ATOM_SELECTOR_PARAMETERS_BY_NAME[algorithm](**atom_selector_parameter_dictionary)


def create_atom_selector(atom_selector_parameters: BaseAtomSelectorParameters) -> BaseAtomSelector:
    return ATOM_SELECTOR_BY_NAME[atom_selector_parameters.algorithm](atom_selector_parameters)
