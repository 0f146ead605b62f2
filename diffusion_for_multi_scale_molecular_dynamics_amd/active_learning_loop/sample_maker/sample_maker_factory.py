"""From a configuration dictionary to a sample maker (src/.../active_learning_loop/sample_maker/sample_maker_factory.py:28-129)."""
from typing import Any, AnyStr, Dict, Optional

from ...generators.axl_generator import SamplingParameters
from ...models.score_networks.score_network import ScoreNetwork
from ...noise_schedulers.noise_parameters import NoiseParameters
from ..atom_selector.atom_selector_factory import create_atom_selector
from ..atom_selector.base_atom_selector import BaseAtomSelectorParameters
from ..excisor.base_excisor import BaseEnvironmentExcisionArguments
from ..excisor.excisor_factory import create_excisor
from .base_sample_maker import BaseSampleMaker, BaseSampleMakerArguments
from .excise_and_noop_sample_maker import ExciseAndNoOpSampleMaker, ExciseAndNoOpSampleMakerArguments
from .excise_and_random_sample_maker import ExciseAndRandomSampleMaker, ExciseAndRandomSampleMakerArguments
from .excise_and_repaint_sample_maker import ExciseAndRepaintSampleMaker, ExciseAndRepaintSampleMakerArguments
from .no_op_sample_maker import NoOpSampleMaker, NoOpSampleMakerArguments

SAMPLE_MAKER_PARAMETERS_BY_NAME = dict(noop=NoOpSampleMakerArguments, excise_and_noop=ExciseAndNoOpSampleMakerArguments,
                                       excise_and_repaint=ExciseAndRepaintSampleMakerArguments,
                                       excise_and_random=ExciseAndRandomSampleMakerArguments)
_EXCISING = ("excise_and_repaint", "excise_and_random", "excise_and_noop")


def create_sample_maker_parameters(sample_maker_dictionary: Dict[AnyStr, Any]) -> BaseSampleMakerArguments:
    """The arguments dataclass that the dictionary's `algorithm` names, built from the whole dictionary (:47-57)."""
    algorithm = sample_maker_dictionary["algorithm"]
    assert algorithm in SAMPLE_MAKER_PARAMETERS_BY_NAME.keys(), \
        f"Sample maker method {algorithm} is not implemented. Possible choices are {SAMPLE_MAKER_PARAMETERS_BY_NAME.keys()}"
    return SAMPLE_MAKER_PARAMETERS_BY_NAME[algorithm](**sample_maker_dictionary)


def create_sample_maker(sample_maker_parameters: BaseSampleMakerArguments, atom_selector_parameters: BaseAtomSelectorParameters,
                        excisor_parameters: Optional[BaseEnvironmentExcisionArguments] = None,
                        noise_parameters: Optional[NoiseParameters] = None,
                        sampling_parameters: Optional[SamplingParameters] = None,
                        diffusion_model: Optional[ScoreNetwork] = None, device: Optional[str] = "cpu") -> BaseSampleMaker:
    """The sample maker of `sample_maker_parameters.algorithm` with its atom selector and, for the excising makers, its
    excisor (:73-129).  "noop" goes with no excisor or the noop one; "excise_and_*" needs a real one."""
    algorithm = sample_maker_parameters.algorithm
    assert algorithm in SAMPLE_MAKER_PARAMETERS_BY_NAME.keys(), \
        f"Sample maker method {algorithm} is not implemented. Possible choices are {SAMPLE_MAKER_PARAMETERS_BY_NAME.keys()}"
    atom_selector = create_atom_selector(atom_selector_parameters)
    excisor = None if excisor_parameters is None else create_excisor(excisor_parameters)
    if algorithm == "noop":
        assert excisor is None or excisor_parameters.algorithm == "noop", \
            ("It is nonsensical to specify an excisor different from 'noop' when the sample maker is 'noop'. "
             "Review input for consistency.")
        return NoOpSampleMaker(sample_maker_parameters, atom_selector=atom_selector)
    if algorithm not in _EXCISING:
        raise NotImplementedError(f"Algorithm {algorithm} is not implemented.")
    assert excisor is not None and excisor_parameters.algorithm != "noop", \
        ("It is nonsensical to specify a NoOp excisor when the sample maker is 'excise_and_*'. "
         "Review input for consistency.")
    if algorithm == "excise_and_repaint":
        return ExciseAndRepaintSampleMaker(sample_maker_arguments=sample_maker_parameters, atom_selector=atom_selector,
                                           environment_excisor=excisor, noise_parameters=noise_parameters,
                                           sampling_parameters=sampling_parameters, diffusion_model=diffusion_model,
                                           device=device)
    maker = ExciseAndRandomSampleMaker if algorithm == "excise_and_random" else ExciseAndNoOpSampleMaker
    return maker(sample_maker_arguments=sample_maker_parameters, atom_selector=atom_selector, environment_excisor=excisor)
