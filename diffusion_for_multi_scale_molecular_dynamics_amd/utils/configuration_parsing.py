"""The reference's utils/configuration_parsing.py: a parameter dataclass chosen by an identifier field of its configuration."""
from dataclasses import dataclass
from typing import Any, Dict


def create_parameters_from_configuration_dictionary(configuration: Dict[str, Any], identifier: str,
                                                    options: Dict[str, dataclass]) -> dataclass:
    """options[configuration[identifier]](**configuration)  (:5-35); the two assertions carry the reference's messages."""
    assert identifier in configuration.keys(), \
        f"The identifier field '{identifier}' is missing from the configuration dictionary."
    option_id = configuration[identifier]
    assert option_id in options.keys(), f"The option field '{option_id}' is missing from the options dictionary."
    return options[option_id](**configuration)
