"""The `metrics:` block of a configuration (src/.../metrics/sampling_metrics_parameters.py:4-19)."""
from dataclasses import dataclass


@dataclass(kw_only=True)
class SamplingMetricsParameters:
    """What metrics should be computed given that samples have been generated."""

    compute_energies: bool = False  # should the energies be computed
    compute_structure_factor: bool = False  # should the structure factor (distances distribution) be recorded
    structure_factor_max_distance: float = 10.0  # cutoff for the structure factor
    record_lattice_parameters: bool = False  # should the lattice parameters distributions be recorded
