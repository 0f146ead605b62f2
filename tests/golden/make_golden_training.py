"""Generate the training fixture tests/golden/training/gaussian_raw.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_training.py

The reference's data/diffusion/gaussian_data_module.py imports `lightning`, which is not installed here: a stub module whose
LightningDataModule is an empty class stands in for it (a third party's class, nothing of the reference).  The reference's
GaussianDataModuleParameters, GaussianDataModule.__init__, get_raw_dataset and setup then run unchanged, on the host.

Per configuration (`main_`: 2 atoms in 3 dimensions, 160 + 64 samples, sigma_d 0.02, seed 1234, the lattice free; `toy_`: the
reference's toy problem, 2 atoms in 1 dimension, 16 + 8 samples, sigma_d 0.01, seed 42, the lattice fixed) the arrays
  train_X [M, N, D], train_A [M, N], train_L [M, D (D + 1) / 2], train_F [M, N, D], train_natom [M], train_energy [M]
  valid_...                                                                       the same of the validation set
are the CLEAN fields of the datasets setup() builds: setup() is run as it is (its transform noises on torch's global generator,
which the raw draws do not use), its datasets' clean fields are stacked, and they are asserted equal to two get_raw_dataset calls on
one generator seeded with random_seed -- training first.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs its stubs, imports the reference, brings the writer)

lightning = types.ModuleType("lightning")
lightning.LightningDataModule = type("LightningDataModule", (), {"__init__": lambda self: None})
sys.modules.setdefault("lightning", lightning)

from diffusion_for_multi_scale_molecular_dynamics.data.diffusion.gaussian_data_module import (  # noqa: E402
    GaussianDataModule, GaussianDataModuleParameters)
from diffusion_for_multi_scale_molecular_dynamics.namespace import (ATOM_TYPES, LATTICE_PARAMETERS,  # noqa: E402
                                                                     RELATIVE_COORDINATES)

DIRECTORY = "training"
FILE = "gaussian_raw.npz"
CONFIGURATIONS = {
    "main": dict(batch_size=64, elements=["Si"], spatial_dimension=3, use_fixed_lattice_parameters=False, use_optimal_transport=False,
                 random_seed=1234, number_of_atoms=2, sigma_d=0.02,
                 equilibrium_relative_coordinates=[[0.25, 0.25, 0.25], [0.75, 0.75, 0.75]], train_dataset_size=160,
                 valid_dataset_size=64),
    "toy": dict(batch_size=8, elements=["Si"], spatial_dimension=1, use_fixed_lattice_parameters=True, use_optimal_transport=False,
                random_seed=42, number_of_atoms=2, sigma_d=0.01, equilibrium_relative_coordinates=[[0.25], [0.75]],
                train_dataset_size=16, valid_dataset_size=8)}
NAMES = {"X": RELATIVE_COORDINATES, "A": ATOM_TYPES, "L": LATTICE_PARAMETERS, "F": mg.CARTESIAN_FORCES, "natom": "natom",
         "energy": "potential_energy"}


def configuration(name):
    noise = mg.NoiseParameters(total_time_steps=20, sigma_min=1e-3, sigma_max=0.4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        parameters = GaussianDataModuleParameters(noise_parameters=noise, **CONFIGURATIONS[name])
    module = GaussianDataModule(parameters)
    torch.manual_seed(7)                    # the transform's own draws: not recorded, not part of the raw datasets
    module.setup()
    rng = torch.Generator()
    rng.manual_seed(parameters.random_seed)
    arrays = {}
    for split, dataset, size in (("train", module.train_dataset, parameters.train_dataset_size),
                                 ("valid", module.valid_dataset, parameters.valid_dataset_size)):
        raw = module.get_raw_dataset(size, rng)
        assert len(dataset) == size
        for short, key in NAMES.items():
            stacked = torch.stack([sample[key] for sample in dataset])
            assert torch.equal(stacked, raw[key]), (name, split, key)
            arrays[f"{name}_{split}_{short}"] = mg._np(stacked)
    return arrays


def golden_training():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    arrays = {}
    for name in CONFIGURATIONS:
        arrays.update(configuration(name))
    mg.save(os.path.join(DIRECTORY, FILE), **arrays)


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_training()
