"""What the tests of the training epoch share: the time-index draw restated on the oracle's Philox, a schedule made of a
denoising-loss fixture's recorded tables, small random datasets and the Gaussian data module's test configuration."""
import os

import numpy as np
import torch

from conftest import GOLDEN
from denoising_loss_cases import fixture

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels

DIRECTORY = os.path.join(GOLDEN, "training")
GAUSSIAN_FILE = "gaussian_raw.npz"
FILES = [GAUSSIAN_FILE]
INDEX_SEED = 20251021          # the recorded seed of the time-index statistics


def time_index(oracle, seed: int, call: int, draw: int, row: int, total_time_steps: int) -> int:
    """(w T) >> 32 of word 0 of Philox4x32-10 at counter (row, call << 8, draw, MDX_TAG_TRAIN_TIME_INDEX), key = seed: integers only."""
    w = oracle.philox(int(row), (int(call) << 8) & 0xFFFFFFFF, int(draw), _hip.TAG_TRAIN_TIME_INDEX, seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)[0]
    return (int(w) * int(total_time_steps)) >> 32


def fixture_schedule(case: str, device) -> kernels.DeviceSchedule:
    """A DeviceSchedule whose rows are the recorded tables of a denoising-loss fixture (the vectors no kernel of these tests reads
    are zeros)."""
    g = fixture(case)
    t = lambda key: torch.from_numpy(np.ascontiguousarray(g[key])).to(device)       # noqa: E731
    T, C = g["table_q"].shape[:2]
    unused = torch.zeros(T, device=device)
    return kernels.DeviceSchedule(T, C, 1e-3, t("table_time"), t("table_sigma"), unused, unused, unused, unused, unused, unused, unused,
                                  t("table_q"), t("table_q_bar"), t("table_q_bar_tm1"))


def fixture_dataset(case: str, device):
    g = fixture(case)
    return tuple(torch.from_numpy(np.ascontiguousarray(g[key])).to(device) for key in ("x0", "a0", "l0"))


def random_dataset(rows: int, atoms: int, dimension: int, num_classes: int, device, seed: int = 5):
    """x0 in [0, 1), a0 in [0, C - 1), l0 around 5: made on the host generator, moved once."""
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(rows, atoms, dimension, generator=g)
    a0 = torch.randint(0, num_classes - 1, (rows, atoms), generator=g)
    l0 = 5.0 + torch.rand(rows, dimension * (dimension + 1) // 2, generator=g)
    return x0.to(device), a0.to(device), l0.to(device)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(bits(a.contiguous()), bits(b.contiguous())))


def gaussian_parameters(**changes):
    """The Gaussian data module of the epoch tests: 2 atoms in 3 dimensions, 160 training and 64 validation samples, batches of
    64 (so the training epoch has a tail of 32)."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.training import GaussianDataModuleParameters
    values = dict(batch_size=64, elements=["Si"], spatial_dimension=3, use_fixed_lattice_parameters=False,
                  noise_parameters=NoiseParameters(total_time_steps=20, sigma_min=1e-3, sigma_max=0.4), use_optimal_transport=False,
                  random_seed=1234, number_of_atoms=2, sigma_d=0.02,
                  equilibrium_relative_coordinates=[[0.25, 0.25, 0.25], [0.75, 0.75, 0.75]], train_dataset_size=160,
                  valid_dataset_size=64)
    values.update(changes)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # "Using diffusion on lattice parameters": the reference's own warning
        return GaussianDataModuleParameters(**values)
