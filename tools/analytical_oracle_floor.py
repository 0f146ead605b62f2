"""The CPU oracle's own rounding distance on the analytical sampling job (no GPU involved).

    python tools/analytical_oracle_floor.py

oracle.reference_sampler.OracleLangevinGenerator with Philox draws around the torch restatement of the analytical network
(tests/nets.py::GaussianWellScoreNetwork: diamond sites of Si 1x1x1, sigma_d 0.05, kmax 4), B 16, M 1, sigma 1e-4 .. 0.25, run
twice with the same draws: the network evaluated in binary32, and in binary64 behind a binary32 interface.  Prints, per T, the
rel-L2 distance of the final coordinates on the torus -- what no binary32 sampler can be held below at that T, and the source
of the T 20 bar of tests/test_analytical_score_gpu.py::test_sampler_runs_the_network_in_the_captured_loop."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nets  # noqa: E402
from conftest import torus_rel_l2  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import (  # noqa: E402
    PredictorCorrectorSamplingParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, NOISE, NOISY_AXL_COMPOSITION  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters  # noqa: E402
from oracle.reference_sampler import OracleLangevinGenerator, PhiloxNoise  # noqa: E402

SEED = 20250815


class InBinary64(torch.nn.Module):
    """A score network evaluated in binary64 behind a binary32 interface."""

    def __init__(self, net):
        super().__init__()
        self.net = net.double()

    def forward(self, batch, conditional=None):
        batch = dict(batch)
        comp = batch[NOISY_AXL_COMPOSITION]
        batch[NOISY_AXL_COMPOSITION] = AXL(A=comp.A, X=comp.X.double(), L=comp.L.double())
        batch[NOISE] = batch[NOISE].double()
        out = self.net(batch, conditional)
        return AXL(A=out.A.float(), X=out.X.float(), L=out.L.float())


def main():
    sites = np.load(os.path.join(ROOT, "tests", "golden", "analytical", "diamond.npz"))["sites"]
    for T in (20, 50, 200):
        noise = NoiseParameters(total_time_steps=T, sigma_min=1e-4, sigma_max=0.25)
        sampling = PredictorCorrectorSamplingParameters(
            number_of_atoms=8, num_atom_types=1, number_of_samples=16, number_of_corrector_steps=1,
            use_fixed_lattice_parameters=True, cell_dimensions=[5.43, 5.43, 5.43], rng_mode="device", seed=SEED)
        runs = [OracleLangevinGenerator(noise, sampling, net, noise=PhiloxNoise(SEED, 0)).sample(16)
                for net in (nets.GaussianWellScoreNetwork(sites, 0.05, 4), InBinary64(nets.GaussianWellScoreNetwork(sites, 0.05, 4)))]
        print(json.dumps(dict(total_time_steps=T, binary32_vs_binary64_torus_rel_l2=torus_rel_l2(runs[0].X, runs[1].X))), flush=True)


if __name__ == "__main__":
    main()
