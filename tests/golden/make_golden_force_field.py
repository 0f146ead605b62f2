"""Generate the force-field fixtures ff_c3.npz, ff_images.npz and ff_clipped.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_force_field.py

The reference's own ForceFieldAugmentedScoreNetwork (models/score_networks/force_field_augmented_score_network.py:44-236,
with utils/neighbors.py:36-224) around the echo network of make_golden.py: `forces` is what get_relative_coordinates_pseudo_force
returned, `out_X` what forward() returned (the input X plus the forces).  The stubs for the packages the reference imports
but this image lacks, the echo network and the writer are make_golden.py's, imported from it unchanged.

  ff_c3       B 8, N 64: Si 2x2x2 diamond sites with noise, cells 10.86 x (1, 1.1, 1.2), rc 2.5, s 5.0 (the C3 shape's cell)
  ff_images   B 4, N 8, cell 4.0 x (1, 1.1, 1.2), rc 2.5: rc > L_min / 2.2, so the 27-image sweep; pairs have two images within
              the cutoff, and structure 0 holds a pair at exactly d = rc (relative dx = 0.625 along the 4.0 axis: 2.5 exactly,
              d^2 = 6.25 = rc^2 -- an edge by <=, contributing zero)
  ff_clipped  B 4, N 8, lattice lengths below 1.0 (clipped to min_box_size 1.0), rc 0.9; structure 0 holds two coincident
              atoms (0 < d^2: no edge, no contribution)
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

from diffusion_for_multi_scale_molecular_dynamics.models.score_networks.force_field_augmented_score_network import (  # noqa: E402
    ForceFieldAugmentedScoreNetwork, ForceFieldParameters)


def _fixture(name, X, L, rc, strength):
    B, N, _ = X.shape
    base = mg.FakeAXLNetwork(mg.ScoreNetworkParameters(architecture="dummy", spatial_dimension=3, num_atom_types=1))
    ff = ForceFieldAugmentedScoreNetwork(base, ForceFieldParameters(radial_cutoff=rc, strength=strength))
    batch = {mg.NOISY_AXL_COMPOSITION: mg.AXL(A=torch.zeros(B, N, dtype=torch.long), X=X, L=L),
             mg.TIME: torch.zeros(B, 1), mg.NOISE: torch.zeros(B, 1), mg.CARTESIAN_FORCES: torch.zeros(B, N, 3)}
    forces = ff.get_relative_coordinates_pseudo_force(batch)
    out = ff(batch, conditional=False)
    mg.save(name + ".npz", X=mg._np(X), L=mg._np(L), rc=np.array(rc), strength=np.array(strength), forces=mg._np(forces),
            out_X=mg._np(out.X))


def _cells(B, length, scale=(1.0, 1.1, 1.2)):
    return torch.tensor([length * scale[0], length * scale[1], length * scale[2], 0, 0, 0.0]).repeat(B, 1)


def golden_force_field():
    g = torch.Generator().manual_seed(2606)
    # C3 shape: diamond sites with noise
    B = 8
    sites = mg._diamond_sites(2)
    X = torch.remainder(sites[None] + 0.02 * torch.randn(B, 64, 3, generator=g), 1.0)
    _fixture("ff_c3", X, _cells(B, 10.86), 2.5, 5.0)
    # 27-image path, two images within the cutoff, a pair at exactly d = rc
    B = 4
    X = torch.rand(B, 8, 3, generator=g)
    X[0, 0] = torch.tensor([0.125, 0.25, 0.5])
    X[0, 1] = torch.tensor([0.75, 0.25, 0.5])           # dx = 0.625 x 4.0 = 2.5 exactly (and 1.5 through the other image)
    X[1, 0] = torch.tensor([0.25, 0.5, 0.5])
    X[1, 1] = torch.tensor([0.75, 0.5, 0.5])            # dx = 0.5 x 4.0 = 2.0 through both images along x
    _fixture("ff_images", X, _cells(B, 4.0), 2.5, 5.0)
    # lattice lengths below min_box_size, two coincident atoms
    X = torch.rand(B, 8, 3, generator=g)
    X[0, 1] = X[0, 0]
    L = torch.cat([0.5 + 0.45 * torch.rand(B, 3, generator=g), torch.zeros(B, 3)], dim=1)
    _fixture("ff_clipped", X, L, 0.9, 2.0)


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_force_field()
