"""Generate the regression-regularizer fixtures tests/golden/regression/* by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_regression.py

The reference's AnalyticalScoreNetwork and EquivariantAnalyticalScoreNetwork (models/score_networks/) are the target networks.
Its regularizers/regression_regularizer.py itself CANNOT be imported here: it reaches `mace` through the score-network factory,
and make_golden.py's stubs (imported from it unchanged, with the writer) do not cover that.  The whole-call cases therefore run
the reference's ten-line flow (regression_regularizer.py:47-68) in this script, on the reference's own network classes.

OPERAND cases hold to the fused kernel: recorded binary32 operands, and the reference's AnalyticalScoreNetwork evaluated in
binary64 on float64 copies of them (get_probabilities_and_normalized_scores of the module after .double(), as
make_golden_analytical.py does), then the loss expression in binary64, with M = B N D.  Arrays of a case:
  x f32 [B, N, D], sigma f32 [B], sites f32 [N, D], sigma_d, kmax, permutations; s f32 [B, N, D]
  target64 [B, N, D]; gradient64 = 2 (s - t) / M; per_structure64 [B] = sum over the structure of (s - t)^2; loss64 = sum / M
    n1_d1 (B 1)            one element
    n5_d3 (B 3)            15 elements: a partial wavefront; one sigma per structure (0.05, 0.2, 0.45)
    n65_d2 (B 2)           130 elements: more than two wavefronts
    n216_d3 (B 2)          648 elements: more than one pass of the 256-thread workgroup
    ewald (B 3, N 5, D 3)  sigma 0.5: sigma_eff above 1 / sqrt(2 pi), the Ewald form
    placed (B 3, N 5, D 3) structure 0 holds x - site = 0 (atom 0), 1/2 exactly (atom 1) and 1 - 2^-24 (atom 2)
    toy_perm2_d1 (B 4)     the reference's own regression configuration (analysis_and_sanity_checks/toy_problems/training/
                           analytical_regression_regularizer/specific_config.yaml, copied beside the cases as
                           toy_regression_regularizer.yaml: settings only): N 2, D 1, kmax 5, sigma_d 0.01, permutations on
    perm3_d2 (B 3)         6 permutations, kmax 1
    perm8_d3 (B 2)         40 320 permutations, the kernel's cap
    given_n5_d3 (B 3), given_n700_d3 (B 2)    given-target mode: `target` f32 [B, N, D] stands for x, sigma and the sites;
                           target64 is its promotion.  2 100 elements: beyond one pass
Even structures are uniform in the cell, odd ones the sites plus noise of width sigma_d.  Scores are drawn around the target so
that |s - t| is of the order of |t|; every per_structure64 is asserted positive and finite; the sums are of squares, so no
reduced value is a cancellation.

WHOLE-CALL cases (`analytical`, `analytical_perm`, `equivariant`): B 4, N 4, D 3, a small MLP as the regularized network,
regularizer_lambda_weight 2.5.  Under torch.manual_seed(seed): X = torch.rand(B, N, D); the modified batch; the target
network's .X; the MLP's .X (both forwards with conditional=None, one torch.rand(1) each); loss = mean(errors ** 2).  Arrays:
  batch_A, batch_X, batch_L, batch_time, batch_noise     the augmented batch (forces are zeros)
  net/<key>                                              the MLP's state_dict
  sites [N, D], sigma_d, kmax, permutations              the target network
  drawn_X, s, target f32 [B, N, D]; loss, weighted_loss f32; weight, seed
  target64 [B, N, D]                                     the target network after .double() on float64 copies of drawn_X, noise
  next_rand f32 [1]                                      torch.rand(1) drawn after the call: the CPU generator's state
"""
import os
import shutil
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)
import make_golden_transport as mt  # noqa: E402  (the equivariant network in binary64: its Transporter64)

import diffusion_for_multi_scale_molecular_dynamics as reference_package  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.models.score_networks.analytical_score_network import (  # noqa: E402
    AnalyticalScoreNetwork, AnalyticalScoreNetworkParameters)

DIRECTORY = "regression"
YAML = "toy_regression_regularizer.yaml"
YAML_SOURCE = ("analysis_and_sanity_checks", "toy_problems", "training", "analytical_regression_regularizer", "specific_config.yaml")
ANALYTICAL_CASES = {      # name -> (B, N, D), seed, sigma per structure, kmax, sigma_d, permutations
    "n1_d1": ((1, 1, 1), 1711, (0.1,), 4, 0.05, False),
    "n5_d3": ((3, 5, 3), 1721, (0.05, 0.2, 0.45), 4, 0.05, False),
    "n65_d2": ((2, 65, 2), 1731, (0.2, 0.2), 4, 0.05, False),
    "n216_d3": ((2, 216, 3), 1741, (0.05, 0.05), 2, 0.05, False),
    "ewald": ((3, 5, 3), 1751, (0.5, 0.5, 0.5), 4, 0.05, False),
    "placed": ((3, 5, 3), 1761, (0.1, 0.1, 0.1), 4, 0.05, False),
    "toy_perm2_d1": ((4, 2, 1), 1771, (0.01, 0.05, 0.2, 0.5), 5, 0.01, True),
    "perm3_d2": ((3, 3, 2), 1781, (0.05, 0.2, 0.45), 1, 0.03, True),
    "perm8_d3": ((2, 8, 3), 1791, (0.2, 0.1), 2, 0.05, True)}
GIVEN_CASES = {"given_n5_d3": ((3, 5, 3), 1801), "given_n700_d3": ((2, 700, 3), 1811)}
WHOLE_CALL_CASES = {"analytical": 1821, "analytical_perm": 1822, "equivariant": 1823}
FILES = [name + ".npz" for name in list(ANALYTICAL_CASES) + list(GIVEN_CASES) + list(WHOLE_CALL_CASES)] + [YAML]
B, N, D, WEIGHT = 4, 4, 3, 2.5
CELL = [5.43] * D


def _analytical(dimension, atoms, kmax, sigma_d, permutations, sites):
    return AnalyticalScoreNetwork(AnalyticalScoreNetworkParameters(
        spatial_dimension=dimension, number_of_atoms=atoms, num_atom_types=1, kmax=kmax, sigma_d=sigma_d,
        equilibrium_relative_coordinates=sites.tolist(), use_permutation_invariance=permutations))


def _sites(name, atoms, dimension, g):
    if name == "toy_perm2_d1":
        return torch.tensor([[0.25], [0.75]])
    if name == "placed":
        sites = torch.randint(0, 8, (atoms, dimension), generator=g) / 8.0
        sites[2] = 0.0
        return sites
    return torch.rand(atoms, dimension, generator=g)


def _coordinates(name, sites, sigma_d, batch, g):
    atoms, dimension = sites.shape
    x = torch.rand(batch, atoms, dimension, generator=g)
    for b in range(1, batch, 2):
        x[b] = torch.remainder(sites + sigma_d * torch.randn(atoms, dimension, generator=g), 1.0)
    x[x >= 1.0] = 0.0
    if name == "placed":
        x[0, 0] = sites[0]                                                                   # 0
        x[0, 1] = torch.where(sites[1] < 0.5, sites[1] + 0.5, sites[1] - 0.5)                # 1/2, exactly
        x[0, 2] = 1.0 - 2.0**-24                                                             # the largest binary32 below 1
    return x


def _score_around(target64, g):
    """A binary32 score with |s - t| of the order of |t| (and of 0.05 where t is 0)."""
    return (target64 * (1.0 + 0.5 * torch.randn(target64.shape, generator=g, dtype=torch.float64))).float() + \
        0.05 * torch.randn(target64.shape, generator=g)


def _loss64(s, target64):
    errors = s.double() - target64
    elements = errors.numel()
    out = dict(target64=target64, gradient64=2.0 * errors / elements, per_structure64=(errors**2).sum(dim=(1, 2)),
               loss64=(errors**2).sum() / elements)
    assert all(bool(torch.isfinite(v).all()) for v in out.values()) and bool((out["per_structure64"] > 0.0).all())
    return out


def analytical_case(name):
    (batch, atoms, dimension), seed, sigmas, kmax, sigma_d, permutations = ANALYTICAL_CASES[name]
    g = torch.Generator().manual_seed(seed)
    sites = _sites(name, atoms, dimension, g)
    x = _coordinates(name, sites, sigma_d, batch, g)
    sigma = torch.tensor(sigmas, dtype=torch.float32)
    net64 = _analytical(dimension, atoms, kmax, sigma_d, permutations, sites).double()
    full = sigma.double().view(batch, 1, 1).expand(batch, atoms, dimension).contiguous()
    with torch.no_grad(), np.errstate(all="ignore"):
        _, target64 = net64.get_probabilities_and_normalized_scores(x.double(), full)
    assert target64.dtype == torch.float64 and target64.shape == x.shape
    s = _score_around(target64, g)
    arrays = dict(x=mg._np(x), sigma=mg._np(sigma), sites=mg._np(sites), sigma_d=np.array(sigma_d), kmax=np.array(kmax),
                  permutations=np.array(permutations), s=mg._np(s), seed=np.array(seed))
    arrays.update({key: mg._np(value) for key, value in _loss64(s, target64).items()})
    if name == "placed":
        difference = x[0].double() - sites.double()
        assert bool((difference[0] == 0.0).all()) and bool((difference[1].abs() == 0.5).all())
        assert bool((difference[2] == 1.0 - 2.0**-24).all())
    return arrays


def given_case(name):
    shape, seed = GIVEN_CASES[name]
    g = torch.Generator().manual_seed(seed)
    target = torch.randn(*shape, generator=g)
    s = _score_around(target.double(), g)
    arrays = dict(target=mg._np(target), s=mg._np(s), seed=np.array(seed))
    arrays.update({key: mg._np(value) for key, value in _loss64(s, target.double()).items()})
    return arrays


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    composition = mg.AXL(A=torch.zeros(B, N, dtype=torch.int64), X=torch.rand(B, N, D, generator=g),
                         L=torch.tensor(CELL + [0.0] * (D * (D - 1) // 2)).repeat(B, 1))
    return {mg.NOISY_AXL_COMPOSITION: composition, mg.TIME: torch.tensor([[0.1], [0.4], [0.7], [1.0]]),
            mg.NOISE: torch.tensor([[0.02], [0.1], [0.3], [0.5]]), mg.CARTESIAN_FORCES: torch.zeros(B, N, D)}


def whole_call_case(name):
    seed = WHOLE_CALL_CASES[name]
    net = mg._mlp(N, 1, seed=seed, hidden=32)
    sites = torch.rand(N, D, generator=torch.Generator().manual_seed(seed + 10))
    kmax, sigma_d, permutations = 4, 0.05, name == "analytical_perm"
    if name == "equivariant":      # (the reference's EquivariantAnalyticalScoreNetwork as built, and after .double())
        target_score_network, net64 = mt._networks(D, N, kmax, sigma_d, True, sites)
    else:
        target_score_network = _analytical(D, N, kmax, sigma_d, permutations, sites)
        net64 = _analytical(D, N, kmax, sigma_d, permutations, sites).double()
    augmented_batch = _batch(seed + 1)

    # the reference's flow (regularizers/regression_regularizer.py:47-68)
    torch.manual_seed(seed + 2)
    with torch.no_grad():
        original_noisy_composition = augmented_batch[mg.NOISY_AXL_COMPOSITION]
        relative_coordinates = torch.rand(*original_noisy_composition.X.shape)
        modified_batch = dict(augmented_batch)
        modified_batch[mg.NOISY_AXL_COMPOSITION] = mg.AXL(A=original_noisy_composition.A, X=relative_coordinates,
                                                          L=original_noisy_composition.L)
        target = target_score_network(modified_batch).X
        s = net(modified_batch).X
        loss = torch.mean((s - target)**2)
    next_rand = torch.rand(1)
    weighted = WEIGHT * loss

    full = augmented_batch[mg.NOISE].double().view(B, 1, 1).expand(B, N, D).contiguous()
    with torch.no_grad(), np.errstate(all="ignore"):
        if name == "equivariant":
            target64 = net64.get_normalized_scores(relative_coordinates.double(), full)
        else:
            _, target64 = net64.get_probabilities_and_normalized_scores(relative_coordinates.double(), full)
    assert target64.dtype == torch.float64 and bool(torch.isfinite(loss)) and float(loss) > 0.0
    assert float(torch.linalg.norm(target.double() - target64) / torch.linalg.norm(target64)) < 1e-4
    composition = augmented_batch[mg.NOISY_AXL_COMPOSITION]
    return dict(batch_A=mg._np(composition.A), batch_X=mg._np(composition.X), batch_L=mg._np(composition.L),
                batch_time=mg._np(augmented_batch[mg.TIME]), batch_noise=mg._np(augmented_batch[mg.NOISE]),
                sites=mg._np(sites), sigma_d=np.array(sigma_d), kmax=np.array(kmax), permutations=np.array(permutations),
                drawn_X=mg._np(relative_coordinates), s=mg._np(s), target=mg._np(target), target64=mg._np(target64),
                loss=mg._np(loss), weighted_loss=mg._np(weighted), weight=np.array(WEIGHT), seed=np.array(seed + 2),
                next_rand=mg._np(next_rand), **mg._state_dict_np(net))


def golden_regression():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    for name in ANALYTICAL_CASES:
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **analytical_case(name))
    for name in GIVEN_CASES:
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **given_case(name))
    for name in WHOLE_CALL_CASES:
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **whole_call_case(name))
    # the reference's own `regularizer:` block: a file that holds only settings
    checkout = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(reference_package.__file__))))
    shutil.copyfile(os.path.join(checkout, *YAML_SOURCE), os.path.join(mg.OUT, DIRECTORY, YAML))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_regression()
