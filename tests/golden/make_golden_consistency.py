"""Generate the consistency-regularizer fixtures tests/golden/consistency/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_consistency.py

The reference's ConsistencyRegularizer (regularizers/consistency_regularizer.py:46-308).  The stubs for the packages the
reference imports but this image lacks and the writer are make_golden.py's, imported from it unchanged.

OPERAND cases hold to the fused kernel and to get_score_target: recorded binary32 operands, and the reference evaluated in
binary64 on float64 copies of them -- its own get_score_target (sigmas handed over as float64 tensors, so that its
`torch.tensor(start_sigma**2 - end_sigma**2).sqrt()` stays in binary64), then its loss expression.  Arrays of a case:
  x_start, x_end, s f32 [B, N, D]; sigma_start, sigma_end f32 [1] (or [B]: per_structure_sigma); kmax
  target64 [B, N, D]; per_structure64 [B] = sum over the structure of s (s - 2 t); loss64 = sum / B; gradient64 = 2 (s - t) / B
  magnitude_per_structure64 [B], magnitude64: the sums of |s (s - 2 t)| behind them
    n1_d1 (B 1)           one element: less than a wavefront
    n5_d3 (B 3)           15 elements: a partial wavefront
    n65_d2 (B 2)          130 elements: more than two wavefronts
    n216_d3 (B 2)         648 elements: more than one pass of a 256-thread workgroup
    ewald                 (B 3, N 5, D 3) sigma 0.5 -> 0.2: sigma_eff above 1 / sqrt(2 pi), the Ewald form
    end_zero              (B 3, N 5, D 3) sigma_end = 0, as for end index 0
    placed                (B 3, N 5, D 3) structure 0 holds x_start - x_end = 0, 1/2, -1/2, -1e-20 (wraps to 0) and 1 - 2^-24
    kmax1                 (B 3, N 5, D 3) kmax = 1
    per_structure_sigma   (B 3, N 5, D 3) one sigma_start and sigma_end per structure
Every reduced value r satisfies |r| >= 1e-6 x the sum of |terms| behind it (else the case is drawn again with the next seed):
the tests' bound of one binary32 rounding of r is then far above the binary64 summation error, whatever the order.

WHOLE-CALL cases: B 4, N 8, D 3, T 10, maximum_number_of_steps 3, one corrector step, sigma in [0.05, 0.5] (sigma_eff > 0.02
asserted), regularizer_lambda_weight 2.5.  compute_weighted_regularizer_loss of the reference under torch.manual_seed, with a
small MLP as both networks (`mlp`) and with an analytical trajectory network (`analytical`).  Arrays:
  batch_A, batch_X, batch_L, batch_time, batch_noise       the augmented batch (forces are zeros)
  net/<key>                                                the MLP's state_dict
  schedule_time, schedule_sigma [T]                        the reference's Noise
  batch_index, start_index, end_index, end_time, end_sigma, start_time, start_sigma
  start_X; end_A, end_X, end_L; s, target f32 [B, N, D]; loss, weighted_loss f32; weight, seed
  analytical: sites [N, D], sigma_d, analytical_kmax
`none_valid`: the same batch with every time below schedule_time[3]; the reference returns 0.0 (`weighted_loss`).
"""
import os
import sys
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

from diffusion_for_multi_scale_molecular_dynamics.models.score_networks.analytical_score_network import \
    AnalyticalScoreNetworkParameters  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.regularizers.consistency_regularizer import (  # noqa: E402
    ConsistencyRegularizer, ConsistencyRegularizerParameters)

DIRECTORY = "consistency"
OPERAND_CASES = {      # name -> (B, N, D), seed, sigma_start, sigma_end, kmax
    "n1_d1": ((1, 1, 1), 1511, 0.1, 0.04, 4), "n5_d3": ((3, 5, 3), 1521, 0.1, 0.04, 4), "n65_d2": ((2, 65, 2), 1531, 0.2, 0.15, 4),
    "n216_d3": ((2, 216, 3), 1541, 0.05, 0.02, 4), "ewald": ((3, 5, 3), 1551, 0.5, 0.2, 4), "end_zero": ((3, 5, 3), 1561, 0.03, 0.0, 4),
    "placed": ((3, 5, 3), 1571, 0.1, 0.04, 4), "kmax1": ((3, 5, 3), 1581, 0.3, 0.1, 1),
    "per_structure_sigma": ((3, 5, 3), 1591, (0.1, 0.45, 0.02), (0.04, 0.1, 0.0), 4)}
WHOLE_CALL_CASES = {"mlp": 1601, "analytical": 1602}
FILES = [name + ".npz" for name in list(OPERAND_CASES) + list(WHOLE_CALL_CASES) + ["none_valid"]]
CANCELLATION_FLOOR = 1e-6
B, N, D, T, STEPS, WEIGHT = 4, 8, 3, 10, 3, 2.5
NOISE_KW = dict(sigma_min=0.05, sigma_max=0.5)
CELL = [5.43] * D


def _regularizer(kmax=4, analytical=None, weight=1.0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        noise_parameters = mg.NoiseParameters(total_time_steps=T, **NOISE_KW)
        sampling_parameters = mg.PredictorCorrectorSamplingParameters(
            number_of_corrector_steps=1, number_of_atoms=N, number_of_samples=B, spatial_dimension=D, num_atom_types=1,
            use_fixed_lattice_parameters=True, cell_dimensions=CELL)
    return ConsistencyRegularizer(ConsistencyRegularizerParameters(
        maximum_number_of_steps=STEPS, kmax_target_score=kmax, noise_parameters=noise_parameters,
        sampling_parameters=sampling_parameters, analytical_score_network_parameters=analytical,
        regularizer_lambda_weight=weight))


def _operands(name, seed):
    (batch, atoms, dimension), _, sigma_start, sigma_end, _ = OPERAND_CASES[name]
    g = torch.Generator().manual_seed(seed)
    x_start, x_end = torch.rand(batch, atoms, dimension, generator=g), torch.rand(batch, atoms, dimension, generator=g)
    s = torch.randn(batch, atoms, dimension, generator=g)
    if name == "placed":
        x_end[0] = torch.randint(0, 8, (atoms, dimension), generator=g) / 8.0
        x_start[0] = x_end[0]                                                    # 0
        x_start[0, 1] = torch.where(x_end[0, 1] < 0.5, x_end[0, 1] + 0.5, x_end[0, 1] - 0.5)     # +1/2 and -1/2, exactly
        x_start[0, 2], x_end[0, 2] = 0.0, 1e-20                                 # a tiny negative difference: wraps to 0
        x_start[0, 3], x_end[0, 3] = 1.0 - 2.0**-24, 0.0                        # the largest binary32 below 1
    words = lambda value: torch.tensor(value, dtype=torch.float32).reshape(-1)
    return x_start, x_end, s, words(sigma_start), words(sigma_end)


def _evaluate64(x_start, x_end, s, sigma_start, sigma_end, kmax):
    shape = (-1, 1, 1) if sigma_start.numel() > 1 else ()
    AXL = mg.AXL
    start, end = AXL(A=None, X=x_start.double(), L=None), AXL(A=None, X=x_end.double(), L=None)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # torch.tensor(a tensor)
        target = _regularizer(kmax).get_score_target(start, end, sigma_start.double().reshape(shape), sigma_end.double().reshape(shape))
    assert target.dtype == torch.float64 and target.shape == x_start.shape
    score, batch = s.double(), x_start.shape[0]
    terms = score * (score - 2.0 * target)
    return dict(target64=target, per_structure64=terms.sum(dim=(1, 2)), loss64=torch.sum(terms) / batch,
                gradient64=2.0 * (score - target) / batch, magnitude_per_structure64=terms.abs().sum(dim=(1, 2)),
                magnitude64=terms.abs().sum() / batch)


def operand_case(name):
    _, seed, _, _, kmax = OPERAND_CASES[name]
    while True:
        x_start, x_end, s, sigma_start, sigma_end = _operands(name, seed)
        out = _evaluate64(x_start, x_end, s, sigma_start, sigma_end, kmax)
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), name
        kept = bool((out["per_structure64"].abs() >= CANCELLATION_FLOOR * out["magnitude_per_structure64"]).all()) and \
            bool(out["loss64"].abs() >= CANCELLATION_FLOOR * out["magnitude64"])
        if kept:
            break
        seed += 1
    arrays = dict(x_start=mg._np(x_start), x_end=mg._np(x_end), s=mg._np(s), sigma_start=mg._np(sigma_start),
                  sigma_end=mg._np(sigma_end), kmax=np.array(kmax), seed=np.array(seed))
    arrays.update({key: mg._np(value) for key, value in out.items()})
    return arrays


def _batch(time_indices, noise, seed):
    g = torch.Generator().manual_seed(seed)
    composition = mg.AXL(A=torch.randint(0, 2, (B, N), generator=g), X=torch.rand(B, N, D, generator=g),
                         L=torch.tensor(CELL + [0.0] * (D * (D - 1) // 2)).repeat(B, 1))
    indices = torch.tensor(time_indices)
    return {mg.NOISY_AXL_COMPOSITION: composition, mg.TIME: noise.time[indices].reshape(B, 1).clone(),
            mg.NOISE: noise.sigma[indices].reshape(B, 1).clone(), mg.CARTESIAN_FORCES: torch.zeros(B, N, D)}


def _schedule(regularizer, net):
    generator = mg.LangevinGenerator(noise_parameters=regularizer.noise_parameters,
                                     sampling_parameters=regularizer.sampling_parameters, axl_network=net)
    return generator.noise


def whole_call_case(name):
    seed = WHOLE_CALL_CASES[name]
    net = mg._mlp(N, 1, seed=seed, hidden=32)
    analytical, extra = None, {}
    if name == "analytical":
        sites = torch.rand(N, D, generator=torch.Generator().manual_seed(seed + 10))
        analytical = AnalyticalScoreNetworkParameters(spatial_dimension=D, number_of_atoms=N, num_atom_types=1, kmax=4, sigma_d=0.05,
                                                      equilibrium_relative_coordinates=sites.tolist())
        extra = dict(sites=mg._np(sites), sigma_d=np.array(0.05), analytical_kmax=np.array(4))
    regularizer = _regularizer(analytical=analytical, weight=WEIGHT)
    noise = _schedule(regularizer, net)
    batch = _batch([1, 6, 9, 4], noise, seed + 1)
    seen = {}
    original = dict(start=regularizer.generate_starting_composition, ends=regularizer.get_partial_trajectory_start_and_end,
                    target=regularizer.get_score_target)

    def generate_starting_composition(composition, batch_index):
        seen["batch_index"], seen["start"] = int(batch_index), original["start"](composition, batch_index)
        return seen["start"]

    def get_partial_trajectory_start_and_end(start_time, noise_):
        seen["start_time"], seen["ends"] = start_time, original["ends"](start_time, noise_)
        return seen["ends"]

    def get_score_target(start, end, start_sigma, end_sigma):
        seen["end"], seen["start_sigma"], seen["target"] = end, start_sigma, original["target"](start, end, start_sigma, end_sigma)
        return seen["target"]

    regularizer.generate_starting_composition = generate_starting_composition
    regularizer.get_partial_trajectory_start_and_end = get_partial_trajectory_start_and_end
    regularizer.get_score_target = get_score_target
    handle = net.register_forward_hook(lambda module, inputs, output: seen.__setitem__("s", output.X))
    torch.manual_seed(seed + 2)
    with torch.no_grad(), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        weighted = regularizer.compute_weighted_regularizer_loss(net, batch, current_epoch=0)
    handle.remove()
    start_index, end_index, end_time, end_sigma = seen["ends"]
    effective = float(torch.sqrt(torch.as_tensor(seen["start_sigma"]).double()**2 - torch.as_tensor(end_sigma).double()**2))
    assert effective > 0.02 and int(end_index) > 0, (name, effective)
    s, target = seen["s"], seen["target"]
    loss = torch.sum(s * (s - 2.0 * target)) / B
    assert torch.equal(weighted, WEIGHT * loss) and bool(torch.isfinite(loss))
    composition = batch[mg.NOISY_AXL_COMPOSITION]
    arrays = dict(batch_A=mg._np(composition.A), batch_X=mg._np(composition.X), batch_L=mg._np(composition.L),
                  batch_time=mg._np(batch[mg.TIME]), batch_noise=mg._np(batch[mg.NOISE]), schedule_time=mg._np(noise.time),
                  schedule_sigma=mg._np(noise.sigma), batch_index=np.array(seen["batch_index"]), start_index=np.array(int(start_index)),
                  end_index=np.array(int(end_index)), end_time=mg._np(torch.as_tensor(end_time)),
                  end_sigma=mg._np(torch.as_tensor(end_sigma)), start_time=mg._np(seen["start_time"]),
                  start_sigma=mg._np(seen["start_sigma"]), start_X=mg._np(seen["start"].X), end_A=mg._np(seen["end"].A),
                  end_X=mg._np(seen["end"].X), end_L=mg._np(seen["end"].L), s=mg._np(s), target=mg._np(target), loss=mg._np(loss),
                  weighted_loss=mg._np(weighted), weight=np.array(WEIGHT), seed=np.array(seed + 2), **extra, **mg._state_dict_np(net))
    assert torch.equal(seen["start"].A, composition.A[seen["batch_index"]].expand(B, N))
    return arrays


def none_valid_case():
    net = mg._mlp(N, 1, seed=WHOLE_CALL_CASES["mlp"], hidden=32)
    regularizer = _regularizer(weight=WEIGHT)
    noise = _schedule(regularizer, net)
    batch = _batch([0, 1, 2, 0], noise, 1611)
    torch.manual_seed(1612)
    with torch.no_grad():
        weighted = regularizer.compute_weighted_regularizer_loss(net, batch, current_epoch=0)
    assert float(weighted) == 0.0
    composition = batch[mg.NOISY_AXL_COMPOSITION]
    return dict(batch_A=mg._np(composition.A), batch_X=mg._np(composition.X), batch_L=mg._np(composition.L),
                batch_time=mg._np(batch[mg.TIME]), batch_noise=mg._np(batch[mg.NOISE]), schedule_time=mg._np(noise.time),
                schedule_sigma=mg._np(noise.sigma), weighted_loss=mg._np(weighted), weight=np.array(WEIGHT))


def golden_consistency():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    for name in OPERAND_CASES:
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **operand_case(name))
    for name in WHOLE_CALL_CASES:
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **whole_call_case(name))
    mg.save(os.path.join(DIRECTORY, "none_valid.npz"), **none_valid_case())


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_consistency()
