"""Generate the denoising-loss fixtures tests/golden/denoising_loss/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_denoising_loss.py

What the reference's AXLDiffusionLightningModel._generic_step (models/axl_diffusion_lightning_model.py:243-346) computes for a
batch NoisingTransform._transform_from_noise_sample (data/diffusion/noising_transform.py:122-200) noised, evaluated by the
reference's own functions -- get_coordinates_sigma_normalized_score on map_relative_coordinates_to_unit_cell,
get_lattice_sigma_normalized_score, scale_sigma_by_number_of_atoms, create_loss_calculator's three calculators -- as built
(binary32) and in binary64 ON THE BINARY32 OPERANDS.  The Lightning module itself cannot be imported here (no lightning); the
step is driven call by call in `_step`.  The stubs for the packages the reference imports but this image lacks and the writer
are make_golden.py's, imported from it unchanged.

Every case has T = 12 time steps and B = 12 structures noised with get_noise_from_indices(arange(T)): every time index appears
once, index 0 (the NLL branch) included.  sigma_min 1e-3, sigma_max 0.5: both branches of the wrapped score, on either side of
1 / sqrt(2 pi).  The noisers' draws come from a seeded generator and are stored, so only reachable pairs (a_t is a_0 or MASK)
occur.  One file per case, (C, N, D, P) = classes with MASK, atoms, spatial dimension, lattice parameters:
  c2_n1_d1_p1, c3_n5_d3_p6, c8_n65_d2_p3    logits 3 randn with the MASK logit at -inf; c8_n65_d2_p3 is one atom past a wavefront
  clip             (3, 5, 3, 6), logits +-30: the eps clip of the probabilities acts
  placed           (3, 5, 3, 6), rows placed by hand after the transform: structure 5 xt == x0; structure 6 x0 on multiples of
                   1/8 and xt = x0 +- 1/2 exactly; structure 7 every atom masked; structure 8 no atom masked
  sigma0_control   (3, 5, 3, 6), weighted_mse with sigma0 0.1 and exponent 200: the binary32 rounding of sigma0 changes the
                   weights by 200 x 1.5e-9 = 3e-7 of their value, beyond one binary32 rounding
Arrays of a file:
  shape [4] = (C, N, D, P); kmax; ce_weight, eps; sigma0, exponent (of weighted_mse); lambda [3] = (A, X, L)
  table_time, table_sigma [T]; table_q, table_q_bar, table_q_bar_tm1 [T, C, C]     the reference's schedule
  x0, l0 f32, a0 int64                                                              the clean batch
  draw_x [B, N, D], draw_a [B, N, C], draw_l [B, P]                                 the noisers' draws, in the reference's order
  time, noise [B, 1], time_indices [B], transform_xt, transform_at, transform_lt    the transform's outputs (its Q matrices are
                                                                                    the table rows of time_indices, asserted)
  xt, at, lt                                        the loss's operands: the transform's outputs, but for the rows `placed` moves
  sigma_n [B] f32, sigma_n_divisor f32              scale_sigma_by_number_of_atoms as _generic_step calls it (N^(1/P)), binary32
  predicted_x, logits, predicted_l f32              the network's outputs (3 randn logits, MASK at -inf)
  target_x64, target_l64, loss_a64, per_atom terms q64, p64, vb64, ce64 (N <= 5 only)       binary64 on the binary32 operands
  target_x32, target_l32, loss_a32                                                           the reference as built
  and for <algorithm> in mse, weighted_mse (X and L both):
  <algorithm>_loss_x64, _loss_l64, _per_structure64 [B, 4] = (mean A, mean X, mean L, aggregate), _loss64; the same with 32
  <algorithm>_calculator_x64, _calculator_l64       the calculators in binary64 on (prediction, binary32(target64), sigmas): what a
                                                    caller of calculate_unreduced_loss with binary32 tensors asks for
Asserted here: every recorded value is finite; sigma / sigma_n_divisor == sigma_n bit for bit; the transform's matrices are the
table rows; at is a0 or MASK everywhere.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

from diffusion_for_multi_scale_molecular_dynamics.data.diffusion.noising_transform import NoisingTransform  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.loss import create_loss_calculator  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.loss.loss_parameters import create_loss_parameters  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.namespace import (  # noqa: E402
    ATOM_TYPES, LATTICE_PARAMETERS, NOISE, NOISY_ATOM_TYPES, NOISY_LATTICE_PARAMETERS, NOISY_RELATIVE_COORDINATES, Q_BAR_MATRICES,
    Q_BAR_TM1_MATRICES, Q_MATRICES, RELATIVE_COORDINATES, TIME, TIME_INDICES)
from diffusion_for_multi_scale_molecular_dynamics.noise_schedulers.noise_parameters import NoiseParameters  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.noisers.atom_types_noiser import AtomTypesNoiser  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.noisers.lattice_noiser import LatticeNoiser  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.noisers.relative_coordinates_noiser import RelativeCoordinatesNoiser  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.score.gaussian_score import get_lattice_sigma_normalized_score  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.score.wrapped_gaussian_score import \
    get_coordinates_sigma_normalized_score  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.utils.basis_transformations import \
    map_relative_coordinates_to_unit_cell  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.utils.d3pm_utils import class_index_to_onehot  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.utils.noise_utils import scale_sigma_by_number_of_atoms  # noqa: E402

DIRECTORY = "denoising_loss"
T = B = 12
KMAX = 4
ALGORITHMS = ("mse", "weighted_mse")
CASES = {      # name -> (C, N, D, P), seed
    "c2_n1_d1_p1": ((2, 1, 1, 1), 1411), "c3_n5_d3_p6": ((3, 5, 3, 6), 1412), "c8_n65_d2_p3": ((8, 65, 2, 3), 1413),
    "clip": ((3, 5, 3, 6), 1414), "placed": ((3, 5, 3, 6), 1415), "sigma0_control": ((3, 5, 3, 6), 1416)}
FILES = [name + ".npz" for name in CASES]
WEIGHTED = {"sigma0_control": dict(sigma0=0.1, exponent=200.0)}
PER_ATOM_TERMS_UP_TO = 5


def _loss_parameters(algorithm, name):
    block = dict(algorithm=algorithm, **(WEIGHTED.get(name, {}) if algorithm == "weighted_mse" else {}))
    return create_loss_parameters(dict(loss=dict(coordinates=block, lattice_parameters=dict(block))))


def _step(operands, parameters, cast, rounded_target=False):
    """_generic_step's arithmetic after the network's forward, by the reference's functions, in the dtype `cast` makes."""
    c = {key: (cast(value) if value.is_floating_point() else value) for key, value in operands.items()}
    x0, xt, l0, lt, a0, at = c["x0"], c["xt"], c["l0"], c["lt"], c["a0"], c["at"]
    _, N, D = x0.shape
    P, C = l0.shape[-1], c["logits"].shape[-1]
    sigmas = c["noise"].reshape(-1, 1, 1).repeat(1, N, D)
    sigmas_for_lattice = c["noise"].reshape(-1, 1).repeat(1, P)
    target_x = get_coordinates_sigma_normalized_score(map_relative_coordinates_to_unit_cell(xt - x0), sigmas, kmax=KMAX)
    target_l = get_lattice_sigma_normalized_score(lt, l0, c["sigma_n"].reshape(-1, 1).repeat(1, P))
    calculator = create_loss_calculator(parameters)
    out = dict(target_x=target_x, target_l=target_l)
    if rounded_target:
        out["calculator_x"] = calculator.X.calculate_unreduced_loss(c["predicted_x"], cast(target_x.float()), sigmas)
        out["calculator_l"] = calculator.L.calculate_unreduced_loss(c["predicted_l"], cast(target_l.float()), sigmas_for_lattice)
    out["loss_x"] = calculator.X.calculate_unreduced_loss(c["predicted_x"], target_x, sigmas)
    out["loss_l"] = calculator.L.calculate_unreduced_loss(c["predicted_l"], target_l, sigmas_for_lattice)
    one_hot_a0, one_hot_at = cast(class_index_to_onehot(a0, C)), cast(class_index_to_onehot(at, C))
    matrices = dict(q_matrices=c["q"].unsqueeze(1).expand(-1, N, -1, -1), q_bar_matrices=c["q_bar"].unsqueeze(1).expand(-1, N, -1, -1),
                    q_bar_tm1_matrices=c["q_bar_tm1"].unsqueeze(1).expand(-1, N, -1, -1))
    out["loss_a"] = calculator.A.calculate_unreduced_loss(
        predicted_logits=c["logits"], one_hot_real_atom_types=one_hot_a0, one_hot_noisy_atom_types=one_hot_at,
        time_indices=c["time_indices"], **matrices)
    out["q"] = calculator.A.get_q_atm1_given_at_and_a0(one_hot_a0=one_hot_a0, one_hot_at=one_hot_at, small_epsilon=parameters.A.eps, **matrices)
    out["p"] = calculator.A.get_p_atm1_given_at(predicted_logits=c["logits"], one_hot_at=one_hot_at, small_epsilon=parameters.A.eps,
                                                **matrices)
    out["vb"] = calculator.A.variational_bound_loss_term(c["logits"], one_hot_a0, one_hot_at, time_indices=c["time_indices"], **matrices)
    out["ce"] = calculator.A.cross_entropy_loss_term(c["logits"], one_hot_a0)
    means = [out["loss_a"].mean(dim=(-2, -1)), out["loss_x"].mean(dim=(-2, -1)), out["loss_l"].mean(dim=-1)]
    aggregate = parameters.X.lambda_weight * means[1] + parameters.L.lambda_weight * means[2] + parameters.A.lambda_weight * means[0]
    out["per_structure"] = torch.stack(means + [aggregate], dim=1)
    out["loss"] = torch.mean(aggregate)
    return out


def case_arrays(name):
    (C, N, D, P), seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, N, D, generator=g)
    a0 = torch.randint(0, C - 1, (B, N), generator=g)
    l0 = 4.0 + 2.0 * torch.rand(B, P, generator=g)
    draws = dict(x=torch.randn(B, N, D, generator=g), a=torch.rand(B, N, C, generator=g), l=torch.randn(B, P, generator=g))
    if name == "placed":
        x0[6] = torch.randint(0, 8, (N, D), generator=g) / 8.0
    transform = NoisingTransform(NoiseParameters(total_time_steps=T, sigma_min=1e-3, sigma_max=0.5), num_atom_types=C - 1,
                                 spatial_dimension=D, use_fixed_lattice_parameters=False, use_optimal_transport=False)
    noise_sample = transform.noise_scheduler.get_noise_from_indices(torch.arange(T))
    all_noise, _ = transform.noise_scheduler.get_all_sampling_parameters()
    originals = (RelativeCoordinatesNoiser._get_gaussian_noise, AtomTypesNoiser._get_uniform_noise, LatticeNoiser._get_gaussian_noise)
    RelativeCoordinatesNoiser._get_gaussian_noise = staticmethod(lambda shape: draws["x"].reshape(shape))
    AtomTypesNoiser._get_uniform_noise = staticmethod(lambda shape: draws["a"].reshape(shape))
    LatticeNoiser._get_gaussian_noise = staticmethod(lambda shape: draws["l"].reshape(shape))
    try:
        with torch.no_grad():
            batch = transform._transform_from_noise_sample(
                {RELATIVE_COORDINATES: x0.clone(), ATOM_TYPES: a0.clone(), LATTICE_PARAMETERS: l0.clone()}, noise_sample)
    finally:
        RelativeCoordinatesNoiser._get_gaussian_noise, AtomTypesNoiser._get_uniform_noise, LatticeNoiser._get_gaussian_noise = \
            [staticmethod(f) for f in originals]
    tables = dict(q=all_noise.q_matrix.detach(), q_bar=all_noise.q_bar_matrix.detach(), q_bar_tm1=all_noise.q_bar_tm1_matrix.detach())
    indices = batch[TIME_INDICES]
    for key, table in ((Q_MATRICES, "q"), (Q_BAR_MATRICES, "q_bar"), (Q_BAR_TM1_MATRICES, "q_bar_tm1")):
        assert torch.equal(batch[key], tables[table][indices][:, None].expand(-1, N, -1, -1)), key
    transform_xt, transform_at, transform_lt = batch[NOISY_RELATIVE_COORDINATES], batch[NOISY_ATOM_TYPES], batch[NOISY_LATTICE_PARAMETERS]
    xt, at, lt = transform_xt.clone(), transform_at.clone(), transform_lt.clone()
    if name == "placed":
        xt[5] = x0[5]
        xt[6] = torch.where(x0[6] < 0.5, x0[6] + 0.5, x0[6] - 0.5)
        at[7] = C - 1
        at[8] = a0[8]
    assert bool(((at == a0) | (at == C - 1)).all())
    noise = batch[NOISE]
    sigma_n = scale_sigma_by_number_of_atoms(noise.repeat(1, P), torch.ones_like(l0) * N, spatial_dimension=P)
    divisor = torch.pow(torch.ones_like(l0) * N, 1 / P)
    assert bool((sigma_n == sigma_n[:, :1]).all()) and bool((divisor == divisor[0, 0]).all())
    assert torch.equal(noise[:, 0] / divisor[0, 0], sigma_n[:, 0])
    predicted_x, predicted_l = torch.randn(B, N, D, generator=g), torch.randn(B, P, generator=g)
    logits = 3.0 * torch.randn(B, N, C, generator=g)
    if name == "clip":
        logits = torch.where(logits > 0, 30.0, -30.0)
    logits[..., -1] = -torch.inf
    operands = dict(x0=x0, xt=xt, l0=l0, lt=lt, a0=a0, at=at, noise=noise, sigma_n=sigma_n[:, 0].contiguous(), predicted_x=predicted_x,
                    predicted_l=predicted_l, logits=logits, time_indices=indices, q=tables["q"][indices], q_bar=tables["q_bar"][indices],
                    q_bar_tm1=tables["q_bar_tm1"][indices])
    weighted = _loss_parameters("weighted_mse", name)
    arrays = dict(shape=np.array([C, N, D, P]), kmax=np.array(KMAX), ce_weight=np.array(weighted.A.ce_weight), eps=np.array(weighted.A.eps),
                  sigma0=np.array(weighted.X.sigma0), exponent=np.array(weighted.X.exponent),
                  **{"lambda": np.array([weighted.A.lambda_weight, weighted.X.lambda_weight, weighted.L.lambda_weight])},
                  table_time=mg._np(all_noise.time), table_sigma=mg._np(all_noise.sigma), table_q=mg._np(tables["q"]),
                  table_q_bar=mg._np(tables["q_bar"]), table_q_bar_tm1=mg._np(tables["q_bar_tm1"]),
                  x0=mg._np(x0), l0=mg._np(l0), a0=mg._np(a0), draw_x=mg._np(draws["x"]), draw_a=mg._np(draws["a"]), draw_l=mg._np(draws["l"]),
                  time=mg._np(batch[TIME]), noise=mg._np(noise), time_indices=mg._np(indices), transform_xt=mg._np(transform_xt),
                  transform_at=mg._np(transform_at), transform_lt=mg._np(transform_lt), xt=mg._np(xt), at=mg._np(at), lt=mg._np(lt),
                  sigma_n=mg._np(operands["sigma_n"]), sigma_n_divisor=mg._np(divisor[0, 0]), predicted_x=mg._np(predicted_x),
                  logits=mg._np(logits), predicted_l=mg._np(predicted_l))
    shared = ["target_x", "target_l", "loss_a"]
    for algorithm in ALGORITHMS:
        parameters = _loss_parameters(algorithm, name)
        with torch.no_grad():
            out64 = _step(operands, parameters, lambda t: t.double(), rounded_target=True)
            out32 = _step(operands, parameters, lambda t: t)
        assert all(v.dtype == torch.float64 for v in out64.values()) and all(v.dtype == torch.float32 for v in out32.values())
        for key, value in list(out64.items()) + list(out32.items()):
            assert bool(torch.isfinite(value).all()), (name, algorithm, key)
        for key in shared + (["q", "p", "vb", "ce"] if N <= PER_ATOM_TERMS_UP_TO else []):
            if key + "64" in arrays:
                assert np.array_equal(arrays[key + "64"], mg._np(out64[key]))       # the same for both algorithms
            arrays[key + "64"] = mg._np(out64[key])
        for key in shared:
            arrays[key + "32"] = mg._np(out32[key])
        for key in ("loss_x", "loss_l", "per_structure", "loss"):
            arrays[f"{algorithm}_{key}64"], arrays[f"{algorithm}_{key}32"] = mg._np(out64[key]), mg._np(out32[key])
        arrays[f"{algorithm}_calculator_x64"], arrays[f"{algorithm}_calculator_l64"] = mg._np(out64["calculator_x"]), mg._np(out64["calculator_l"])
    arrays["masked_fraction"] = np.array(float((at == C - 1).float().mean()))
    arrays["float32_target_error"] = np.array(float((out32["target_x"].double() - out64["target_x"]).abs().max()))
    return arrays


def golden_denoising_loss():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    for name in CASES:
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **case_arrays(name))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_denoising_loss()
