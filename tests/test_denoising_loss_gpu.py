"""The fused loss kernel (mdx_denoising_loss), the calculators, NoisingTransform's training transform and `denoising_loss` on the
GPU against what the REFERENCE computed in binary64 on the binary32 operands (tests/golden/denoising_loss/*.npz, made by
tests/golden/make_golden_denoising_loss.py).  Everything is fed the RECORDED tables and operands.

The bound is `denoising_loss_cases.excess` <= 0: |got - reference64| <= 2^-23 |reference64| + 1e-12, one binary32 rounding of a
binary64 evaluation whose terms are at most -log(1e-8) = 18.4."""
import numpy as np
import pytest
import torch

from denoising_loss_cases import ALGORITHMS, CASES, binary32, distance, excess, fixture, fraction, scalars, tensors

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
from diffusion_for_multi_scale_molecular_dynamics_amd.loss import create_loss_calculator, denoising_loss
from diffusion_for_multi_scale_molecular_dynamics_amd.loss.loss_parameters import create_loss_parameters
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.score_network import (ScoreNetwork,
                                                                                                   ScoreNetworkParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (ATOM_TYPES, AXL, AXL_COMPOSITION, LATTICE_PARAMETERS, NOISE,
                                                                        NOISY_ATOM_TYPES, NOISY_AXL_COMPOSITION,
                                                                        NOISY_LATTICE_PARAMETERS, NOISY_RELATIVE_COORDINATES,
                                                                        Q_BAR_MATRICES, Q_BAR_TM1_MATRICES, Q_MATRICES,
                                                                        RELATIVE_COORDINATES, TIME, TIME_INDICES)

pytestmark = pytest.mark.gpu

PAIRS = [(case, algorithm) for case in CASES for algorithm in ALGORITHMS]
_RUNS = {}


def _bits(t):
    return t.view(torch.int32)


def run(case, algorithm, cuda):
    """The kernel's outputs of a case, computed once and left unchanged."""
    if (case, algorithm) not in _RUNS:
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        out = kernels.denoising_loss(**tensors(case, cuda), **scalars(case, algorithm), with_terms=True, status=status)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        _RUNS[(case, algorithm)] = out
    return _RUNS[(case, algorithm)]


def records(case, algorithm):
    """output name -> (binary64 record, the reference's binary32 record or None) of a case."""
    g = fixture(case)
    out = dict(target_x=(g["target_x64"], g["target_x32"]), target_l=(g["target_l64"], g["target_l32"]),
               loss_a=(g["loss_a64"], g["loss_a32"]), loss_x=(g[f"{algorithm}_loss_x64"], g[f"{algorithm}_loss_x32"]),
               loss_l=(g[f"{algorithm}_loss_l64"], g[f"{algorithm}_loss_l32"]),
               per_structure=(g[f"{algorithm}_per_structure64"], g[f"{algorithm}_per_structure32"]))
    if "q64" in g:
        out.update(q_atm1=(g["q64"], None), p_atm1=(g["p64"], None), vb_term=(g["vb64"], None), ce_term=(g["ce64"], None))
    return out


@pytest.mark.parametrize("case, algorithm", PAIRS)
def test_every_output_of_the_kernel_against_the_binary64_record(case, algorithm, cuda):
    out = run(case, algorithm, cuda)
    failures = []
    for name, (reference64, reference32) in records(case, algorithm).items():
        got = getattr(out, name)
        over, own = excess(got, reference64), distance(got, reference64)
        theirs = distance(reference32, reference64) if reference32 is not None else float("inf")
        print(f"{case} {algorithm} {name}: {fraction(got, reference64):.3f} of the bound, distance {own:.3e}, the reference's float32 {theirs:.3e}")
        if over > 0.0 or own > theirs:
            failures.append((name, over, own, theirs))
    assert not failures, failures


@pytest.mark.parametrize("case, algorithm", PAIRS)
def test_the_calculators_reproduce_the_records(case, algorithm, cuda):
    """The reference's operands: full-shape sigmas, one-hot vectors, per-atom matrices that are expand() views of the
    per-structure rows.  The coordinates' and lattice calculators take the binary32 target, so their record is the reference's
    calculator in binary64 on that rounded target."""
    g = fixture(case)
    C, N, D, P = (int(v) for v in g["shape"])
    t = lambda key: torch.from_numpy(np.ascontiguousarray(g[key])).to(cuda)
    block = dict(algorithm=algorithm)
    if algorithm == "weighted_mse":
        block.update(sigma0=float(g["sigma0"]), exponent=float(g["exponent"]))
    calculator = create_loss_calculator(create_loss_parameters(dict(loss=dict(coordinates=block, lattice_parameters=dict(block)))))
    sigma = t("noise")
    loss_x = calculator.X.calculate_unreduced_loss(t("predicted_x"), t("target_x64").float(), sigma.reshape(-1, 1, 1).expand(-1, N, D))
    loss_l = calculator.L.calculate_unreduced_loss(t("predicted_l"), t("target_l64").float(), sigma.expand(-1, P))
    assert excess(loss_x, g[f"{algorithm}_calculator_x64"]) <= 0.0 and excess(loss_l, g[f"{algorithm}_calculator_l64"]) <= 0.0
    rows = [t(key)[t("time_indices")] for key in ("table_q", "table_q_bar", "table_q_bar_tm1")]
    matrices = [m.unsqueeze(1).expand(-1, N, -1, -1) for m in rows]
    one_hot_a0 = torch.nn.functional.one_hot(t("a0"), C).float()
    one_hot_at = torch.nn.functional.one_hot(t("at"), C).float()
    loss_a = calculator.A.calculate_unreduced_loss(t("logits"), one_hot_a0, one_hot_at, t("time_indices"), *matrices)
    assert excess(loss_a, g["loss_a64"]) <= 0.0
    assert torch.equal(_bits(loss_a), _bits(run(case, algorithm, cuda).loss_a))          # the same kernel, the same bits
    if "q64" in g:
        eps = float(g["eps"])
        assert excess(calculator.A.cross_entropy_loss_term(t("logits"), one_hot_a0), g["ce64"]) <= 0.0
        assert excess(calculator.A.variational_bound_loss_term(t("logits"), one_hot_a0, one_hot_at, *matrices, t("time_indices")),
                      g["vb64"]) <= 0.0
        assert excess(calculator.A.get_q_atm1_given_at_and_a0(one_hot_a0, one_hot_at, *matrices, eps), g["q64"]) <= 0.0
        assert excess(calculator.A.get_p_atm1_given_at(t("logits"), one_hot_at, *matrices, eps), g["p64"]) <= 0.0


class RecordedNetwork(ScoreNetwork):
    """A score network that returns the recorded predictions."""

    def __init__(self, case, device):
        g = fixture(case)
        super().__init__(ScoreNetworkParameters(architecture="recorded", spatial_dimension=int(g["shape"][2]),
                                                num_atom_types=int(g["shape"][0]) - 1))
        self.predictions = AXL(*[torch.from_numpy(g[key]).to(device) for key in ("logits", "predicted_x", "predicted_l")])

    def _forward_unchecked(self, batch, conditional=False):
        return AXL(A=self.predictions.A.clone(), X=self.predictions.X.clone(), L=self.predictions.L.clone())


def noised_batch(case, device):
    g = fixture(case)
    N = int(g["shape"][1])
    t = lambda key: torch.from_numpy(np.ascontiguousarray(g[key])).to(device)
    batch = {RELATIVE_COORDINATES: t("x0"), ATOM_TYPES: t("a0"), LATTICE_PARAMETERS: t("l0"), NOISY_RELATIVE_COORDINATES: t("xt"),
             NOISY_ATOM_TYPES: t("at"), NOISY_LATTICE_PARAMETERS: t("lt"), TIME: t("time"), NOISE: t("noise"),
             TIME_INDICES: t("time_indices")}
    for key, table in ((Q_MATRICES, "table_q"), (Q_BAR_MATRICES, "table_q_bar"), (Q_BAR_TM1_MATRICES, "table_q_bar_tm1")):
        batch[key] = t(table)[batch[TIME_INDICES]].unsqueeze(1).expand(-1, N, -1, -1)
    return batch


@pytest.mark.parametrize("case, algorithm", PAIRS)
def test_denoising_loss_reproduces_the_records_with_one_launch(case, algorithm, cuda, monkeypatch):
    g = fixture(case)
    block = dict(algorithm=algorithm)
    if algorithm == "weighted_mse":
        block.update(sigma0=float(g["sigma0"]), exponent=float(g["exponent"]))
    parameters = create_loss_parameters(dict(loss=dict(coordinates=block, lattice_parameters=dict(block))))
    launches = []
    call = _hip.call
    monkeypatch.setattr(kernels, "call", lambda name, *args: (launches.append(name), call(name, *args))[1])
    batch = noised_batch(case, cuda)
    out = denoising_loss(RecordedNetwork(case, cuda), batch, loss_parameters=parameters, kmax_target_score=int(g["kmax"]))
    assert launches == ["mdx_denoising_loss"]
    assert set(out) == {"unreduced_loss", "loss", "sigmas", "model_predictions", "target_coordinates_normalized_conditional_scores",
                        "target_lattice_normalized_conditional_scores", AXL_COMPOSITION, NOISY_AXL_COMPOSITION, TIME,
                        "per_structure_loss", "status"}
    kernels.raise_loss_status(out["status"])
    assert excess(out["unreduced_loss"].A, g["loss_a64"]) <= 0.0
    assert excess(out["unreduced_loss"].X, g[f"{algorithm}_loss_x64"]) <= 0.0
    assert excess(out["unreduced_loss"].L, g[f"{algorithm}_loss_l64"]) <= 0.0
    assert excess(out["target_coordinates_normalized_conditional_scores"], g["target_x64"]) <= 0.0
    assert excess(out["target_lattice_normalized_conditional_scores"], g["target_l64"]) <= 0.0
    assert excess(out["per_structure_loss"], g[f"{algorithm}_per_structure64"][:, 3]) <= 0.0
    assert out["loss"].dim() == 0 and excess(out["loss"], g[f"{algorithm}_loss64"]) <= 0.0
    assert torch.equal(out["sigmas"], batch[NOISE].reshape(-1, 1, 1).expand_as(batch[RELATIVE_COORDINATES]))
    assert out[AXL_COMPOSITION].X is batch[RELATIVE_COORDINATES] and out[NOISY_AXL_COMPOSITION].A is batch[NOISY_ATOM_TYPES]
    assert out[TIME] is batch[TIME] and torch.equal(out["model_predictions"].A, torch.from_numpy(g["logits"]).to(cuda))
    # the same launch as the kernel's own test, sigma_n made inside it: the same bits
    assert torch.equal(_bits(out["unreduced_loss"].L), _bits(run(case, algorithm, cuda).loss_l))
    assert torch.equal(_bits(out["per_structure_loss"]), _bits(run(case, algorithm, cuda).per_structure[:, 3]))


def test_defaults_are_create_loss_parameters_of_nothing(cuda):
    out = denoising_loss(RecordedNetwork("c3_n5_d3_p6", cuda), noised_batch("c3_n5_d3_p6", cuda))
    assert torch.equal(_bits(out["per_structure_loss"]), _bits(run("c3_n5_d3_p6", "mse", cuda).per_structure[:, 3]))


@pytest.mark.parametrize("case", CASES)
def test_the_transform_from_a_noise_sample_with_the_recorded_draws(case, cuda, monkeypatch):
    """NoisingTransform._transform_from_noise_sample on the recorded schedule rows and draws: noisy X, A and L equal the
    reference's bit for bit; the matrices are expand() views of the per-structure rows."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.data.diffusion.noising_transform import NoisingTransform
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_scheduler import Noise
    from diffusion_for_multi_scale_molecular_dynamics_amd.noisers.atom_types_noiser import AtomTypesNoiser
    from diffusion_for_multi_scale_molecular_dynamics_amd.noisers.lattice_noiser import LatticeNoiser
    from diffusion_for_multi_scale_molecular_dynamics_amd.noisers.relative_coordinates_noiser import RelativeCoordinatesNoiser
    g = fixture(case)
    C, N, D, P = (int(v) for v in g["shape"])
    t = lambda key: torch.from_numpy(np.ascontiguousarray(g[key]))
    monkeypatch.setattr(RelativeCoordinatesNoiser, "_get_gaussian_noise", staticmethod(lambda shape: t("draw_x").reshape(shape)))
    monkeypatch.setattr(AtomTypesNoiser, "_get_uniform_noise", staticmethod(lambda shape: t("draw_a").reshape(shape)))
    monkeypatch.setattr(LatticeNoiser, "_get_gaussian_noise", staticmethod(lambda shape: t("draw_l").reshape(shape)))
    transform = NoisingTransform(NoiseParameters(total_time_steps=12, sigma_min=1e-3, sigma_max=0.5), num_atom_types=C - 1,
                                 spatial_dimension=D, use_fixed_lattice_parameters=False, use_optimal_transport=False, device=cuda)
    unused = torch.zeros(12, device=cuda)
    sample = Noise(time=t("table_time").to(cuda), sigma=t("table_sigma").to(cuda), sigma_squared=unused, g=unused, g_squared=unused,
                   beta=unused, alpha_bar=unused, q_matrix=t("table_q").to(cuda), q_bar_matrix=t("table_q_bar").to(cuda),
                   q_bar_tm1_matrix=t("table_q_bar_tm1").to(cuda), indices=torch.arange(12, device=cuda))
    batch = {RELATIVE_COORDINATES: t("x0").to(cuda), ATOM_TYPES: t("a0").to(cuda), LATTICE_PARAMETERS: t("l0").to(cuda)}
    out = transform._transform_from_noise_sample(batch, sample)
    assert out is batch
    assert np.array_equal(out[NOISY_RELATIVE_COORDINATES].cpu().numpy(), g["transform_xt"])
    assert np.array_equal(out[NOISY_ATOM_TYPES].cpu().numpy(), g["transform_at"])
    assert np.array_equal(out[NOISY_LATTICE_PARAMETERS].cpu().numpy(), g["transform_lt"])
    assert np.array_equal(out[TIME].cpu().numpy(), g["time"]) and np.array_equal(out[NOISE].cpu().numpy(), g["noise"])
    assert np.array_equal(out[TIME_INDICES].cpu().numpy(), g["time_indices"])
    for key, rows in ((Q_MATRICES, sample.q_matrix), (Q_BAR_MATRICES, sample.q_bar_matrix), (Q_BAR_TM1_MATRICES, sample.q_bar_tm1_matrix)):
        assert out[key].shape == (12, N, C, C) and out[key].data_ptr() == rows.data_ptr()
        assert N == 1 or out[key].stride(1) == 0
        assert torch.equal(out[key][:, N - 1], rows)


def test_transform_returns_the_table_rows_of_the_indices_it_reports(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd.data.diffusion.noising_transform import NoisingTransform
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    g = fixture("c3_n5_d3_p6")
    t = lambda key: torch.from_numpy(g[key]).to(cuda)
    transform = NoisingTransform(NoiseParameters(total_time_steps=12, sigma_min=1e-3, sigma_max=0.5), num_atom_types=2,
                                 spatial_dimension=3, use_optimal_transport=False, device=cuda)
    torch.manual_seed(3)
    out = transform.transform({RELATIVE_COORDINATES: t("x0"), ATOM_TYPES: t("a0"), LATTICE_PARAMETERS: t("l0")})
    tables, indices = transform.noise_scheduler.tables, out[TIME_INDICES]
    assert indices.shape == (12,) and indices.dtype == torch.int64 and int(indices.min()) >= 0 and int(indices.max()) < 12
    assert torch.equal(out[TIME], tables.time[indices].reshape(-1, 1)) and torch.equal(out[NOISE], tables.sigma[indices].reshape(-1, 1))
    for key, table in ((Q_MATRICES, tables.q_matrix), (Q_BAR_MATRICES, tables.q_bar_matrix), (Q_BAR_TM1_MATRICES, tables.q_bar_tm1_matrix)):
        assert out[key].shape == (12, 5, 3, 3) and out[key].stride(1) == 0 and torch.equal(out[key][:, 4], table[indices])
    xt, at = out[NOISY_RELATIVE_COORDINATES], out[NOISY_ATOM_TYPES]
    assert xt.shape == (12, 5, 3) and bool(((xt >= 0) & (xt < 1)).all()) and bool(((at == out[ATOM_TYPES]) | (at == 2)).all())
    assert out[NOISY_LATTICE_PARAMETERS].shape == (12, 6)
    with pytest.raises(NotImplementedError, match="use_optimal_transport=True"):
        NoisingTransform(NoiseParameters(total_time_steps=12, sigma_min=1e-3, sigma_max=0.5), num_atom_types=2, spatial_dimension=3)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_a_prediction_equal_to_the_target_gives_no_coordinates_loss(algorithm, cuda):
    """Where the target is an operand -- the calculators, which run the same kernel -- a prediction equal to it gives exactly 0.
    In the fused launch the loss is taken against the binary64 target (that is what keeps it within one rounding of the binary64
    record), and the target the caller sees is that value rounded to binary32: fed back as the prediction it leaves the
    rounding's own square, at most (2^-24 |target|)^2 times the weight."""
    case = "c8_n65_d2_p3"
    g = fixture(case)
    out = run(case, algorithm, cuda)
    block = dict(algorithm=algorithm)
    calculator = create_loss_calculator(create_loss_parameters(dict(loss=dict(coordinates=block, lattice_parameters=dict(block)))))
    sigmas = torch.from_numpy(g["noise"]).to(cuda).reshape(-1, 1, 1).expand_as(out.target_x)
    loss = calculator.X.calculate_unreduced_loss(out.target_x, out.target_x, sigmas)
    assert loss.shape == out.target_x.shape and bool((loss == 0.0).all())
    fused = kernels.denoising_loss(**tensors(case, cuda, predicted_x=out.target_x), **scalars(case, algorithm))
    assert torch.equal(_bits(fused.target_x), _bits(out.target_x))
    weights = np.exp(binary32(g["exponent"]) * (g["noise"].astype(np.float64) - binary32(g["sigma0"]))).reshape(-1, 1, 1) + 1.0 \
        if algorithm == "weighted_mse" else 1.0
    bound = (2.0**-24 * np.abs(g["target_x64"]))**2 * weights * (1.0 + 2.0**-20)
    print(f"{algorithm}: largest fused loss at prediction = target {float(fused.loss_x.max()):.3e}")
    assert bool((fused.loss_x.cpu().numpy().astype(np.float64) <= bound + 1e-45).all())
    assert excess(fused.loss_a, g["loss_a64"]) <= 0.0                      # the other parts do not move


def test_negative_controls_miss_the_bound(cuda):
    case = "c3_n5_d3_p6"
    g = fixture(case)
    logits = torch.from_numpy(g["logits"]).to(cuda)
    logits[3, 2, 0] += 1e-3
    moved = kernels.denoising_loss(**tensors(case, cuda, logits=logits), **scalars(case, "mse"))
    assert excess(moved.loss_a, g["loss_a64"]) > 0.0 and excess(moved.per_structure, g["mse_per_structure64"]) > 0.0
    assert excess(moved.loss_x, g["mse_loss_x64"]) <= 0.0
    indices = torch.from_numpy(g["time_indices"]).to(cuda)
    indices[4] += 1
    shifted = kernels.denoising_loss(**tensors(case, cuda, time_indices=indices), **scalars(case, "mse"))
    assert excess(shifted.loss_a, g["loss_a64"]) > 0.0
    # sigma0 as the Python double instead of the binary32 buffer's value: 200 x |0.1 - binary32(0.1)| = 3e-7 of every weight
    control = fixture("sigma0_control")
    unrounded = scalars("sigma0_control", "weighted_mse")
    unrounded.update(x_sigma0=float(control["sigma0"]), l_sigma0=float(control["sigma0"]))
    assert unrounded["x_sigma0"] != binary32(control["sigma0"]) and unrounded["x_exponent"] == 200.0
    out = kernels.denoising_loss(**tensors("sigma0_control", cuda), **unrounded)
    assert excess(out.loss_x, control["weighted_mse_loss_x64"]) > 0.0 and excess(out.loss_l, control["weighted_mse_loss_l64"]) > 0.0
    assert excess(run("sigma0_control", "weighted_mse", cuda).loss_x, control["weighted_mse_loss_x64"]) <= 0.0


def test_captured_in_a_graph_and_replayed_the_kernel_gives_the_eager_bits(cuda):
    case, algorithm = "c8_n65_d2_p3", "weighted_mse"
    eager = run(case, algorithm, cuda)
    operands, numbers = tensors(case, cuda), scalars(case, algorithm)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    again = kernels.denoising_loss(**operands, **numbers, with_terms=True, status=status)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(eager, again))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = kernels.denoising_loss(**operands, **numbers, with_terms=True, status=status)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(eager, captured))
    assert int(status.item()) == 0


def test_limits_and_value_assertions(cuda):
    z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=cuda)
    with pytest.raises(MdxError, match="status -2"):                      # N = 1025: refused before anything is launched
        kernels.denoising_loss(x0=z(1, 1025, 3), xt=z(1, 1025, 3), predicted_x=z(1, 1025, 3), sigma=z(1) + 0.1)
    with pytest.raises(MdxError, match="status -2"):                      # C = 9
        kernels.denoising_loss(a0=z(1, 4, dtype=torch.int64), at=z(1, 4, dtype=torch.int64), logits=z(1, 4, 9),
                               time_indices=z(1, dtype=torch.int64), q_matrices=z(2, 9, 9), q_bar_matrices=z(2, 9, 9),
                               q_bar_tm1_matrices=z(2, 9, 9))
    with pytest.raises(MdxError, match="status -2"):                      # P = 7
        kernels.denoising_loss(l0=z(1, 7), lt=z(1, 7), predicted_l=z(1, 7), sigma_n=z(1) + 0.1)
    # N = 1024 is served: four atoms per thread
    big = kernels.denoising_loss(x0=z(2, 1024, 3), xt=z(2, 1024, 3) + 0.25, predicted_x=z(2, 1024, 3), sigma=z(2) + 0.1)
    small = kernels.denoising_loss(x0=z(2, 1, 3), xt=z(2, 1, 3) + 0.25, predicted_x=z(2, 1, 3), sigma=z(2) + 0.1)
    assert torch.equal(_bits(big.loss_x), _bits(small.loss_x.expand(2, 1024, 3).contiguous()))
    # a NaN logit is the reference's "pathological logits"; a time index outside the tables reads nothing and gives NaNs
    case = "c3_n5_d3_p6"
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    logits = torch.from_numpy(fixture(case)["logits"]).to(cuda)
    logits[1, 1, 0] = float("nan")
    kernels.denoising_loss(**tensors(case, cuda, logits=logits), **scalars(case, "mse"), status=status)
    with pytest.raises(AssertionError, match="Logits are pathological"):
        kernels.raise_loss_status(status)
    assert int(status.item()) == 0
    indices = torch.from_numpy(fixture(case)["time_indices"]).to(cuda)
    indices[2] = 12
    out = kernels.denoising_loss(**tensors(case, cuda, time_indices=indices), **scalars(case, "mse"), status=status)
    with pytest.raises(IndexError, match="time index outside"):
        kernels.raise_loss_status(status)
    assert bool(torch.isnan(out.loss_a[2]).all()) and not bool(torch.isnan(out.loss_a[3]).any())
    assert bool(torch.isnan(out.per_structure[2, 3])) and excess(out.loss_x, fixture(case)["mse_loss_x64"]) <= 0.0
