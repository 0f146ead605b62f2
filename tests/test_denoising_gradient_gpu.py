"""The fused loss-and-gradient kernel (mdx_denoising_loss_gradient), kernels.denoising_loss_and_gradient, the differentiable
`denoising_loss` and `training_loss` on the GPU against the REFERENCE's float64 autograd on the binary32 operands
(tests/golden/denoising_gradient/*.npz, made by tests/golden/make_golden_denoising_gradient.py).

The bound is `denoising_loss_cases.excess` <= 0: |got - reference64| <= 2^-23 |reference64| + 1e-12, one binary32 rounding of a
binary64 evaluation -- which is what the kernel is.  tests/test_denoising_gradient_cpu.py shows that a binary64 evaluation of the
closed form in another operation order stays below 2e-5 of that bound on every element of every case, so no case carries a
floor of its own."""
import pytest
import torch

import nets
from denoising_gradient_cases import ALGORITHMS, CASES, GRADIENTS, closed_form, gradient_fixture, operands, scalars, tensors
from denoising_loss_cases import excess, fraction
from test_denoising_loss_gpu import RecordedNetwork, noised_batch

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
from diffusion_for_multi_scale_molecular_dynamics_amd.loss import denoising_loss, training_loss
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.analytical_score_network import \
    AnalyticalScoreNetworkParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION,
                                                                        NOISY_RELATIVE_COORDINATES, TIME)
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers import RegressionRegularizer, RegressionRegularizerParameters

pytestmark = pytest.mark.gpu

PAIRS = [(case, algorithm) for case in CASES for algorithm in ALGORITHMS]
PARTS = dict(X=("x0", "xt", "predicted_x", "sigma"), A=("a0", "at", "logits", "time_indices", "q_matrices", "q_bar_matrices",
                                                         "q_bar_tm1_matrices"), L=("l0", "lt", "predicted_l", "sigma_n", "sigma"))
SMALL = "c3_n5_d3_p6"
_RUNS = {}


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return (a is None and b is None) or torch.equal(_bits(a), _bits(b))


def run(case, algorithm, cuda):
    """The kernel's outputs of a case, computed once and left unchanged."""
    if (case, algorithm) not in _RUNS:
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        out = kernels.denoising_loss_and_gradient(**tensors(case, cuda), **scalars(case, algorithm), with_terms=True, status=status)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        _RUNS[(case, algorithm)] = out
    return _RUNS[(case, algorithm)]


@pytest.mark.parametrize("case, algorithm", PAIRS)
def test_the_gradients_and_the_loss_against_the_float64_autograd_record(case, algorithm, cuda):
    out, g = run(case, algorithm, cuda), gradient_fixture(case)
    assert out.loss.dim() == 0 and out.loss.dtype == torch.float32 and not out.loss.requires_grad
    failures = []
    for name in GRADIENTS + ("loss",):
        got, reference64 = getattr(out, name), g[f"{algorithm}_{name}64"]
        print(f"{case} {algorithm} {name}: {fraction(got, reference64):.3f} of the bound")
        if excess(got, reference64) > 0.0:
            failures.append((name, excess(got, reference64)))
    assert not failures, failures
    assert bool((out.gradient_a[..., -1] == 0.0).all())                    # the MASK logit is -inf: an exact zero, no 0 x inf


@pytest.mark.parametrize("case, algorithm", PAIRS)
def test_every_forward_output_is_the_forward_kernels(case, algorithm, cuda):
    out = run(case, algorithm, cuda)
    forward = kernels.denoising_loss(**tensors(case, cuda), **scalars(case, algorithm), with_terms=True)
    for name in kernels.DenoisingLoss._fields:
        assert getattr(forward, name) is not None and _same(getattr(out, name), getattr(forward, name)), name


@pytest.mark.parametrize("case, algorithm", PAIRS)
def test_each_part_alone_gives_the_bits_of_the_whole(case, algorithm, cuda):
    whole, everything, numbers = run(case, algorithm, cuda), tensors(case, cuda), scalars(case, algorithm)
    for part, names in PARTS.items():
        alone = kernels.denoising_loss_and_gradient(**{name: everything[name] for name in names}, **numbers)
        for other in "XAL":
            gradient = getattr(alone, "gradient_" + other.lower())
            if other == part:
                assert _same(gradient, getattr(whole, "gradient_" + other.lower())), (part, other)
            else:
                assert gradient is None, (part, other)
    # the atom types without the tables have a cross-entropy term, no loss and so no gradient
    no_tables = kernels.denoising_loss_and_gradient(a0=everything["a0"], logits=everything["logits"], **numbers, with_terms=True)
    assert no_tables.gradient_a is None and no_tables.ce_term is not None and float(no_tables.loss) == 0.0


def test_a_gradient_without_its_part_is_refused(cuda, monkeypatch):
    everything, numbers = tensors(SMALL, cuda), scalars(SMALL, "mse")
    calls = []
    monkeypatch.setattr(kernels, "call", lambda name, *arguments: calls.append((name, list(arguments))))
    kernels.denoising_loss_and_gradient(**{name: everything[name] for name in PARTS["L"]}, **numbers)
    (name, arguments), = calls
    assert name == "mdx_denoising_loss_gradient"
    position = {parameter: i for i, (_, parameter) in enumerate(_hip.ABI.functions[name].params)}
    assert arguments[position["predicted_x"]] is None and arguments[position["gradient_x"]] is None
    _hip.call(name, *arguments)                                             # as it stands it is served
    for gradient, shape in (("gradient_x", (12, 5, 3)), ("gradient_a", (12, 5, 3))):
        refused = list(arguments)
        refused[position[gradient]] = torch.zeros(shape, device=cuda)
        with pytest.raises(MdxError, match="status -1"):
            _hip.call(name, *refused)
    # the atom types' gradient needs the tables as well as the logits
    calls.clear()
    kernels.denoising_loss_and_gradient(a0=everything["a0"], logits=everything["logits"], **numbers)
    (name, arguments), = calls
    arguments[position["gradient_a"]] = torch.zeros(12, 5, 3, device=cuda)
    with pytest.raises(MdxError, match="status -1"):
        _hip.call(name, *arguments)
    with pytest.raises(ValueError, match="batch_divisor must be positive"):
        kernels.denoising_loss_and_gradient(**everything, **numbers, batch_divisor=0.0)


def test_the_batch_divisor_divides_the_gradients_and_the_loss(cuda):
    out = kernels.denoising_loss_and_gradient(**tensors(SMALL, cuda), **scalars(SMALL, "weighted_mse"), batch_divisor=3.0)
    expected = closed_form(SMALL, "weighted_mse", batch_divisor=3.0)
    for name in GRADIENTS + ("loss",):
        assert excess(getattr(out, name), expected[name]) <= 0.0, name
    assert _same(out.per_structure, run(SMALL, "weighted_mse", cuda).per_structure)
    assert not _same(out.gradient_x, run(SMALL, "weighted_mse", cuda).gradient_x)


def test_two_launches_and_a_captured_graph_give_the_same_bits(cuda):
    case, algorithm = "c4_n300_d3_p6", "weighted_mse"
    eager = run(case, algorithm, cuda)
    everything, numbers = tensors(case, cuda), scalars(case, algorithm)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    again = kernels.denoising_loss_and_gradient(**everything, **numbers, with_terms=True, status=status)
    assert all(_same(a, b) for a, b in zip(eager, again))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                           # one stream: the launch, then the total
        captured = kernels.denoising_loss_and_gradient(**everything, **numbers, with_terms=True, status=status)
    for _ in range(3):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(_same(a, b) for a, b in zip(eager, captured))
    assert int(status.item()) == 0


def test_an_atom_type_outside_its_range_gives_nans_in_its_row_only(cuda):
    case, algorithm = SMALL, "mse"
    clean = run(case, algorithm, cuda)
    a0 = torch.from_numpy(operands(case)["a0"].copy()).to(cuda)
    a0[3, 1] = 3                                                            # = C
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    out = kernels.denoising_loss_and_gradient(**tensors(case, cuda, a0=a0), **scalars(case, algorithm), status=status)
    assert bool(torch.isnan(out.gradient_a[3, 1]).all()) and int(status.item()) == _hip.STATUS_LOSS_INDEX
    assert bool(torch.isnan(out.loss)) and bool(torch.isnan(out.per_structure[3, 3]))
    others = [b for b in range(12) if b != 3]
    for name in GRADIENTS:
        assert _same(getattr(out, name)[others], getattr(clean, name)[others]), name
    assert _same(out.gradient_x, clean.gradient_x) and _same(out.gradient_l, clean.gradient_l)
    assert not bool(torch.isnan(out.gradient_a[3, [0, 2, 3, 4]]).any())
    with pytest.raises(IndexError, match="atom type outside"):
        kernels.raise_loss_status(status)
    # an invalid sigma: the structure's X (and with weighted_mse L) gradients are NaN with the forward's bit
    sigma = tensors(case, cuda)["sigma"].clone()
    sigma[5] = -1.0
    out = kernels.denoising_loss_and_gradient(**tensors(case, cuda, sigma=sigma), **scalars(case, algorithm), status=status)
    assert bool(torch.isnan(out.gradient_x[5]).all()) and int(status.item()) == _hip.STATUS_ANALYTICAL_SIGMA
    others = [b for b in range(12) if b != 5]
    assert _same(out.gradient_x[others], clean.gradient_x[others]) and _same(out.gradient_a, clean.gradient_a)


def test_backward_returns_the_kernels_buffers(cuda):
    everything, numbers = tensors(SMALL, cuda), scalars(SMALL, "weighted_mse")
    leaves = {name: everything[name].clone().requires_grad_() for name in ("predicted_x", "logits")}
    out = kernels.denoising_loss_and_gradient(**{**everything, **leaves}, **numbers)
    assert out.loss.requires_grad and _same(out.loss.detach(), run(SMALL, "weighted_mse", cuda).loss)
    assert not out.gradient_x.requires_grad and not out.loss_x.requires_grad
    (3 * out.loss).backward()
    assert torch.equal(leaves["predicted_x"].grad, 3 * out.gradient_x) and torch.equal(leaves["logits"].grad, 3 * out.gradient_a)
    assert everything["predicted_l"].grad is None and out.gradient_l is not None
    assert not kernels.denoising_loss_and_gradient(**everything, **numbers).loss.requires_grad


def _network(cuda, seed=11):
    return nets.mlp_net(5, 2, hidden=32, seed=seed).to(cuda)


def test_the_differentiable_loss_reaches_the_parameters_through_the_buffers(cuda):
    batch = noised_batch(SMALL, cuda)
    net = _network(cuda)
    out = denoising_loss(net, batch, differentiable=True)
    assert out["loss"].requires_grad and out["loss"].dim() == 0
    assert not out["model_predictions"].X.requires_grad and not out["unreduced_loss"].A.requires_grad
    out["loss"].backward()
    kernels.raise_loss_status(out["status"])
    parameters = [p for p in net.parameters() if p.grad is not None]
    assert parameters and all(bool(torch.isfinite(p.grad).all()) for p in parameters)
    assert any(bool(p.grad.abs().sum() > 0) for p in parameters)
    # a second identical forward, the kernel's buffers as grad_outputs: the same bits
    augmented = {TIME: batch[TIME], NOISE: batch[NOISE], NOISY_AXL_COMPOSITION: out[NOISY_AXL_COMPOSITION],
                 CARTESIAN_FORCES: torch.zeros_like(out[NOISY_AXL_COMPOSITION].X)}
    predictions = net(augmented, conditional=None)
    assert torch.equal(predictions.X.detach(), out["model_predictions"].X)
    buffers = out["prediction_gradients"]
    expected = torch.autograd.grad([predictions.X, predictions.A, predictions.L], parameters,
                                   grad_outputs=[buffers.X, buffers.A, buffers.L])
    for p, e in zip(parameters, expected):
        assert torch.equal(p.grad, e)
    # the loss is the forward's: the kernel adds the twelve unrounded aggregates, the wrapper's mean the rounded ones, each
    # within 2^-24 of a term that is at most twelve times the mean
    plain = denoising_loss(net, batch)
    assert plain["loss"].grad_fn is None and "prediction_gradients" not in plain
    assert _same(plain["per_structure_loss"], out["per_structure_loss"])
    torch.testing.assert_close(out["loss"].detach(), plain["loss"], rtol=13 * 2.0**-24, atol=0.0)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_not_differentiable_is_todays_loss(algorithm, cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd.loss.loss_parameters import create_loss_parameters
    block = dict(algorithm=algorithm)
    parameters = create_loss_parameters(dict(loss=dict(coordinates=block, lattice_parameters=dict(block))))
    batch, network = noised_batch(SMALL, cuda), RecordedNetwork(SMALL, cuda)
    default = denoising_loss(network, batch, loss_parameters=parameters)
    explicit = denoising_loss(network, batch, loss_parameters=parameters, differentiable=False)
    forward = kernels.denoising_loss(**tensors(SMALL, cuda), **scalars(SMALL, algorithm))      # the case holds the defaults
    expected = forward.per_structure[:, 3].mean(dtype=torch.float64).to(torch.float32)
    for out in (default, explicit):
        assert out["loss"].grad_fn is None and not out["loss"].requires_grad and _same(out["loss"], expected)
    differentiable = denoising_loss(network, batch, loss_parameters=parameters, differentiable=True)
    assert not differentiable["loss"].requires_grad            # the recorded network has no parameter: nothing asks for a gradient
    assert _same(differentiable["unreduced_loss"].A, default["unreduced_loss"].A)


class StubRegularizer:
    def __init__(self, parameter, runs):
        self.parameter, self.runs, self.calls = parameter, runs, []

    def can_regularizer_run(self):
        return self.runs

    def compute_weighted_regularizer_loss(self, score_network, augmented_batch, current_epoch):
        self.calls.append((score_network, augmented_batch, current_epoch))
        return 0.5 * (self.parameter**2).sum()


def test_training_loss_adds_the_weighted_regularizer_loss(cuda):
    batch, net = noised_batch(SMALL, cuda), _network(cuda)
    alone = training_loss(net, batch)
    assert "regularizer_loss" not in alone and alone["loss"].requires_grad
    assert _same(alone["loss"].detach(), denoising_loss(net, batch, differentiable=True)["loss"].detach())
    parameter = next(net.parameters())
    stub = StubRegularizer(parameter, runs=True)
    out = training_loss(net, batch, regularizer=stub, current_epoch=7)
    (network, augmented, epoch), = stub.calls
    assert network is net and epoch == 7 and augmented[NOISY_AXL_COMPOSITION].X is batch[NOISY_RELATIVE_COORDINATES]
    assert torch.equal(out["regularizer_loss"].detach(), 0.5 * (parameter.detach()**2).sum())
    assert torch.equal(out["loss"].detach(), alone["loss"].detach() + out["regularizer_loss"].detach())
    out["loss"].backward()
    only_denoising = torch.autograd.grad(alone["loss"], parameter)[0]
    torch.testing.assert_close(parameter.grad, only_denoising + parameter.detach(), rtol=1e-6, atol=1e-9)
    idle = StubRegularizer(parameter, runs=False)
    out = training_loss(net, batch, regularizer=idle)
    assert "regularizer_loss" not in out and not idle.calls and _same(out["loss"].detach(), alone["loss"].detach())


def test_training_loss_with_the_regression_regularizer_fills_finite_gradients(cuda):
    batch, net = noised_batch(SMALL, cuda), _network(cuda)
    sites = torch.rand(5, 3, generator=torch.Generator().manual_seed(5))
    target = AnalyticalScoreNetworkParameters(spatial_dimension=3, number_of_atoms=5, num_atom_types=2, kmax=4, sigma_d=0.1,
                                              equilibrium_relative_coordinates=sites.tolist(), use_permutation_invariance=False)
    regularizer = RegressionRegularizer(RegressionRegularizerParameters(score_network_parameters=target,
                                                                        regularizer_lambda_weight=0.25)).to(cuda)
    torch.manual_seed(3)
    out = training_loss(net, batch, regularizer=regularizer, current_epoch=0)
    assert regularizer.last_call["path"] == "kernel" and out["regularizer_loss"].requires_grad
    assert torch.equal(out["regularizer_loss"].detach(), 0.25 * regularizer.last_call["loss"].detach())
    out["loss"].backward()
    kernels.raise_loss_status(out["status"])
    parameters = [p for p in net.parameters() if p.grad is not None]
    assert parameters and all(bool(torch.isfinite(p.grad).all()) for p in parameters)
    total, regularization = out["loss"].detach(), out["regularizer_loss"].detach()
    assert bool(torch.isfinite(total)) and float(total) > float(regularization) > 0.0
