"""The fused regression kernel (mdx_regression_loss), kernels.regression_loss and the RegressionRegularizer on the GPU against
what the REFERENCE computed (tests/golden/regression/*.npz, made by tests/golden/make_golden_regression.py): the operand cases
in binary64 on the recorded binary32 operands, the whole-call cases as built.

The bound is `denoising_loss_cases.excess` <= 0: |got - reference64| <= 2^-23 |reference64| + 1e-12, one binary32 rounding of a
binary64 evaluation that agrees with the reference's; every reduced value is a sum of squares, so none is a cancellation.

Whole calls: the regularized network is an MLP whose binary32 forward on the GPU is not the CPU's bit for bit, so the recorded
loss (the reference's binary32 mean on ITS score) is held at the MLP's own agreement, and the bound above is put where it
belongs: on the kernel's loss against formula64 on the score the call used and the recorded binary64 target at the drawn X,
which is bit-equal to the record's."""
import numpy as np
import pytest
import torch

from denoising_loss_cases import excess, fraction
from regression_cases import (ANALYTICAL_CASES, B, D, GIVEN_CASES, N, OPERAND_CASES, WHOLE_CALL_CASES, augmented_batch, fixture,
                              formula64, mlp, operands, regularizer)
from test_equivariant_analytical_gpu import BAR_CASE, BAR_STRUCTURE, _per_structure
from test_analytical_score_gpu import _rel

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd import regularizers as module
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import NOISE, NOISY_AXL_COMPOSITION

pytestmark = pytest.mark.gpu

OUTPUTS = ("target", "gradient", "per_structure", "loss")
_RUNS = {}


def _bits(t):
    return t.view(torch.int32)


def run(case, cuda):
    """The kernel's outputs of a case, computed once and left unchanged."""
    if case not in _RUNS:
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        (score,), keywords = operands(case, cuda)
        out = kernels.regression_loss(score, **keywords, status=status)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        _RUNS[case] = out
    return _RUNS[case]


@pytest.mark.parametrize("case", OPERAND_CASES)
def test_every_output_of_the_kernel_against_the_binary64_record(case, cuda):
    out, g = run(case, cuda), fixture(case)
    assert out.loss.dim() == 0 and out.per_structure.shape == (g["s"].shape[0],) and out.target.shape == out.gradient.shape == g["s"].shape
    assert all(t.dtype == torch.float32 and t.device == cuda for t in out)
    failures = []
    for name in OUTPUTS:
        got, reference64 = getattr(out, name), g[name + "64"]
        print(f"{case} {name}: {fraction(got, reference64):.3f} of the bound")
        if excess(got, reference64) > 0.0:
            failures.append((name, excess(got, reference64)))
    assert not failures, failures


@pytest.mark.parametrize("case", ANALYTICAL_CASES)
def test_the_target_is_bit_equal_to_the_analytical_kernel(case, cuda):
    (score,), k = operands(case, cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    scores, _ = kernels.analytical_score(k["relative_coordinates"], k["sigmas"], k["equilibrium_relative_coordinates"],
                                         k["sigma_d_square"], k["kmax"], k["use_permutation_invariance"], status=status)
    assert torch.equal(_bits(run(case, cuda).target), _bits(scores))
    # without a score only the target is made: the same bits
    alone = kernels.regression_loss(**k, status=status)
    assert alone.gradient is None and alone.per_structure is None and alone.loss is None
    assert torch.equal(_bits(alone.target), _bits(scores)) and int(status.item()) == 0


@pytest.mark.parametrize("case", GIVEN_CASES)
def test_a_score_equal_to_the_given_target_gives_exact_zeros(case, cuda):
    (_,), k = operands(case, cuda)
    out = kernels.regression_loss(k["target"].clone(), target=k["target"])
    assert torch.equal(_bits(out.target), _bits(k["target"]))
    assert float(out.loss) == 0.0 and not bool(out.per_structure.any()) and not bool(out.gradient.any())


@pytest.mark.parametrize("case", ["n216_d3", "perm8_d3", "given_n700_d3"])
def test_two_launches_and_a_captured_graph_give_the_same_bits(case, cuda):
    eager = run(case, cuda)
    (score,), keywords = operands(case, cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    again = kernels.regression_loss(score, **keywords, status=status)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(eager, again))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # nothing in the call reads on the host: the capture succeeds
        captured = kernels.regression_loss(score, **keywords, status=status)
    for _ in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(eager, captured))
    assert int(status.item()) == 0


@pytest.mark.parametrize("case", ["n5_d3", "perm3_d2"])
def test_an_invalid_sigma_or_coordinate_gives_nans_in_its_structure_only(case, cuda):
    good = run(case, cuda)
    (score,), k = operands(case, cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)

    def check(out, bad, bit, message):
        assert int(status.item()) == bit
        assert bool(torch.isnan(out.target[bad]).all()) and bool(torch.isnan(out.gradient[bad]).all())
        assert bool(torch.isnan(out.per_structure[bad])) and bool(torch.isnan(out.loss))
        for b in set(range(3)) - {bad}:
            assert all(torch.equal(_bits(getattr(out, name)[b]), _bits(getattr(good, name)[b])) for name in OUTPUTS[:3])
        with pytest.raises(AssertionError, match=message):
            kernels.raise_analytical_status(status)
        assert int(status.item()) == 0

    for value in (0.0, -0.1, float("inf"), float("nan")):
        sigmas = k["sigmas"].clone()
        sigmas[1] = value
        check(kernels.regression_loss(score, **dict(k, sigmas=sigmas), status=status), 1, _hip.STATUS_ANALYTICAL_SIGMA,
              "sigma should be larger than zero")
    for value in (float("nan"), 1.0, -1e-3):
        moved = k["relative_coordinates"].clone()
        moved[2, 1, 1] = value
        check(kernels.regression_loss(score, **dict(k, relative_coordinates=moved), status=status), 2,
              _hip.STATUS_ANALYTICAL_COORDINATES, "relative coordinates")


def test_limits_and_shapes_are_argument_checks(cuda):
    z = lambda *shape: torch.zeros(*shape, device=cuda)
    analytical = lambda shape, kmax=4, permutations=False: kernels.regression_loss(
        z(*shape) + 0.5, relative_coordinates=z(*shape) + 0.25, sigmas=z(shape[0]) + 0.1, equilibrium_relative_coordinates=z(*shape[1:]),
        sigma_d_square=0.0025, kmax=kmax, use_permutation_invariance=permutations)
    for arguments in (((1, 2, 3), 65), ((1, 2, 4), 4), ((1, 1025, 3), 4), ((1, 9, 3), 4, True)):
        with pytest.raises(MdxError, match="status -2"):           # MDX_ERR_UNSUPPORTED, before anything is launched
            analytical(*arguments)
    torch.cuda.synchronize()                                       # nothing faulted: the device still answers
    # the largest structure is served, and agrees with a small one element for element
    big, small = analytical((2, 1024, 3), 64), analytical((2, 1, 3), 64)
    assert torch.equal(_bits(big.target), _bits(small.target.expand(2, 1024, 3).contiguous()))
    assert float(small.loss) > 0.0 and abs(float(big.loss) / float(small.loss) - 1.0) < 1e-6      # every e is the same: the mean is e^2
    assert torch.equal(_bits(big.gradient * 1024.0), _bits((small.gradient).expand(2, 1024, 3).contiguous()))      # 2 e / M, M x 2^10
    # given-target mode has no such limits
    wide = kernels.regression_loss(z(1, 1500, 5) + 0.5, target=z(1, 1500, 5) + 0.25)
    assert float(wide.loss) == 0.0625 and float(wide.per_structure[0]) == 0.0625 * 7500
    with pytest.raises(ValueError, match="score has shape"):
        kernels.regression_loss(z(2, 3, 2), target=z(2, 3, 3))
    with pytest.raises(ValueError, match="equilibrium_relative_coordinates has shape"):
        kernels.regression_loss(z(2, 3, 3), relative_coordinates=z(2, 3, 3), sigmas=z(2) + 0.1, equilibrium_relative_coordinates=z(2, 3),
                                sigma_d_square=0.0025, kmax=4)
    with pytest.raises(ValueError, match="one value per structure"):
        kernels.regression_loss(z(2, 3, 3), relative_coordinates=z(2, 3, 3), sigmas=z(3) + 0.1, equilibrium_relative_coordinates=z(3, 3),
                                sigma_d_square=0.0025, kmax=4)
    with pytest.raises(ValueError, match="needs sigmas, kmax"):
        kernels.regression_loss(z(2, 3, 3), relative_coordinates=z(2, 3, 3), equilibrium_relative_coordinates=z(3, 3), sigma_d_square=0.0025)
    with pytest.raises(ValueError, match="not both"):
        kernels.regression_loss(z(2, 3, 3), target=z(2, 3, 3), relative_coordinates=z(2, 3, 3))
    with pytest.raises(ValueError, match="needs a score"):
        kernels.regression_loss(target=z(2, 3, 3))


@pytest.mark.parametrize("case", ["n5_d3", "n216_d3", "perm3_d2", "given_n700_d3"])
def test_backward_returns_the_kernels_gradient(case, cuda):
    g = fixture(case)
    (s,), keywords = operands(case, cuda)
    score = s.clone().requires_grad_()
    out = kernels.regression_loss(score, **keywords)
    assert out.loss.requires_grad and torch.equal(_bits(out.loss.detach()), _bits(run(case, cuda).loss))
    out.loss.backward()
    assert excess(score.grad, g["gradient64"]) <= 0.0 and torch.equal(_bits(score.grad), _bits(out.gradient))
    score.grad = None
    (3.0 * kernels.regression_loss(score, **keywords).loss).backward()
    assert torch.equal(score.grad, 3.0 * out.gradient)
    assert not kernels.regression_loss(s, **keywords).loss.requires_grad


@pytest.mark.parametrize("case", WHOLE_CALL_CASES)
def test_the_whole_call_in_reference_mode_against_the_reference(case, cuda, monkeypatch):
    g = fixture(case)
    net = mlp(g).to(cuda)
    r = regularizer(case, weight=float(g["weight"])).to(cuda)
    assert r.rng_mode == "reference"
    batch = augmented_batch(g, cuda)
    forwards = []
    target_class = type(r.target_score_network)
    original = target_class._forward_unchecked
    monkeypatch.setattr(target_class, "_forward_unchecked",
                        lambda self, *a, **k: (forwards.append(self), original(self, *a, **k))[1])
    torch.manual_seed(int(g["seed"]))
    weighted = r.compute_weighted_regularizer_loss(net, batch, current_epoch=0)
    next_rand = torch.rand(1)
    used = r.last_call
    # the reference's draws on the CPU generator: the coordinates bit for bit, and the state it leaves behind
    assert np.array_equal(used["relative_coordinates"].cpu().numpy(), g["drawn_X"]) and used["relative_coordinates"].device == cuda
    assert np.array_equal(next_rand.numpy(), g["next_rand"])
    # the fused analytical path runs no target forward
    fused = case != "equivariant"
    assert used["path"] == ("kernel" if fused else "network") and len(forwards) == (0 if fused else 1)
    assert batch[NOISY_AXL_COMPOSITION].X is not used["relative_coordinates"]           # the caller's batch is left as it was
    # the regularized network's score: the MLP's binary32 forward, at the bar of the MLP's own GPU tests
    torch.testing.assert_close(used["normalized_scores"].detach().cpu(), torch.from_numpy(g["s"]), rtol=1e-4, atol=1e-5)
    target = used["target_normalized_scores"]
    if fused:
        print(f"{case} target: {fraction(target, g['target64']):.3f} of the bound")
        assert excess(target, g["target64"]) <= 0.0
        expected = formula64(used["normalized_scores"].detach().cpu().numpy(), g["target64"])
    else:
        # the equivariant network's own forward: the bars of tests/test_equivariant_analytical_gpu.py against binary64
        got = target.cpu().numpy().astype(np.float64)
        print(f"{case} target: rel-L2 vs binary64 {_rel(got, g['target64']):.2e}")
        assert _rel(got, g["target64"]) <= BAR_CASE and (_per_structure(got, g["target64"]) <= BAR_STRUCTURE).all()
        expected = formula64(used["normalized_scores"].detach().cpu().numpy(), target.cpu().numpy())
    loss = used["loss"].detach()
    print(f"{case}: loss {float(loss):.7f} (the reference's {float(g['loss']):.7f}), {fraction(loss, expected['loss']):.3f} of the bound")
    for name in ("gradient", "per_structure", "loss"):
        assert excess(used[name].detach(), expected[name]) <= 0.0, name
    assert weighted.dim() == 0 and torch.equal(weighted.detach(), float(g["weight"]) * loss)
    assert excess(weighted.detach(), float(g["weight"]) * expected["loss"]) <= 0.0
    np.testing.assert_allclose(float(loss), float(g["loss"]), rtol=1e-4)
    np.testing.assert_allclose(float(weighted.detach()), float(g["weighted_loss"]), rtol=1e-4)
    kernels.raise_analytical_status(r.status)
    assert int(r.status.item()) == 0


def test_the_weighted_loss_carries_the_weight_to_the_score(cuda):
    g = fixture("analytical")
    weight = float(g["weight"])
    r = regularizer("analytical", weight=weight).to(cuda)
    batch = augmented_batch(g, cuda)
    score = torch.from_numpy(g["s"]).to(cuda).requires_grad_()

    class Fixed(torch.nn.Module):
        def _check_batch(self, batch):
            pass

        def forward(self, batch):
            from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL
            return AXL(A=None, X=score, L=None)

    torch.manual_seed(int(g["seed"]))
    weighted = r.compute_weighted_regularizer_loss(Fixed(), batch, current_epoch=0)
    assert weighted.requires_grad
    weighted.backward()
    assert torch.equal(score.grad, weight * r.last_call["gradient"])
    assert excess(r.last_call["gradient"], formula64(g["s"], g["target64"])["gradient"]) <= 0.0
    # and through a real network: the loss reaches the parameters
    net = mlp(g).to(cuda)
    torch.manual_seed(int(g["seed"]))
    r.compute_weighted_regularizer_loss(net, batch, current_epoch=0).backward()
    parameters = [p for p in net.parameters() if p.grad is not None]
    assert parameters and any(bool(p.grad.abs().sum() > 0) for p in parameters)
    used = r.last_call
    upstream = weight * used["gradient"]
    modified = dict(batch)
    modified[NOISY_AXL_COMPOSITION] = batch[NOISY_AXL_COMPOSITION]._replace(X=used["relative_coordinates"])
    expected = torch.autograd.grad(net(modified, conditional=False).X, parameters, grad_outputs=upstream, allow_unused=True)
    for p, e in zip(parameters, expected):
        if e is not None:
            torch.testing.assert_close(p.grad, e, rtol=1e-4, atol=1e-7)


@pytest.mark.parametrize("case", ["analytical_perm", "equivariant"])
def test_device_mode_draws_on_the_device(case, cuda, monkeypatch):
    g = fixture(case)
    net = mlp(g).to(cuda)
    batch = augmented_batch(g, cuda)
    host_draw = torch.rand

    def no_host_coordinates(*size, **keywords):
        assert size == (1,), f"torch.rand{size}: the coordinates were drawn on the host"
        return host_draw(*size, **keywords)
    monkeypatch.setattr(module.torch, "rand", no_host_coordinates)
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (_ for _ in ()).throw(AssertionError("a host copy was made")))
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (_ for _ in ()).throw(AssertionError("a host read was made")))
    drawn, losses = [], []
    for seed in (5, 5, 6):
        r = regularizer(case, rng_mode="device", seed=seed).to(cuda)
        for _ in range(2):
            with torch.no_grad():
                losses.append(r.compute_regularizer_loss(net, batch))
            drawn.append(r.last_call["relative_coordinates"])
        assert r._call_counter == 2
    monkeypatch.undo()
    assert all(x.device == cuda and x.shape == (B, N, D) and x.dtype == torch.float32 for x in drawn)
    assert all(bool(((x >= 0.0) & (x < 1.0)).all()) for x in drawn) and all(bool(torch.isfinite(v)) for v in losses)
    # the same seed and call give the same bits; another call or seed another draw
    assert torch.equal(_bits(drawn[0]), _bits(drawn[2])) and torch.equal(_bits(drawn[1]), _bits(drawn[3]))
    assert torch.equal(_bits(losses[0]), _bits(losses[2])) and torch.equal(_bits(losses[1]), _bits(losses[3]))
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[0], drawn[4])
    kernels.raise_analytical_status(r.status)
    with pytest.raises(ValueError, match="rng_mode"):
        regularizer(case, rng_mode="philox").to(cuda).compute_regularizer_loss(net, batch)
