"""The consistency regularizer without a GPU: the modules and their parameter objects, the host-side methods against the
reference's recorded indices, the refusal of host tensors, the C ABI's new entry, and the fixtures' own float64 agreement."""
import dataclasses

import numpy as np
import pytest
import torch

from consistency_cases import (B, D, N, OPERAND_CASES, STEPS, T, WHOLE_CALL_CASES, augmented_batch, fixture, formula64, host_noise,
                               mlp, numpy_score, regularizer)
from denoising_loss_cases import excess, fraction

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION, TIME
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers import consistency_regularizer as module
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers.consistency_regularizer import (
    ConsistencyRegularizer, ConsistencyRegularizerParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers.regularizer import Regularizer, RegularizerParameters


def test_the_entry_is_in_the_abi():
    assert "mdx_consistency_loss" in _hip.ABI_SYMBOLS and _hip.ABI_VERSION == 14
    f = _hip.ABI.functions["mdx_consistency_loss"]
    assert f.streamed and f.params[-2] == ("uint32_t*", "status")
    kinds = dict((name, kind) for kind, name in f.params)
    # the sigmas are device words: nothing is read on the host
    assert kinds["sigma_start"] == kinds["sigma_end"] == "const float*" and kinds["sigma_stride"] == "int"
    assert kinds["target"] == kinds["gradient"] == kinds["per_structure"] == kinds["loss"] == "float*"
    assert hasattr(_hip.lib(), "mdx_consistency_loss")


def test_names_and_defaults():
    fields = {f.name: f.default for f in dataclasses.fields(RegularizerParameters)}
    assert fields["regularizer_lambda_weight"] == 1.0 and fields["number_of_burn_in_epochs"] == 0
    assert fields["type"] is dataclasses.MISSING
    fields = {f.name: f.default for f in dataclasses.fields(ConsistencyRegularizerParameters)}
    assert fields["type"] == "consistency" and fields["kmax_target_score"] == 4 and fields["analytical_score_network_parameters"] is None
    assert all(fields[name] is dataclasses.MISSING for name in ("maximum_number_of_steps", "noise_parameters", "sampling_parameters"))
    assert issubclass(ConsistencyRegularizerParameters, RegularizerParameters) and issubclass(ConsistencyRegularizer, Regularizer)
    assert issubclass(Regularizer, torch.nn.Module)
    for name in ("get_augmented_batch_for_fixed_time", "get_partial_trajectory_start_and_end", "generate_starting_composition",
                 "get_score_target", "compute_regularizer_loss", "compute_weighted_regularizer_loss", "can_regularizer_run"):
        assert callable(getattr(ConsistencyRegularizer, name))
    r = regularizer()
    assert r.can_regularizer_run() is True and r.weight == 1.0 and r.maximum_number_of_steps == STEPS and r.kmax_target_score == 4
    assert r.analytical_score_network is None
    assert isinstance(regularizer(fixture("analytical")).analytical_score_network, module.AnalyticalScoreNetwork)
    with pytest.raises(NotImplementedError, match="child class"):
        Regularizer(RegularizerParameters(type="none")).compute_regularizer_loss(None, {})


def test_the_weight_must_be_positive_and_burn_in_returns_zero():
    with pytest.raises(AssertionError, match="weight must be positive"):
        RegularizerParameters(type="any", regularizer_lambda_weight=0.0)
    with pytest.raises(AssertionError, match="weight must be positive"):
        regularizer(weight=-1.0)
    r = regularizer()
    r.number_of_burn_in_epochs = 2
    for epoch in (0, 1):          # neither the network nor the batch is looked at
        out = r.compute_weighted_regularizer_loss(None, None, current_epoch=epoch)
        assert isinstance(out, torch.Tensor) and out.dim() == 0 and float(out) == 0.0


@pytest.mark.parametrize("steps", [1, 3, 12])
def test_partial_trajectory_start_and_end_over_the_schedule(steps):
    """The reference's own sweep (tests/regularizers/test_consistency_regularizer.py:131-159): every start index with a jitter
    of +-5e-7 on its time."""
    noise = host_noise(fixture("mlp"))
    r = regularizer(steps=steps)
    jitter = 1e-6 * (torch.rand(T, generator=torch.Generator().manual_seed(3)) - 0.5)
    for start, delta in zip(range(1, T + 1), jitter):
        end = max(start - steps, 0)
        got_start, got_end, end_time, end_sigma = r.get_partial_trajectory_start_and_end(noise.time[start - 1] + delta, noise)
        assert (got_start, got_end) == (start, end)
        if end == 0:
            assert end_time == 0.0 and end_sigma == 0.0 and isinstance(end_time, float) and isinstance(end_sigma, float)
        else:
            assert end_time == noise.time[end - 1] and end_sigma == noise.sigma[end - 1]


def test_augmented_batch_for_a_fixed_time():
    g = fixture("mlp")
    composition = augmented_batch(g, "cpu")[NOISY_AXL_COMPOSITION]
    batch = regularizer().get_augmented_batch_for_fixed_time(composition, 0.25, torch.tensor(0.125))
    assert set(batch) == {NOISY_AXL_COMPOSITION, NOISE, TIME, CARTESIAN_FORCES}
    assert batch[NOISY_AXL_COMPOSITION] is composition
    assert batch[TIME].shape == batch[NOISE].shape == (B, 1) and batch[TIME].dtype == batch[NOISE].dtype == torch.float32
    assert bool((batch[TIME] == 0.25).all()) and bool((batch[NOISE] == 0.125).all())
    assert batch[CARTESIAN_FORCES].shape == (B, N, D) and not bool(batch[CARTESIAN_FORCES].any())


def test_the_starting_composition_repeats_one_element():
    g = fixture("mlp")
    composition = augmented_batch(g, "cpu")[NOISY_AXL_COMPOSITION]
    lattice = composition.L + torch.arange(B).reshape(B, 1)
    r = regularizer()
    torch.manual_seed(11)
    start = r.generate_starting_composition(AXL(A=composition.A, X=composition.X, L=lattice), 2)
    torch.manual_seed(11)
    assert torch.equal(start.X, torch.rand(B, N, D))              # the reference's draw on the CPU generator
    assert start.X.shape == composition.X.shape and bool(((start.X >= 0) & (start.X < 1)).all())
    assert start.A.shape == (B, N) and start.A.dtype == torch.int64 and bool((start.A == composition.A[2]).all())
    assert start.L.shape == (B, 6) and bool((start.L == lattice[2]).all())


@pytest.mark.parametrize("case", WHOLE_CALL_CASES)
def test_the_recorded_indices_come_out_of_the_host_methods(case):
    g = fixture(case)
    noise, r = host_noise(g), regularizer()
    times = torch.from_numpy(g["batch_time"])[:, 0]
    valid = times > noise.time[STEPS]
    assert valid.tolist() == [False, True, True, True] and bool(valid[int(g["batch_index"])])
    torch.manual_seed(int(g["seed"]))                            # the reference's pick is the first draw of the call
    picked = int(torch.arange(B)[valid][torch.randint(int(valid.sum()), ())])
    assert picked == int(g["batch_index"])
    start, end, end_time, end_sigma = r.get_partial_trajectory_start_and_end(times[picked], noise)
    assert (start, end) == (int(g["start_index"]), int(g["end_index"])) and end > 0
    assert np.array_equal(np.asarray(end_time), g["end_time"]) and np.array_equal(np.asarray(end_sigma), g["end_sigma"])
    assert np.array_equal(times[picked].numpy(), g["start_time"])
    assert np.array_equal(g["batch_noise"][picked, 0], g["start_sigma"])
    # the start X follows the pick on the CPU generator
    composition = augmented_batch(g, "cpu")[NOISY_AXL_COMPOSITION]
    assert np.array_equal(r.generate_starting_composition(composition, picked).X.numpy(), g["start_X"])
    effective = np.sqrt(float(g["start_sigma"])**2 - float(g["end_sigma"])**2)
    assert effective > 0.02


def test_a_batch_without_a_valid_time_gives_zero_without_a_kernel(monkeypatch):
    g = fixture("none_valid")

    def no_kernel(name, *args):
        raise AssertionError(f"{name} was called")
    monkeypatch.setattr(kernels, "call", no_kernel)
    r = regularizer(weight=float(g["weight"]))
    out = r.compute_weighted_regularizer_loss(mlp(seed=1), augmented_batch(g, "cpu"), current_epoch=0)
    assert isinstance(out, torch.Tensor) and out.dim() == 0 and float(out) == 0.0 == float(g["weighted_loss"])
    assert r.last_call is None and r.status is None


def test_host_tensors_are_refused():
    g = fixture("mlp")
    r = regularizer()
    with pytest.raises(MdxError, match="no CPU fallback"):
        r.compute_weighted_regularizer_loss(mlp(g), augmented_batch(g, "cpu"), current_epoch=0)
    x = torch.from_numpy(g["start_X"])
    start, end = AXL(A=None, X=x, L=None), AXL(A=None, X=torch.from_numpy(g["end_X"]), L=None)
    with pytest.raises(MdxError, match="no CPU fallback"):
        r.get_score_target(start, end, 0.1, 0.05)
    with pytest.raises(MdxError, match="no CPU fallback"):
        kernels.consistency_loss(x, x, x, sigma_start=0.1, sigma_end=0.05)
    with pytest.raises(MdxError, match="no CPU fallback"):
        kernels.consistency_loss(x, x, sigma_start=torch.tensor(0.1), sigma_end=0.05)


@pytest.mark.parametrize("case", OPERAND_CASES)
def test_a_float64_restatement_agrees_with_the_fixture(case):
    """consistency_cases.formula64 on numpy_score, rounded once to binary32, is within the GPU tests' bound of the reference's
    binary64 record: the bound holds for an evaluation that shares no code with the reference or the kernel."""
    g = fixture(case)
    out = formula64(g["x_start"], g["x_end"], g["s"], g["sigma_start"], g["sigma_end"], int(g["kmax"]), numpy_score)
    for name in ("target", "per_structure", "loss", "gradient"):
        rounded, reference64 = out[name].astype(np.float32), g[name + "64"]
        print(f"{case} {name}: {fraction(rounded, reference64):.3f} of the bound")
        assert excess(rounded, reference64) <= 0.0, name
    # the condition the fixtures were drawn under: no reduced value is a cancellation
    assert np.all(np.abs(g["per_structure64"]) >= 1e-6 * g["magnitude_per_structure64"])
    assert abs(g["loss64"]) >= 1e-6 * g["magnitude64"]


def test_what_the_operand_cases_hold():
    threshold = 1.0 / np.sqrt(2.0 * np.pi)
    effective = lambda g: np.sqrt(g["sigma_start"].astype(np.float64)**2 - g["sigma_end"].astype(np.float64)**2)
    assert effective(fixture("ewald")).min() > threshold and effective(fixture("n5_d3")).max() < threshold
    assert float(fixture("end_zero")["sigma_end"][0]) == 0.0 and int(fixture("kmax1")["kmax"]) == 1
    per_structure = fixture("per_structure_sigma")
    assert per_structure["sigma_start"].shape == per_structure["sigma_end"].shape == (3,)
    assert (effective(per_structure) > threshold).tolist() == [False, True, False]
    assert [fixture(case)["x_start"][0].size for case in ("n1_d1", "n5_d3", "n65_d2", "n216_d3")] == [1, 15, 130, 648]
    g = fixture("placed")
    difference = g["x_start"][0].astype(np.float64) - g["x_end"][0].astype(np.float64)
    assert np.all(difference[0] == 0.0) and np.all(np.abs(difference[1]) == 0.5)
    assert np.all((difference[2] < 0.0) & (difference[2] > -1e-19)) and np.all(difference[3] == 1.0 - 2.0**-24)
    assert np.all(g["target64"][0, :3] == 0.0) and np.all(g["target64"][0, 3] > 0.0)
