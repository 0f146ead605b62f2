"""The denoising loss's gradient without a GPU: the C ABI's new entry, the Python surface, what the fixtures hold, and the closed
form of include/mdx_hip.h restated in float64 numpy against every fixture element at 1/16 of the GPU test's bound -- a
binary64 evaluation in another operation order than torch's autograd meets the bound with room for the kernel's one rounding."""
import inspect

import numpy as np
import pytest

from denoising_gradient_cases import ALGORITHMS, CASES, GRADIENTS, LARGE, closed_form, gradient_fixture, operands

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, loss


def test_the_entry_is_in_the_abi():
    assert "mdx_denoising_loss_gradient" in _hip.ABI_SYMBOLS and _hip.ABI_VERSION == 14
    forward, gradient = _hip.ABI.functions["mdx_denoising_loss"], _hip.ABI.functions["mdx_denoising_loss_gradient"]
    # the forward's arguments in the same order, six more, then status and the stream last as everywhere
    assert gradient.params[:len(forward.params) - 2] == forward.params[:-2] and gradient.params[-2:] == forward.params[-2:]
    assert gradient.params[len(forward.params) - 2:-2] == (
        ("double", "batch_divisor"), ("float*", "gradient_x"), ("float*", "gradient_a"), ("float*", "gradient_l"),
        ("double*", "structure_sums"), ("float*", "loss"))
    assert gradient.streamed and hasattr(_hip.lib(), "mdx_denoising_loss_gradient")
    text = open(_hip.HEADER_PATH).read()
    assert "MDX_API int mdx_denoising_loss_gradient(" in text


def test_the_python_surface():
    assert inspect.signature(loss.denoising_loss).parameters["differentiable"].default is False
    assert list(inspect.signature(loss.training_loss).parameters) == [
        "axl_network", "noised_batch", "loss_parameters", "regularizer", "current_epoch", "kmax_target_score", "conditional"]
    assert inspect.signature(loss.training_loss).parameters["current_epoch"].default == 0
    fields = kernels.DenoisingLossGradient._fields
    assert fields == kernels.DenoisingLoss._fields + ("gradient_x", "gradient_a", "gradient_l", "loss")
    assert inspect.signature(kernels.denoising_loss_and_gradient).parameters["batch_divisor"].default is None
    with pytest.raises(TypeError, match="unexpected keyword arguments \\['sigma_x'\\]"):
        kernels.denoising_loss_and_gradient(sigma_x=None)


def test_what_the_fixtures_hold():
    for case in CASES:
        g, o = gradient_fixture(case), operands(case)
        C, N, D, P = (int(v) for v in o["shape"])
        assert np.array_equal(o["time_indices"], np.arange(12))              # one structure at time index 0, eleven above
        for algorithm in ALGORITHMS:
            shapes = dict(gradient_x=(12, N, D), gradient_a=(12, N, C), gradient_l=(12, P), loss=())
            for name, shape in shapes.items():
                value = g[f"{algorithm}_{name}64"]
                assert value.dtype == np.float64 and value.shape == shape and np.isfinite(value).all(), (case, algorithm, name)
            assert (g[f"{algorithm}_gradient_a64"][..., C - 1] == 0.0).all()
            assert np.abs(g[f"{algorithm}_gradient_x64"]).max() < np.finfo(np.float32).max
        assert np.array_equal(g["mse_gradient_a64"], g["weighted_mse_gradient_a64"])
        assert float(g["softmax_clip_margin"]) >= 1e-6 and float(g["posterior_clip_margin"]) >= 1e-6
    assert (gradient_fixture("c2_n1_d1_p1")["mse_gradient_a64"] == 0.0).all()      # two classes, one of them real: the zero case
    assert tuple(operands(LARGE)["shape"]) == (4, 300, 3, 6) and "x0" in gradient_fixture(LARGE)
    assert 1e32 < np.abs(gradient_fixture("sigma0_control")["weighted_mse_gradient_x64"]).max() < 3.4e38
    assert float(gradient_fixture("clip")["posterior_clip_margin"]) < 1.0          # the clip acts next to decisive elements


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_the_closed_form_in_float64_numpy_meets_a_sixteenth_of_the_bound(case, algorithm):
    g, own = gradient_fixture(case), closed_form(case, algorithm)
    for name in GRADIENTS + ("loss",):
        reference = g[f"{algorithm}_{name}64"]
        assert own[name].shape == reference.shape
        bound = (2.0**-23 * np.abs(reference) + 1e-12) / 16.0
        worst = float((np.abs(own[name] - reference) / bound).max())
        print(f"{case} {algorithm} {name}: {worst:.3e} of a sixteenth of the bound")
        assert worst <= 1.0, (case, algorithm, name, worst)


def test_the_closed_form_scales_with_the_batch_divisor():
    for name, value in closed_form("c3_n5_d3_p6", "mse", batch_divisor=3.0).items():
        assert np.allclose(value * 3.0, closed_form("c3_n5_d3_p6", "mse")[name] * 12.0, rtol=1e-14, atol=0.0)
