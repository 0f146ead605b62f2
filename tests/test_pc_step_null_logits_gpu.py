"""mdx_pc_step_update without logits.  With ONE atom type (C = 2) the network's logits are (finite, -inf) -- the MASK logit is
forced to -inf -- and the update makes the same of every finite first logit; a null pointer stands for them.  A, X and L of
the null call equal those of calls with several finite values, in predictor and corrector steps, with the device RNG and
with host draws, greedy and not, fixed lattice and free.  With C = 3 a null pointer is refused.  B = 3, N = 5."""
import warnings

import pytest
import torch

import cases
from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MDX_CORRECTOR, MDX_PREDICTOR, PcFlags, Rng
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_scheduler import NoiseScheduler

pytestmark = pytest.mark.gpu

B, N, T = 3, 5, 6


def _tables(device, num_classes):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return NoiseScheduler(NoiseParameters(**cases.noise_ns(T)), num_classes=num_classes, device=device).tables


def _inputs(device, C, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, C, (B, N), generator=g)
    a[0] = C - 1                                              # one structure fully masked (the greedy rule looks at that)
    x = torch.rand(B, N, 3, generator=g)
    lat = torch.tensor([5.43, 5.43, 5.43, 0.0, 0.0, 0.0]).repeat(B, 1)
    score_x = torch.randn(B, N, 3, generator=g)
    score_l = torch.randn(B, 6, generator=g)
    u01 = torch.rand(B, N, C, generator=g).clip(min=1e-8)
    draws = dict(z=torch.randn(B, N, 3, generator=g), gumbel=-torch.log(-torch.log(u01)), u=torch.rand(B, N, generator=g),
                 z_lattice=torch.randn(B, 6, generator=g))
    to = lambda t: t.to(device).contiguous()
    return to(a), to(x), to(lat), to(score_x), to(score_l), {k: to(v) for k, v in draws.items()}


def _update(sched, mode, index_i, flags, fixed, a, x, lat, logits, score_x, score_l, draws, host_draws):
    a_out, x_out, l_out = torch.empty_like(a), torch.empty_like(x), torch.empty_like(lat)
    status = torch.zeros(1, dtype=torch.int32, device=x.device)
    d = draws if host_draws else dict(z=None, gumbel=None, u=None, z_lattice=None)
    rng = Rng(0, 0, 2, 0, 0, None) if host_draws else Rng(20250815, 3, 2, 0 if mode == MDX_PREDICTOR else 1, 0, None)
    kernels.pc_step_update(sched, mode, index_i, None, flags, a, x, lat, logits, score_x, None if fixed else score_l,
                           d["z"], d["gumbel"], d["u"], None if fixed else d["z_lattice"], rng, a_out, x_out,
                           lat if fixed else l_out, status)
    torch.cuda.synchronize()
    return a_out, x_out, lat if fixed else l_out, int(status.item())


@pytest.mark.parametrize("host_draws", [False, True])
@pytest.mark.parametrize("mode,index_i", [(MDX_PREDICTOR, T), (MDX_PREDICTOR, 3), (MDX_PREDICTOR, 1), (MDX_CORRECTOR, 2),
                                          (MDX_CORRECTOR, 0)])
@pytest.mark.parametrize("greedy,one,fixed", [(False, False, True), (True, True, True), (True, False, False)])
def test_null_logits_equal_any_finite_logit(cuda, host_draws, mode, index_i, greedy, one, fixed):
    C = 2
    sched = _tables(cuda, C)
    flags = PcFlags(int(greedy), int(one), int(fixed), 1, 1e-8)          # (the corrector updates the types too)
    a, x, lat, score_x, score_l, draws = _inputs(cuda, C, seed=17 + index_i)
    got = _update(sched, mode, index_i, flags, fixed, a, x, lat, None, score_x, score_l, draws, host_draws)
    for l0 in (0.0, -7.25, 3.0e4, 1.0e-30):
        logits = torch.empty(B, N, C, device=cuda)
        logits[..., 0] = l0 * torch.linspace(0.5, 1.5, N, device=cuda)                # not the same value on every atom
        logits[..., 1] = -float("inf")
        want = _update(sched, mode, index_i, flags, fixed, a, x, lat, logits, score_x, score_l, draws, host_draws)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
        assert got[3] == want[3]
    assert not torch.equal(got[1], x)                                               # the step did run


def test_null_logits_with_more_classes_are_refused(cuda):
    C = 3
    sched = _tables(cuda, C)
    flags = PcFlags(0, 0, 1, 1, 1e-8)
    a, x, lat, score_x, score_l, draws = _inputs(cuda, C, seed=5)
    with pytest.raises(_hip.MdxError, match=rf"status {_hip.ERR_INVALID_ARG}\b"):
        _update(sched, MDX_PREDICTOR, 3, flags, True, a, x, lat, None, score_x, score_l, draws, False)
    logits = torch.randn(B, N, C, device=cuda)
    logits[..., C - 1] = -float("inf")
    _update(sched, MDX_PREDICTOR, 3, flags, True, a, x, lat, logits, score_x, score_l, draws, False)    # with them: accepted


def test_a_step_that_leaves_the_types_alone_needs_none(cuda):
    """(as before: update_atom_types = 0 never read the logits)"""
    sched = _tables(cuda, 3)
    flags = PcFlags(0, 0, 1, 0, 1e-8)
    a, x, lat, score_x, score_l, draws = _inputs(cuda, 3, seed=6)
    a_out, x_out, _, status = _update(sched, MDX_CORRECTOR, 2, flags, True, a, x, lat, None, score_x, score_l, draws, False)
    assert status == 0 and not torch.equal(x_out, x)
