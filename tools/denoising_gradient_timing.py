"""The loss and its three gradients from the fused loss-and-gradient launch beside the three calculators' torch path under
autograd, and the untouched forward launch, on the same GPU.

    python tools/denoising_gradient_timing.py [--rounds R] [--calls K]

  B 512, D 3, C 3 (two elements and MASK), P 6, T 1000, N in 8, 64, 216: the operands of tools/denoising_loss_time.py.

Both sides start from three leaf predictions and end with their .grad filled:
  fused        `kernels.denoising_loss_and_gradient` (mdx_denoising_loss_gradient and the one-workgroup total) and
               `loss.backward()`: the autograd function's three multiplications by grad_output, no second launch
  calculators  what the package had before: the wrapped-Gaussian score kernel for the coordinates' target, then
               `create_loss_calculator(...)`'s three calculators on predictions that require grad -- their plain-torch
               expressions, one-hot vectors and [B, N, C, C] expand() views --, the three means, the mean over the batch,
               `backward()`
Neither makes a host read.  An autograd backward is not captured here, so both are timed as eager calls: after WARMUP rounds,
R rounds that ALTERNATE the two sides, each K calls between two device events; per side the median (min .. max) of the rounds,
microseconds per call.  `forward_us` is `kernels.denoising_loss` (mdx_denoising_loss, the forward instantiation) as
tools/denoising_loss_time.py measures it: 50 launches in one hipGraph, one value per replay.

Per shape one JSON line, with max_difference = the largest |fused gradient - calculators' gradient| over the three, relative to
the largest gradient of its kind (the calculators are binary32), and the two losses."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from denoising_loss_time import ATOMS, BATCH, CE_WEIGHT, CLASSES, EPS, KMAX, LATTICE, PER_GRAPH, captured_us, inputs, spread  # noqa: E402

from diffusion_for_multi_scale_molecular_dynamics_amd import kernels  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.loss import create_loss_calculator  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.loss.loss_parameters import create_loss_parameters  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.utils.d3pm_utils import class_index_to_onehot  # noqa: E402

WARMUP = 3
PREDICTIONS = ("predicted_x", "logits", "predicted_l")


def leaves(c):
    return {name: c[name].detach().clone().requires_grad_() for name in PREDICTIONS}


def fused_step(c, status):
    own = leaves(c)
    out = kernels.denoising_loss_and_gradient(**{**c, **own}, kmax=KMAX, ce_weight=CE_WEIGHT, eps=EPS, status=status)
    out.loss.backward()
    return out.loss.detach(), own


def calculators_step(c, calculator):
    own = leaves(c)
    B, N, D = c["x0"].shape
    sigmas = c["sigma"].reshape(-1, 1, 1).expand(B, N, D)
    with torch.no_grad():
        delta = torch.remainder(c["xt"] - c["x0"], 1.0)
        delta = torch.where(delta == 1.0, torch.zeros_like(delta), delta)
        target_x = kernels.wrapped_gaussian_sigma_normalized_score(delta, sigmas.contiguous(), KMAX)
        target_l = -(c["lt"] - c["l0"]) / c["sigma_n"].reshape(-1, 1)
    loss_x = calculator.X.calculate_unreduced_loss(own["predicted_x"], target_x, sigmas)
    loss_l = calculator.L.calculate_unreduced_loss(own["predicted_l"], target_l, c["sigma"].reshape(-1, 1).expand(B, LATTICE))
    indices = c["time_indices"]
    matrices = [table.index_select(0, indices).unsqueeze(1).expand(B, N, CLASSES, CLASSES)
                for table in (c["q_matrices"], c["q_bar_matrices"], c["q_bar_tm1_matrices"])]
    loss_a = calculator.A.calculate_unreduced_loss(own["logits"], class_index_to_onehot(c["a0"], CLASSES),
                                                   class_index_to_onehot(c["at"], CLASSES), indices, *matrices)
    loss = torch.mean(loss_x.mean(dim=(-2, -1)) + loss_l.mean(dim=-1) + loss_a.mean(dim=(-2, -1)))
    loss.backward()
    return loss.detach(), own


def timed_us(function, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        function()
    stop.record()
    torch.cuda.synchronize()
    return 1000.0 * start.elapsed_time(stop) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    calculator = create_loss_calculator(create_loss_parameters({}))
    for N in ATOMS:
        c = inputs(N, device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        fused = lambda: fused_step(c, status)  # noqa: E731
        calculators = lambda: calculators_step(c, calculator)  # noqa: E731
        loss_fused, own_fused = fused()
        loss_calculators, own_calculators = calculators()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        difference = max(float((own_fused[name].grad - own_calculators[name].grad).abs().max() / own_fused[name].grad.abs().max())
                         for name in PREDICTIONS)
        rounds = dict(fused=[], calculators=[])
        for r in range(WARMUP + args.rounds):
            for name, function in (("fused", fused), ("calculators", calculators)):
                value = timed_us(function, args.calls)
                if r >= WARMUP:
                    rounds[name].append(value)
        with torch.no_grad():
            forward_us = captured_us(lambda: kernels.denoising_loss(**c, kmax=KMAX, ce_weight=CE_WEIGHT, eps=EPS, status=status),
                                     PER_GRAPH, args.rounds)
        print(json.dumps(dict(batch=BATCH, atoms=N, fused_us=spread(rounds["fused"]), calculators_us=spread(rounds["calculators"]),
                              forward_us=spread(forward_us), loss_fused=float(loss_fused), loss_calculators=float(loss_calculators),
                              max_difference=difference)), flush=True)


if __name__ == "__main__":
    main()
