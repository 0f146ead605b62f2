"""The fused denoising-loss launch beside the same quantities from the package's other pieces and plain torch on the same GPU.

    python tools/denoising_loss_time.py [--replays R]

  B 512, D 3, C 3 (two elements and MASK), P 6, T 1000, N in 8, 64, 216; a random time index per structure; predictions randn.

Per shape one JSON line:
  kernel_us          `kernels.denoising_loss` (mdx_denoising_loss, one launch, the [T, C, C] tables read at the time indices):
                     50 launches captured into one hipGraph on a side stream after three warm-up launches; one replay between two
                     device events, over 50; R replays, median (min .. max)
  kernel_eager_us    the same call from Python, R calls between two device events (launch overhead and the ten output allocations
                     included)
  torch_chain_us     `torch_chain` below: the reference's flow (models/axl_diffusion_lightning_model.py:243-346) on the pieces the
                     package had before this kernel -- the wrapped-Gaussian score kernel for the coordinates' target, utils/d3pm_utils
                     on one-hot vectors and [B, N, C, C] expand() views of the matrices, torch's mse, softmax, kl_div and means -- in
                     binary32, some sixty launches.  No host read either, so it is captured and timed the same way (one chain per
                     graph); chain_eager_us is R eager calls between two device events
  max_difference     max |aggregate_kernel - aggregate_chain| / aggregate over the batch: the chain is binary32"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusion_for_multi_scale_molecular_dynamics_amd import kernels  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_scheduler import NoiseScheduler  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.utils.d3pm_utils import (class_index_to_onehot,  # noqa: E402
                                                                               get_probability_at_previous_time_step)

BATCH, DIMENSION, CLASSES, LATTICE, STEPS, ATOMS = 512, 3, 3, 6, 1000, (8, 64, 216)
KMAX, CE_WEIGHT, EPS = 4, 0.001, 1e-8
PER_GRAPH = 50


def torch_chain(c):
    """(aggregate [B], unreduced losses) by the reference's flow in binary32 on device tensors."""
    B, N, D = c["x0"].shape
    sigmas = c["sigma"].reshape(-1, 1, 1).expand(B, N, D)
    delta = torch.remainder(c["xt"] - c["x0"], 1.0)
    delta = torch.where(delta == 1.0, torch.zeros_like(delta), delta)
    target_x = kernels.wrapped_gaussian_sigma_normalized_score(delta, sigmas.contiguous(), KMAX)
    sigma_n = c["sigma"].reshape(-1, 1) / torch.pow(torch.ones_like(c["l0"]) * N, 1 / LATTICE)
    target_l = -(c["lt"] - c["l0"]) / sigma_n
    loss_x = torch.nn.functional.mse_loss(c["predicted_x"], target_x, reduction="none")
    loss_l = torch.nn.functional.mse_loss(c["predicted_l"], target_l, reduction="none")
    one_hot_a0, one_hot_at = class_index_to_onehot(c["a0"], CLASSES), class_index_to_onehot(c["at"], CLASSES)
    indices = c["time_indices"]
    matrices = [table.index_select(0, indices).unsqueeze(1).expand(B, N, CLASSES, CLASSES)
                for table in (c["q_matrices"], c["q_bar_matrices"], c["q_bar_tm1_matrices"])]
    q = get_probability_at_previous_time_step(one_hot_a0, one_hot_at, *matrices, small_epsilon=EPS)
    p = get_probability_at_previous_time_step(c["logits"], one_hot_at, *matrices, small_epsilon=EPS,
                                              probability_at_zeroth_timestep_are_logits=True)
    log_p = torch.log(p.clip(min=EPS))
    vb = torch.nn.functional.kl_div(log_p, q, reduction="none")
    first = (indices == 0).reshape(-1, 1, 1)
    vb = torch.where(first, -log_p * one_hot_a0, vb)
    nll = -torch.nn.functional.log_softmax(c["logits"], dim=-1)
    nll[..., -1] = 0.0
    loss_a = vb + CE_WEIGHT * one_hot_a0 * nll
    aggregate = loss_x.mean(dim=(-2, -1)) + loss_l.mean(dim=-1) + loss_a.mean(dim=(-2, -1))
    return aggregate, (loss_a, loss_x, loss_l)


def inputs(N, device):
    g = torch.Generator().manual_seed(29 + N)
    tables = NoiseScheduler(NoiseParameters(total_time_steps=STEPS, sigma_min=1e-3, sigma_max=0.5), num_classes=CLASSES, device=device).tables
    indices = torch.randint(0, STEPS, (BATCH,), generator=g).to(device)
    sigma = tables.sigma[indices].contiguous()
    x0 = torch.rand(BATCH, N, DIMENSION, generator=g).to(device)
    xt = torch.remainder(x0 + sigma.reshape(-1, 1, 1) * torch.randn(BATCH, N, DIMENSION, generator=g).to(device), 1.0)
    xt = torch.where(xt == 1.0, torch.zeros_like(xt), xt)
    a0 = torch.randint(0, CLASSES - 1, (BATCH, N), generator=g).to(device)
    masked = torch.rand(BATCH, N, generator=g).to(device) > tables.alpha_bar[indices].reshape(-1, 1)
    at = torch.where(masked, torch.full_like(a0, CLASSES - 1), a0)
    l0 = (4.0 + 2.0 * torch.rand(BATCH, LATTICE, generator=g)).to(device)
    sigma_n = sigma / kernels.root_of_atom_count(N, LATTICE)
    lt = l0 + sigma_n.reshape(-1, 1) * torch.randn(BATCH, LATTICE, generator=g).to(device)
    logits = (3.0 * torch.randn(BATCH, N, CLASSES, generator=g)).to(device)
    logits[..., -1] = -torch.inf
    return dict(x0=x0, xt=xt.contiguous(), predicted_x=torch.randn(BATCH, N, DIMENSION, generator=g).to(device), sigma=sigma, a0=a0,
                at=at.contiguous(), logits=logits, time_indices=indices, q_matrices=tables.q_matrix, q_bar_matrices=tables.q_bar_matrix,
                q_bar_tm1_matrices=tables.q_bar_tm1_matrix, l0=l0, lt=lt, predicted_l=torch.randn(BATCH, LATTICE, generator=g).to(device),
                sigma_n=sigma_n.contiguous())


def spread(values):
    return dict(median=round(statistics.median(values), 2), min=round(min(values), 2), max=round(max(values), 2))


def captured_us(function, per_graph, replays):
    """`function` captured per_graph times into one hipGraph on a side stream; microseconds of one call, one value per replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        function()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(per_graph):
                function()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graph.replay()
    torch.cuda.synchronize()
    out = []
    for _ in range(replays):
        start.record()
        graph.replay()
        stop.record()
        torch.cuda.synchronize()
        out.append(1000.0 * start.elapsed_time(stop) / per_graph)
    return out


def eager_us(function, replays):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        function()
    stop.record()
    torch.cuda.synchronize()
    return 1000.0 * start.elapsed_time(stop) / replays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    for N in ATOMS:
        c = inputs(N, device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        fused = lambda: kernels.denoising_loss(**c, kmax=KMAX, ce_weight=CE_WEIGHT, eps=EPS, status=status)  # noqa: E731
        chain = lambda: torch_chain(c)  # noqa: E731
        with torch.no_grad():
            for _ in range(3):
                out = fused()
                aggregate, _ = chain()
            torch.cuda.synchronize()
            assert int(status.item()) == 0
            difference = float(((out.per_structure[:, 3] - aggregate).abs() / aggregate.abs()).max())
            kernel_us = captured_us(fused, PER_GRAPH, args.replays)
            kernel_eager_us = eager_us(fused, args.replays)
            chain_us = captured_us(chain, 1, args.replays)
            chain_eager_us = eager_us(chain, args.replays)
        print(json.dumps(dict(batch=BATCH, atoms=N, dimension=DIMENSION, classes=CLASSES, kernel_us=spread(kernel_us),
                              kernel_eager_us=round(kernel_eager_us, 2), torch_chain_us=spread(chain_us),
                              chain_eager_us=round(chain_eager_us, 2), max_difference=difference)), flush=True)


if __name__ == "__main__":
    main()
