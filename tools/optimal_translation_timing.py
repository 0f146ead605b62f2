"""The optimal-translation kernel beside the reference's flow in plain torch on the same GPU.

    python tools/optimal_translation_timing.py [--replays R]

  B 512, D 3, N in 8, 64, 216; half of the structures y = wrap(x + s + N(0, 0.02^2)) (a sample against its sites), half uniform.

Per shape one JSON line:
  kernel_us          `kernels.optimal_translation` (mdx_optimal_translation, one launch): 50 launches captured into one hipGraph on a
                     side stream after three warm-up launches; one replay between two device events, over 50; R replays, median
                     (min .. max)
  kernel_eager_us    the same call from Python, R calls between two device events (launch overhead included)
  torch_chain_us     `torch_chain` below: the reference's flow (transport/optimal_translation.py) restated in plain torch -- crossings,
                     a sort, a cumulative sum, the plateau test, a host read of the candidate count, the gather of the candidates'
                     columns, atan2 displacements, two dense [candidates, B, D] scratch tensors and an argmin.  Its size depends on the
                     data, so it cannot be captured: R eager calls after three warm-ups, each between two device synchronisations,
                     wall clock, median (min .. max)
  candidates         the chain's candidate count over the batch
  max_difference     max |tau_kernel - tau_chain| over the batch: the chain is binary32"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusion_for_multi_scale_molecular_dynamics_amd import kernels  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.transport.distance import get_geodesic_displacements  # noqa: E402

TAU_RANGE_MIN, TAU_RANGE_MAX = -0.5, 0.5
BATCH, DIMENSION, ATOMS = 512, 3, (8, 64, 216)
PER_GRAPH = 50


def torch_chain(x, y):
    """(tau [B, D], number of candidates) by the reference's flow, plain torch on the inputs' device."""
    delta = y - x
    B, N, D = delta.shape
    l0 = torch.floor(delta + TAU_RANGE_MIN + 0.5)
    crossings = -(delta - l0 + TAU_RANGE_MIN)
    ordered = crossings.sort(dim=1).values
    left = torch.cat([torch.full_like(ordered[:, :1], TAU_RANGE_MIN), ordered], dim=1)
    right = torch.cat([ordered, torch.full_like(ordered[:, :1], TAU_RANGE_MAX)], dim=1)
    first = l0.sum(dim=1, keepdim=True)
    plateaus = torch.cat([first, (ordered < TAU_RANGE_MAX).cumsum(dim=1) + first], dim=1)
    rhs = plateaus / N - delta.mean(dim=1, keepdim=True)
    mask = (rhs > left) & (rhs < right)
    structure, _, alpha = mask.nonzero(as_tuple=True)          # the host learns the candidate count here
    taus = rhs[mask]
    displacements = get_geodesic_displacements(x[structure, :, alpha], y[structure, :, alpha] + taus[:, None])
    costs = (displacements**2).sum(dim=1)
    candidates = torch.arange(len(taus), device=x.device)
    tau_matrix = torch.full((len(taus), B, D), torch.inf, device=x.device)
    tau_matrix[candidates, structure, alpha] = taus
    cost_matrix = torch.full((len(taus), B, D), torch.inf, device=x.device)
    cost_matrix[candidates, structure, alpha] = costs
    return tau_matrix.gather(0, cost_matrix.argmin(dim=0).unsqueeze(0)).squeeze(0), len(taus)


def inputs(N, device):
    g = torch.Generator().manual_seed(13 + N)
    x = torch.rand(BATCH, N, DIMENSION, generator=g)
    y = torch.rand(BATCH, N, DIMENSION, generator=g)
    half = BATCH // 2
    y[:half] = torch.remainder(x[:half] + torch.rand(half, 1, DIMENSION, generator=g) + 0.02 * torch.randn(half, N, DIMENSION, generator=g), 1.0)
    y[y == 1.0] = 0.0
    return x.to(device), y.to(device)


def spread(values):
    return dict(median=round(statistics.median(values), 2), min=round(min(values), 2), max=round(max(values), 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    for N in ATOMS:
        x, y = inputs(N, device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        for _ in range(3):
            tau = kernels.optimal_translation(x, y, status=status)
            reference, candidates = torch_chain(x, y)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        difference = float((tau - reference).abs().max())

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            kernels.optimal_translation(x, y, status=status)
            with torch.cuda.graph(graph, stream=side):
                for _ in range(PER_GRAPH):
                    captured = kernels.optimal_translation(x, y, status=status)
        torch.cuda.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        graph.replay()
        torch.cuda.synchronize()
        kernel_us = []
        for _ in range(args.replays):
            start.record()
            graph.replay()
            stop.record()
            torch.cuda.synchronize()
            kernel_us.append(1000.0 * start.elapsed_time(stop) / PER_GRAPH)
        assert torch.equal(captured, tau)

        start.record()
        for _ in range(args.replays):
            kernels.optimal_translation(x, y, status=status)
        stop.record()
        torch.cuda.synchronize()
        eager_us = 1000.0 * start.elapsed_time(stop) / args.replays

        chain_us = []
        for _ in range(args.replays):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            torch_chain(x, y)
            torch.cuda.synchronize()
            chain_us.append(1e6 * (time.perf_counter() - t0))
        print(json.dumps(dict(batch=BATCH, atoms=N, dimension=DIMENSION, kernel_us=spread(kernel_us), kernel_eager_us=round(eager_us, 2),
                              torch_chain_us=spread(chain_us), candidates=candidates,
                              max_difference=difference)), flush=True)


if __name__ == "__main__":
    main()
