"""The fused consistency launch beside the same quantities from the package's other pieces and plain torch on the same GPU, and
one whole call of the consistency regularizer.

    python tools/consistency_loss_timing.py [--replays R] [--calls K]

  kernel    B 512, D 3, N in 8, 64, 216; sigma 0.1 -> 0.04 as device words; x_start, x_end uniform, the score randn.  Per shape one
            JSON line:
    kernel_us          `kernels.consistency_loss` (mdx_consistency_loss: one launch per structure set and the one-thread total):
                       50 calls captured into one hipGraph on a side stream after a warm-up call; one replay between two device
                       events, over 50; R replays, median (min .. max)
    kernel_eager_us    the same call from Python, R calls between two device events (launch overhead, the five output allocations)
    torch_chain_us     `torch_chain` below: the reference's flow (regularizers/consistency_regularizer.py:208-306) on what the
                       package had before this kernel -- torch's remainder for the wrap, `kernels.wrapped_gaussian_sigma_normalized_
                       score` for the score, torch for sigma_eff, the scaling, the sums and 2 (s - t) / B -- in binary32.  No host
                       read either: captured and timed the same way (one chain per graph); chain_eager_us is R eager calls
    max_difference     |loss_kernel - loss_chain| / |loss_kernel|: the chain is binary32
  call      bench.py's C2 network (MLP, N 8, B 1024) and C3 network (EGNN 4 x 256, N 64, B 512) with their noise and sampling
            settings, maximum_number_of_steps 5, rng_mode device; a batch whose times are schedule entries drawn from the upper half
            of the schedule.  compute_regularizer_loss under no_grad, K calls after two warm-up calls, each between a device
            synchronisation and the next; ms per call, median (min .. max), with `use_hip_graph` false (eager) and true (captured
            loop, kept across calls)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd import kernels  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, CARTESIAN_FORCES, NOISE, NOISY_AXL_COMPOSITION, TIME  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_scheduler import NoiseScheduler  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.regularizers.consistency_regularizer import (  # noqa: E402
    ConsistencyRegularizer, ConsistencyRegularizerParameters)

BATCH, DIMENSION, ATOMS, KMAX = 512, 3, (8, 64, 216), 4
SIGMA_START, SIGMA_END = 0.1, 0.04
PER_GRAPH = 50
MAXIMUM_NUMBER_OF_STEPS = 5


def torch_chain(c):
    """(loss, target, gradient) by the reference's flow in binary32 on device tensors."""
    x_start, x_end, s = c["x_start"], c["x_end"], c["s"]
    batch = x_start.shape[0]
    delta = torch.remainder(x_start - x_end, 1.0)
    delta = torch.where(delta == 1.0, torch.zeros_like(delta), delta)
    effective = (c["sigma_start"]**2 - c["sigma_end"]**2).sqrt() * torch.ones_like(x_start)
    target = (c["sigma_start"] / effective) * kernels.wrapped_gaussian_sigma_normalized_score(delta, effective, KMAX)
    loss = torch.sum(s * (s - 2.0 * target)) / batch
    return loss, target, 2.0 * (s - target) / batch


def inputs(N, device):
    g = torch.Generator().manual_seed(31 + N)
    draw = lambda f: f(BATCH, N, DIMENSION, generator=g).to(device)
    word = lambda value: torch.full((1,), value, dtype=torch.float32, device=device)
    return dict(x_start=draw(torch.rand), x_end=draw(torch.rand), s=draw(torch.randn), sigma_start=word(SIGMA_START),
                sigma_end=word(SIGMA_END))


def spread(values, digits=2):
    return dict(median=round(statistics.median(values), digits), min=round(min(values), digits), max=round(max(values), digits))


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


def time_kernel(device, replays):
    for N in ATOMS:
        c = inputs(N, device)
        status = torch.zeros(1, dtype=torch.int32, device=device)
        fused = lambda: kernels.consistency_loss(c["x_start"], c["x_end"], c["s"], sigma_start=c["sigma_start"],  # noqa: E731
                                                 sigma_end=c["sigma_end"], kmax=KMAX, status=status)
        chain = lambda: torch_chain(c)  # noqa: E731
        with torch.no_grad():
            for _ in range(3):
                out = fused()
                loss, _, _ = chain()
            torch.cuda.synchronize()
            assert int(status.item()) == 0
            difference = abs(float(out.loss) - float(loss)) / abs(float(out.loss))
            kernel_us = captured_us(fused, PER_GRAPH, replays)
            kernel_eager_us = eager_us(fused, replays)
            chain_us = captured_us(chain, 1, replays)
            chain_eager_us = eager_us(chain, replays)
        print(json.dumps(dict(batch=BATCH, atoms=N, dimension=DIMENSION, kernel_us=spread(kernel_us),
                              kernel_eager_us=round(kernel_eager_us, 2), torch_chain_us=spread(chain_us),
                              chain_eager_us=round(chain_eager_us, 2), max_difference=difference)), flush=True)


def time_call(name, device, use_graph, calls):
    w = bench.WORKLOADS[name]
    batch, n = w["batch"], w["n_atoms"]
    _, noise, sampling, net = bench.build_generator(w, device, 0, batch, use_graph=use_graph)
    regularizer = ConsistencyRegularizer(ConsistencyRegularizerParameters(
        maximum_number_of_steps=MAXIMUM_NUMBER_OF_STEPS, noise_parameters=noise, sampling_parameters=sampling))
    g = torch.Generator().manual_seed(37)
    composition = AXL(A=torch.zeros(batch, n, dtype=torch.int64, device=device), X=torch.rand(batch, n, 3, generator=g).to(device),
                      L=torch.tensor([w["cell"]] * 3 + [0.0] * 3, device=device).repeat(batch, 1))
    tables = NoiseScheduler(noise, num_classes=w["num_atom_types"] + 1, device=device).tables
    indices = torch.randint(noise.total_time_steps // 2, noise.total_time_steps, (batch,), generator=g).to(device)
    times, sigmas = tables.time[indices].reshape(batch, 1).clone(), tables.sigma[indices].reshape(batch, 1).clone()
    augmented = {NOISY_AXL_COMPOSITION: composition, TIME: times, NOISE: sigmas, CARTESIAN_FORCES: torch.zeros_like(composition.X)}
    torch.manual_seed(41)
    elapsed = []
    with torch.no_grad():
        for k in range(calls + 2):
            torch.cuda.synchronize()
            begin = time.perf_counter()
            loss = regularizer.compute_regularizer_loss(net, augmented)
            torch.cuda.synchronize()
            if k >= 2:
                elapsed.append(1000.0 * (time.perf_counter() - begin))
    kernels.raise_analytical_status(regularizer.status)
    print(json.dumps(dict(workload=name, batch=batch, atoms=n, maximum_number_of_steps=MAXIMUM_NUMBER_OF_STEPS,
                          corrector_steps=w["M"], use_hip_graph=use_graph, call_ms=spread(elapsed, 3), last_loss=float(loss))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--skip-calls", action="store_true", help="the kernel's lines only")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    time_kernel(device, args.replays)
    if not args.skip_calls:
        for name in ("C2", "C3"):
            for use_graph in (False, True):
                time_call(name, device, use_graph, args.calls)


if __name__ == "__main__":
    main()
