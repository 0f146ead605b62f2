"""Time the sampler iteration of `algorithm: adaptive_corrector` at the C3 shape, or at the C2 (MLP) shape with --mlp.

C3 = Si 2x2x2 (N 64), EGNN 4 x 256 with the radius graph and the split-f16 edge chain, batch 512, M 2, rng_mode device --
bench.py's C3 network and settings under AdaptiveCorrectorGenerator.  --mlp: bench.py's C2 network and settings (N 8, MLP
template, batch 1024, M 1), where the network is small and the launches between the forward and the update dominate.

By default the iteration runs on the device-resident loop, captured into a hipGraph (use_hip_graph true).  --eager runs the
generator's eager loop instead (_guarded_iteration per time index, what sample() does without a graph): the only way a tree
from before the adaptive corrector's batch statistics ran in HIP can run, so the same file times both sides of that change.

One JSON line: ms per iteration (host clock around `--steps` iterations that end in a device synchronise, after `--warmup`
iterations), whether the iteration was captured, and the warnings the sampler gave.

    python tools/adaptive_corrector_c3.py --steps 20 --warmup 5 [--mlp] [--eager]
"""
import argparse
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.adaptive_corrector import AdaptiveCorrectorGenerator  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.langevin_generator import IterationLoop  # noqa: E402


class EagerLoop:
    """The generator's eager loop (LangevinGenerator._run_loop without a graph), with bench.advance's wrap-around."""

    def __init__(self, gen, start, total):
        self.gen, self.composition, self.total, self.index = gen, start, total, total - 1
        self.forces = torch.zeros_like(start.X)
        self.graph = None

    def advance(self, iterations):
        for _ in range(iterations):
            self.composition = self.gen._guarded_iteration(self.composition, self.index, self.forces)
            self.index = self.index - 1 if self.index > 0 else self.total - 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mlp", action="store_true", help="the C2 network and settings (MLP, batch 1024) instead of C3's")
    ap.add_argument("--eager", action="store_true", help="the generator's eager loop (no device-resident loop, no graph)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    device = torch.device("cuda:0")
    name = "C2" if args.mlp else "C3"
    w = bench.WORKLOADS[name]
    batch, T = w["batch"], w["noise"]["total_time_steps"]
    _, noise, sampling, net = bench.build_generator(w, device, 0, batch, use_graph=False)
    if not args.mlp:
        net.edge_chain_precision = "f16x3"
    sampling.algorithm = "adaptive_corrector"
    sampling.use_hip_graph = not args.eager
    gen = AdaptiveCorrectorGenerator(noise, sampling, net)
    with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        gen._prepare(device)
        gen._begin_call(device)
        start = gen.initialize(batch, device)
        if args.eager:
            loop = EagerLoop(gen, start, T)
            advance = lambda n: loop.advance(n)                       # noqa: E731
        else:
            loop = IterationLoop(gen, start, T, use_graph=gen._capture_safe(start))
            advance = lambda n: bench.advance(loop, n, T)             # noqa: E731
        advance(args.warmup)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        advance(args.steps)
        torch.cuda.synchronize(device)
        elapsed = time.perf_counter() - t0
        gen.check_status()
    ms = elapsed * 1e3 / args.steps
    print(json.dumps(dict(workload=name, algorithm="adaptive_corrector", batch=batch, steps=args.steps, warmup=args.warmup,
                          ms_per_iteration=round(ms, 4), structures_per_s_at_T=round(batch / (T * ms * 1e-3), 3),
                          captured=loop.graph is not None, eager=args.eager,
                          f16_range_fallbacks=gen.f16_range_fallbacks,
                          warnings=sorted({str(c.message)[:120] for c in caught}))))


if __name__ == "__main__":
    main()
