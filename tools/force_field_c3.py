"""Time the C3 sampler iteration with a `force_field:` block (radial_cutoff 2.5, strength 5.0) around the benchmark's EGNN.

C3 = Si 2x2x2 (N 64), EGNN 4 x 256 with the radius graph and the split-f16 edge chain, batch 512, M 2, rng_mode device,
use_hip_graph true -- bench.py's C3 generator with ForceFieldAugmentedScoreNetwork around its network.  The iteration is
captured when the wrapped network says it can be (the generator's own test); otherwise it is launched eagerly, as the sampler
would.  One JSON line: ms per iteration (host clock around `--steps` iterations that end in a device synchronise, after
`--warmup` iterations), whether the iteration was captured, and the warnings the sampler gave.  `--plain` times the same
generator without the wrapper; `--eager` launches every iteration (for a kernel trace of one forward, tools/kernel_sequence.py).

    python tools/force_field_c3.py --steps 20 --warmup 5 [--plain] [--eager]
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
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.langevin_generator import (IterationLoop,  # noqa: E402
                                                                                             LangevinGenerator)
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.force_field_augmented_score_network import (  # noqa: E402
    ForceFieldAugmentedScoreNetwork, ForceFieldParameters)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--plain", action="store_true", help="no force-field wrapper (the C3 reference figure)")
    ap.add_argument("--eager", action="store_true", help="launch every iteration eagerly (for a kernel trace of one forward)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    device = torch.device("cuda:0")
    w = bench.WORKLOADS["C3"]
    batch, T = w["batch"], w["noise"]["total_time_steps"]
    gen, noise, sampling, net = bench.build_generator(w, device, 0, batch, use_graph=True)
    net.edge_chain_precision = "f16x3"
    if not args.plain:
        gen = LangevinGenerator(noise, sampling,
                                ForceFieldAugmentedScoreNetwork(net, ForceFieldParameters(radial_cutoff=2.5, strength=5.0)))
    with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        gen._prepare(device)
        gen._begin_call(device)
        start = gen.initialize(batch, device)
        use_graph = not args.eager and gen._capture_safe(start)
        loop = IterationLoop(gen, start, T, use_graph=use_graph)
        bench.advance(loop, args.warmup, T)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        bench.advance(loop, args.steps, T)
        torch.cuda.synchronize(device)
        elapsed = time.perf_counter() - t0
        gen.check_status()
    ms = elapsed * 1e3 / args.steps
    print(json.dumps(dict(workload="C3", force_field=None if args.plain else dict(radial_cutoff=2.5, strength=5.0),
                          batch=batch, steps=args.steps, warmup=args.warmup, ms_per_iteration=round(ms, 3),
                          structures_per_s_at_T=round(batch / (T * ms * 1e-3), 3),
                          captured=getattr(loop, "graph", None) is not None,
                          warnings=sorted({str(c.message)[:120] for c in caught}))))


if __name__ == "__main__":
    main()
