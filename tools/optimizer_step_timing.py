"""The fused optimizer step (FusedAdam: mdx_adam_step, with mdx_gradient_norm when clipping) beside torch.optim.AdamW's three
implementations on the same GPU, at the parameter shapes of the production-size EGNN and of the C2 MLP.

    python tools/optimizer_step_timing.py [--rounds R] [--steps K] [--only fused|torch] [--shapes egnn_c3|mlp_c2] [--out FILE]

Parameter lists with the shapes of tests/nets.py::egnn_c3_net(1) (138 tensors, 4 738 679 parameters) and of bench.py's
mlp_template(1, 8) (BASELINE configs[1]); values and static gradients are seeded, every variant owns its copies.  In ONE process,
after WARMUP steps of each, R rounds that ALTERNATE all variants, each K steps between two device events; per variant the median
(min .. max) of the rounds in microseconds per step.  lr 1e-3, weight_decay 1e-2, max_norm 0.1.

  fused            FusedAdam.step(); "+clip": gradient_clip_val 0.1 (three launches); "+zero": zero_gradients (the same launch)
  torch_default    torch.optim.AdamW as the reference's load_optimizer constructs it (torch picks the implementation)
  torch_foreach    the same with foreach=True
  torch_fused      the same with fused=True
  each torch variant also with clip_grad_norm_(parameters, 0.1) before the step ("+clip") and zero_grad(set_to_none=False)
  after it ("+zero"), where the fused step includes those passes

One JSON line per shape set: per variant the step times, and for the fused variants `arrays` = the binary32 arrays a step must
move (7: read p, g, m, v, write p, m, v; +1 with zeroing; +1 for the norm's read of g) and `gbytes_per_s_of_step_time` = those
bytes over the STEP time between events (launch gaps included: not a kernel's share of peak; the kernels' own times come from a
`rocprofv3 --kernel-trace --stats` run of this tool with `--only fused --shapes egnn_c3`, in a run of its own)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from diffusion_for_multi_scale_molecular_dynamics_amd.models.optimizer import FusedAdam  # noqa: E402

WARMUP, LR, WEIGHT_DECAY, MAX_NORM = 20, 1e-3, 1e-2, 0.1
MODES = ("", "+clip", "+zero", "+clip+zero")


def shape_sets():
    import nets
    from bench import mlp_template
    return {"egnn_c3": [tuple(p.shape) for p in nets.egnn_c3_net(1).parameters()],
            "mlp_c2": [tuple(p.shape) for p in mlp_template(1, 8).parameters()]}


def parameters_of(shapes, device, seed):
    generator = torch.Generator(device="cpu").manual_seed(seed)
    parameters = []
    for shape in shapes:
        q = torch.nn.Parameter(torch.randn(shape, generator=generator).to(device))
        q.grad = (0.01 * torch.randn(shape, generator=generator)).to(device)
        parameters.append(q)
    return parameters


def fused_variant(shapes, device, mode):
    parameters = parameters_of(shapes, device, 7)
    optimizer = FusedAdam(parameters, lr=LR, weight_decay=WEIGHT_DECAY, decoupled_weight_decay=True)
    optimizer.gradient_clip_val = MAX_NORM if "clip" in mode else 0.0
    optimizer.zero_gradients = "zero" in mode
    return optimizer.step


def torch_variant(shapes, device, mode, **implementation):
    parameters = parameters_of(shapes, device, 7)
    optimizer = torch.optim.AdamW(parameters, lr=LR, weight_decay=WEIGHT_DECAY, **implementation)

    def step():
        if "clip" in mode:
            torch.nn.utils.clip_grad_norm_(parameters, MAX_NORM)
        optimizer.step()
        if "zero" in mode:
            optimizer.zero_grad(set_to_none=False)
    return step


def timed(step, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        step()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1000.0 / steps


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--rounds", type=int, default=7)
    parser.add_argument("--steps", type=int, default=200)
    parser.add_argument("--only", choices=("fused", "torch"), default=None)
    parser.add_argument("--shapes", choices=("egnn_c3", "mlp_c2"), default=None, help="one shape set only (a profiler run)")
    parser.add_argument("--out", default=None)
    arguments = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_step_timing needs a GPU: a time taken elsewhere says nothing about it")
    device = torch.device("cuda:0")
    lines = []
    for name, shapes in shape_sets().items():
        if arguments.shapes not in (None, name):
            continue
        elements = sum(int(torch.Size(shape).numel()) for shape in shapes)
        variants = {}
        for mode in MODES:
            if arguments.only != "torch":
                variants["fused" + mode] = fused_variant(shapes, device, mode)
            if arguments.only != "fused":
                variants["torch_default" + mode] = torch_variant(shapes, device, mode)
                variants["torch_foreach" + mode] = torch_variant(shapes, device, mode, foreach=True)
                variants["torch_fused" + mode] = torch_variant(shapes, device, mode, fused=True)
        for step in variants.values():
            for _ in range(WARMUP):
                step()
        torch.cuda.synchronize()
        times = {key: [] for key in variants}
        for _ in range(arguments.rounds):
            for key, step in variants.items():
                times[key].append(timed(step, arguments.steps))
        report = dict(shapes=name, tensors=len(shapes), elements=elements, rounds=arguments.rounds, steps=arguments.steps,
                      device=torch.cuda.get_device_name(0), variants={})
        for key, values in times.items():
            entry = dict(us_per_step=round(statistics.median(values), 2), min=round(min(values), 2), max=round(max(values), 2))
            if key.startswith("fused"):
                entry["arrays"] = 7 + ("zero" in key) + ("clip" in key)
                entry["gbytes_per_s_of_step_time"] = round(entry["arrays"] * 4 * elements / (entry["us_per_step"] * 1e-6) / 1e9, 1)
            report["variants"][key] = entry
        lines.append(json.dumps(report))
        print(lines[-1], flush=True)
    if arguments.out:
        os.makedirs(os.path.dirname(os.path.abspath(arguments.out)), exist_ok=True)
        with open(arguments.out, "w") as stream:
            stream.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
