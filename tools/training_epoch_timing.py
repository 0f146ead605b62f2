#!/usr/bin/env python3
"""The training epoch's noising and its routes beside the flow they replace, in ONE process, alternating round by round.

    python tools/training_epoch_timing.py [--rounds R] [--calls K] [--epochs E] [--out FILE]

(a) one batch noised: `kernels.noise_training_batch` (mdx_noise_training_batch: gather by an epoch's permutation + time index +
    schedule rows + the three noisers, one launch) against `NoisingTransform.transform` on a batch that is ALREADY gathered (the
    flow before it: torch.randint, the table gathers, three host draws and uploads, the one-hot build and check, F1 / F2 / F3)
    at B 512, d 3, C 3, T 1000, N 8 / 64 / 216: microseconds per call, K eager calls between two device events; and 50 launches
    of the kernel in one hipGraph, its own figure.
(b) one epoch's training batches of the template MLP (hidden 64 x 3, N 8; dataset 8192, B 512: 16 steps), each epoch ended by
    the one host read of its loss sum:
      before            per batch: index_select of the three clean fields, NoisingTransform.transform,
                        FusedMlpTrainingStep.step(captured=True)          (the pieces the package had)
      fit captured      training._CapturedEpoch.run: one hipGraph replay per batch
      fit general       BatchNoiser.noise + loss.optimisation_step on the PyTorch network under autograd
      fit general, fused_training     the same with MLPScoreNetwork.fused_training = True
    milliseconds per epoch between two device synchronisations under a host clock, E epochs per round (300: the fastest
    route's round is then longer than a second).
(c) the C-ABI entry points one step of each route calls (for the captured route: what its graph holds), and the device kernels
    torch's profiler counts per step.
Every figure is printed with the spread of its rounds (minimum, median, maximum); the bar of a ratio is the spread of `before`.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, loss, training  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.data.diffusion.noising_transform import NoisingTransform  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.mlp_score_network import (  # noqa: E402
    MLPScoreNetwork, MLPScoreNetworkParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (ATOM_TYPES, LATTICE_PARAMETERS,  # noqa: E402
                                                                        RELATIVE_COORDINATES)
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters  # noqa: E402

DEVICE = torch.device("cuda:0")
NOISE = NoiseParameters(total_time_steps=1000, sigma_min=1e-3, sigma_max=0.5)
ROWS, BATCH = 8192, 512


def spread(values):
    return dict(minimum=min(values), median=statistics.median(values), maximum=max(values))


def dataset(atoms, types=2, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {RELATIVE_COORDINATES: torch.rand(ROWS, atoms, 3, generator=g).to(DEVICE),
            ATOM_TYPES: torch.randint(0, types, (ROWS, atoms), generator=g).to(DEVICE),
            LATTICE_PARAMETERS: (5.0 + torch.rand(ROWS, 6, generator=g)).to(DEVICE)}


def between_events(function, calls):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        function()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1000.0 / calls          # microseconds per call


def noising(atoms, rounds, calls):
    data = dataset(atoms)
    noiser = training.BatchNoiser(NOISE, num_atom_types=2, spatial_dimension=3, seed=7, device=DEVICE)
    transform = NoisingTransform(NOISE, num_atom_types=2, spatial_dimension=3, use_optimal_transport=False, device=DEVICE)
    permutation = torch.randperm(ROWS, device=DEVICE)
    cursor = torch.zeros(1, dtype=torch.int32, device=DEVICE)
    buffers = kernels.noised_training_batch_buffers(BATCH, atoms, 3, 3, DEVICE)
    gathered = {key: t[permutation[:BATCH]].contiguous() for key, t in data.items()}
    tables = noiser.noise_scheduler.tables

    def new():
        kernels.noise_training_batch(tables, data[RELATIVE_COORDINATES], data[ATOM_TYPES], data[LATTICE_PARAMETERS], BATCH,
                                     rows=permutation, cursor=cursor, rng=noiser.rng(None), out=buffers, status=noiser.status)

    def before():
        transform.transform(dict(gathered))

    for _ in range(3):
        new(), before()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(50):
            new()
    figures = dict(kernel_eager=[], transform_before=[], kernel_in_graph=[])
    for _ in range(rounds):
        figures["kernel_eager"].append(between_events(new, calls))
        figures["transform_before"].append(between_events(before, max(calls // 4, 1)))
        figures["kernel_in_graph"].append(between_events(graph.replay, max(calls // 10, 1)) / 50.0)
    kernels.raise_noising_status(noiser.status)
    return {name: spread(values) for name, values in figures.items()}


def template(fused_training=False):
    torch.manual_seed(1234)
    net = MLPScoreNetwork(MLPScoreNetworkParameters(
        number_of_atoms=8, num_atom_types=1, n_hidden_dimensions=3, hidden_dimensions_size=64,
        relative_coordinates_embedding_dimensions_size=32, noise_embedding_dimensions_size=16,
        time_embedding_dimensions_size=16, atom_type_embedding_dimensions_size=1,
        lattice_parameters_embedding_dimensions_size=1)).to(DEVICE)
    net.fused_training = fused_training
    return net


HYPER = dict(optimizer=dict(name="adamw", learning_rate=1e-3, weight_decay=1e-2))


def module():
    data = dataset(8, types=1)
    valid = {key: t[:BATCH].clone() for key, t in data.items()}
    made = training.DeviceDataModule(data, valid, NOISE, num_atom_types=1, spatial_dimension=3, batch_size=BATCH, seed=7, device=DEVICE)
    made.noise_once_at_setup = False
    return made


class Before:
    """The epoch the package's earlier pieces allow: gather, NoisingTransform.transform, the captured step."""

    def __init__(self):
        self.data, self.net = module(), template()
        self.step = loss.FusedMlpTrainingStep(self.net, loss.configure_optimizers(HYPER, self.net)["optimizer"])
        self.transform = NoisingTransform(NOISE, num_atom_types=1, spatial_dimension=3, use_optimal_transport=False, device=DEVICE)
        self.total = torch.zeros(1, dtype=torch.float64, device=DEVICE)

    def batch(self, permutation, start):
        rows = permutation[start:start + BATCH]
        batch = self.transform.transform({key: t.index_select(0, rows) for key, t in self.data.train_dataset.items()})
        return self.step.step(batch, captured=True)

    def epoch(self, epoch):
        permutation = self.data.shuffle(epoch)
        self.total.zero_()
        for start in range(0, ROWS, BATCH):
            self.total.add_(self.batch(permutation, start)["loss"].to(torch.float64), alpha=float(BATCH))
        return self.total.tolist()


class Captured:
    def __init__(self):
        self.data, self.net = module(), template()
        step = loss.FusedMlpTrainingStep(self.net, loss.configure_optimizers(HYPER, self.net)["optimizer"])
        self.runner = training._CapturedEpoch(step, self.data)

    def epoch(self, epoch):
        return self.runner.run(epoch).tolist()


class General:
    def __init__(self, fused_training):
        self.data, self.net = module(), template(fused_training)
        self.optimizer = loss.configure_optimizers(HYPER, self.net)["optimizer"]
        self.total = torch.zeros(1, dtype=torch.float64, device=DEVICE)

    def batch(self, index, batch):
        return loss.optimisation_step(self.net, batch, self.optimizer, batch_index=index)

    def epoch(self, epoch):
        self.total.zero_()
        for index, batch in enumerate(self.data.train_batches(epoch)):
            self.total.add_(self.batch(index, batch)["loss"].detach().to(torch.float64), alpha=float(BATCH))
        return self.total.tolist()


def epochs(rounds, count):
    routes = {"before": Before(), "fit_captured": Captured(), "fit_general": General(False), "fit_general_fused_training": General(True)}
    for route in routes.values():                 # every shape warm: kernels loaded, graphs captured, allocator settled
        for epoch in range(3):
            route.epoch(epoch)
    torch.cuda.synchronize()
    figures = {name: [] for name in routes}
    for r in range(rounds):
        for name, route in routes.items():
            torch.cuda.synchronize()
            start = time.perf_counter()
            for epoch in range(count):
                route.epoch(3 + r * count + epoch)
            torch.cuda.synchronize()
            figures[name].append((time.perf_counter() - start) * 1000.0 / count)
    return {name: spread(values) for name, values in figures.items()}, routes


def launches(routes):
    """Entry points per step (by wrapping kernels.call) and device kernels per step (torch's profiler)."""
    out = {}
    seen = []
    call = _hip.call
    kernels.call = lambda name, *args: (seen.append(name), call(name, *args))[1]
    try:
        permutation = routes["before"].data.shuffle(0)
        del seen[:]
        routes["before"].batch(permutation, 0)
        out["before"] = dict(entry_points=list(seen), note="the step's own five calls are inside its graph")
        runner = routes["fit_captured"].runner
        del seen[:]
        runner.launches(runner.step._prepare(BATCH), *runner.full, BATCH, 0, runner.cursor, flat=torch.empty_like(runner.step.flat))
        out["fit_captured"] = dict(entry_points_in_the_graph=list(seen) + ["(the optimizer's step: mdx_adam_step)"])
        for name in ("fit_general", "fit_general_fused_training"):
            del seen[:]
            routes[name].batch(0, next(iter(routes[name].data.train_batches(0))))
            out[name] = dict(entry_points=list(seen))
    finally:
        kernels.call = call
    steps = {"before": lambda: routes["before"].batch(permutation, 0), "fit_captured": runner.graph.replay,
             "fit_general": lambda: routes["fit_general"].batch(0, next(iter(routes["fit_general"].data.train_batches(0)))),
             "fit_general_fused_training": lambda: routes["fit_general_fused_training"].batch(
                 0, next(iter(routes["fit_general_fused_training"].data.train_batches(0))))}
    for name, step in steps.items():
        step()
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as profile:
            for _ in range(4):
                step()
            torch.cuda.synchronize()
        device = [e for e in profile.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[name]["device_kernels_per_step"] = len(device) / 4.0
    return out


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--calls", type=int, default=200, help="eager calls between two device events, per round")
    parser.add_argument("--epochs", type=int, default=300, help="epochs per round and route: a window of 1 s and more")
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    record = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, calls=args.calls, epochs=args.epochs, noising_us={},
                  epoch_ms={}, launches={})
    for atoms in (8, 64, 216):
        record["noising_us"][f"N{atoms}"] = noising(atoms, args.rounds, args.calls)
        print(json.dumps({f"noising_us N{atoms}": record["noising_us"][f"N{atoms}"]}), flush=True)
    record["epoch_ms"], routes = epochs(args.rounds, args.epochs)
    print(json.dumps({"epoch_ms": record["epoch_ms"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    record["launches"] = launches(routes)
    print(json.dumps({"launches": record["launches"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
