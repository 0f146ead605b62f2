"""One frame's repainted candidates: all environments in ONE batch against one generator per environment.

    python tools/excise_and_repaint_timing.py [--rounds R] [--environments E] [--samples S] [--steps T] [--networks mlp,egnn]

E environments (K_e = 4 or 5 pinned atoms, as around a vacancy in diamond Si), S samples each, T time steps, M = 1, rng_mode
device, captured loop (use_hip_graph).  Two networks: the MLP of tests/nets.py at N = 8 and the hidden-32 radial-cutoff EGNN at
N = 64.  Three legs, alternated R times after one warm-up pass each; the host clock around work that ends in a device
synchronise, milliseconds per frame (E x S samples):

  batched            PerSampleConstrainedLangevinGenerator: set_environments + ONE sample(E S) on the kept graph
  sequential_kept    E ConstrainedLangevinGenerators built and warmed up once, each sample(S) on its own kept graph: the
                     least a per-environment flow can cost
  sequential_fresh   a NEW ConstrainedLangevinGenerator per environment, sample(S) each -- what the reference's sample maker does
                     (and ExciseAndRepaintSampleMaker with batch_environments=False): every environment pays its capture

and `excision`: one launch of mdx_excise_environments for E central atoms of a 512-atom frame (device events, 50 calls).
Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import excise_cases as ec  # noqa: E402
import nets  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd import kernels  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.constrained_langevin_generator import (  # noqa: E402
    ConstrainedLangevinGenerator, PerSampleConstrainedLangevinGenerator)
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import (  # noqa: E402
    PredictorCorrectorSamplingParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.sampling_constraint import SamplingConstraint  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters  # noqa: E402

NETWORKS = {"mlp": (8, 6.5, lambda: nets.mlp_net(8, 1, seed=1234)),
            "egnn": (64, 10.86, lambda: nets.egnn_net(1, "radial_cutoff", 4.5, hidden=32, seed=1234))}


def tables(E, N, rng):
    counts = torch.tensor([4 + e % 2 for e in range(E)], dtype=torch.int32)
    cx = torch.from_numpy(rng.random((E, 5, 3), dtype=np.float32))
    return cx, torch.zeros(E, 5, dtype=torch.int64), None, counts


def constraints(cx, counts):
    return [SamplingConstraint(elements=["Si"], constrained_relative_coordinates=cx[e, :int(k)].clone(),
                               constrained_atom_types=torch.zeros(int(k), dtype=torch.int64),
                               constrained_indices=torch.arange(int(k))) for e, k in enumerate(counts)]


def timed(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--environments", type=int, default=16)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--networks", default="mlp,egnn")
    args = ap.parse_args()
    device = torch.device("cuda:0")
    E, S, T = args.environments, args.samples, args.steps
    rng = np.random.default_rng(5)
    noise = NoiseParameters(**dict(ec.NOISE, total_time_steps=T))
    for name in args.networks.split(","):
        N, box, make = NETWORKS[name]
        net = make().to(device)
        sampling = PredictorCorrectorSamplingParameters(
            number_of_atoms=N, num_atom_types=1, number_of_samples=S, number_of_corrector_steps=1, use_fixed_lattice_parameters=True,
            cell_dimensions=[box] * 3, rng_mode="device", seed=616, use_hip_graph=True)
        cx, ca, _, counts = tables(E, N, rng)
        pins = constraints(cx, counts)
        batched = PerSampleConstrainedLangevinGenerator(noise, sampling, net, elements=["Si"])
        kept = [ConstrainedLangevinGenerator(noise, sampling, net, pin) for pin in pins]

        def run_batched():
            batched.set_environments((cx, ca, None, counts), S)
            return batched.sample(E * S, device)

        def run_kept():
            return [g.sample(S, device) for g in kept]

        def run_fresh():
            return [ConstrainedLangevinGenerator(noise, sampling, net, pin).sample(S, device) for pin in pins]

        legs = dict(batched=run_batched, sequential_kept=run_kept, sequential_fresh=run_fresh)
        times = {leg: [] for leg in legs}
        with torch.no_grad():
            for run in legs.values():                    # warm-up: code objects, the captures of the kept generators
                run()
            for _ in range(args.rounds):
                for leg, run in legs.items():
                    times[leg].append(timed(run))
        captured = "graph_loop" in batched._buffers and all("graph_loop" in g._buffers for g in kept)
        medians = {leg: float(np.median(v)) for leg, v in times.items()}
        for leg, values in times.items():
            print(json.dumps(dict(measurement="frame", network=name, leg=leg, atoms=N, environments=E, samples_per_environment=S,
                                  steps=T, correctors=1, captured=captured, ms_per_frame=[round(v, 2) for v in values],
                                  median_ms_per_frame=round(medians[leg], 2))), flush=True)
        print(json.dumps(dict(measurement="frame_ratio", network=name,
                              sequential_kept_over_batched=round(medians["sequential_kept"] / medians["batched"], 2),
                              sequential_fresh_over_batched=round(medians["sequential_fresh"] / medians["batched"], 2))), flush=True)

    x = torch.from_numpy(np.mod(ec.diamond_sites(4) + rng.normal(0, 0.004, (512, 3)), 1)).to(device)
    sides = torch.full((3,), 21.72, dtype=torch.float64, device=device)
    new_sides = torch.full((3,), 6.5, dtype=torch.float64, device=device)
    central = torch.from_numpy(rng.choice(512, E, replace=False)).to(device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    call = lambda: kernels.excise_environments(x, sides, central, radial_cutoff=3.0, new_box_sides=new_sides,  # noqa: E731
                                               capacity=8, status=status)
    for _ in range(3):
        call()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(50):
        call()
    stop.record()
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    print(json.dumps(dict(measurement="excision", atoms=512, environments=E, radial_cutoff=3.0,
                          us_per_call=round(1000.0 * start.elapsed_time(stop) / 50, 1))), flush=True)


if __name__ == "__main__":
    main()
