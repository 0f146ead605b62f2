"""The Stillinger-Weber kernel at the sampler's shapes: thermally displaced diamond crystals, one call per batch.

    python tools/stillinger_weber_timing.py [--repeats R]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/stillinger_weber_timing.py

  C3  B 512, N 64   Si 2x2x2, Si.sw
  C4  B 512, N 64   SiGe 2x2x2 (two types, random species), SiGe.sw
  C5  B 256, N 216  Si 3x3x3, Si.sw

Prints one JSON line per shape: microseconds per call between two device events around R calls (launch overhead included; the
kernel's own time is what the profiler's trace shows), and the energy per atom as a sanity figure.  The coefficient files are
the test fixtures (the package ships none)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stillinger_weber_cases as cases  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd import kernels  # noqa: E402

SHAPES = {"C3": (2, 512, cases.SI_SW, ["Si"], 5.43), "C4": (2, 512, cases.SIGE_SW, ["Si", "Ge"], 5.54),
          "C5": (3, 256, cases.SI_SW, ["Si"], 5.43)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    rng = np.random.default_rng(5)
    for name, (n, batch, path, elements, lattice) in SHAPES.items():
        x, sides = cases.displaced_crystal(n, batch, seed=7, lattice=lattice)
        types = rng.integers(0, len(elements), size=x.shape[:2])
        table = torch.from_numpy(cases.table(path, elements)).to(device)
        inputs = [torch.from_numpy(np.ascontiguousarray(t)).to(device) for t in (x, sides, types)]
        status = torch.zeros(1, dtype=torch.int32, device=device)
        words = int(kernels.lib().mdx_stillinger_weber_workspace_doubles(batch, x.shape[1], kernels.SW_NEIGHBOUR_CAPACITY))
        workspace = torch.empty(words, dtype=torch.float64, device=device)
        for _ in range(3):
            energies, _ = kernels.stillinger_weber_energy_forces(*inputs, table, status=status, workspace=workspace)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.repeats):
            energies, _ = kernels.stillinger_weber_energy_forces(*inputs, table, status=status, workspace=workspace)
        stop.record()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        print(json.dumps(dict(shape=name, batch=batch, atoms=x.shape[1], types=len(elements),
                              us_per_call=round(1000.0 * start.elapsed_time(stop) / args.repeats, 1),
                              workspace_MiB=round(words * 8 / 2 ** 20, 1),
                              mean_energy_per_atom_eV=round(float(energies.mean()) / x.shape[1], 6))), flush=True)


if __name__ == "__main__":
    main()
