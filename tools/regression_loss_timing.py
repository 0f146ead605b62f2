"""The fused regression launch beside the same quantities from the pieces the package had before it, on the same GPU.

    python tools/regression_loss_timing.py [--replays R]

B 512, D 3; N 8, 64 and 216 without permutations and N 8 with them (40 320 per structure); sigma_d 0.05, kmax 4, one sigma per
structure drawn from [0.01, 0.5]; x uniform, the sites uniform, the score randn.  Per shape one JSON line:
    kernel_us          `kernels.regression_loss` (mdx_regression_loss: one launch over the structures and the one-workgroup total):
                       calls captured into one hipGraph on a side stream after a warm-up call (50 per graph; 5 with
                       permutations); one replay between two device events, over the calls; R replays, median (min .. max)
    kernel_eager_us    the same call from Python, R calls between two device events (launch overhead, the five output allocations)
    pieces_us          `pieces` below: `kernels.analytical_score` (the target, rounded to binary32), then torch for the error, the
                       per-structure sums of squares, the mean and 2 (s - t) / M -- in binary32.  No host read either: captured and
                       timed the same way; pieces_eager_us is R eager calls
    loss_kernel, loss_pieces, max_difference     the two losses and |loss_kernel - loss_pieces| / |loss_kernel|: the pieces are
                       binary32
The timing helpers are tools/consistency_loss_timing.py's."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from consistency_loss_timing import captured_us, eager_us, spread  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics_amd import kernels  # noqa: E402

BATCH, DIMENSION, KMAX, SIGMA_D = 512, 3, 4, 0.05
SHAPES = ((8, False), (64, False), (216, False), (8, True))      # (atoms, permutations)


def pieces(c):
    """(loss, target, gradient, per_structure) from the analytical kernel and binary32 torch on device tensors."""
    target, _ = kernels.analytical_score(c["x"], c["sigma"], c["sites"], SIGMA_D**2, KMAX, c["permutations"])
    errors = c["s"] - target
    squares = errors**2
    return squares.mean(), target, 2.0 * errors / errors.numel(), squares.sum(dim=(1, 2))


def inputs(N, permutations, device):
    g = torch.Generator().manual_seed(43 + N)
    draw = lambda f, *shape: f(*shape, generator=g).to(device)
    return dict(x=draw(torch.rand, BATCH, N, DIMENSION), s=draw(torch.randn, BATCH, N, DIMENSION),
                sites=draw(torch.rand, N, DIMENSION), sigma=0.01 + 0.49 * draw(torch.rand, BATCH), permutations=permutations)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=20)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    for N, permutations in SHAPES:
        c = inputs(N, permutations, device)
        per_graph = 5 if permutations else 50
        status = torch.zeros(1, dtype=torch.int32, device=device)
        fused = lambda: kernels.regression_loss(c["s"], relative_coordinates=c["x"], sigmas=c["sigma"],  # noqa: E731
                                                equilibrium_relative_coordinates=c["sites"], sigma_d_square=SIGMA_D**2, kmax=KMAX,
                                                use_permutation_invariance=permutations, status=status)
        chain = lambda: pieces(c)  # noqa: E731
        with torch.no_grad():
            for _ in range(3):
                out = fused()
                loss = chain()[0]
            torch.cuda.synchronize()
            assert int(status.item()) == 0
            difference = abs(float(out.loss) - float(loss)) / abs(float(out.loss))
            kernel_us = captured_us(fused, per_graph, args.replays)
            kernel_eager_us = eager_us(fused, args.replays)
            pieces_us = captured_us(chain, per_graph, args.replays)
            pieces_eager_us = eager_us(chain, args.replays)
        print(json.dumps(dict(batch=BATCH, atoms=N, dimension=DIMENSION, permutations=permutations, kernel_us=spread(kernel_us),
                              kernel_eager_us=round(kernel_eager_us, 2), pieces_us=spread(pieces_us),
                              pieces_eager_us=round(pieces_eager_us, 2), loss_kernel=float(out.loss), loss_pieces=float(loss),
                              max_difference=difference)), flush=True)


if __name__ == "__main__":
    main()
