"""Generate the optimal-translation fixtures tests/golden/optimal_translation/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_optimal_translation.py

The reference's own transport/optimal_translation.py, evaluated as built (binary32) and in binary64.  The stubs for the packages
the reference imports but this image lacks and the writer are make_golden.py's, imported from it unchanged.  For the binary64 run
torch's default dtype is binary64 around the call: the reference fills its scratch matrices (torch.ones) in the default dtype and
`tau_matrix[...] = tau_alphas` refuses mixed dtypes.

One file per (family, N); a file holds the case for every spatial dimension D, its arrays under the prefix `d<D>_`.  B = 5
structures unless said otherwise, inputs from a seeded torch.Generator.
  uniform     x, y ~ U[0, 1)                                                  N in 1, 2, 3, 8, 63, 64, 65, 255, 256
  shift       y = wrap(x + s), s ~ U[0, 1) per structure and dimension        N in 1, 8, 64, 256
  shiftnoise  y = wrap(x + s + N(0, 0.02^2))                                  N in 1, 8, 64, 256
  unbounded   x, y ~ 3 N(0, 1)                                                N in 3, 64
  equal       y = x: tau is exactly 0                                         N in 8, 65
  duplicates  uniform, the last atom a copy of the first (x and y): equal crossings        N in 8, 65
  shared      x [N, D] against y [B, N, D]; the reference gets x expanded     N in 8, 64
  boundary    the minimum on tau = +-1/2: no candidate, the reference's entry is +inf.  `boundary_n1` B 2, N 1, D 1,
              x 0.25, y (0.75, 0.50) -> (inf, -0.25); `boundary_n2` B 1, N 2, D 2 -> (inf, -0.2)
Per dimension (prefix d<D>_):
  x [B, N, D] f32 ([N, D] in `shared`), y [B, N, D] f32                      the inputs
  tau32 [B, D] f32, tau64 [B, D] f64                                          find_squared_geodesic_distance_minimizing_translation
  count64 [B, D] int32                                                        candidates per (b, alpha), binary64
  cost64 [B, D] f64                                                           D^2(x, y + tau64) in binary64 (+inf where tau64 is): the
                                                                              reference's d = (y + tau64) - x, g = d - round(d) (exact in
                                                                              binary64), the squares summed with math.fsum
  cost64_atan2 [B, D] f64                                                     the same through the reference's get_geodesic_displacements,
                                                                              atan2(sin 2 pi d, cos 2 pi d) / 2 pi, summed by torch
  atan2_cost_error                                                            max |cost64_atan2 - cost64| / cost64 where cost64 > 0: the
                                                                              reference's own rounding (2 pi d near a multiple of 2 pi
                                                                              carries an absolute error, so a displacement of 1e-8 keeps
                                                                              seven or eight digits: up to 3e-9 in `shift`, where the costs are 1e-14)
  taus32 f32, batch32, alpha32 int64 [candidates]                             find_self_consistent_taus(y - x), binary32
  taus64 f64, batch64, alpha64 int64 [candidates]                             the same in binary64
  cost_gap64                                                                  the smallest binary64 gap between the best and the second-
                                                                              best candidate cost of one (b, alpha); inf with no such pair
  rhs_margin64                                                                the smallest binary64 distance of a plateau's right-hand
                                                                              side from one of that plateau's two boundaries
  degenerate_plateaus                                                         `shift` only: plateaus left out of rhs_margin64, see below
  tau_rounding                                                                max |tau32 - tau64| over the finite entries (recorded only)
Asserted here:
  1. cost_gap64 > 1e-6 in every case: the candidate a binary64 evaluation picks does not depend on the rounding of the costs.
  2. rhs_margin64 >= 1e-5 in the uniform, shift, shiftnoise and unbounded families (the seeds below were picked so that it holds):
     the candidate SET does not depend on the order of a sum.  In `shift` (no noise) every crossing of a (b, alpha) is 1/2 - s up
     to the binary32 rounding of x + s, so the N - 1 inner plateaus are narrower than 1e-5 and the right-hand side of plateau N/2,
     1/2 - s, cannot keep that distance from them for any seed.  Those plateaus (width < 1e-5) are counted in
     degenerate_plateaus and held to what the margin is there for instead: N is a power of two and every y - x is a multiple of
     2^-24 below 1 in size, so the sums, the divisions by N and the right-hand sides are EXACT in binary64 in any order.
  3. +inf appears in tau64 in the boundary files only, at the entries named above.
The outputs of the reference's two elementwise helpers (compute_integer_ells_and_tau_crossing_points,
get_plateau_values_and_boundaries) are not recorded: they would be three quarters of the bytes and nothing here reads them.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

from diffusion_for_multi_scale_molecular_dynamics.transport import optimal_translation as ot  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.transport.distance import get_geodesic_displacements  # noqa: E402

DIRECTORY = "optimal_translation"
B = 5
COST_GAP, RHS_MARGIN = 1e-6, 1e-5
MARGIN_FAMILIES = ("uniform", "shift", "shiftnoise", "unbounded")
CASES = [("uniform", n) for n in (1, 2, 3, 8, 63, 64, 65, 255, 256)] + [("shift", n) for n in (1, 8, 64, 256)] + \
    [("shiftnoise", n) for n in (1, 8, 64, 256)] + [("unbounded", n) for n in (3, 64)] + [("equal", n) for n in (8, 65)] + \
    [("duplicates", n) for n in (8, 65)] + [("shared", n) for n in (8, 64)]
FILES = [f"{family}_n{n}.npz" for family, n in CASES] + ["boundary_n1.npz", "boundary_n2.npz"]
# (family, N, D) -> seed where the default, 1300 + 10 * (index of the case) + D, misses assertion 2: the first of default + 1000 t that holds
SEEDS = {("uniform", 63, 3): 2343, ("uniform", 64, 1): 2351, ("uniform", 65, 2): 2362, ("uniform", 255, 1): 3371,
         ("uniform", 255, 3): 27373, ("uniform", 256, 1): 2381, ("uniform", 256, 2): 38382, ("uniform", 256, 3): 32383,
         ("shiftnoise", 64, 2): 2452, ("shiftnoise", 256, 1): 2461}


def _wrap(t):
    t = torch.remainder(t, 1.0)
    t[t == 1.0] = 0.0
    return t


def _draw(family, g, N, D):
    x = torch.rand(B, N, D, generator=g)
    if family in ("uniform", "duplicates"):
        y = torch.rand(B, N, D, generator=g)
        if family == "duplicates":
            x[:, -1], y[:, -1] = x[:, 0], y[:, 0]
    elif family == "shift":
        y = _wrap(x + torch.rand(B, 1, D, generator=g))
    elif family == "shiftnoise":
        y = _wrap(x + torch.rand(B, 1, D, generator=g) + 0.02 * torch.randn(B, N, D, generator=g))
    elif family == "unbounded":
        x, y = 3.0 * torch.randn(B, N, D, generator=g), 3.0 * torch.randn(B, N, D, generator=g)
    elif family == "equal":
        y = x.clone()
    elif family == "shared":
        x, y = torch.rand(N, D, generator=g), torch.rand(B, N, D, generator=g)
    else:
        raise ValueError(family)
    return x, y


def _in_binary64(function, *arguments):
    torch.set_default_dtype(torch.float64)
    try:
        return function(*[a.double() for a in arguments])
    finally:
        torch.set_default_dtype(torch.float32)


def _candidate_costs(x, y, taus, batch, alpha):
    """D^2(x, y + tau) of every candidate, in the precision of the inputs."""
    displacements = get_geodesic_displacements(x[batch, :, alpha], y[batch, :, alpha] + taus[:, None])
    return (displacements**2).sum(dim=1)


def _record(family, x, y):
    """The arrays of one dimension of one case, and the three measured values."""
    full_x = x if x.dim() == 3 else x[None].expand_as(y).contiguous()
    batch, N, D = y.shape
    with torch.no_grad():
        tau32 = ot.find_squared_geodesic_distance_minimizing_translation(full_x, y)
        tau64 = _in_binary64(ot.find_squared_geodesic_distance_minimizing_translation, full_x, y)
        taus32, batch32, alpha32 = ot.find_self_consistent_taus(y - full_x)
        x64, y64 = full_x.double(), y.double()
        delta64 = y64 - x64
        taus64, batch64, alpha64 = _in_binary64(ot.find_self_consistent_taus, delta64)
        plateaus64, left64, right64 = _in_binary64(ot.get_plateau_values_and_boundaries,
                                                   *_in_binary64(ot.compute_integer_ells_and_tau_crossing_points, delta64))
        costs64 = _candidate_costs(x64, y64, taus64, batch64, alpha64)
    assert tau32.dtype == torch.float32 and tau64.dtype == torch.float64 and taus64.dtype == torch.float64
    count64 = torch.zeros(batch, D, dtype=torch.int32)
    cost64 = torch.full((batch, D), torch.inf, dtype=torch.float64)
    cost64_atan2 = cost64.clone()
    cost_gap = torch.inf
    for b in range(batch):
        for a in range(D):
            mine = costs64[(batch64 == b) & (alpha64 == a)]
            count64[b, a] = len(mine)
            if len(mine):
                ordered = mine.sort().values
                cost64_atan2[b, a] = ordered[0]
                d = (y64[b, :, a] + tau64[b, a]) - x64[b, :, a]
                cost64[b, a] = math.fsum(((d - d.round())**2).tolist())
                assert bool(taus64[(batch64 == b) & (alpha64 == a)][mine.argmin()] == tau64[b, a])
                if len(mine) > 1:
                    cost_gap = min(cost_gap, float(ordered[1] - ordered[0]))
    assert bool((torch.isinf(tau64) == (count64 == 0)).all()) and bool((torch.isinf(tau32) == torch.isinf(tau64)).all())
    rhs64 = plateaus64 / N - delta64.mean(dim=1, keepdim=True)
    distance = torch.minimum((rhs64 - left64).abs(), (rhs64 - right64).abs())
    degenerate = torch.zeros_like(distance, dtype=torch.bool)
    if family == "shift":
        degenerate = (right64 - left64) < RHS_MARGIN
        scaled = delta64 * 2.0**24
        assert N & (N - 1) == 0 and bool((scaled == scaled.round()).all()) and bool((delta64.abs() < 1.0).all())
    rhs_margin = float(distance[~degenerate].min())
    finite = torch.isfinite(tau64)
    tau_rounding = float((tau32.double() - tau64)[finite].abs().max()) if bool(finite.any()) else 0.0
    positive = torch.isfinite(cost64) & (cost64 > 0)
    atan2_cost_error = float(((cost64_atan2 - cost64).abs() / cost64)[positive].max()) if bool(positive.any()) else 0.0
    arrays = dict(x=mg._np(x), y=mg._np(y), tau32=mg._np(tau32), tau64=mg._np(tau64), count64=mg._np(count64), cost64=mg._np(cost64),
                  cost64_atan2=mg._np(cost64_atan2), atan2_cost_error=np.array(atan2_cost_error),
                  taus32=mg._np(taus32), batch32=mg._np(batch32), alpha32=mg._np(alpha32),
                  taus64=mg._np(taus64), batch64=mg._np(batch64), alpha64=mg._np(alpha64), cost_gap64=np.array(cost_gap),
                  rhs_margin64=np.array(rhs_margin), degenerate_plateaus=np.array(int(degenerate.sum())),
                  tau_rounding=np.array(tau_rounding))
    return arrays, cost_gap, rhs_margin


def case_arrays(family, N, D, seed):
    x, y = _draw(family, torch.Generator().manual_seed(seed), N, D)
    arrays, cost_gap, rhs_margin = _record(family, x, y)
    assert cost_gap > COST_GAP, f"{family} N {N} D {D} seed {seed}: cost gap {cost_gap:.3e}"
    assert family not in MARGIN_FAMILIES or rhs_margin >= RHS_MARGIN, f"{family} N {N} D {D} seed {seed}: rhs margin {rhs_margin:.3e}"
    assert not np.isinf(arrays["tau64"]).any(), f"{family} N {N} D {D} seed {seed}: an entry without a candidate"
    return arrays


def _save(name, per_dimension):
    arrays = {f"d{D}_{key}": value for D, one in per_dimension.items() for key, value in one.items()}
    arrays["dimensions"] = np.array(sorted(per_dimension))
    mg.save(os.path.join(DIRECTORY, name), **arrays)


def golden_optimal_translation():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    for index, (family, N) in enumerate(CASES):
        _save(f"{family}_n{N}.npz", {D: case_arrays(family, N, D, SEEDS.get((family, N, D), 1300 + 10 * index + D)) for D in (1, 2, 3)})
    # the boundary cases: y - x = 1/2 exactly for one (b, alpha), whose squared distance is least at tau = +-1/2
    arrays, _, _ = _record("boundary", torch.tensor([[[0.25]], [[0.25]]]), torch.tensor([[[0.75]], [[0.50]]]))
    assert np.array_equal(arrays["tau64"], np.array([[np.inf], [-0.25]])), arrays["tau64"]
    _save("boundary_n1.npz", {1: arrays})
    arrays, _, _ = _record("boundary", torch.tensor([[[0.25, 0.1], [0.5, 0.2]]]), torch.tensor([[[0.75, 0.4], [0.0, 0.3]]]))
    assert np.isinf(arrays["tau64"][0, 0]) and abs(arrays["tau64"][0, 1] + 0.2) < 1e-7, arrays["tau64"]
    _save("boundary_n2.npz", {2: arrays})


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_optimal_translation()
