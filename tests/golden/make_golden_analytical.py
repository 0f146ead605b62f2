"""Generate the analytical-score fixtures tests/golden/analytical/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_analytical.py

The reference's own AnalyticalScoreNetwork (models/score_networks/analytical_score_network.py:68-298) and the two functions of
score/wrapped_gaussian_score.py it is made of.  The stubs for the packages the reference imports but this image lacks and the
writer are make_golden.py's, imported from it unchanged.

One file per case.  A case is evaluated at SIGMAS (`big`: at 0.01, 0.39 and 0.41; both sides of the 1 / sqrt(2 pi) = 0.39894 threshold between the reference's
formulas); the first half of its B structures is uniform in the cell, the second half the sites plus noise of width sigma_d.
Per case:
  D, N, kmax, sigma_d, permutations, sites          the network
  X [S,B,N,D] f32, sigma [S,B] f32                  the inputs (S noise levels; one sigma per structure)
  score32 [S,B,N,D] f32, prob32 [S,B] f32           get_probabilities_and_normalized_scores of the module as built (binary32)
  score64 [S,B,N,D] f64, prob64 [S,B] f64           the same module and inputs after .double()
  floor_case [S], floor_structure [S,B]             |score32 - score64| / |score64| (L2): the reference's own binary32 error
  finite32 [S,B]                                    False where the binary32 module's own output holds a NaN or inf (at kmax 0 its
                                                    formula 1b is exp(-x) / exp(-x), which underflows to 0 / 0 in binary32 long
                                                    before it does in binary64); the floors there are NaN
  state_keys, state_shapes, state_dtypes            the module's state_dict
`mixed_sigma` holds two levels instead: level 0 draws every structure's sigma from SIGMAS, level 1 every ELEMENT's
(`sigma_elements` [B,N,D], evaluated through the public method).
The reference picks one of three formulas per element by comparing (sigma_eff, u) with binary32 constants: a structure in which
the binary32 and the binary64 evaluation pick different formulas for some element is drawn again (`redrawn` counts them), so
no case compared against the binary64 output holds such an element.  `edges` is built by hand to sit ON those boundaries (x
equal to a site, x - site = -1e-8, u = 0.5 exactly) and is not redrawn: it is compared against the binary32 output.

wrapped_gaussian.npz is an elementwise grid for the two functions, u x sigma x kmax in binary32 with the reference's binary64
results (`score64`, `log64`: [kmax, sigma, u]) and get_sigma_normalized_score_brute_force's Python floats (`brute`).
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

from diffusion_for_multi_scale_molecular_dynamics.models.score_networks.analytical_score_network import (  # noqa: E402
    AnalyticalScoreNetwork, AnalyticalScoreNetworkParameters)
from diffusion_for_multi_scale_molecular_dynamics.score import wrapped_gaussian_score as wgs  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.utils.basis_transformations import \
    map_relative_coordinates_to_unit_cell  # noqa: E402

SIGMAS = (1e-3, 0.01, 0.05, 0.2, 0.39, 0.41, 0.5)
DIRECTORY = "analytical"


def _network(D, N, kmax, sigma_d, permutations, sites):
    return AnalyticalScoreNetwork(AnalyticalScoreNetworkParameters(
        spatial_dimension=D, number_of_atoms=N, num_atom_types=1, kmax=kmax, sigma_d=sigma_d,
        equilibrium_relative_coordinates=sites.tolist(), use_permutation_invariance=permutations))


def _branches(net, x, sigma):
    """The formula each element of the reference's evaluation takes, in the precision of (net, x, sigma): 0 = 1a, 1 = 1b,
    2 = the Ewald form; [P, B, N, D]."""
    u = map_relative_coordinates_to_unit_cell(x.unsqueeze(0) - net.all_x0.unsqueeze(1))
    effective = torch.sqrt(net.sigma_d_square + sigma**2).unsqueeze(0).expand_as(u)
    flat_u, flat_s = u.reshape(-1), effective.reshape(-1)
    out = torch.full(flat_u.shape, -1, dtype=torch.int64)
    for value, mask in enumerate((wgs._get_small_sigma_small_u_mask, wgs._get_small_sigma_large_u_mask, wgs._get_large_sigma_mask)):
        out[mask(flat_u, flat_s)] = value
    assert (out >= 0).all()
    return out.reshape(u.shape)


def _same_branches(net, net64, x, sigma):
    """Per structure: do the binary32 and the binary64 evaluation pick the same formula for every element?"""
    same = _branches(net, x, sigma) == _branches(net64, x.double(), sigma.double())
    return same.permute(1, 0, 2, 3).reshape(x.shape[0], -1).all(dim=1)


def _draw(g, net, net64, sites, sigma_d, sigma, B, redraw=True):
    """B structures -- the first half uniform, the rest sites + sigma_d noise -- with one sigma per structure broadcast to
    [B,N,D]; a structure whose branches differ between the precisions is drawn again."""
    N, D = sites.shape
    X = torch.empty(B, N, D)
    redrawn = 0
    for b in range(B):
        for attempt in range(1000):
            if b < B // 2:
                x = torch.rand(1, N, D, generator=g)
            else:
                x = torch.remainder(sites[None] + sigma_d * torch.randn(1, N, D, generator=g), 1.0)
                x[x == 1.0] = 0.0
            if not redraw or bool(_same_branches(net, net64, x, sigma[b:b + 1])):
                break
            redrawn += 1
        else:
            raise RuntimeError("no structure with equal branches in 1000 draws")
        X[b] = x[0]
    return X, redrawn


def _evaluate(net, net64, X, sigma_full):
    with torch.no_grad(), np.errstate(all="ignore"):
        p32, s32 = net.get_probabilities_and_normalized_scores(X, sigma_full)
        p64, s64 = net64.get_probabilities_and_normalized_scores(X.double(), sigma_full.double())
    B = X.shape[0]
    finite = torch.isfinite(s32.reshape(B, -1)).all(dim=1)
    diff = (s32.double() - s64).reshape(B, -1)
    floor_structure = torch.linalg.norm(diff, dim=1) / torch.linalg.norm(s64.reshape(B, -1), dim=1)
    floor_structure[~finite] = float("nan")
    floor_case = torch.linalg.norm(diff[finite]) / torch.linalg.norm(s64.reshape(B, -1)[finite]) if finite.any() else torch.tensor(float("nan"))
    return dict(score32=s32, prob32=p32, score64=s64, prob64=p64, floor_structure=floor_structure, floor_case=floor_case,
                finite32=finite)


def _state_record(net):
    state = net.state_dict()
    return dict(state_keys=np.array(list(state)), state_shapes=np.array([str(tuple(v.shape)) for v in state.values()]),
                state_dtypes=np.array([str(v.dtype) for v in state.values()]))


def _save(name, net, sites, sigma_d, levels, extra=None):
    arrays = dict(D=np.array(sites.shape[1]), N=np.array(sites.shape[0]), kmax=np.array(net.kmax), sigma_d=np.array(sigma_d),
                  permutations=np.array(bool(net.use_permutation_invariance)), sites=mg._np(sites))
    for key in levels[0]:
        arrays[key] = np.stack([mg._np(level[key]) if isinstance(level[key], torch.Tensor) else np.asarray(level[key])
                                for level in levels])
    arrays.update(_state_record(net))
    arrays.update(extra or {})
    mg.save(os.path.join(DIRECTORY, name + ".npz"), **arrays)


def _case(name, seed, D, N, kmax, sigma_d, permutations, B, sites, sigmas=SIGMAS):
    g = torch.Generator().manual_seed(seed)
    net = _network(D, N, kmax, sigma_d, permutations, sites)
    net64 = _network(D, N, kmax, sigma_d, permutations, sites).double()
    levels = []
    for sigma_value in sigmas:
        sigma = torch.full((B,), sigma_value)
        full = sigma.view(B, 1, 1).expand(B, N, D).contiguous()
        X, redrawn = _draw(g, net, net64, sites, sigma_d, full, B)
        levels.append(dict(X=X, sigma=sigma, redrawn=redrawn, **_evaluate(net, net64, X, full)))
    _save(name, net, sites, sigma_d, levels)


def _mixed_sigma(seed):
    D, N, kmax, sigma_d, B = 3, 4, 4, 0.05, 8
    g = torch.Generator().manual_seed(seed)
    sites = torch.rand(N, D, generator=g)
    net, net64 = _network(D, N, kmax, sigma_d, True, sites), _network(D, N, kmax, sigma_d, True, sites).double()
    choices = torch.tensor(SIGMAS)
    # level 0: one sigma per structure
    sigma = choices[torch.randint(0, len(SIGMAS), (B,), generator=g)]
    full = sigma.view(B, 1, 1).expand(B, N, D).contiguous()
    X0, redrawn0 = _draw(g, net, net64, sites, sigma_d, full, B)
    level0 = dict(X=X0, sigma=sigma, redrawn=redrawn0, **_evaluate(net, net64, X0, full))
    # level 1: one sigma per element (`sigma` holds each structure's first, for the record only)
    elements = choices[torch.randint(0, len(SIGMAS), (B, N, D), generator=g)]
    X1, redrawn1 = _draw(g, net, net64, sites, sigma_d, elements, B)
    level1 = dict(X=X1, sigma=elements[:, 0, 0].clone(), redrawn=redrawn1, **_evaluate(net, net64, X1, elements))
    _save("mixed_sigma", net, sites, sigma_d, [level0, level1], extra=dict(sigma_elements=mg._np(elements)))


def _edges():
    """Atoms ON the boundaries between the reference's formulas, beside atoms at an ordinary displacement (so that the case's
    norm is that of an ordinary case and the boundary elements are held in absolute terms)."""
    D, N, kmax, sigma_d, B = 3, 4, 4, 0.05, 3
    sites = torch.tensor([[2e-8, 0.25, 0.5], [0.25, 0.25, 0.25], [0.5, 0.75, 0.25], [0.75, 0.5, 0.125]])
    net, net64 = _network(D, N, kmax, sigma_d, False, sites), _network(D, N, kmax, sigma_d, False, sites).double()
    displaced = torch.remainder(sites + torch.tensor([0.11, -0.07, 0.05]), 1.0)
    X = torch.stack([displaced.clone(), displaced.clone(), displaced.clone()])
    X[0, :2] = sites[:2]                                # x equal to a site
    X[1, 0, 0] = 1e-8                                   # x - site = -1e-8: the binary32 fraction rounds to 1 and becomes 0
    X[2, :2] = torch.remainder(sites[:2] + 0.5, 1.0)    # u = 0.5 exactly (0.75 against 0.25, ...)
    X[2, 0, 0] = 0.5
    levels = []
    for sigma_value in SIGMAS:
        sigma = torch.full((B,), sigma_value)
        full = sigma.view(B, 1, 1).expand(B, N, D).contiguous()
        levels.append(dict(X=X, sigma=sigma, redrawn=0, **_evaluate(net, net64, X, full)))
    _save("edges", net, sites, sigma_d, levels)


def _wrapped_gaussian():
    one, half = np.float32(1.0), np.float32(0.5)
    thr = np.float32(wgs.SIGMA_THRESHOLD.item())
    u = np.array([0.0, 1e-7, 0.25, np.nextafter(half, np.float32(0)), half, np.nextafter(half, one), 0.75,
                  np.nextafter(one, np.float32(0))], dtype=np.float32)
    sigma = np.array([1e-4, 1e-3, 0.01, 0.1, np.nextafter(thr, np.float32(0)), thr, np.nextafter(thr, one), 0.5, 1.0, 5.0],
                     dtype=np.float32)
    kmaxes = np.array([0, 1, 4, 10])
    uu = torch.from_numpy(u).double().view(1, -1).expand(len(sigma), len(u)).contiguous()
    ss = torch.from_numpy(sigma).double().view(-1, 1).expand(len(sigma), len(u)).contiguous()
    score64, log64, brute = [], [], []
    with np.errstate(all="ignore"):
        for kmax in kmaxes.tolist():
            score64.append(mg._np(wgs.get_coordinates_sigma_normalized_score(uu, ss, kmax)))
            log64.append(mg._np(wgs.get_log_wrapped_gaussians(uu.view(len(sigma), len(u), 1, 1), ss.view(len(sigma), len(u), 1, 1), kmax)))
            brute.append([[wgs.get_sigma_normalized_score_brute_force(float(a), float(s), kmax) for a in u] for s in sigma])
    mg.save(os.path.join(DIRECTORY, "wrapped_gaussian.npz"), u=u, sigma=sigma, kmax=kmaxes, score64=np.stack(score64),
            log64=np.stack(log64), brute=np.array(brute, dtype=np.float64))


def golden_analytical():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    g = torch.Generator().manual_seed(907)
    _case("toy1d", 1, 1, 2, 5, 0.01, True, 16, torch.tensor([[0.25], [0.75]]))      # the reference's own YAML block
    _case("diamond", 2, 3, 8, 4, 0.05, False, 8, mg._diamond_sites(1))              # dist_analytic.npz's network
    _case("perm4", 3, 3, 4, 4, 0.05, True, 8, torch.rand(4, 3, generator=g))
    _case("perm3_2d", 4, 2, 3, 1, 0.03, True, 8, torch.rand(3, 2, generator=g))     # kmax 1: the truncation is visible
    _case("perm5", 5, 3, 5, 2, 0.02, True, 4, torch.rand(5, 3, generator=g))        # 120 permutations: two wavefronts
    _case("perm7", 6, 3, 7, 1, 0.05, True, 2, torch.rand(7, 3, generator=g))        # 5 040: several rounds per lane
    _case("big", 7, 3, 216, 2, 0.05, False, 2, mg._diamond_sites(3),                # the workgroup loops over the atoms;
          sigmas=(0.01, 0.39, 0.41))                                                 # three levels keep the file small
    _case("kmax0", 8, 3, 2, 0, 0.05, True, 8, torch.rand(2, 3, generator=g))
    _mixed_sigma(9)
    _edges()
    _wrapped_gaussian()


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_analytical()
