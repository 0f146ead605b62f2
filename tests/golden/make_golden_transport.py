"""Generate the optimal-transport fixtures tests/golden/transport/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_transport.py

The reference's own Transporter (transport/transporter.py:13-196) and EquivariantAnalyticalScoreNetwork
(models/score_networks/equivariant_analytical_score_network.py), evaluated as built (binary32) and in binary64.  The stubs for
the packages the reference imports but this image lacks and the writer are make_golden.py's, imported from it unchanged.

The reference cannot evaluate itself in binary64 as written: _find_permutation_and_cost builds torch.eye(n) in binary32 and the
later einsum refuses the mixed dtypes.  Transporter64 below casts that one matrix to the cost's dtype; nothing else changes.

One file per case.  The first half of a case's B structures is uniform in the cell, the second half a random permutation of the
sites plus noise of width sigma_d plus a random global translation.  Random sites are drawn with |mean exp(2 pi i site)| >= 0.05
in every dimension (below that the reference's own centre is rounding noise).  Per case:
  D, N, kmax, sigma_d, symmetries, sites [N,D], operations [O,D,D]     the transporter / network
  X [B,N,D] f32 (and MU [B,N,D] f32 in the per-structure-mu case)     the inputs
  centre64 [B,D], x_invariant64 [B,N,D], mu_invariant64 [.,N,D]       get_atan2_translation / get_translation_invariant, binary64
  image32 [B,N,D] f32, image64 [B,N,D] f64                             get_optimal_transport
  operation32, operation64 [B]; col_idx32, col_idx64 [B,O,N]           the chosen operation; the column of each row, per operation
  costs64 [B,O]                                                        the optimal cost per operation
  cost_matrices64 [2,O,N,N]                                            N <= 8 only: the first two structures' cost matrices
  stable [B]                                                           both precisions pick the same permutation for every
                                                                       operation, and the same operation
  agree [B]                                                            image32 and image64 within 1e-6 on the torus
  compare_discrete                                                     False for the cases whose operations tie exactly
  sigma [S], score32 [S,B,N,D] f32, score64 [S,B,N,D] f64              get_normalized_scores at SIGMAS (shared-mu cases)
  floor_structure [S,B]                                                |score32 - score64| / |score64| (L2)
  state_keys, state_shapes, state_dtypes                               the network's state_dict
In a case with compare_discrete, a structure that is not stable is drawn again (`redrawn` counts them; at most one per eight
structures, asserted here).  With N = 2 inversion maps the two points onto themselves and operations tie exactly: the chosen
operation differs between the precisions as a matter of course, and only the image and the score are to be compared.
`toy1d` holds the reference's toy sites [[0.25], [0.75]], whose centre is degenerate (mean exp(2 pi i site) = 0): what the
reference does is recorded, and `agree` says where its two precisions give the same image.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

from diffusion_for_multi_scale_molecular_dynamics.models.score_networks.equivariant_analytical_score_network import (  # noqa: E402
    EquivariantAnalyticalScoreNetwork, EquivariantAnalyticalScoreNetworkParameters)
from diffusion_for_multi_scale_molecular_dynamics.transport.transporter import Transporter  # noqa: E402

SIGMAS = (0.01, 0.2, 0.5)
DIRECTORY = "transport"


class Transporter64(Transporter):
    """The reference's Transporter with the permutation matrix in the cost's dtype (see the module docstring)."""

    def _find_permutation_and_cost(self, cost_matrix):
        permutation, cost = super()._find_permutation_and_cost(cost_matrix)
        return permutation.to(cost_matrix.dtype), cost


def _networks(D, N, kmax, sigma_d, symmetries, sites):
    def one():
        return EquivariantAnalyticalScoreNetwork(EquivariantAnalyticalScoreNetworkParameters(
            spatial_dimension=D, number_of_atoms=N, num_atom_types=1, kmax=kmax, sigma_d=sigma_d,
            equilibrium_relative_coordinates=sites.tolist(), use_point_group_symmetries=symmetries))
    net, net64 = one(), one().double()
    net64.transporter = Transporter64(net64.symmetries)
    return net, net64


def _stages(transporter, x, mu):
    """Every stage of get_optimal_transport, in the precision of the inputs."""
    with torch.no_grad():
        x_invariant = transporter.get_translation_invariant(x)
        mu_invariant = transporter.get_translation_invariant(mu)
        matrices = transporter._get_all_cost_matrices(x_invariant, mu_invariant)
        B, O, N, _ = matrices.shape
        col_idx = torch.empty(B, O, N, dtype=torch.int32)
        costs = torch.empty(B, O, dtype=matrices.dtype)
        for b in range(B):
            for o in range(O):
                permutation, cost = transporter._find_permutation_and_cost(matrices[b, o])
                col_idx[b, o] = permutation.argmax(dim=0)          # permutation = eye(n)[:, col_idx]
                costs[b, o] = cost
        image = transporter.get_optimal_transport(x, mu)
    return dict(centre=transporter.get_atan2_translation(x), x_invariant=x_invariant, mu_invariant=mu_invariant, matrices=matrices,
                col_idx=col_idx, costs=costs, operation=costs.argmin(dim=1).to(torch.int32), image=image)


def _torus_distance(a, b):
    diff = a.double() - b.double()
    return (diff - torch.round(diff)).abs().reshape(a.shape[0], -1).max(dim=1).values


def _random_sites(g, N, D):
    for _ in range(1000):
        sites = torch.rand(N, D, generator=g)
        if (torch.exp(2j * torch.pi * sites.double()).mean(dim=0).abs() >= 0.05).all():
            return sites
    raise RuntimeError("no sites with a resolved centre in 1000 draws")


def _draw_structure(g, b, B, sites, sigma_d):
    N, D = sites.shape
    if b < B // 2:
        return torch.rand(1, N, D, generator=g)
    permutation = torch.randperm(N, generator=g)
    x = torch.remainder(sites[permutation][None] + sigma_d * torch.randn(1, N, D, generator=g) + torch.rand(1, 1, D, generator=g), 1.0)
    x[x == 1.0] = 0.0
    return x


def _record(t32, t64, X, MU, compare_discrete, redrawn, N):
    s32 = _stages(t32, X, MU)
    s64 = _stages(t64, X.double(), MU.double())
    stable = (s32["col_idx"] == s64["col_idx"]).reshape(X.shape[0], -1).all(dim=1) & (s32["operation"] == s64["operation"])
    arrays = dict(X=mg._np(X), centre64=mg._np(s64["centre"]), x_invariant64=mg._np(s64["x_invariant"]),
                  image32=mg._np(s32["image"]), image64=mg._np(s64["image"]), operation32=mg._np(s32["operation"]),
                  operation64=mg._np(s64["operation"]), col_idx32=mg._np(s32["col_idx"]), col_idx64=mg._np(s64["col_idx"]),
                  costs64=mg._np(s64["costs"]), stable=mg._np(stable), agree=mg._np(_torus_distance(s32["image"], s64["image"]) <= 1e-6),
                  compare_discrete=np.array(compare_discrete), redrawn=np.array(redrawn))
    if N <= 8:
        arrays["cost_matrices64"] = mg._np(s64["matrices"][:2])
    return arrays, s64


def _case(name, seed, D, N, symmetries, B, sigma_d, kmax, sites=None, compare_discrete=True):
    g = torch.Generator().manual_seed(seed)
    sites = _random_sites(g, N, D) if sites is None else sites
    net, net64 = _networks(D, N, kmax, sigma_d, symmetries, sites)
    t32, t64 = net.transporter, net64.transporter
    mu = sites[None]
    X = torch.empty(B, N, D)
    redrawn = 0
    for b in range(B):
        for attempt in range(1000):
            x = _draw_structure(g, b, B, sites, sigma_d)
            if not compare_discrete:
                break
            s32, s64 = _stages(t32, x, mu), _stages(t64, x.double(), mu.double())
            if bool((s32["col_idx"] == s64["col_idx"]).all()) and bool((s32["operation"] == s64["operation"]).all()):
                break
            redrawn += 1
        else:
            raise RuntimeError("no stable structure in 1000 draws")
        X[b] = x[0]
    assert redrawn <= B // 8, f"{name}: {redrawn} structures of {B} were drawn again"
    MU = mu.expand(B, N, D).contiguous()
    arrays, s64 = _record(t32, t64, X, MU, compare_discrete, redrawn, N)
    arrays["mu_invariant64"] = mg._np(s64["mu_invariant"][:1])
    score32, score64, floors = [], [], []
    with torch.no_grad():
        for sigma in SIGMAS:
            full = torch.full((B, N, D), sigma)
            a, c = net.get_normalized_scores(X, full), net64.get_normalized_scores(X.double(), full.double())
            score32.append(mg._np(a))
            score64.append(mg._np(c))
            diff = (a.double() - c).reshape(B, -1)
            floors.append(mg._np(torch.linalg.norm(diff, dim=1) / torch.linalg.norm(c.reshape(B, -1), dim=1)))
    state = net.state_dict()
    arrays.update(D=np.array(D), N=np.array(N), kmax=np.array(kmax), sigma_d=np.array(sigma_d), symmetries=np.array(symmetries),
                  sites=mg._np(sites), operations=mg._np(net.symmetries), sigma=np.array(SIGMAS, dtype=np.float32),
                  score32=np.stack(score32), score64=np.stack(score64), floor_structure=np.stack(floors),
                  state_keys=np.array(list(state)), state_shapes=np.array([str(tuple(v.shape)) for v in state.values()]),
                  state_dtypes=np.array([str(v.dtype) for v in state.values()]))
    mg.save(os.path.join(DIRECTORY, name + ".npz"), **arrays)


def _noising_case(name, seed, D, N, B, sigma):
    """The noising transform's use (data/diffusion/noising_transform.py:153-158): the identity operation alone, mu per structure:
    get_optimal_transport(x0, xt) with xt = x0 noised at `sigma`."""
    g = torch.Generator().manual_seed(seed)
    operations = torch.eye(D).unsqueeze(0)
    t32, t64 = Transporter(operations), Transporter64(operations.double())
    X = torch.empty(B, N, D)
    MU = torch.empty(B, N, D)
    redrawn = 0
    for b in range(B):
        for attempt in range(1000):
            x0 = torch.rand(1, N, D, generator=g)
            xt = torch.remainder(x0 + sigma * torch.randn(1, N, D, generator=g), 1.0)
            xt[xt == 1.0] = 0.0
            s32, s64 = _stages(t32, x0, xt), _stages(t64, x0.double(), xt.double())
            if bool((s32["col_idx"] == s64["col_idx"]).all()):
                break
            redrawn += 1
        else:
            raise RuntimeError("no stable structure in 1000 draws")
        X[b], MU[b] = x0[0], xt[0]
    assert redrawn <= B // 8, f"{name}: {redrawn} structures of {B} were drawn again"
    arrays, s64 = _record(t32, t64, X, MU, True, redrawn, N)
    arrays.update(D=np.array(D), N=np.array(N), MU=mg._np(MU), mu_invariant64=mg._np(s64["mu_invariant"]), operations=mg._np(operations),
                  noise_sigma=np.array(sigma))
    mg.save(os.path.join(DIRECTORY, name + ".npz"), **arrays)


def golden_transport():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    _case("d1_n3", 11, 1, 3, True, 16, 0.05, 4)
    _case("d2_n3", 12, 2, 3, True, 16, 0.05, 4)
    _case("d3_n5", 13, 3, 5, True, 16, 0.05, 4)
    _case("d3_n8", 14, 3, 8, True, 16, 0.03, 4)
    _case("d3_n8_identity", 15, 3, 8, False, 16, 0.03, 4)
    _case("d3_n2_ties", 16, 3, 2, True, 16, 0.05, 4, compare_discrete=False)
    _case("toy1d", 17, 1, 2, True, 16, 0.01, 5, sites=torch.tensor([[0.25], [0.75]]), compare_discrete=False)
    _case("d3_n64", 18, 3, 64, True, 4, 0.02, 2)            # one column per lane, every lane busy
    _case("d3_n65", 19, 3, 65, True, 4, 0.02, 2)            # two columns per lane, a ragged tail
    _noising_case("noising_d3_n8", 20, 3, 8, 16, 0.1)


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_transport()
