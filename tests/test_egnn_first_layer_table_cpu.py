"""The grid problem of the first EGNN layer's distance table (kernels.egnn_table_grid), host side."""
import math

import torch

from diffusion_for_multi_scale_molecular_dynamics_amd import kernels


def test_grid_abscissae_are_exact_and_laid_out_by_class_pair():
    D = 6
    n_even = kernels.egnn_table_points(D)
    assert (n_even - 3) / kernels.TABLE_INV_SPACING >= math.sqrt(2 * D)       # rho <= 2 sqrt(n_k) has its four points
    for n_classes in (2, 3):
        classes, coord, edges = kernels.egnn_table_grid(n_classes, n_even, D, "cpu")
        K = 2 * n_even - 1
        assert classes.shape[0] == coord.shape[0] == n_classes * (K + 1) and edges.shape[0] == n_classes ** 2 * K
        assert bool((edges[1:, 0] >= edges[:-1, 0]).all())                    # sorted by source
        rows = torch.arange(edges.shape[0])
        p, r = rows // K, rows % K
        assert torch.equal(classes[edges[:, 0]], p // n_classes) and torch.equal(classes[edges[:, 1]], p % n_classes)
        # the chain's |c_src - c_dst|^2 (sources at the origin) is rho_k^2 exactly, rho_k = k h / 2
        k = torch.where(r < n_even, 2 * r, 2 * (r - n_even) + 1)
        c = coord[edges[:, 1]] - coord[edges[:, 0]]
        r2 = torch.zeros(edges.shape[0], dtype=torch.float32)
        for j in range(D):
            r2 = r2 + c[:, j] * c[:, j]
        want = (k.double() / (2 * kernels.TABLE_INV_SPACING)) ** 2
        assert torch.equal(r2.double(), want)
        assert bool((k.double() ** 2 < 2 ** 24).all())
