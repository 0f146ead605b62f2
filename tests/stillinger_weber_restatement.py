"""The tests' own binary64 NumPy evaluation of the Stillinger-Weber potential (LAMMPS `pair_style sw`, metal units), written
from the formula and from nothing else:

    E    = sum_i sum_{j>i} phi2(r_ij) + sum_i sum_{j != i} sum_{k>j} phi3(r_ij, r_ik, theta_jik)        over all periodic images
    phi2 = A eps [B (sigma/r)^p - (sigma/r)^q] exp(sigma / (r - a sigma))                               r < a sigma, entry (ti,tj,tj)
    phi3 = lambda eps (cos theta - cos theta0)^2 exp(g_ij s_ij / (r_ij - a_ij s_ij)) exp(g_ik s_ik / (r_ik - a_ik s_ik))
           lambda, eps, cos theta0 of entry (ti,tj,tk); the ij leg's sigma, a, gamma of (ti,tj,tj), the ik leg's of (ti,tk,tk)

One loop over the centres; for each, the explicit list of its neighbours over the 27 images of an orthogonal box (complete while
every side >= the largest a sigma), every pair term halved between its two centres, every triplet of the centre, analytic forces.
Beside (E, F) it returns S = sum |terms| and S_F = max over atoms of sum |force contributions| (Euclidean norm of each
contribution): the scales a binary64 evaluation in another order may differ by, times a few ulp.

Table columns: eps, sigma, a, lambda, gamma, cos theta0, A, B, p, q.
"""
import itertools

import numpy as np

EPS, SIGMA, A_CUT, LAMBDA, GAMMA, COS0, BIG_A, BIG_B, P, Q = range(10)
IMAGES = np.array(list(itertools.product((-1.0, 0.0, 1.0), repeat=3)))          # [27,3], image 13 is the cell itself


def phi2(r, entry):
    """The pair term and its derivative in r."""
    eps, sigma, a = entry[..., EPS], entry[..., SIGMA], entry[..., A_CUT]
    big_a, big_b, p, q = entry[..., BIG_A], entry[..., BIG_B], entry[..., P], entry[..., Q]
    sp, sq = (sigma / r) ** p, (sigma / r) ** q
    e = np.exp(sigma / (r - a * sigma))
    value = big_a * eps * (big_b * sp - sq) * e
    slope = big_a * eps * (-p * big_b * sp + q * sq) / r * e - value * sigma / (r - a * sigma) ** 2
    return value, slope


def energy_and_forces(positions, box, types, table, three_body_sigma_gamma_from_ijk=False):
    """positions [N,3] (Angstrom), box [3] (orthogonal sides), types [N] int, table [n,n,n,10] -> E, F [N,3], S, S_F.

    three_body_sigma_gamma_from_ijk: the OTHER reading of the mixed-species rule (both legs' sigma and gamma from the (ti,tj,tk)
    entry): what the tests show the kernel does NOT compute."""
    positions = np.asarray(positions, dtype=np.float64)
    box = np.asarray(box, dtype=np.float64)
    types = np.asarray(types)
    table = np.asarray(table, dtype=np.float64)
    n = positions.shape[0]
    shifts = IMAGES * box[None, :]
    energy, scale = 0.0, 0.0
    forces = np.zeros((n, 3))
    force_scale = np.zeros(n)

    def add(atoms, vectors):
        np.add.at(forces, atoms, vectors)
        np.add.at(force_scale, atoms, np.linalg.norm(vectors, axis=-1))

    for i in range(n):
        ti = types[i]
        d = (positions[None, :, :] + shifts[:, None, :] - positions[i]).reshape(-1, 3)           # [27 N, 3], image-major
        who = np.tile(np.arange(n), 27)
        r = np.linalg.norm(d, axis=1)
        pair_entry = table[ti, types[who], types[who]]
        inside = (r < pair_entry[:, A_CUT] * pair_entry[:, SIGMA]) & ~((who == i) & (np.arange(27 * n) // n == 13))
        d, r, who, pair_entry = d[inside], r[inside], who[inside], pair_entry[inside]
        if len(r) == 0:
            continue
        # pair terms: half of phi2 belongs to this centre, the other half to the neighbour's own sweep
        value, slope = phi2(r, pair_entry)
        energy += 0.5 * value.sum()
        scale += 0.5 * np.abs(value).sum()
        pull = (0.5 * slope / r)[:, None] * d                          # d(phi2 / 2)/d r_j = -d(phi2 / 2)/d r_i
        add(np.full(len(r), i), pull)
        add(who, -pull)
        # triplets of this centre
        ja, ka = np.triu_indices(len(r), k=1)
        if len(ja) == 0:
            continue
        tj, tk = types[who[ja]], types[who[ka]]
        triple = table[ti, tj, tk]
        leg1 = triple if three_body_sigma_gamma_from_ijk else pair_entry[ja]
        leg2 = triple if three_body_sigma_gamma_from_ijk else pair_entry[ka]
        d1, d2, r1, r2 = d[ja], d[ka], r[ja], r[ka]
        c1, c2 = pair_entry[ja][:, A_CUT] * pair_entry[ja][:, SIGMA], pair_entry[ka][:, A_CUT] * pair_entry[ka][:, SIGMA]
        g1, g2 = leg1[:, GAMMA] * leg1[:, SIGMA], leg2[:, GAMMA] * leg2[:, SIGMA]
        e1, e2 = np.exp(g1 / (r1 - c1)), np.exp(g2 / (r2 - c2))
        cos = (d1 * d2).sum(axis=1) / (r1 * r2)
        delta = cos - triple[:, COS0]
        strength = triple[:, LAMBDA] * triple[:, EPS] * e1 * e2
        value = strength * delta ** 2
        energy += value.sum()
        scale += np.abs(value).sum()
        # dE/d d1 = value * (-g1 / (r1 - c1)^2) d1 / r1 + 2 strength delta (d2 / (r1 r2) - cos d1 / r1^2), likewise for d2
        grad1 = (value * (-g1 / (r1 - c1) ** 2) / r1)[:, None] * d1 + \
            (2.0 * strength * delta)[:, None] * (d2 / (r1 * r2)[:, None] - (cos / r1 ** 2)[:, None] * d1)
        grad2 = (value * (-g2 / (r2 - c2) ** 2) / r2)[:, None] * d2 + \
            (2.0 * strength * delta)[:, None] * (d1 / (r1 * r2)[:, None] - (cos / r2 ** 2)[:, None] * d2)
        add(who[ja], -grad1)
        add(who[ka], -grad2)
        add(np.full(len(ja), i), grad1 + grad2)
    return energy, forces, scale, float(force_scale.max()) if n else 0.0


def batch(relative_coordinates, lattice_sides, types, table, **options):
    """The same on a batch at binary32 inputs promoted once: position = relative x side in binary64."""
    relative = np.asarray(relative_coordinates).astype(np.float64)
    sides = np.asarray(lattice_sides).astype(np.float64)[:, :3]
    out = [energy_and_forces(relative[b] * sides[b][None, :], sides[b], np.asarray(types)[b], table, **options)
           for b in range(relative.shape[0])]
    return (np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out]),
            np.array([o[3] for o in out]))


def neighbour_counts(relative_coordinates, lattice_sides, types, table):
    """[B,N]: neighbours of every atom inside the symmetric list cutoff max(a sigma of (ti,tj,tj), of (tj,ti,ti))."""
    relative = np.asarray(relative_coordinates).astype(np.float64)
    sides = np.asarray(lattice_sides).astype(np.float64)[:, :3]
    types = np.asarray(types)
    cut = table[..., A_CUT] * table[..., SIGMA]
    counts = np.zeros(relative.shape[:2], dtype=np.int64)
    for b in range(relative.shape[0]):
        pos = relative[b] * sides[b][None, :]
        t = types[b]
        d = pos[None, None, :, :] + (IMAGES * sides[b])[:, None, None, :] - pos[None, :, None, :]     # [27, i, j, 3]
        r = np.linalg.norm(d, axis=-1)
        pair = np.maximum(cut[t[:, None], t[None, :], t[None, :]], cut[t[None, :], t[:, None], t[:, None]])
        counts[b] = ((r < pair[None]) & (r > 0.0)).sum(axis=(0, 2))
    return counts
