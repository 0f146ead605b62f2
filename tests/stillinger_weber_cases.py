"""Inputs of the Stillinger-Weber tests (binary32 relative coordinates, box sides and int64 types, as the sampler hands them
over) and the loaders of their fixtures.  Types index the SORTED element list: with ["Si", "Ge"], Ge is 0 and Si is 1."""
import os

import numpy as np

from conftest import GOLDEN

SW_DIR = os.path.join(GOLDEN, "stillinger_weber")
SI_SW, SIGE_SW = os.path.join(SW_DIR, "Si.sw"), os.path.join(SW_DIR, "SiGe.sw")
A_SI = 5.43

_BASIS = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0], [.25, .25, .25], [.25, .75, .75], [.75, .25, .75],
                   [.75, .75, .25]])


def lammps_frames():
    return np.load(os.path.join(SW_DIR, "lammps_si8_frames.npz"))


def table(path, elements):
    from diffusion_for_multi_scale_molecular_dynamics_amd.utils.structure_utils import read_stillinger_weber_coefficients
    return read_stillinger_weber_coefficients(path, elements).numpy()


def diamond_sites(n):
    """[8 n^3, 3] relative coordinates of n x n x n conventional diamond cells; atom 8 c + s is site s of cell c (sites 0-3 one
    fcc sublattice, 4-7 the other)."""
    cells = np.array([[i, j, k] for i in range(n) for j in range(n) for k in range(n)], dtype=np.float64)
    return ((cells[:, None, :] + _BASIS[None, :, :]) / n).reshape(-1, 3)


def sublattice(n):
    """[8 n^3] 0 / 1: which fcc sublattice a diamond site belongs to (zincblende: one species each)."""
    return np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), n ** 3)


def displaced_crystal(n, batch, seed, lattice=A_SI, stretch=(1.0, 1.0, 1.0), displacement=0.08):
    """Thermally displaced diamond: Gaussian displacements of `displacement` Angstrom on the sites."""
    rng = np.random.default_rng(seed)
    sides = np.array([lattice * n * s for s in stretch])
    x = diamond_sites(n)[None] + rng.normal(size=(batch, 8 * n ** 3, 3)) * displacement / sides
    x = np.mod(x, 1.0).astype(np.float32)
    return x, np.tile(sides.astype(np.float32), (batch, 1))


def random_gas(n_atoms, batch, seed, low=5.0, high=10.0):
    """Uniform random atoms in boxes with sides uniform in [low, high] Angstrom."""
    rng = np.random.default_rng(seed)
    return rng.random((batch, n_atoms, 3)).astype(np.float32), rng.uniform(low, high, size=(batch, 3)).astype(np.float32)


def with_angles(sides):
    """[B,6] lattice parameters: the sides and three zero angles, as the sampler's L."""
    return np.concatenate([sides, np.zeros_like(sides)], axis=1)


def restatement_cases():
    """name -> (relative f32 [B,N,3], sides f32 [B,3], types int64 [B,N], coefficient file, elements)."""
    rng = np.random.default_rng(99)
    cases = {}
    for n, batch in ((1, 512), (2, 16), (3, 4)):
        x, sides = displaced_crystal(n, batch, seed=10 + n)
        cases[f"si_n{8 * n ** 3}"] = (x, sides, np.zeros(x.shape[:2], dtype=np.int64), SI_SW, ["Si"])
    x, sides = displaced_crystal(2, 16, seed=20, lattice=5.54)
    cases["sige_n64_random_species"] = (x, sides, rng.integers(0, 2, size=x.shape[:2]), SIGE_SW, ["Si", "Ge"])
    x, sides = displaced_crystal(2, 8, seed=21, stretch=(1.0, 1.04, 0.97))
    cases["si_n64_orthorhombic"] = (x, sides, np.zeros(x.shape[:2], dtype=np.int64), SI_SW, ["Si"])
    for n_atoms in (8, 12, 16):
        x, sides = random_gas(n_atoms, 32, seed=30 + n_atoms)
        cases[f"gas_n{n_atoms}"] = (x, sides, np.zeros(x.shape[:2], dtype=np.int64), SI_SW, ["Si"])
    x, sides = random_gas(12, 16, seed=40)
    cases["gas_n12_sige"] = (x, sides, rng.integers(0, 2, size=x.shape[:2]), SIGE_SW, ["Si", "Ge"])
    return cases


def gradient_case():
    """One displaced Si 1x1x1 crystal whose relative coordinates are multiples of 2^-20 (so shifts of 2^-12 and 2^-13 are exact in
    binary32) in a 5.43 A box."""
    x, sides = displaced_crystal(1, 1, seed=50)
    x = (np.round(x.astype(np.float64) * 2 ** 20) / 2 ** 20).astype(np.float32)
    return x, sides, np.zeros((1, 8), dtype=np.int64)


STENCIL_H = (2.0 ** -12, 2.0 ** -13)


def stencil_forces(energy_of, x, sides):
    """-dE/dr by the five-point stencil at relative steps h = 2^-12 and 2^-13, Richardson-extrapolated in h (the stencil's
    error is O(h^4): (16 D(h/2) - D(h)) / 15).  energy_of(relative f32 [M,N,3]) -> energies [M].  x: [1,N,3]."""
    n = x.shape[1]
    shifted, index = [], []
    for h in STENCIL_H:
        for atom in range(n):
            for axis in range(3):
                for m in (-2, -1, 1, 2):
                    y = x[0].copy()
                    y[atom, axis] = np.float32(y[atom, axis] + np.float32(m * h))
                    assert float(y[atom, axis]) == float(x[0, atom, axis]) + m * h              # exact in binary32
                    shifted.append(y)
                    index.append((h, atom, axis, m))
    energies = np.asarray(energy_of(np.stack(shifted)), dtype=np.float64)
    value = {key: e for key, e in zip(index, energies)}
    out = np.zeros((n, 3))
    for atom in range(n):
        for axis in range(3):
            d = []
            for h in STENCIL_H:
                e = {m: value[(h, atom, axis, m)] for m in (-2, -1, 1, 2)}
                d.append((e[-2] - 8.0 * e[-1] + 8.0 * e[1] - e[2]) / (12.0 * h * float(sides[0, axis])))
            out[atom, axis] = -(16.0 * d[1] - d[0]) / 15.0
    return out
