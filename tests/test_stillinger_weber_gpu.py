"""The Stillinger-Weber kernel (mdx_stillinger_weber_energy_forces) and what stands on it: against the record LAMMPS wrote,
against the tests' binary64 restatement on identical inputs, anchors that need no restatement, the mixed-species rule, forces
as the energy's gradient, determinism and capture, the status paths, and the CLI writing energies.pt.

Bars against the restatement (tests/stillinger_weber_restatement.py): |dE| <= 1e-11 S and |dF| <= 1e-10 S_F per structure,
with S = sum |energy terms| and S_F = max over atoms of sum |force contributions|.  Both sides are binary64 on the same
binary32 inputs and differ by a few ulp per term and by the order of the sums: about 1e-13 S, two (three) orders of slack."""
import numpy as np
import pytest
import torch
import yaml

import stillinger_weber_cases as cases
import stillinger_weber_restatement as restatement
from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, sample_diffusion
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (ATOM_TYPES, AXL, AXL_COMPOSITION, LATTICE_PARAMETERS,
                                                                          RELATIVE_COORDINATES)
from diffusion_for_multi_scale_molecular_dynamics_amd.utils.structure_utils import (
    StillingerWeberParameters, compute_stillinger_weber_energies_and_forces)

pytestmark = pytest.mark.gpu

E_BAR, F_BAR = 1e-11, 1e-10


def _gpu(cuda, x, sides, types, table, **options):
    """The kernel on numpy inputs -> (energies [B], forces [B,N,3]) as numpy binary64."""
    energies, forces = kernels.stillinger_weber_energy_forces(
        torch.from_numpy(np.ascontiguousarray(x)).to(cuda), torch.from_numpy(np.ascontiguousarray(sides)).to(cuda),
        torch.from_numpy(np.ascontiguousarray(types)).to(cuda), torch.from_numpy(table).to(cuda), **options)
    return energies.cpu().numpy(), None if forces is None else forces.cpu().numpy()


def _phi2(r, entry):
    return float(restatement.phi2(np.float64(r), np.asarray(entry))[0])


def test_against_the_lammps_record(cuda):
    """The 11 frames at binary32 inputs (relative = x / box, side = box, both rounded to binary32): every frame within 1.2e-5 eV
    and 3.2e-4 eV/A of the record (the bars of the CPU test: twice what binary64 shows, set by the dump's 6 digits), the GPU and
    the restatement at those same inputs within the restatement bars.

    Frame 0 to 1e-10 eV: its positions are exact in the dump, but the box side 5.43 is not a binary32 number
    (float32(5.43) = 5.43 - 1.7e-7), and the crystal at 5.43 A is under a little pressure: at the rounded side the energy moves
    by 5.0e-9 eV (the restatement shows the same 5.05e-9).  The potential depends on lengths through r / sigma alone, so frame 0
    is ALSO evaluated in the length unit in which the box is exact in binary32 -- side 5.5, relative coordinates multiples of
    1/4, sigma' = sigma * 5.5 / 5.43 in the binary64 table: the same energy, forces times 5.43 / 5.5 -- and THAT is held to the
    record's -34.6927860387157 eV within 1e-10 eV."""
    frames = cases.lammps_frames()
    table = cases.table(cases.SI_SW, ["Si"])
    sides = frames["box"].astype(np.float32)
    x = np.mod(frames["x"] / frames["box"][:, None, :], 1.0).astype(np.float32)
    types = np.zeros((11, 8), dtype=np.int64)
    energies, forces = _gpu(cuda, x, cases.with_angles(sides), types, table)
    want_e, want_f, scale, force_scale = restatement.batch(x, sides, types, table)
    for k in range(11):
        print(f"frame {k}: GPU - record {abs(energies[k] - frames['pot_eng'][k]):.3e} eV, "
              f"{np.abs(forces[k] - frames['f'][k]).max():.3e} eV/A; GPU - restatement {abs(energies[k] - want_e[k]) / scale[k]:.2e} S, "
              f"{np.abs(forces[k] - want_f[k]).max() / force_scale[k]:.2e} S_F")
    assert np.abs(energies - frames["pot_eng"]).max() <= 1.2e-5
    assert np.abs(forces - frames["f"]).max() <= 3.2e-4
    assert np.all(np.abs(energies - want_e) <= E_BAR * scale)
    assert np.all(np.abs(forces - want_f).max(axis=(1, 2)) <= F_BAR * force_scale)
    # frame 0 in the unit where its box is a binary32 number
    unit = 5.5 / 5.43
    scaled = table.copy()
    scaled[..., restatement.SIGMA] *= unit
    x0 = (frames["x"][:1] / 5.43).astype(np.float32)
    assert np.array_equal(x0.astype(np.float64) * 4.0, np.round(x0.astype(np.float64) * 4.0))
    e0, f0 = _gpu(cuda, x0, np.full((1, 3), 5.5, dtype=np.float32), types[:1], scaled)
    print(f"frame 0, exact box: GPU - record {abs(e0[0] - frames['pot_eng'][0]):.3e} eV, forces {np.abs(f0 * unit - frames['f'][:1]).max():.3e}")
    assert abs(e0[0] - frames["pot_eng"][0]) <= 1e-10
    assert np.abs(f0 * unit - frames["f"][:1]).max() <= 1e-10


@pytest.mark.parametrize("name", list(cases.restatement_cases()))
def test_against_the_restatement(cuda, name):
    x, sides, types, path, elements = cases.restatement_cases()[name]
    table = cases.table(path, elements)
    lattice = cases.with_angles(sides) if x.shape[1] % 16 else sides          # both lattice strides
    energies, forces = _gpu(cuda, x, lattice, types, table)
    want_e, want_f, scale, force_scale = restatement.batch(x, sides, types, table)
    ratio_e = np.abs(energies - want_e) / scale
    ratio_f = np.abs(forces - want_f).max(axis=(1, 2)) / force_scale
    print(f"{name}: B {x.shape[0]} N {x.shape[1]}: max |dE| / S = {ratio_e.max():.3e}, max |dF| / S_F = {ratio_f.max():.3e}")
    assert np.all(ratio_e <= E_BAR) and np.all(ratio_f <= F_BAR)
    # energies alone: the same bits
    only_e, none = _gpu(cuda, x, lattice, types, table, with_forces=False)
    assert none is None and np.array_equal(only_e, energies)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_perfect_diamond_silicon(cuda, n):
    """E = 2 N phi2(a sqrt(3) / 4) to 1e-11 relative: four first neighbours per atom at the tetrahedral angle (the three-body term
    vanishes), the second neighbours at a / sqrt(2) = 3.84 A outside a sigma = 3.771 A; a = the binary32 side / n.
    Forces <= 1e-10 eV/A where the sites are binary32 numbers (1 x 1 x 1, 2 x 2 x 2: multiples of 1/8).  The sites of 3 x 3 x 3
    are multiples of 1/12, which binary32 rounds by up to 2^-25 x 16.29 A = 4.9e-7 A: the crystal handed over is not perfect, and
    the forces AT THOSE SITES are 9.2e-6 eV/A (the restatement's figure, a stiffness of ~10 eV/A^2 times the rounding) -- no
    evaluation gives less.  There the forces are held to the restatement at the same rounded sites within the force bar; the
    energy, stationary at the perfect sites, keeps the 1e-11."""
    table = cases.table(cases.SI_SW, ["Si"])
    count = 8 * n ** 3
    x = cases.diamond_sites(n)[None].astype(np.float32)
    sides = np.full((1, 3), cases.A_SI * n, dtype=np.float32)
    a = float(sides[0, 0]) / n
    assert a / np.sqrt(2.0) > table[0, 0, 0, 1] * table[0, 0, 0, 2]
    types = np.zeros((1, count), dtype=np.int64)
    energies, forces = _gpu(cuda, x, sides, types, table)
    want = 2.0 * count * _phi2(a * np.sqrt(3.0) / 4.0, table[0, 0, 0])
    print(f"diamond {n}^3: E = {energies[0]:.12f} eV, formula {want:.12f}, max |F| = {np.abs(forces).max():.3e}")
    assert abs(energies[0] - want) <= 1e-11 * abs(want)
    if n < 3:
        assert np.abs(forces).max() <= 1e-10
    else:
        _, want_f, _, force_scale = restatement.batch(x, sides, types, table)
        assert np.abs(forces - want_f).max() <= F_BAR * force_scale[0] and np.abs(forces).max() <= 2e-5


def test_zincblende_sige_and_the_single_species_limit(cuda):
    """Zincblende SiGe through SiGe.sw: E = 2 N phi2_SiGe(d) (every bond is Si-Ge, every angle tetrahedral).  And all-Si types
    through SiGe.sw give the bits of a single-species call with its Si entry."""
    table = cases.table(cases.SIGE_SW, ["Si", "Ge"])
    ge, si = 0, 1
    a, n = 5.625, 2            # a binary32 number with a / sqrt(2) = 3.977 A beyond the largest cutoff (Ge-Ge, 3.926 A)
    count = 8 * n ** 3
    x = cases.diamond_sites(n)[None].astype(np.float32)
    side = np.full((1, 3), a * n, dtype=np.float32)
    assert a / np.sqrt(2.0) > (table[..., 1] * table[..., 2]).max()
    energies, forces = _gpu(cuda, x, side, cases.sublattice(n)[None].astype(np.int64), table)
    want = 2.0 * count * _phi2(a * np.sqrt(3.0) / 4.0, table[si, ge, ge])
    print(f"zincblende: E = {energies[0]:.12f} eV, formula {want:.12f}, max |F| = {np.abs(forces).max():.3e}")
    assert abs(energies[0] - want) <= 1e-11 * abs(want) and np.abs(forces).max() <= 1e-10
    xd, sides = cases.displaced_crystal(2, 8, seed=60)
    both = _gpu(cuda, xd, sides, np.full(xd.shape[:2], si, dtype=np.int64), table)
    single = _gpu(cuda, xd, sides, np.zeros(xd.shape[:2], dtype=np.int64), np.ascontiguousarray(table[si:si + 1, si:si + 1, si:si + 1]))
    assert np.array_equal(both[0], single[0]) and np.array_equal(both[1], single[1])


def test_mixed_species_rule_is_resolved(cuda):
    """The three-body legs take sigma, a, gamma from the (i, j, j) and (i, k, k) entries (LAMMPS's rule).  The other reading --
    both legs' sigma and gamma from the (i, j, k) entry -- is a different function on the SiGe case: measured on the CPU, the two
    restatements differ by >= 1.7e7 force bars on every structure and by 1e3 - 8e6 energy bars (median 3e6; on one structure the
    changes of the two legs nearly cancel in the energy), so the GPU, inside one bar of the first, is > 1000 bars from the
    second.  No LAMMPS run pins the mixed rule: the record is single-species."""
    x, sides, types, path, elements = cases.restatement_cases()["sige_n64_random_species"]
    table = cases.table(path, elements)
    energies, forces = _gpu(cuda, x, sides, types, table)
    other_e, other_f, scale, force_scale = restatement.batch(x, sides, types, table, three_body_sigma_gamma_from_ijk=True)
    ratio_e = np.abs(energies - other_e) / (E_BAR * scale)
    ratio_f = np.abs(forces - other_f).max(axis=(1, 2)) / (F_BAR * force_scale)
    print(f"other rule: energy {ratio_e.min():.3e} .. {ratio_e.max():.3e} bars, forces {ratio_f.min():.3e} .. {ratio_f.max():.3e} bars")
    assert ratio_f.min() > 1000.0 and ratio_e.min() > 1000.0


# what the restatement shows between its own stencil and its analytic forces on cases.gradient_case(), measured on the CPU
# (eV/A): round-off of the energies (~1e-14 eV) over the step (2^-13 x 5.43 A), the stencil's own error being O(h^4)
RESTATEMENT_STENCIL_DISTANCE = 1.24e-11


def test_forces_are_the_gradient_of_the_energy(cuda):
    x, sides, types = cases.gradient_case()
    table = cases.table(cases.SI_SW, ["Si"])
    _, forces = _gpu(cuda, x, sides, types, table)

    def energy_of(shifted):
        m = shifted.shape[0]
        return _gpu(cuda, shifted, np.tile(sides, (m, 1)), np.tile(types, (m, 1)), table, with_forces=False)[0]

    numeric = cases.stencil_forces(energy_of, x, sides)
    distance = np.abs(numeric - forces[0]).max()
    print(f"stencil of the GPU energies vs the GPU forces: {distance:.3e} eV/A (max |F| {np.abs(forces).max():.3f}); "
          f"bar {2 * RESTATEMENT_STENCIL_DISTANCE:.3e}")
    assert distance <= 2.0 * RESTATEMENT_STENCIL_DISTANCE


def _bits(t):
    return t.view(torch.int64)


def test_determinism_and_capture(cuda):
    x, sides, types, path, elements = cases.restatement_cases()["sige_n64_random_species"]
    dev = [torch.from_numpy(np.ascontiguousarray(t)).to(cuda) for t in (x, sides, types, cases.table(path, elements))]
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    first = kernels.stillinger_weber_energy_forces(*dev, status=status)
    second = kernels.stillinger_weber_energy_forces(*dev, status=status)
    assert torch.equal(_bits(first[0]), _bits(second[0])) and torch.equal(_bits(first[1]), _bits(second[1]))
    assert not torch.isnan(first[0]).any()
    # no host read with a caller's status word: the call is captured, and its replay writes the same bits
    workspace = torch.empty(int(_hip.lib().mdx_stillinger_weber_workspace_doubles(x.shape[0], x.shape[1], 64)),
                            dtype=torch.float64, device=cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = kernels.stillinger_weber_energy_forces(*dev, status=status, workspace=workspace)
    captured[0].fill_(0.0)
    captured[1].fill_(0.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(first[0]), _bits(captured[0])) and torch.equal(_bits(first[1]), _bits(captured[1]))
    assert int(status.item()) == 0


def test_status_paths(cuda):
    table = cases.table(cases.SI_SW, ["Si"])
    x, sides = cases.displaced_crystal(1, 3, seed=70)
    types = np.zeros((3, 8), dtype=np.int64)
    dev = lambda *arrays: [torch.from_numpy(np.ascontiguousarray(t)).to(cuda) for t in arrays]          # noqa: E731
    good_e, good_f = _gpu(cuda, x, sides, types, table)
    # a side below a sigma = 3.771 A: NaN for that structure alone, and the bit
    short = sides.copy()
    short[1, 2] = 3.7
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    e, f = kernels.stillinger_weber_energy_forces(*dev(x, short, types, table), status=status)
    assert int(status.item()) == _hip.STATUS_CUTOFF_TOO_LARGE
    assert torch.isnan(e[1]) and torch.isnan(f[1]).all() and np.array_equal(e[[0, 2]].cpu().numpy(), good_e[[0, 2]])
    assert np.array_equal(f[[0, 2]].cpu().numpy(), good_f[[0, 2]])
    with pytest.raises(_hip.MdxError, match="shorter than the largest cutoff"):
        kernels.stillinger_weber_energy_forces(*dev(x, short, types, table))
    # a MASK type (= the number of types) and a negative one
    for bad in (1, -1):
        masked = types.copy()
        masked[2, 5] = bad
        status.zero_()
        e, f = kernels.stillinger_weber_energy_forces(*dev(x, sides, masked, table), status=status)
        assert int(status.item()) == _hip.STATUS_SW_ATOM_TYPE
        assert torch.isnan(e[2]) and torch.isnan(f[2]).all() and np.array_equal(e[:2].cpu().numpy(), good_e[:2])
        with pytest.raises(_hip.MdxError, match="outside the parameter table"):
            kernels.stillinger_weber_energy_forces(*dev(x, sides, masked, table))
    # neighbour overflow: the densest test case has 20 neighbours on an atom (counted by the restatement), the default
    # capacity 64 covers every case; a capacity of 19 raises, and the sample-contract function grows it
    densest = 0
    for name, (cx, cs, ct, path, elements) in cases.restatement_cases().items():
        densest = max(densest, int(restatement.neighbour_counts(cx, cs, ct, cases.table(path, elements)).max()))
    print(f"densest neighbour list of the cases: {densest}")
    assert densest == 20 and densest <= kernels.SW_NEIGHBOUR_CAPACITY
    gx, gs, gt, path, elements = cases.restatement_cases()["gas_n16"]
    status.zero_()
    e, f = kernels.stillinger_weber_energy_forces(*dev(gx, gs, gt, table), neighbour_capacity=19, status=status)
    counts = restatement.neighbour_counts(gx, gs, gt, table).max(axis=1)
    assert int(status.item()) == _hip.STATUS_SW_NEIGHBOURS
    assert np.array_equal(torch.isnan(e).cpu().numpy(), counts > 19) and (counts > 19).any() and (counts <= 19).any()
    with pytest.raises(kernels.StillingerWeberNeighbourCapacityError, match="neighbour_capacity=19"):
        kernels.stillinger_weber_energy_forces(*dev(gx, gs, gt, table), neighbour_capacity=19)
    assert np.array_equal(_gpu(cuda, gx, gs, gt, table, neighbour_capacity=20)[0], _gpu(cuda, gx, gs, gt, table)[0])
    # limits
    with pytest.raises(_hip.MdxError, match="unsupported"):
        kernels.stillinger_weber_energy_forces(torch.zeros(1, 1025, 3, device=cuda), torch.full((1, 3), 50.0, device=cuda),
                                               torch.zeros(1, 1025, dtype=torch.int64, device=cuda), dev(table)[0])


def test_sample_contract(cuda, tmp_path):
    """compute_stillinger_weber_energies_and_forces: AXL_COMPOSITION or the three keys, CPU inputs moved to the device, angles
    ignored, a negative side clipped to 1.0 and a side below 3.0 A skipped with energy 0, both with a warning."""
    parameters = StillingerWeberParameters(sw_coeff_filename=cases.SI_SW, elements=["Si"])
    x, sides = cases.displaced_crystal(1, 4, seed=80)
    types = np.zeros((4, 8), dtype=np.int64)
    want_e, want_f = _gpu(cuda, x, sides, types, cases.table(cases.SI_SW, ["Si"]))
    lattice = cases.with_angles(sides)
    lattice[:, 3:] = 0.3                                                     # angles are zeroed by the contract: not read
    axl = AXL(A=torch.from_numpy(types), X=torch.from_numpy(x), L=torch.from_numpy(lattice))
    e, f = compute_stillinger_weber_energies_and_forces({AXL_COMPOSITION: axl}, parameters)
    assert e.is_cuda and e.dtype == torch.float64 and e.shape == (4,) and f.shape == (4, 8, 3) and f.dtype == torch.float64
    assert np.array_equal(e.cpu().numpy(), want_e) and np.array_equal(f.cpu().numpy(), want_f)
    keys = {RELATIVE_COORDINATES: axl.X.to(cuda), LATTICE_PARAMETERS: axl.L.to(cuda), ATOM_TYPES: axl.A.to(cuda)}
    e2, _ = compute_stillinger_weber_energies_and_forces(keys, parameters)
    assert np.array_equal(e2.cpu().numpy(), want_e)
    bad = lattice.copy()
    bad[1, 0] = -2.0            # clipped to 1.0, then below 3.0: skipped
    bad[3, 1] = 2.9             # skipped
    with pytest.warns(UserWarning) as record:
        e3, f3 = compute_stillinger_weber_energies_and_forces({AXL_COMPOSITION: axl._replace(L=torch.from_numpy(bad))}, parameters)
    messages = " ".join(str(w.message) for w in record)
    assert "negative lattice parameter" in messages and "smaller than 3.0 Angstrom" in messages
    assert e3[1] == 0.0 and e3[3] == 0.0 and not f3[1].any() and not f3[3].any()
    assert np.array_equal(e3[[0, 2]].cpu().numpy(), want_e[[0, 2]]) and np.array_equal(f3[[0, 2]].cpu().numpy(), want_f[[0, 2]])
    assert axl.L[1, 0] == lattice[1, 0]                                      # the inputs are not modified
    # a dense gas beyond the default capacity: the capacity grows, nothing is truncated
    gx, gs = cases.random_gas(96, 2, seed=81, low=6.0, high=6.5)
    gt = np.zeros((2, 96), dtype=np.int64)
    table = cases.table(cases.SI_SW, ["Si"])
    assert restatement.neighbour_counts(gx, gs, gt, table).max() > kernels.SW_NEIGHBOUR_CAPACITY
    dense = {RELATIVE_COORDINATES: torch.from_numpy(gx), LATTICE_PARAMETERS: torch.from_numpy(gs), ATOM_TYPES: torch.from_numpy(gt)}
    e4, f4 = compute_stillinger_weber_energies_and_forces(dense, parameters)
    want = restatement.batch(gx, gs, gt, table)
    assert np.all(np.abs(e4.cpu().numpy() - want[0]) <= E_BAR * want[2])
    assert np.all(np.abs(f4.cpu().numpy() - want[1]).max(axis=(1, 2)) <= F_BAR * want[3])


def test_cli_writes_energies(cuda, tmp_path):
    """Random-init MLP, 10 time steps, `oracle: name: stillinger_weber`: energies.pt is the CPU float64 [n_samples] tensor of the
    function on the contents of samples.pt, within the restatement bar; `name: lammps` still writes none."""
    (tmp_path / "Si.sw").write_text(open(cases.SI_SW).read())
    cfg = dict(noise=dict(total_time_steps=10, sigma_min=1e-4, sigma_max=0.25),
               sampling=dict(algorithm="predictor_corrector", spatial_dimension=3, number_of_atoms=8, number_of_samples=12,
                             sample_batchsize=5, num_atom_types=1, number_of_corrector_steps=1,
                             use_fixed_lattice_parameters=True, cell_dimensions=[5.43, 5.43, 5.43]),
               elements=["Si"], oracle=dict(name="stillinger_weber", sw_coeff_filename="Si.sw"),
               model=dict(score_network=dict(architecture="mlp", number_of_atoms=8, num_atom_types=1, n_hidden_dimensions=2,
                                             hidden_dimensions_size=16, relative_coordinates_embedding_dimensions_size=8,
                                             noise_embedding_dimensions_size=4, time_embedding_dimensions_size=4,
                                             atom_type_embedding_dimensions_size=1,
                                             lattice_parameters_embedding_dimensions_size=1)))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    sample_diffusion.main(["--config", str(tmp_path / "config.yaml"), "--output", str(tmp_path / "out"), "--device", "cuda",
                           "--random_init_seed", "3"])
    energies = torch.load(tmp_path / "out" / "energies.pt")
    assert energies.dtype == torch.float64 and energies.shape == (12,) and not energies.is_cuda
    samples = torch.load(tmp_path / "out" / "samples.pt", weights_only=False)
    parameters = StillingerWeberParameters(sw_coeff_filename=str(tmp_path / "Si.sw"), elements=["Si"])
    again, _ = compute_stillinger_weber_energies_and_forces(samples, parameters)
    assert torch.equal(_bits(again.cpu()), _bits(energies))
    axl = samples[AXL_COMPOSITION]
    want = restatement.batch(axl.X.cpu().numpy(), axl.L.cpu().numpy(), axl.A.cpu().numpy(), cases.table(cases.SI_SW, ["Si"]))
    assert np.all(np.abs(energies.numpy() - want[0]) <= E_BAR * want[2]) and want[2].min() > 0.0
    log = (tmp_path / "out" / "console.log").read_text()
    assert "Compute energy from Oracle..." in log and "Writing energies to disk..." in log and "energies.pt is not" not in log
    (tmp_path / "lammps.yaml").write_text(yaml.safe_dump(dict(cfg, oracle=dict(name="lammps", sw_coeff_filename="Si.sw"))))
    sample_diffusion.main(["--config", str(tmp_path / "lammps.yaml"), "--output", str(tmp_path / "lammps"), "--device", "cuda",
                           "--random_init_seed", "3"])
    assert not (tmp_path / "lammps" / "energies.pt").exists()
    assert "energies.pt is not" in (tmp_path / "lammps" / "console.log").read_text()
