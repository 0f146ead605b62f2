"""GPU tests of the excise-and-random path: mdx_random_fill_environments against the reference's recorded samples
(tests/golden/excise_and_random/, made by tests/golden/make_golden_excise_and_random.py) and against the numpy restatement of
tests/excise_random_cases.py, mdx_random_fill_proposals, and the sample makers end to end.

Bars.  Atom types, coordinates, active indices, attempts and accepted flags: exact (a sample's coordinates are copies of the
inputs, or corner + u / p rounded as numpy rounds it).  min_distance: 1e-12 Angstrom against the restatement (one sqrt of the
same binary64 sum; the last place of sqrt and nothing more).  The uniform draws: mean and decile counts within 5 standard
deviations, with a fixed seed."""
import logging
from unittest import mock

import numpy as np
import pytest
import torch

import excise_cases as ec
import excise_random_cases as rc
from conftest import load_golden

pytestmark = pytest.mark.gpu

S, M = rc.SAMPLES_PER_ENVIRONMENT, rc.MAX_ATTEMPTS


def _kernels():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    return kernels, _hip


def _axl():
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL
    return AXL


def _fill(cuda, uniforms, types, voxels, partition, cx, ca, counts, active, environment, sides, threshold, status=None):
    """kernels.random_fill_environments on numpy inputs -> dict of numpy outputs."""
    kernels, _ = _kernels()
    dev = lambda v, dtype: None if v is None else torch.tensor(np.asarray(v), dtype=dtype, device=cuda)      # noqa: E731
    out = kernels.random_fill_environments(
        dev(uniforms, torch.float64), dev(types, torch.int32), dev(voxels, torch.int32), partition, dev(cx, torch.float64),
        dev(ca, torch.int64), dev(counts, torch.int32), dev(active, torch.int32), dev(environment, torch.int32),
        dev(sides, torch.float64), threshold, status=status)
    return dict(zip(("X", "A", "active", "attempts", "accepted", "min_distance"), [t.cpu().numpy() for t in out]))


def _compare_with_restatement(got, uniforms, types, voxels, partition, cx, ca, counts, environment, sides, threshold):
    worst = 0.0
    for b, e in enumerate(environment):
        want = rc.fill(uniforms[b], types[b], None if voxels is None else voxels[b], partition, cx[e, :counts[e]],
                       ca[e, :counts[e]], sides[e], threshold)
        assert np.array_equal(got["X"][b], want["X"]) and np.array_equal(got["A"][b], want["A"]), b
        assert got["attempts"][b] == want["attempts"] and bool(got["accepted"][b]) == want["accepted"], b
        if np.isfinite(want["min_distance"]):
            worst = max(worst, abs(got["min_distance"][b] - want["min_distance"]))
    assert worst <= 1e-12, worst
    return worst


# ------------------------------------------------------------------------------------------------------------------
# 1. the fill kernel against the reference's recorded samples
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.case_names())
def test_fill_kernel_reproduces_the_recorded_samples(cuda, case):
    g = load_golden(f"excise_and_random/{case}.npz")
    voxels = g["voxels"] if "voxels" in g else None
    partition = [int(p) for p in g["partition"]] if voxels is not None else None
    E = len(g["counts"])
    environment = np.repeat(np.arange(E), S)
    sides = np.tile(g["box"][:3], (E, 1))
    for t, threshold in enumerate(g["thresholds"]):
        got = _fill(cuda, g["uniforms"], g["types"], voxels, partition, g["constrained_x"], g["constrained_a"], g["counts"],
                    g["central"], environment, sides, float(threshold))
        assert got["X"].dtype == np.float64 and got["A"].dtype == np.int64
        assert np.array_equal(got["X"], g[f"t{t}_X"]) and np.array_equal(got["A"], g[f"t{t}_A"]), (case, t)
        assert np.array_equal(got["active"], g[f"t{t}_active"]) and np.array_equal(got["attempts"], g[f"t{t}_attempts"])
        assert np.array_equal(got["accepted"].astype(bool), g[f"t{t}_accepted"])
        worst = _compare_with_restatement(got, g["uniforms"], g["types"], voxels, partition, g["constrained_x"], g["constrained_a"],
                                          g["counts"], environment, sides, float(threshold))
        recorded = g["distances"][np.arange(len(environment)), got["attempts"] - 1]         # the reference's own distances
        assert np.abs(got["min_distance"] - recorded).max() <= 1e-12
        print(f"{case}, threshold {threshold}: attempts {list(got['attempts'])}, max |d - d_restated| = {worst:.1e}")


# ------------------------------------------------------------------------------------------------------------------
# 2. one and two dimensions, edge cases, status
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("voxel", [False, True])
def test_fill_kernel_in_one_and_two_dimensions(cuda, d, voxel):
    rng = np.random.default_rng(10 * d + voxel)
    E, K, N, attempts = 2, 3, 7, 3
    B = E * 2
    uniforms, types = rng.random((B, attempts, N, d)), rng.integers(0, 3, size=(B, attempts, N))
    partition = [3, 2][:d] if voxel else None
    voxels = rng.integers(0, int(np.prod(partition)), size=(B, attempts, N)) if voxel else None
    cx, ca = rng.random((E, K, d)), rng.integers(0, 3, size=(E, K))
    counts, sides = np.array([3, 2]), np.array([[5.0, 6.0][:d], [4.0, 7.0][:d]])
    environment = np.array([0, 0, 1, 1])
    seen = set()
    for threshold in (0.0, 0.2, 0.6):
        got = _fill(cuda, uniforms, types, voxels, partition, cx, ca, counts, [1, 0], environment, sides, threshold)
        _compare_with_restatement(got, uniforms, types, voxels, partition, cx, ca, counts, environment, sides, threshold)
        assert list(got["active"]) == [1, 1, 0, 0]
        seen |= set(got["attempts"])
    assert len(seen) > 1                                        # (the thresholds do make the kernel retry)


def test_fill_kernel_edge_cases(cuda):
    rng = np.random.default_rng(99)
    N, attempts = 6, 3
    uniforms, types = rng.random((4, attempts, N, 3)), rng.integers(0, 2, size=(4, attempts, N))
    uniforms[3, :, 4] = uniforms[3, :, 5] = [0.1, 0.1, 0.1]           # sample 3: two proposed sites coincide in every attempt
    uniforms[3, :, 0] = [0.5, 0.5, 0.52]
    cx, ca = rng.random((3, N, 3)), rng.integers(0, 2, size=(3, N))
    cx[2, 0] = [0.5, 0.5, 0.5]
    counts, sides = np.array([N, 1, 1]), np.full((3, 3), 7.0)
    environment = np.array([0, 1, 1, 2])
    got = _fill(cuda, uniforms, types, None, None, cx, ca, counts, [N - 1, 0, 0], environment, sides, 0.0)
    _compare_with_restatement(got, uniforms, types, None, None, cx, ca, counts, environment, sides, 0.0)
    # count = N: nothing is generated -- the sample is the environment
    assert np.array_equal(got["X"][0], cx[0]) and np.array_equal(got["A"][0], ca[0]) and got["active"][0] == N - 1
    # count = 1: the constrained atom and the five sites it did not take, in their order
    assert np.array_equal(got["X"][1][0], cx[1, 0]) and got["A"][1][0] == ca[1, 0]
    assert all(any(np.array_equal(row, site) for site in uniforms[1, 0]) for row in got["X"][1][1:])
    # a threshold of 0 accepts the first attempt when no two atoms coincide ...
    assert list(got["attempts"][:3]) == [1, 1, 1] and got["accepted"][:3].all() and (got["min_distance"][:3] > 0).all()
    # ... and rejects coincident atoms: distance 0, every attempt used, the last one returned
    assert got["min_distance"][3] == 0.0 and got["attempts"][3] == attempts and not got["accepted"][3]
    assert np.array_equal(got["X"][3][0], cx[2, 0]) and np.array_equal(got["X"][3][-1], [0.1, 0.1, 0.1])
    # max_attempts = 1: one attempt, returned whatever its distance
    got = _fill(cuda, uniforms[:, :1], types[:, :1], None, None, cx, ca, counts, [0, 0, 0], environment, sides, 100.0)
    assert list(got["attempts"]) == [1] * 4 and not got["accepted"].any()
    _compare_with_restatement(got, uniforms[:, :1], types[:, :1], None, None, cx, ca, counts, environment, sides, 100.0)


def test_fill_kernel_ties_go_to_the_lower_site(cuda):
    """Two sites mirror each other around the constrained atom: it takes the lower one, whichever side that is."""
    for flip in (False, True):
        pair = [[0.25, 0.5, 0.5], [0.75, 0.5, 0.5]][::-1 if flip else 1]
        uniforms = np.array([[[[0.1, 0.1, 0.1]] + pair + [[0.9, 0.9, 0.9]]]])
        got = _fill(cuda, uniforms, np.arange(4).reshape(1, 1, 4), None, None, [[[0.5, 0.5, 0.5]]], [[7]], [1], [0], [0],
                    [[4.0, 4.0, 4.0]], 0.5)
        assert list(got["A"][0]) == [7, 0, 2, 3] and np.array_equal(got["X"][0][2], pair[1])


def test_fill_kernel_status(cuda):
    _, _hip = _kernels()
    rng = np.random.default_rng(5)
    uniforms, types = rng.random((2, 2, 4, 3)), np.zeros((2, 2, 4), dtype=int)
    cx, ca, sides = rng.random((2, 5, 3)), np.zeros((2, 5), dtype=int), np.full((2, 3), 6.0)

    def word(counts, active, environment):
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        got = _fill(cuda, uniforms, types, None, None, cx, ca, counts, active, environment, sides, 0.5, status=status)
        return int(status.item()), got

    bits, got = word([5, 2], [0, 0], [0, 1])
    assert bits == _hip.STATUS_RANDOM_FILL_COUNT and got["attempts"][0] == 0 and not got["X"][0].any() and got["attempts"][1] >= 1
    bits, got = word([2, 2], [0, 0], [0, 2])
    assert bits == _hip.STATUS_RANDOM_FILL_ENVIRONMENT and got["attempts"][1] == 0 and not got["X"][1].any()
    assert word([2, 2], [0, 2], [0, 1])[0] == _hip.STATUS_RANDOM_FILL_ENVIRONMENT          # the active atom is not constrained
    assert word([2, 0], [0, 0], [0, 1])[0] == _hip.STATUS_RANDOM_FILL_ENVIRONMENT          # an empty environment has none
    assert word([2, 4], [1, 3], [1, 0])[0] == 0
    with pytest.raises(AssertionError, match="There are more constrained atoms 5 than total number of atoms 4."):
        _fill(cuda, uniforms, types, None, None, cx, ca, [5, 2], [0, 0], [0, 1], sides, 0.5)
    with pytest.raises(IndexError):
        _fill(cuda, uniforms, types, None, None, cx, ca, [2, 2], [0, 0], [0, -1], sides, 0.5)
    too_many = _hip.RANDOM_FILL_MAX_ATOMS + 1
    with pytest.raises(_hip.MdxError, match="at most 3 spatial dimensions and 1024 atoms"):
        _fill(cuda, np.zeros((1, 1, too_many, 3)), np.zeros((1, 1, too_many)), None, None, cx, ca, [2, 2], [0, 0], [0], sides, 0.5)
    with pytest.raises(_hip.MdxError, match="at most 3 spatial dimensions"):
        _fill(cuda, np.zeros((1, 1, 4, 4)), np.zeros((1, 1, 4)), None, None, np.zeros((2, 5, 4)), ca, [2, 2], [0, 0], [0],
              np.full((2, 4), 6.0), 0.5)


# ------------------------------------------------------------------------------------------------------------------
# 3. the proposals
# ------------------------------------------------------------------------------------------------------------------
def _proposals(cuda, seed, call, first, B, attempts, N, d, C, V):
    kernels, _ = _kernels()
    return [None if t is None else t.cpu().numpy() for t in kernels.random_fill_proposals(seed, call, first, B, attempts, N, d, C, V, cuda)]


def test_proposals_ranges_and_voxel_occupancy(cuda):
    for N, V in ((24, 18), (8, 8), (5, 8), (37, 4)):
        uniforms, types, voxels = _proposals(cuda, 11, 0, 0, 3, M, N, 3, 3, V)
        assert uniforms.shape == (3, M, N, 3) and uniforms.dtype == np.float64 and types.dtype == voxels.dtype == np.int32
        assert (uniforms >= 0).all() and (uniforms < 1).all() and (types >= 0).all() and (types < 3).all()
        assert np.array_equal(uniforms * 2.0 ** 53, np.floor(uniforms * 2.0 ** 53))                  # multiples of 2^-53
        for row in voxels.reshape(-1, N):
            occupancy = np.bincount(row, minlength=V)
            assert len(occupancy) == V and set(occupancy) <= {N // V, -(-N // V)}, (N, V, occupancy)
            assert np.array_equal(row[:(N // V) * V], np.arange((N // V) * V) % V)                   # the full rounds in order
        if N % V:
            assert len({tuple(row[(N // V) * V:]) for row in voxels.reshape(-1, N)}) > 1             # the rest is drawn
    assert _proposals(cuda, 11, 0, 0, 2, M, 8, 2, 1, 0)[2] is None


def test_proposals_are_keyed_by_seed_call_sample_and_attempt(cuda):
    base = _proposals(cuda, 2025, 3, 0, 3, M, 24, 3, 2, 18)
    again = _proposals(cuda, 2025, 3, 0, 3, M, 24, 3, 2, 18)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    head, tail = _proposals(cuda, 2025, 3, 0, 1, M, 24, 3, 2, 18), _proposals(cuda, 2025, 3, 1, 2, M, 24, 3, 2, 18)
    assert all(np.array_equal(a, np.concatenate([h, t])) for a, h, t in zip(base, head, tail))       # the batch cut in two calls
    for other in (_proposals(cuda, 2026, 3, 0, 3, M, 24, 3, 2, 18), _proposals(cuda, 2025, 4, 0, 3, M, 24, 3, 2, 18)):
        assert not np.array_equal(base[0], other[0]) and not np.array_equal(base[1], other[1])
        assert not np.array_equal(base[2], other[2]) and not np.isin(base[0], other[0]).any()
    flat = base[0].reshape(-1)
    assert len(np.unique(flat)) == len(flat)                                                          # samples, attempts, atoms, axes: all distinct


def test_proposals_are_uniform(cuda):
    uniforms, types, _ = _proposals(cuda, 7, 0, 0, 3, 4, 1024, 3, 4, 0)
    u = uniforms.reshape(-1)
    n = len(u)
    assert n == 3 * 4 * 1024 * 3
    assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1.0 / 12.0 / n)
    deciles = np.bincount(np.floor(u * 10).astype(int), minlength=10)
    assert np.abs(deciles - n / 10).max() <= 5 * np.sqrt(n * 0.1 * 0.9), deciles
    counts = np.bincount(types.reshape(-1), minlength=4)
    assert np.abs(counts - types.size / 4).max() <= 5 * np.sqrt(types.size * 0.25 * 0.75), counts
    print(f"uniforms: mean - 1/2 = {u.mean() - 0.5:+.2e}, decile counts {list(deciles)}, type counts {list(counts)}")


# ------------------------------------------------------------------------------------------------------------------
# 4. the makers end to end
# ------------------------------------------------------------------------------------------------------------------
def _maker(shape, algorithm, excisor, threshold=rc.DEFAULT_THRESHOLD, max_attempts=M):
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.atom_selector import atom_selector_factory as sf
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.excisor import excisor_factory as ef
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker import sample_maker_factory as mf
    settings = rc.SHAPES[shape]
    parameters = mf.create_sample_maker_parameters(dict(
        algorithm="excise_and_random", element_list=["Si"], sample_box_size=settings["sample_box_size"],
        total_number_of_atoms=settings["total_number_of_atoms"], number_of_samples_per_substructure=S,
        random_coordinates_algorithm=algorithm, max_attempts=max_attempts, minimal_interatomic_distance=threshold))
    return mf.create_sample_maker(parameters, sf.create_atom_selector_parameters(dict(algorithm="threshold",
                                                                                      uncertainty_threshold=ec.UNCERTAINTY_THRESHOLD)),
                                  ef.create_excisor_parameters(rc.EXCISORS[excisor]))


def _frame():
    a, x, lattice = ec.source_frame()
    return _axl()(A=a, X=x, L=lattice), ec.uncertainties()


def _check_invariants(samples, active, infos, g, N, box, threshold=None):
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker.namespace import (
        AXL_STRUCTURE_IN_NEW_BOX, AXL_STRUCTURE_IN_ORIGINAL_BOX)
    assert len(samples) == len(active) == len(infos) == len(g["counts"]) * S
    for b, (sample, index, info) in enumerate(zip(samples, active, infos)):
        e, count = b // S, g["counts"][b // S]
        assert sample.X.shape == (N, 3) and sample.X.dtype == np.float64 and sample.A.shape == (N,)
        assert np.array_equal(sample.X[:count], g["constrained_x"][e, :count])             # the reference's embedded atoms, bit for bit
        assert np.array_equal(sample.A[:count], g["constrained_a"][e, :count]) and np.array_equal(sample.L, box)
        assert (sample.X >= 0).all() and (sample.X < 1).all()
        assert index.shape == (1,) and np.allclose(sample.X[index[0]], 0.5, atol=1e-12)    # the central atom sits at the centre
        assert set(info) == {"constrained_atom_indices", AXL_STRUCTURE_IN_ORIGINAL_BOX, AXL_STRUCTURE_IN_NEW_BOX}
        assert info["constrained_atom_indices"] == list(range(count))
        assert np.array_equal(info[AXL_STRUCTURE_IN_NEW_BOX].X, g["constrained_x"][e, :count])
        assert np.array_equal(info[AXL_STRUCTURE_IN_ORIGINAL_BOX].L, ec.source_frame()[2])


@pytest.mark.parametrize("shape,algorithm,excisor", [("n8", "true_random", "spherical"), ("n24", "voxel_random", "nearest_neighbors")])
def test_batched_maker_on_the_device_draws(cuda, shape, algorithm, excisor, caplog):
    kernels, _ = _kernels()
    g = load_golden(f"excise_and_random/{rc.case_name(shape, algorithm, excisor)}.npz")
    threshold = float(g["thresholds"][1])
    maker = _maker(shape, algorithm, excisor, threshold)
    maker.rng_mode = "device"
    structure, u = _frame()
    N, box = rc.SHAPES[shape]["total_number_of_atoms"], g["box"]
    torch.manual_seed(321)
    with caplog.at_level(logging.WARNING):
        samples, active, infos = maker.make_samples(structure, u)
    _check_invariants(samples, active, infos, g, N, box)
    # the result is the restatement on the proposals the fill kernel wrote (frame 0 of this maker: call index 0)
    partition = rc.SHAPES[shape]["partition"] if algorithm == "voxel_random" else None
    uniforms, types, voxels = _proposals(cuda, 321, 0, 0, len(samples), M, N, 3, 1, int(np.prod(partition)) if partition else 0)
    exhausted = 0
    for b, sample in enumerate(samples):
        e, count = b // S, g["counts"][b // S]
        want = rc.fill(uniforms[b], types[b], None if voxels is None else voxels[b], partition, g["constrained_x"][e, :count],
                       g["constrained_a"][e, :count], box[:3], threshold)
        assert np.array_equal(sample.X, want["X"]) and np.array_equal(sample.A, want["A"]) and maker.last_attempts[b] == want["attempts"]
        assert (rc.shortest_distance(sample.X, box[:3]) > threshold) == want["accepted"]
        exhausted += not want["accepted"]
    warnings = [r.getMessage() for r in caplog.records if "could not be generated" in r.getMessage()]
    assert len(warnings) == (1 if exhausted else 0) and all(f"({exhausted} samples of this frame)" in w for w in warnings)
    # the next frame draws with the next call index
    again, _, _ = maker.make_samples(structure, u)
    assert not np.array_equal(again[0].X[g["counts"][0]:], samples[0].X[g["counts"][0]:])
    assert maker.make_samples(structure, np.zeros_like(u)) == ([], [], [])


@pytest.mark.parametrize("case", ["n8_voxel_random_spherical", "n24_true_random_nearest_neighbors"])
def test_batched_maker_on_the_recorded_proposals(cuda, case):
    """rng_mode "reference": the host draws, patched to serve the recorded tables in the batched path's order (every attempt of
    sample 0, then of sample 1, ...), give the reference's recorded samples through the whole maker -- excision kernel included."""
    shape, algorithm, excisor = case.split("_", 1)[0], "_".join(case.split("_")[1:3]), case.split("_", 3)[3]
    g = load_golden(f"excise_and_random/{case}.npz")
    voxels = g["voxels"] if "voxels" in g else None
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker import excise_and_random_sample_maker as module
    for t, threshold in enumerate(g["thresholds"]):
        maker = _maker(shape, algorithm, excisor, float(threshold))
        assert maker.rng_mode == "reference" and maker.batch_environments
        served = dict(coordinates=0, types=0, voxels=0)

        def serve(table, key):
            index = served[key]
            served[key] += 1
            return table[index // M, index % M].copy()

        cls = module.ExciseAndRandomSampleMaker
        with mock.patch.object(cls, "generate_random_relative_coordinates", staticmethod(lambda n, d=3: serve(g["uniforms"], "coordinates"))), \
                mock.patch.object(cls, "generate_atom_types", staticmethod(lambda n, c: serve(g["types"], "types"))), \
                mock.patch.object(module, "select_occupied_voxels", lambda v, n: serve(voxels, "voxels")):
            samples, active, infos = maker.make_samples(*_frame())
        assert served["coordinates"] == served["types"] == len(samples) * M
        _check_invariants(samples, active, infos, g, rc.SHAPES[shape]["total_number_of_atoms"], g["box"])
        for b, sample in enumerate(samples):
            assert np.array_equal(sample.X, g[f"t{t}_X"][b]) and np.array_equal(sample.A, g[f"t{t}_A"][b]), (t, b)
            assert active[b][0] == g[f"t{t}_active"][b] and len(infos[b]["constrained_atom_indices"]) == g[f"t{t}_constrained"][b]
        assert np.array_equal(maker.last_attempts, g[f"t{t}_attempts"])


def test_reference_mode_draws_from_numpys_global_generator(cuda):
    maker = _maker("n24", "voxel_random", "spherical")
    g = load_golden("excise_and_random/n24_voxel_random_spherical.npz")
    np.random.seed(77)
    samples, _, _ = maker.make_samples(*_frame())
    np.random.seed(77)
    for b, sample in enumerate(samples):
        uniforms, types, voxels = [], [], []
        for m in range(M):                                              # per attempt: coordinates, occupancy, types
            uniforms.append(np.random.random((24, 3)))
            voxels.append(np.concatenate([np.arange(18), np.random.choice(np.arange(18), size=6, replace=False)]))
            types.append(np.random.randint(0, 1, size=(24,)))
        e, count = b // S, g["counts"][b // S]
        want = rc.fill(uniforms, types, voxels, [3, 3, 2], g["constrained_x"][e, :count], g["constrained_a"][e, :count], g["box"][:3], 0.5)
        assert np.array_equal(sample.X, want["X"]) and np.array_equal(sample.A, want["A"])


@pytest.mark.parametrize("algorithm", rc.ALGORITHMS)
def test_host_flow_with_kernel_excision(cuda, algorithm):
    """batch_environments = False: the excision is the kernel's, the placement the host's, one environment after the other."""
    g = load_golden(f"excise_and_random/n8_{algorithm}_spherical.npz")
    maker = _maker("n8", algorithm, "spherical")
    maker.batch_environments = False
    np.random.seed(12)
    samples, active, infos = maker.make_samples(*_frame())
    _check_invariants(samples, active, infos, g, 8, g["box"])
    assert maker.last_attempts is None
    for sample in samples:
        assert maker.get_shortest_distance_between_atoms(sample.X, sample.L) == pytest.approx(rc.shortest_distance(sample.X, g["box"][:3]), abs=1e-12)


def test_excise_and_noop_maker(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.atom_selector import atom_selector_factory as sf
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.excisor import excisor_factory as ef
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker import sample_maker_factory as mf
    g = load_golden("excise_and_random/n8_true_random_spherical.npz")
    parameters = mf.create_sample_maker_parameters(dict(algorithm="excise_and_noop", element_list=["Si"], sample_box_size=[ec.NEW_BOX] * 3,
                                                        number_of_samples_per_substructure=2))
    maker = mf.create_sample_maker(parameters, sf.create_atom_selector_parameters(dict(algorithm="top_k", top_k_environment=ec.TOP_K)),
                                   ef.create_excisor_parameters(rc.EXCISORS["spherical"]))
    samples, active, infos = maker.make_samples(*_frame())
    assert len(samples) == 6 and [int(a[0]) for a in active] == [0] * 6
    for b, sample in enumerate(samples):
        count = g["counts"][b // 2]
        assert np.array_equal(sample.X, g["constrained_x"][b // 2, :count]) and np.array_equal(sample.L, g["box"])
        assert infos[b]["constrained_atom_indices"] == list(range(count))
