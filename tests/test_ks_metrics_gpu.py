"""The sampling metrics on the GPU: the radix sort per element against numpy.sort, the integer numerator against the fixtures
and the numpy restatement (exact equality), ks_two_sample against the reference's record, graph capture, the validation flow on
the driver fixture and one CLI run that writes metrics.pt."""
import math

import numpy as np
import pytest
import torch
import yaml

import ks_cases as cases
import stillinger_weber_cases as sw_cases
from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, sample_diffusion
from diffusion_for_multi_scale_molecular_dynamics_amd.metrics import KolmogorovSmirnovMetrics, compute_sampling_metrics
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, AXL_COMPOSITION, CARTESIAN_POSITIONS
from diffusion_for_multi_scale_molecular_dynamics_amd.utils.basis_transformations import (get_positions_from_coordinates,
                                                                                          map_lattice_parameters_to_unit_cell_vectors)
from diffusion_for_multi_scale_molecular_dynamics_amd.utils.structure_utils import (StillingerWeberParameters,
                                                                                    compute_distances_in_batch,
                                                                                    compute_stillinger_weber_energies_and_forces)

pytestmark = pytest.mark.gpu
TILE = kernels.KS_SORT_TILE
SIZES = (1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
CONTENTS = ("normal", "all_equal", "seven_values", "sorted", "reversed")


def _content(kind, n, dtype, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        values = rng.normal(size=n) * 10.0 ** rng.integers(-3, 4, size=n)
    elif kind == "all_equal":
        values = np.full(n, -1.25)
    elif kind == "seven_values":
        values = rng.choice(np.array([-3.5, -0.0, 0.0, 1e-3, 2.0, 2.0000002, 1e30]), size=n)
    else:
        values = np.sort(rng.normal(size=n))
        values = values[::-1] if kind == "reversed" else values
    return np.ascontiguousarray(values.astype(dtype))


def _expected_sort(values):
    return np.sort(values.astype(np.float64)) + 0.0              # the widening is exact; -0.0 + 0.0 = +0.0


def _same_bits(got, expected):
    return np.array_equal(got, expected) and np.array_equal(np.signbit(got), np.signbit(expected))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("kind", CONTENTS)
def test_sort_per_element(cuda, kind, dtype):
    for k, n in enumerate(SIZES):
        values = _content(kind, n, dtype, seed=100 + k)
        device_values = torch.from_numpy(values).to(cuda)
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        out = kernels.sort_keys(device_values, status)
        assert out.dtype == torch.float64 and out.shape == (n,)
        assert _same_bits(out.cpu().numpy(), _expected_sort(values)), (kind, n)
        assert np.array_equal(device_values.cpu().numpy().view(np.uint8), values.view(np.uint8))      # the input is unchanged
        assert int(status.item()) == 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sort_special_values_and_nan(cuda, dtype):
    g = cases.fixture("special_values")
    values = np.concatenate([g["a"], g["b"]]).astype(dtype)
    if dtype is np.float64:
        values = np.concatenate([values, [5e-324, -5e-324, 1.7e308, -1.7e308, 1.0 + 2.0 ** -52]])
    out = kernels.sort_keys(torch.from_numpy(values).to(cuda)).cpu().numpy()
    assert _same_bits(out, _expected_sort(values)) and not np.signbit(out[out == 0.0]).any()
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    with_nan = _content("normal", TILE + 1, dtype, seed=7)
    with_nan[TILE] = np.nan
    kernels.sort_keys(torch.from_numpy(with_nan).to(cuda), status)
    assert int(status.item()) == _hip.STATUS_KS_NAN
    other = torch.arange(5, device=cuda)                                                # any other dtype is taken as binary64
    assert kernels.sort_keys(other.flip(0)).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]


def _device_numerator(a, b, cuda, status=None):
    return int(kernels.ks_two_sample_numerator(torch.from_numpy(np.ascontiguousarray(a)).to(cuda),
                                               torch.from_numpy(np.ascontiguousarray(b)).to(cuda), status).item())


@pytest.mark.parametrize("name", [n for n in cases.PAIR_CASES if n != "one_nan"])
def test_numerator_equals_the_fixtures(cuda, name):
    g = cases.fixture(name)
    assert _device_numerator(g["a"], g["b"], cuda) == int(g["numerator"])


@pytest.mark.parametrize("sizes", [(TILE + 1, 3 * TILE + 17), (2 ** 17, 2 ** 17 - 1)])
@pytest.mark.parametrize("ties", [False, True])
def test_numerator_equals_the_restatement_on_random_pairs(cuda, sizes, ties):
    rng = np.random.default_rng(sizes[0] + ties)
    for dtype_a, dtype_b in ((np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64)):
        a, b = rng.normal(size=sizes[0]), rng.normal(0.01, 1.0, size=sizes[1])
        if ties:
            a, b = np.round(a * 40.0) / 8.0, np.round(b * 40.0) / 8.0
        a, b = a.astype(dtype_a), b.astype(dtype_b)
        assert _device_numerator(a, b, cuda) == cases.numerator(a, b), (dtype_a, dtype_b)


@pytest.mark.parametrize("name", cases.PAIR_CASES)
def test_ks_two_sample_against_the_references_record(cuda, name):
    g = cases.fixture(name)
    distance, p_value = kernels.ks_two_sample(torch.from_numpy(g["a"]).to(cuda), torch.from_numpy(g["b"]).to(cuda))
    assert isinstance(distance, float) and isinstance(p_value, float)
    if name == "one_nan":
        assert math.isnan(distance) and math.isnan(p_value)
        return
    print(f"{name}: d = {distance!r} (reference {float(g['statistic'])!r}), limit p = {p_value:.6g}, reference auto p = {float(g['pvalue']):.6g}")
    cases.check_distance(distance, g)
    assert abs(p_value - float(g["limit_sf"])) <= cases.LIMIT_TOLERANCE and 0.0 <= p_value <= 1.0


def test_numerator_captured_once_and_replayed(cuda):
    n1, n2 = TILE + 1, 3 * TILE + 17
    rng = np.random.default_rng(11)
    a, b = torch.zeros(n1, dtype=torch.float32, device=cuda), torch.zeros(n2, dtype=torch.float64, device=cuda)
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    a.copy_(torch.from_numpy(rng.normal(size=n1).astype(np.float32)))
    b.copy_(torch.from_numpy(rng.normal(size=n2)))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        kernels.ks_two_sample_numerator(a, b, status)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        numerator = kernels.ks_two_sample_numerator(a, b, status)
    for replay in range(3):
        new_a, new_b = rng.normal(0.05 * replay, 1.0, size=n1).astype(np.float32), np.round(rng.normal(size=n2) * 50.0) / 50.0
        a.copy_(torch.from_numpy(new_a))
        b.copy_(torch.from_numpy(new_b))
        graph.replay()
        assert int(numerator.item()) == cases.numerator(new_a, new_b), replay
    assert int(status.item()) == 0


def _driver_batches(cuda):
    g = cases.fixture(cases.DRIVER)
    t = lambda key: torch.from_numpy(np.ascontiguousarray(g[key])).to(cuda)
    types = torch.zeros(6, 8, dtype=torch.int64, device=cuda)
    samples = {AXL_COMPOSITION: AXL(A=types, X=t("sample_X"), L=t("sample_L")), CARTESIAN_POSITIONS: t("sample_cartesian_positions")}
    reference = {AXL_COMPOSITION: AXL(A=types, X=t("reference_X"), L=t("reference_L")), "potential_energy": t("potential_energy")}
    return g, samples, reference


def test_driver_fixture_through_the_validation_flow(cuda):
    g, samples, reference = _driver_batches(cuda)
    cutoff = float(g["cutoff"])
    oracle = StillingerWeberParameters(sw_coeff_filename=sw_cases.SI_SW, elements=["Si"])
    block = dict(compute_energies=True, compute_structure_factor=True, structure_factor_max_distance=cutoff, record_lattice_parameters=True)
    results = compute_sampling_metrics(samples, reference, block, oracle_parameters=oracle, sample_batchsize=4)
    assert set(results) == {"validation_ks_distance_energy", "validation_ks_p_value_energy", "validation_ks_distance_structure",
                            "validation_ks_p_value_structure"} | {f"validation_ks_lattice_parameter_{i}" for i in range(6)} | \
        {f"validation_ks_p_value_structure_{i}" for i in range(6)}
    assert all(isinstance(v, float) and math.isfinite(v) for v in results.values())
    # the package's own bags, and the restatement on them: exact
    sample_axl, reference_axl = samples[AXL_COMPOSITION], reference[AXL_COMPOSITION]
    reference_cells = map_lattice_parameters_to_unit_cell_vectors(reference_axl.L)
    own_reference = compute_distances_in_batch(get_positions_from_coordinates(reference_axl.X, reference_cells), reference_cells, cutoff)
    own_samples = compute_distances_in_batch(samples[CARTESIAN_POSITIONS], map_lattice_parameters_to_unit_cell_vectors(sample_axl.L), cutoff)
    own_samples, own_reference = own_samples.cpu().numpy(), own_reference.cpu().numpy()
    assert (own_samples.size, own_reference.size) == (int(g["structure_n1"]), int(g["structure_n2"]))
    assert results["validation_ks_distance_structure"] == cases.distance(own_samples, own_reference)
    # one rank step from the reference's record (the maker keeps the two bags 1e-5 apart: the ranks across the bags agree)
    assert abs(results["validation_ks_distance_structure"] - float(g["structure_statistic"])) <= 1.0 / own_samples.size + 1.0 / own_reference.size
    print(f"structure: d = {results['validation_ks_distance_structure']!r}, reference {float(g['structure_statistic'])!r}")
    for i in range(6):
        assert results[f"validation_ks_lattice_parameter_{i}"] == float(g[f"lattice_{i}_statistic"])
        assert results[f"validation_ks_lattice_parameter_{i}"] == cases.distance(g["sample_L"][:, i], g["reference_L"][:, i])
    energies = compute_stillinger_weber_energies_and_forces(samples, oracle)[0].cpu().numpy()
    assert results["validation_ks_distance_energy"] == cases.distance(energies, g["potential_energy"])
    # the made-up energies of both sets through the class: the reference's record
    metric = KolmogorovSmirnovMetrics()
    metric.register_reference_samples(reference["potential_energy"])
    metric.register_predicted_samples(torch.from_numpy(g["sample_energy"]).to(cuda))
    distance, p_value = metric.compute_kolmogorov_smirnov_distance_and_pvalue()
    assert distance == float(g["energy_statistic"]) and abs(p_value - float(g["energy_limit_sf"])) <= cases.LIMIT_TOLERANCE
    # device chunks stay on the device
    assert metric.reference_chunks[0].is_cuda and metric.predicted_chunks[0].is_cuda


def test_cli_writes_metrics_beside_the_samples(cuda, tmp_path):
    g, _, reference = _driver_batches(cuda)
    torch.save({key: AXL(*(t.cpu() for t in value)) if isinstance(value, AXL) else value.cpu() for key, value in reference.items()},
               tmp_path / "reference.pt")
    cfg = dict(noise=dict(total_time_steps=10, sigma_min=1e-4, sigma_max=0.25),
               sampling=dict(algorithm="predictor_corrector", spatial_dimension=3, number_of_atoms=8, number_of_samples=12,
                             sample_batchsize=5, num_atom_types=1, number_of_corrector_steps=1, use_fixed_lattice_parameters=True,
                             cell_dimensions=[5.43, 5.43, 5.43], rng_mode="device", use_hip_graph=True, seed=5),
               elements=["Si"],
               metrics=dict(compute_structure_factor=True, structure_factor_max_distance=5.0, record_lattice_parameters=True),
               model=dict(score_network=dict(architecture="analytical", number_of_atoms=8, num_atom_types=1, kmax=4, sigma_d=0.05,
                                             equilibrium_relative_coordinates=sw_cases.diamond_sites(1).tolist())))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    sample_diffusion.main(["--config", str(tmp_path / "config.yaml"), "--output", str(tmp_path / "out"), "--device", "cuda",
                           "--reference_samples", str(tmp_path / "reference.pt")])
    assert (tmp_path / "out" / "samples.pt").exists()
    metrics = torch.load(tmp_path / "out" / "metrics.pt", weights_only=False)
    assert set(metrics) == {"validation_ks_distance_structure", "validation_ks_p_value_structure"} | \
        {f"validation_ks_lattice_parameter_{i}" for i in range(6)} | {f"validation_ks_p_value_structure_{i}" for i in range(6)}
    assert all(isinstance(v, float) and math.isfinite(v) and 0.0 <= v <= 1.0 for v in metrics.values())
    assert "validation_ks_distance_structure" in (tmp_path / "out" / "console.log").read_text()
