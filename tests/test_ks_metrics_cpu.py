"""The sampling metrics without a GPU: the C ABI's declarations, the integer numerator's numpy restatement against the reference's
recorded statistic (tests/golden/ks, made from the reference's KolmogorovSmirnovMetrics), the limit-law p-value, the Python
surface against the reference's source text, the class's cap semantics, and every refusal that comes before a launch."""
import ast
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import yaml

import ks_cases as cases
from conftest import ROOT
from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, metrics, sample_diffusion
from diffusion_for_multi_scale_molecular_dynamics_amd.metrics import KolmogorovSmirnovMetrics, compute_sampling_metrics
from diffusion_for_multi_scale_molecular_dynamics_amd.metrics.sampling_metrics_parameters import SamplingMetricsParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, AXL_COMPOSITION, CARTESIAN_POSITIONS

REFERENCE_CLASS = "/root/reference/src/diffusion_for_multi_scale_molecular_dynamics/metrics/kolmogorov_smirnov_metrics.py"
SYMBOLS = ("mdx_sort_keys_workspace_bytes", "mdx_sort_keys", "mdx_ks_two_sample_workspace_bytes", "mdx_ks_two_sample_sorted")


def test_the_header_declares_the_unit_and_the_abi_version_stays():
    header = open(_hip.HEADER_PATH).read()
    for symbol in SYMBOLS:
        assert re.search(r"MDX_API\s+(?:int64_t|int)\s+" + symbol + r"\s*\(", header), symbol
        assert symbol in _hip.ABI_SYMBOLS
    assert _hip.ABI.functions["mdx_sort_keys_workspace_bytes"].restype is _hip.ABI.functions["mdx_ks_two_sample_workspace_bytes"].restype
    assert _hip.STATUS_KS_NAN == 262144 and _hip.KS_MAX_SAMPLES == 2 ** 24 and _hip.ABI_VERSION == 14
    assert kernels.KS_MAX_SAMPLES == _hip.KS_MAX_SAMPLES and kernels.KS_SORT_TILE == _hip.KS_SORT_TILE >= 64
    makefile = open(os.path.join(_hip.CSRC, "Makefile")).read()
    objects = re.search(r"^OBJS\s*=(.*?)(?<!\\)\n", makefile, flags=re.S | re.M).group(1)
    assert "mdx_metrics.o" in objects.split()
    assert "case MDX_STATUS_KS_NAN" in open(os.path.join(_hip.CSRC, "mdx_hip.hip")).read()
    source = open(os.path.join(_hip.CSRC, "mdx_metrics.hip")).read()
    assert not re.search(r"rocprim|hipcub|thrust", source, flags=re.I)                   # hand-written: no vendor sort


@pytest.mark.parametrize("name", [n for n in cases.PAIR_CASES if n != "one_nan"])
def test_the_restatement_gives_every_recorded_numerator_and_the_references_statistic(name):
    g = cases.fixture(name)
    assert (g["a"].size, g["b"].size) == (int(g["n1"]), int(g["n2"]))
    h = cases.numerator(g["a"], g["b"])
    assert h == int(g["numerator"])
    assert cases.numerator(g["b"], g["a"]) == h                                           # the two-sided statistic is symmetric
    cases.check_distance(h / math.lcm(int(g["n1"]), int(g["n2"])), g)


def test_the_fixtures_hold_what_their_names_say():
    assert sorted(os.listdir(cases.DIRECTORY)) == sorted(cases.FILES)
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
                  if f.endswith(".npz"))
    assert all(os.path.getsize(os.path.join(cases.DIRECTORY, f)) <= largest for f in cases.FILES)
    sizes = {name: (int(cases.fixture(name)["n1"]), int(cases.fixture(name)["n2"])) for name in cases.PAIR_CASES}
    assert sizes["single_element"] == (1, 1) and sizes["small_coprime"] == (5, 7) and sizes["equal_sizes"] == (64, 64)
    assert sizes["ties_across_samples"] == (1000, 600) and sizes["boundary_9999_10000"] == (9999, 10000)
    assert sizes["boundary_10001_7"] == (10001, 7) and sizes["asymptotic_20000_12000"] == (20000, 12000)
    assert float(cases.fixture("disjoint_supports")["statistic"]) == 1.0 and int(cases.fixture("identical_samples")["numerator"]) == 0
    g = cases.fixture("special_values")
    assert np.signbit(g["a"][0]) and g["a"][0] == 0 and np.isinf(g["a"]).sum() == 2 and (np.abs(g["a"][4:6]) < 1.2e-38).all()
    g = cases.fixture("ties_across_samples")       # side='right' on BOTH counts decides: a `<` in one of them gives another value
    a, b = np.sort(g["a"].astype(np.float64)), np.sort(g["b"].astype(np.float64))
    both = np.concatenate([a, b])
    for side_a, side_b in (("right", "left"), ("left", "right")):
        mixed = np.abs(np.searchsorted(a, both, side=side_a) * 3 - np.searchsorted(b, both, side=side_b) * 5).max()
        assert int(mixed) != int(g["numerator"])
    g = cases.fixture("binary64_energies")
    assert g["a"].dtype == np.float64 and np.unique(g["a"].astype(np.float32)).size < g["a"].size / 4
    assert cases.numerator(g["a"].astype(np.float32), g["b"].astype(np.float32)) != int(g["numerator"])
    g = cases.fixture("mixed_dtypes")
    assert (g["a"].dtype, g["b"].dtype) == (np.float32, np.float64)
    g = cases.fixture("one_nan")
    assert np.isnan(g["a"]).sum() == 1 and np.isnan(g["statistic"]) and np.isnan(g["pvalue"])


def test_the_limit_law_against_scipys_recorded_values():
    g = cases.fixture("single_element")
    assert g["lambdas"][0] == 0.0 and g["lambdas"][-1] == 40.0
    for lam, expected in zip(g["lambdas"], g["limit_sfs"]):
        assert abs(kernels.kolmogorov_limit_p_value(float(lam)) - float(expected)) <= cases.LIMIT_TOLERANCE, lam
    assert kernels.kolmogorov_limit_p_value(0.0) == 1.0 and kernels.kolmogorov_limit_p_value(-1.0) == 1.0
    assert kernels.kolmogorov_limit_p_value(40.0) == 0.0 and math.isnan(kernels.kolmogorov_limit_p_value(float("nan")))
    for name in cases.PAIR_CASES:
        g = cases.fixture(name)
        if name == "one_nan":
            continue
        lam = cases.scaled(int(g["numerator"]) / math.lcm(int(g["n1"]), int(g["n2"])), g["n1"], g["n2"])
        assert abs(kernels.kolmogorov_limit_p_value(lam) - float(g["limit_sf"])) <= cases.LIMIT_TOLERANCE, name


def test_the_limit_law_against_scipy_itself():
    stats = pytest.importorskip("scipy.stats")
    for lam in np.concatenate([np.linspace(0.01, 3.0, 300), np.linspace(3.0, 40.0, 50)]):
        assert abs(kernels.kolmogorov_limit_p_value(float(lam)) - float(stats.kstwobign.sf(lam))) <= cases.LIMIT_TOLERANCE, lam


def _signatures(tree, class_name):
    node = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == class_name)
    out = {}
    for item in node.body:
        if isinstance(item, ast.FunctionDef) and (not item.name.startswith("_") or item.name == "__init__"):
            positional = item.args.posonlyargs + item.args.args
            defaults = [None] * (len(positional) - len(item.args.defaults)) + [ast.unparse(d) for d in item.args.defaults]
            out[item.name] = list(zip([a.arg for a in positional], defaults))
    return out


@pytest.mark.skipif(not os.path.isfile(REFERENCE_CLASS), reason="the reference is not on this machine")
def test_the_class_has_the_references_methods_parameters_and_defaults():
    theirs = _signatures(ast.parse(open(REFERENCE_CLASS).read()), "KolmogorovSmirnovMetrics")
    ours = _signatures(ast.parse(inspect.getsource(metrics)), "KolmogorovSmirnovMetrics")
    assert set(theirs) == {"__init__", "register_reference_samples", "register_predicted_samples", "reset",
                           "compute_kolmogorov_smirnov_distance_and_pvalue"}
    assert ours == theirs
    imported = {alias.name.split(".")[0] for n in ast.walk(ast.parse(inspect.getsource(metrics))) if isinstance(n, ast.Import)
                for alias in n.names}
    assert not imported & {"scipy", "torchmetrics"}


def test_the_parameters_are_the_references_dataclass():
    p = SamplingMetricsParameters()
    assert (p.compute_energies, p.compute_structure_factor, p.structure_factor_max_distance, p.record_lattice_parameters) == \
        (False, False, 10.0, False)
    with pytest.raises(TypeError):
        SamplingMetricsParameters(True)                                                   # kw_only, as the reference's
    block = dict(compute_energies=False, compute_structure_factor=True, structure_factor_max_distance=5.0)
    assert metrics.as_sampling_metrics_parameters(block) == SamplingMetricsParameters(**block)
    assert metrics.asks_for_anything(block) and not metrics.asks_for_anything({}) and not metrics.asks_for_anything(None)


def test_cap_semantics_and_reset():
    """The reference's cap: a registration is accepted while the count is below the cap, so the count may pass it by one chunk
    (the fixture's record of what the reference accepted); chunks stay where they are given."""
    g = cases.fixture("cap_semantics")
    metric = KolmogorovSmirnovMetrics(maximum_number_of_samples=int(g["cap"]))
    for k in range(3):
        metric.register_predicted_samples(torch.from_numpy(g[f"a{k}"]))
        metric.register_reference_samples(torch.from_numpy(g[f"b{k}"]))
    assert (metric.predicted_count, metric.reference_count) == (11, 12) == (g["a"].size, g["b"].size)
    assert np.array_equal(torch.cat(metric.predicted_chunks).numpy(), g["a"]) and np.array_equal(torch.cat(metric.reference_chunks).numpy(), g["b"])
    assert not metric.predicted_chunks[0].is_cuda                                         # kept where it was given
    with pytest.raises(ValueError, match="no CPU fallback"):
        metric.compute_kolmogorov_smirnov_distance_and_pvalue()
    metric.reset()
    assert (metric.predicted_count, metric.reference_count, metric.predicted_chunks, metric.reference_chunks) == (0, 0, [], [])
    with pytest.raises(ValueError, match="register both"):
        metric.compute_kolmogorov_smirnov_distance_and_pvalue()
    assert KolmogorovSmirnovMetrics().maximum_count == 1_000_000


def test_refusals_before_any_launch(monkeypatch):
    host = torch.arange(4.0)
    for function in (kernels.sort_keys, lambda t: kernels.ks_two_sample_numerator(t, t), lambda t: kernels.ks_two_sample(t, t)):
        with pytest.raises(ValueError, match="no CPU fallback"):
            function(host)
        with pytest.raises(ValueError, match="is empty"):
            function(torch.zeros(0))
        with pytest.raises(ValueError, match="must be a torch.Tensor"):
            function([1.0, 2.0])
    monkeypatch.setattr(kernels, "KS_MAX_SAMPLES", 3)
    with pytest.raises(ValueError, match="more than KS_MAX_SAMPLES = 3"):
        kernels.sort_keys(host)
    with pytest.raises(ValueError, match="more than KS_MAX_SAMPLES = 3"):
        kernels.ks_two_sample(host, host[:2])


def _batches():
    g = torch.Generator().manual_seed(3)
    axl = AXL(A=torch.zeros(4, 8, dtype=torch.int64), X=torch.rand(4, 8, 3, generator=g), L=torch.tensor([[5.43] * 3 + [0.0] * 3] * 4))
    return {AXL_COMPOSITION: axl, CARTESIAN_POSITIONS: axl.X * 5.43}, {AXL_COMPOSITION: axl}


def test_compute_energies_needs_the_stillinger_weber_oracle():
    samples, reference = _batches()
    for oracle in (None, dict(name="lammps")):
        with pytest.raises(ValueError, match="needs an `oracle:` block with `name: stillinger_weber`"):
            compute_sampling_metrics(samples, reference, dict(compute_energies=True), oracle_parameters=oracle)
    assert compute_sampling_metrics(samples, reference, {}) == {}                         # nothing asked: nothing launched


def _config(**extra):
    return dict(noise=dict(total_time_steps=10, sigma_min=1e-4, sigma_max=0.25),
                sampling=dict(algorithm="predictor_corrector", spatial_dimension=3, number_of_atoms=8, number_of_samples=12,
                              sample_batchsize=5, num_atom_types=1, number_of_corrector_steps=1, use_fixed_lattice_parameters=True,
                              cell_dimensions=[5.43, 5.43, 5.43]), elements=["Si"], **extra)


def test_the_reference_samples_flag(tmp_path):
    """The flag is parsed; `compute_energies` without a Stillinger-Weber `oracle:` block and a file that does not exist are
    refused before a network is built (there is no `model:` block and no checkpoint: reaching that point fails differently, as
    the run without the flag does -- the block is then ignored)."""
    def run(cfg, name, *flags):
        (tmp_path / name).write_text(yaml.safe_dump(cfg))
        sample_diffusion.main(["--config", str(tmp_path / name), "--output", str(tmp_path / "out"), "--device", "cpu", *flags])
    torch.save(_batches()[1], tmp_path / "reference.pt")
    with pytest.raises(ValueError, match="needs an `oracle:` block"):
        run(_config(metrics=dict(compute_energies=True)), "energies.yaml", "--reference_samples", str(tmp_path / "reference.pt"))
    with pytest.raises(AssertionError, match="absent.pt' do not exist"):
        run(_config(metrics=dict(record_lattice_parameters=True)), "absent.yaml", "--reference_samples", str(tmp_path / "absent.pt"))
    with pytest.raises(AssertionError, match="Cannot go on"):                             # without the flag: the block is ignored
        run(_config(metrics=dict(compute_energies=True)), "ignored.yaml")
    with pytest.raises(AssertionError, match="Cannot go on"):                             # a block that asks for nothing: likewise
        run(_config(metrics=dict(structure_factor_max_distance=4.0)), "nothing.yaml", "--reference_samples", str(tmp_path / "reference.pt"))
    assert sample_diffusion.metrics_parameters_of(_config(), str(tmp_path / "reference.pt"), None) is None
    parameters = sample_diffusion.metrics_parameters_of(_config(metrics=dict(compute_structure_factor=True)),
                                                        str(tmp_path / "reference.pt"), None)
    assert parameters == SamplingMetricsParameters(compute_structure_factor=True)
    assert not os.path.exists(tmp_path / "out" / "metrics.pt")
