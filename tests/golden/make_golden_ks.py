"""Generate the Kolmogorov-Smirnov fixtures tests/golden/ks/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_ks.py

The reference's KolmogorovSmirnovMetrics (metrics/kolmogorov_smirnov_metrics.py:7-75: scipy.stats.ks_2samp, two-sided,
method='auto', on the predicted samples against the reference samples).  The stubs for the packages the reference imports but
this image lacks and the writer are make_golden.py's, imported from it unchanged; torchmetrics.CatMetric is stubbed here by a
list with update, compute (= torch.cat) and reset.

PAIR cases (tests/ks_cases.py::PAIR_CASES).  Arrays of a case:
  a, b              the predicted and the reference sample as registered (binary32 or binary64); n1, n2 their sizes
  statistic, pvalue the reference's result
  numerator         h of tests/ks_cases.py::numerator; asserted here: h / lcm(n1, n2) == statistic while max(n1, n2) <= 10 000
                    (scipy's exact regime), within 2^-52 above
  limit_sf          scipy.stats.kstwobign.sf(lambda) at lambda = (h / lcm) sqrt(n1 n2 / (n1 + n2)); lambdas, limit_sfs: the
                    same function at fixed arguments, 0 and 40 among them (single_element only)
    single_element 1/1; small_coprime 5/7; equal_sizes 64/64; ties_across_samples 1000/600 small integers;
    negative_side: the maximum comes from c_a n2/g - c_b n1/g < 0 only; second_sample_element: it is attained at an element
    of b only (both asserted); disjoint_supports d = 1; identical_samples h = 0;
    special_values: -0.0 against +0.0, +-inf, denormals, negative values; binary64_energies: values that collide when rounded to
    binary32 (asserted); mixed_dtypes: a binary32, b binary64;
    boundary_9999_10000, boundary_10001_7: either side of scipy's exact regime; asymptotic_20000_12000;
    cap_semantics: a0..a2, b0..b2 registered in turn with maximum_number_of_samples = `cap` = 10; a, b = what was accepted;
    one_nan: one NaN in a; statistic and pvalue are NaN, numerator -1, limit_sf NaN.
DRIVER case (`driver`): two sets of 6 random-gas structures of 8 atoms in a 5.43 A cube (sides jittered by 0.05 A so that
the lattice parameters have a distribution), cutoff 5.0.  reference_X, reference_L, potential_energy; sample_X, sample_L,
sample_cartesian_positions, sample_energy (made up, as potential_energy is).  The distances go through the reference's
compute_distances_in_batch and every bag through the reference's class: structure_*, energy_*, lattice_*[i] hold n1, n2,
statistic, pvalue, numerator.  The seed is advanced until no distance of one bag lies within 1e-5 relative of a distance of
the other, nor of the cutoff: the ranks then do not depend on the last bits of a binary32 distance.  `seed` is recorded.
"""
import math
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)
from ks_cases import DRIVER, EXACT_REGIME, PAIR_CASES, numerator, scaled  # noqa: E402


class _CatMetric:
    """Stand-in for torchmetrics.CatMetric: what the reference's class uses of it."""

    def __init__(self):
        self.chunks = []

    def update(self, values):
        self.chunks.append(values)

    def compute(self):
        return torch.cat(self.chunks)

    def reset(self):
        self.chunks = []


_torchmetrics = types.ModuleType("torchmetrics")
_torchmetrics.CatMetric = _CatMetric
sys.modules.setdefault("torchmetrics", _torchmetrics)

import scipy.stats  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.metrics.kolmogorov_smirnov_metrics import \
    KolmogorovSmirnovMetrics  # noqa: E402

DIRECTORY = "ks"
CAP = 10
SEPARATION = 1e-5
LAMBDAS = (0.0, 0.01, 0.1, 0.3, 0.5, 0.8, 1.0, 1.17, 1.18, 1.19, 1.5, 2.0, 3.0, 5.0, 10.0, 40.0)


def _reference_result(predicted_chunks, reference_chunks, cap=None):
    metric = KolmogorovSmirnovMetrics() if cap is None else KolmogorovSmirnovMetrics(maximum_number_of_samples=cap)
    for chunk in reference_chunks:
        metric.register_reference_samples(torch.from_numpy(np.ascontiguousarray(chunk)))
    for chunk in predicted_chunks:
        metric.register_predicted_samples(torch.from_numpy(np.ascontiguousarray(chunk)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        statistic, pvalue = metric.compute_kolmogorov_smirnov_distance_and_pvalue()
    accepted_a, accepted_b = metric.predicted_samples_metric.compute().numpy(), metric.reference_samples_metric.compute().numpy()
    return float(statistic), float(pvalue), accepted_a, accepted_b


def _record(a, b, statistic, pvalue):
    n1, n2 = a.size, b.size
    if np.isnan(a).any() or np.isnan(b).any():
        assert math.isnan(statistic) and math.isnan(pvalue)
        return dict(n1=np.array(n1), n2=np.array(n2), statistic=np.array(statistic), pvalue=np.array(pvalue),
                    numerator=np.array(-1, dtype=np.int64), limit_sf=np.array(np.nan))
    h = numerator(a, b)
    d = h / math.lcm(n1, n2)
    if max(n1, n2) <= EXACT_REGIME:
        assert d == statistic, (d, statistic)
    else:
        assert abs(d - statistic) <= 2.0 ** -52, (d, statistic)
    return dict(n1=np.array(n1), n2=np.array(n2), statistic=np.array(statistic), pvalue=np.array(pvalue),
                numerator=np.array(h, dtype=np.int64), limit_sf=np.array(float(scipy.stats.kstwobign.sf(scaled(d, n1, n2)))))


def _signed(a, b, points):
    a, b = np.sort(a.astype(np.float64)), np.sort(b.astype(np.float64))
    g = math.gcd(a.size, b.size)
    return np.searchsorted(a, points, side="right").astype(np.int64) * (b.size // g) - \
        np.searchsorted(b, points, side="right").astype(np.int64) * (a.size // g)


def _samples(name):
    """(a, b) of a pair case, or (chunks of a, chunks of b) for cap_semantics."""
    rng = np.random.default_rng(abs(hash_of(name)))
    f32, f64 = np.float32, np.float64
    if name == "single_element":
        return np.array([0.25], f32), np.array([0.75], f32)
    if name == "small_coprime":
        return rng.normal(size=5).astype(f32), rng.normal(size=7).astype(f32)
    if name == "equal_sizes":
        return rng.normal(size=64).astype(f32), rng.normal(0.3, 1.0, size=64).astype(f32)
    if name == "ties_across_samples":
        return rng.integers(0, 12, size=1000).astype(f32), rng.integers(1, 14, size=600).astype(f32)
    if name == "negative_side":
        while True:
            a, b = rng.normal(0.6, 1.0, size=50).astype(f32), rng.normal(0.0, 1.0, size=40).astype(f32)
            v = _signed(a, b, np.concatenate([a, b]).astype(f64))
            if -v.min() > v.max() > 0:
                return a, b
    if name == "second_sample_element":
        while True:
            a, b = rng.normal(0.0, 1.0, size=33).astype(f32), rng.normal(0.0, 1.0, size=21).astype(f32)
            if np.abs(_signed(a, b, b.astype(f64))).max() > np.abs(_signed(a, b, a.astype(f64))).max():
                return a, b
    if name == "disjoint_supports":
        return rng.uniform(0.0, 1.0, size=37).astype(f32), rng.uniform(2.0, 3.0, size=53).astype(f32)
    if name == "identical_samples":
        a = rng.normal(size=129).astype(f32)
        return a, rng.permutation(a)
    if name == "special_values":
        tiny = np.float32(1e-45)
        a = np.array([-0.0, 0.0, np.inf, -np.inf, tiny, -tiny, -1.5, 2.5, -3.0e38, 1.0e-40, -0.0, 7.0], f32)
        b = np.array([0.0, 0.0, -np.inf, np.inf, np.inf, -tiny, tiny, -2.5, 1.5, 3.0e38, -1.0e-40], f32)
        return a, b
    if name == "binary64_energies":
        a, b = -4.33 + 1e-9 * rng.normal(size=200), -4.33 + 1e-9 * rng.normal(0.4, 1.0, size=150)
        assert np.unique(a.astype(f32)).size < a.size / 4 and np.unique(a).size == a.size
        return a.astype(f64), b.astype(f64)
    if name == "mixed_dtypes":
        return rng.normal(size=300).astype(f32), rng.normal(0.1, 1.0, size=170).astype(f64)
    if name == "boundary_9999_10000":
        return rng.normal(size=9999).astype(f32), rng.normal(0.01, 1.0, size=10000).astype(f32)
    if name == "boundary_10001_7":
        return rng.normal(size=10001).astype(f32), rng.normal(size=7).astype(f32)
    if name == "asymptotic_20000_12000":
        return rng.normal(size=20000).astype(f32), rng.normal(0.01, 1.0, size=12000).astype(f32)
    if name == "cap_semantics":
        return [rng.normal(size=n).astype(f32) for n in (4, 7, 5)], [rng.normal(size=n).astype(f32) for n in (6, 6, 6)]
    if name == "one_nan":
        a = rng.normal(size=20).astype(f32)
        a[11] = np.nan
        return a, rng.normal(size=15).astype(f32)
    raise KeyError(name)


def hash_of(name):
    """A seed from the case's name that does not depend on the interpreter's string hashing."""
    return 1700 + sum((k + 1) * ord(c) for k, c in enumerate(name))


def pair_case(name):
    a, b = _samples(name)
    if name == "cap_semantics":
        statistic, pvalue, accepted_a, accepted_b = _reference_result(a, b, cap=CAP)
        assert accepted_a.size == 11 and accepted_b.size == 12           # the count passes the cap by one chunk; the third is refused
        arrays = {f"a{k}": chunk for k, chunk in enumerate(a)}
        arrays.update({f"b{k}": chunk for k, chunk in enumerate(b)}, cap=np.array(CAP))
        a, b = accepted_a, accepted_b
    else:
        statistic, pvalue, accepted_a, accepted_b = _reference_result([a], [b])
        assert accepted_a.dtype == a.dtype and accepted_b.dtype == b.dtype
        arrays = {}
    arrays.update(a=a, b=b, **_record(a, b, statistic, pvalue))
    if name == "single_element":
        arrays.update(lambdas=np.array(LAMBDAS), limit_sfs=np.array([float(scipy.stats.kstwobign.sf(x)) for x in LAMBDAS]))
    if name == "disjoint_supports":
        assert statistic == 1.0
    if name == "identical_samples":
        assert int(arrays["numerator"]) == 0
    return arrays


def _separated(first, second, cutoff):
    first, second = np.unique(first.astype(np.float64)), np.unique(second.astype(np.float64))
    merged = np.concatenate([first, second, [cutoff]])
    owner = np.concatenate([np.zeros(first.size), np.ones(second.size), [2]])
    order = np.argsort(merged, kind="stable")
    merged, owner = merged[order], owner[order]
    close = (np.diff(merged) <= SEPARATION * merged[1:]) & (owner[1:] != owner[:-1])
    return not bool(close.any())


def driver_case():
    compute_distances_in_batch = mg._reference_compute_distances_in_batch()
    B, N, side, cutoff = 6, 8, 5.43, 5.0
    seed = 14000              # (a search from 1801 first held at 14308; started here to keep the maker quick)
    while True:
        g = torch.Generator().manual_seed(seed)
        sets = []
        for _ in range(2):
            X = torch.rand(B, N, 3, generator=g)
            L = torch.cat([side + 0.05 * torch.randn(B, 3, generator=g), torch.zeros(B, 3)], dim=1)
            cell = torch.diag_embed(L[:, :3])
            cart = torch.matmul(X, cell)
            energy = -4.3 * N + 0.5 * torch.randn(B, generator=g, dtype=torch.float64)
            sets.append(dict(X=X, L=L, cart=cart, energy=energy, distances=compute_distances_in_batch(cart, cell, cutoff)))
        reference, sample = sets
        if _separated(mg._np(reference["distances"]), mg._np(sample["distances"]), cutoff):
            break
        seed += 1
    arrays = dict(seed=np.array(seed), cutoff=np.array(cutoff), reference_X=mg._np(reference["X"]), reference_L=mg._np(reference["L"]),
                  potential_energy=mg._np(reference["energy"]), sample_X=mg._np(sample["X"]), sample_L=mg._np(sample["L"]),
                  sample_cartesian_positions=mg._np(sample["cart"]), sample_energy=mg._np(sample["energy"]))
    bags = dict(structure=(sample["distances"], reference["distances"]), energy=(sample["energy"], reference["energy"]))
    for i in range(6):
        bags[f"lattice_{i}"] = (sample["L"][:, i], reference["L"][:, i])
    for key, (predicted, expected) in bags.items():
        a, b = mg._np(predicted), mg._np(expected)
        statistic, pvalue, _, _ = _reference_result([a], [b])
        for field, value in _record(a, b, statistic, pvalue).items():
            arrays[f"{key}_{field}"] = value
    return arrays


def golden_ks():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    for name in PAIR_CASES:
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **pair_case(name))
    mg.save(os.path.join(DIRECTORY, DRIVER + ".npz"), **driver_case())


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_ks()
