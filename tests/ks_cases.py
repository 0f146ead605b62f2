"""The Kolmogorov-Smirnov fixtures (tests/golden/ks/*.npz, made by tests/golden/make_golden_ks.py from the reference's
KolmogorovSmirnovMetrics) as the tests read them: the case list, the loader, and the numpy restatement of the integer numerator.
Imports neither the package nor conftest: the maker imports it too."""
import math
import os

import numpy as np

DIRECTORY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ks")
PAIR_CASES = ("single_element", "small_coprime", "equal_sizes", "ties_across_samples", "negative_side", "second_sample_element",
              "disjoint_supports", "identical_samples", "special_values", "binary64_energies", "mixed_dtypes", "boundary_9999_10000",
              "boundary_10001_7", "asymptotic_20000_12000", "cap_semantics", "one_nan")
DRIVER = "driver"
FILES = [name + ".npz" for name in PAIR_CASES + (DRIVER,)]
EXACT_REGIME = 10000                 # scipy's method='auto' counts paths (and rounds d to h / lcm) while max(n1, n2) <= this
LIMIT_TOLERANCE = 1e-12              # the limit law: a handful of terms of magnitude <= 1, each rounded once
_LOADED = {}


def fixture(name):
    if name not in _LOADED:
        with np.load(os.path.join(DIRECTORY, name + ".npz")) as data:
            _LOADED[name] = {key: data[key] for key in data.files}
    return _LOADED[name]


def numerator(a, b) -> int:
    """h = max over x in a U b of |c_a(x) n2/g - c_b(x) n1/g|, c_s(x) = #{elements of s <= x}, in exact integers: scipy's
    two-sided statistic (searchsorted(..., side='right') on the concatenation, both signs) times lcm(n1, n2)."""
    a, b = np.sort(np.asarray(a, dtype=np.float64).ravel()), np.sort(np.asarray(b, dtype=np.float64).ravel())
    n1, n2 = a.size, b.size
    g = math.gcd(n1, n2)
    both = np.concatenate([a, b])
    count_a = np.searchsorted(a, both, side="right").astype(np.int64)
    count_b = np.searchsorted(b, both, side="right").astype(np.int64)
    return int(np.max(np.abs(count_a * (n2 // g) - count_b * (n1 // g))))


def distance(a, b) -> float:
    """numerator / lcm: one correctly rounded division."""
    return numerator(a, b) / math.lcm(np.size(a), np.size(b))


def scaled(distance_, n1, n2) -> float:
    """lambda = d sqrt(n1 n2 / (n1 + n2)) of the limit law, as kernels.ks_two_sample forms it."""
    return distance_ * math.sqrt(int(n1) * int(n2) / (int(n1) + int(n2)))


def check_distance(value, g):
    """A distance against a fixture's record of the reference: equal in scipy's exact regime, within 2^-52 above it."""
    n1, n2, statistic = int(g["n1"]), int(g["n2"]), float(g["statistic"])
    if max(n1, n2) <= EXACT_REGIME:
        assert value == statistic, (value, statistic)
    else:
        assert abs(value - statistic) <= 2.0 ** -52, (value, statistic)
