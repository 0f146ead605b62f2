"""The training package without a GPU: the C ABI's new entry and its refusals, the Gaussian data module's parameters against the
reference's source text, its raw datasets against what the reference's own module made (tests/golden/training/gaussian_raw.npz),
the time-index draw restated on the oracle's Philox, and the refusals."""
import ast
import ctypes as C
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from training_cases import DIRECTORY, GAUSSIAN_FILE, INDEX_SEED, gaussian_parameters, time_index

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, training
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (ATOM_TYPES, CARTESIAN_FORCES, LATTICE_PARAMETERS,
                                                                        RELATIVE_COORDINATES)
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters

REFERENCE_DATA = "/root/reference/src/diffusion_for_multi_scale_molecular_dynamics/data/diffusion"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_in_the_abi():
    assert "mdx_noise_training_batch" in _hip.ABI_SYMBOLS and _hip.ABI_VERSION == 14
    assert (_hip.TAG_TRAIN_TIME_INDEX, _hip.TAG_TRAIN_Z, _hip.TAG_TRAIN_U, _hip.TAG_TRAIN_LATTICE) == (14, 15, 16, 17)
    tags = [value for name, value in _hip.ABI.constants.items() if name.startswith("TAG_")]
    assert sorted(tags) == list(range(18))                               # no two streams share a tag
    assert _hip.STATUS_NOISING_INDEX == 1048576
    bits = [value for name, value in _hip.ABI.constants.items() if name.startswith("STATUS_")]
    assert len(set(bits)) == len(bits) and all(b & (b - 1) == 0 for b in bits)
    f = _hip.ABI.functions["mdx_noise_training_batch"]
    assert f.streamed and f.params[-2] == ("uint32_t*", "status") and f.params[0] == ("const mdx_schedule_t*", "sched_host")
    kinds = dict((name, kind) for kind, name in f.params)
    assert kinds["rng"] == "mdx_rng_t" and kinds["rows"] == "const int64_t*" and kinds["d_cursor"] == "const int32_t*"
    assert kinds["root"] == "float" and kinds["time_indices_out"] == "int64_t*" and kinds["q_bar_tm1_out"] == "float*"
    # pointers, scalars, the schedule and the RNG request only: no new struct
    assert len(_hip.ABI.structs) == 5
    assert hasattr(_hip.lib(), "mdx_noise_training_batch")
    makefile = open(os.path.join(_hip.CSRC, "Makefile")).read()
    objects = re.search(r"^OBJS\s*=(.*?)(?<!\\)\n", makefile, flags=re.S | re.M).group(1)
    assert "mdx_noising.o" in objects.split() and os.path.exists(os.path.join(_hip.CSRC, "mdx_noising.hip"))
    # the noisers' arithmetic is written once, in the header both units include
    for unit in ("mdx_hip.hip", "mdx_noising.hip"):
        text = open(os.path.join(_hip.CSRC, unit)).read()
        assert '#include "mdx_noisers.hpp"' in text and "int noised_atom_type(" not in text


def test_the_entrys_argument_refusals_need_no_gpu():
    """Every refusal returns before anything is launched: placeholder addresses that are never read."""
    f = _hip.lib().mdx_noise_training_batch
    p = C.c_void_p(64)

    def status(T=10, classes=3, rows_total=100, rows=None, rows_count=0, batch=4, atoms=5, dimension=3, root=1.7, x0=p, tables=p):
        sched = _hip.Schedule(T, classes, 1e-3, tables, tables, tables, tables, tables, tables, tables, tables)
        return f(C.byref(sched), x0, p, p, rows_total, rows, rows_count, 0, None, None, None, None, None, _hip.Rng(1, 0, 1, 0), batch,
                 atoms, dimension, root, 0, p, p, p, p, p, p, p, p, p, p, p, p, None, None)

    invalid, unsupported = _hip.ERR_INVALID_ARG, _hip.ERR_UNSUPPORTED
    assert status(batch=0) == 0                                                             # MDX_OK, nothing launched
    assert status(batch=-1) == status(rows_total=0) == status(atoms=0) == status(dimension=0) == invalid
    assert status(T=0) == status(classes=1) == status(root=0.0) == status(root=float("nan")) == invalid
    assert status(dimension=4) == status(classes=9) == unsupported
    assert status(rows=p, rows_count=0) == invalid and status(rows=p, rows_count=3, batch=0) == 0
    assert status(x0=None) == status(tables=None) == invalid
    # M N >= 2^32: the Philox item is 32 bits wide
    assert status(rows_total=2**32, atoms=1) == status(rows_total=2**29, atoms=8) == status(rows_total=2**31, atoms=2) == invalid
    assert status(rows_total=2**32 - 1, atoms=1, batch=0) == 0 and status(rows_total=2**29 - 1, atoms=8, batch=0) == 0


def _class(tree, name):
    return next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name)


def _fields(node):
    """(bases, annotated fields with their defaults, plain class attributes) of a dataclass in source text."""
    fields = [(item.target.id, ast.unparse(item.annotation), None if item.value is None else ast.unparse(item.value))
              for item in node.body if isinstance(item, ast.AnnAssign)]
    plain = [(ast.unparse(item.targets[0]), ast.unparse(item.value)) for item in node.body if isinstance(item, ast.Assign)]
    return [ast.unparse(b) for b in node.bases], fields, plain


def _assertions(node):
    """[(condition, message)] of every assert of a class, in order, as normalised source text."""
    return [(ast.unparse(a.test), None if a.msg is None else ast.literal_eval(a.msg)) for a in ast.walk(node) if isinstance(a, ast.Assert)]


@pytest.mark.skipif(not os.path.isdir(REFERENCE_DATA), reason="the reference is not on this machine")
def test_parameters_fields_defaults_and_assertions_are_the_references():
    ours = ast.parse(inspect.getsource(training))
    theirs = ast.parse(open(os.path.join(REFERENCE_DATA, "gaussian_data_module.py")).read())
    base = ast.parse(open(os.path.join(REFERENCE_DATA, "data_module_parameters.py")).read())
    for name, tree in (("GaussianDataModuleParameters", theirs), ("DataModuleParameters", base)):
        assert _fields(_class(ours, name)) == _fields(_class(tree, name)), name
        assert _assertions(_class(ours, name)) == _assertions(_class(tree, name)), name
    assert _fields(_class(theirs, "GaussianDataModuleParameters"))[1] == [
        ("noise_parameters", "NoiseParameters", None), ("use_optimal_transport", "bool", None), ("random_seed", "int", None),
        ("number_of_atoms", "int", None), ("sigma_d", "float", "0.01"), ("equilibrium_relative_coordinates", "List[List[float]]", None),
        ("train_dataset_size", "int", "8192"), ("valid_dataset_size", "int", "1024")]
    # the module: the reference's two methods keep their signatures; the constructor gains `device`
    signature = lambda tree, method: [a.arg for a in next(      # noqa: E731
        f for f in _class(tree, "GaussianDataModule").body if isinstance(f, ast.FunctionDef) and f.name == method).args.args]
    for method in ("get_raw_dataset", "setup"):
        assert signature(ours, method) == signature(theirs, method)
    assert signature(ours, "__init__") == signature(theirs, "__init__") + ["device"]


def test_the_dataclass():
    fields = {f.name: f.default for f in dataclasses.fields(training.GaussianDataModuleParameters)}
    assert (fields["sigma_d"], fields["train_dataset_size"], fields["valid_dataset_size"]) == (0.01, 8192, 1024)
    assert (fields["batch_size"], fields["num_workers"], fields["max_atom"], fields["spatial_dimension"]) == (None, 0, 64, 3)
    assert fields["use_fixed_lattice_parameters"] is False and fields["random_seed"] is dataclasses.MISSING
    assert training.GaussianDataModuleParameters.data_source == "gaussian"
    assert "noise_once_at_setup" not in fields and training.DeviceDataModule.noise_once_at_setup is True
    with pytest.raises(AssertionError, match="the sigma_d parameter should be positive"):
        gaussian_parameters(sigma_d=0.0)
    with pytest.raises(AssertionError, match="exactly one list of equilibrium coordinates per atom"):
        gaussian_parameters(number_of_atoms=3)
    with pytest.raises(AssertionError, match="consistent with the spatial dimension"):
        gaussian_parameters(spatial_dimension=2)
    with pytest.raises(AssertionError, match="only be one element type"):
        gaussian_parameters(elements=["Si", "Ge"])
    # like the reference's, the subclass's __post_init__ stands alone: the base class's checks are its own
    with pytest.raises(AssertionError, match="If batch_size is None, valid_batch_size must be specified"):
        training.DataModuleParameters.__post_init__(gaussian_parameters(batch_size=None))


TOY = dict(batch_size=8, spatial_dimension=1, use_fixed_lattice_parameters=True, random_seed=42, sigma_d=0.01,
           equilibrium_relative_coordinates=[[0.25], [0.75]], train_dataset_size=16, valid_dataset_size=8)


@pytest.mark.parametrize("name, changes", [("main", {}), ("toy", TOY)])
def test_the_raw_datasets_are_the_references(name, changes):
    """get_raw_dataset, called as setup() calls it, against the clean fields of the reference module's datasets."""
    with np.load(os.path.join(DIRECTORY, GAUSSIAN_FILE)) as data:
        g = {key: data[key] for key in data.files}
    parameters = gaussian_parameters(**changes)
    module = training.GaussianDataModule(parameters, device="cuda")          # nothing touches the device before setup()
    assert module.train_dataset is None and module.noiser is None
    rng = torch.Generator()
    rng.manual_seed(parameters.random_seed)
    keys = {"X": RELATIVE_COORDINATES, "A": ATOM_TYPES, "L": LATTICE_PARAMETERS, "F": CARTESIAN_FORCES, "natom": "natom",
            "energy": "potential_energy"}
    for split, size in (("train", parameters.train_dataset_size), ("valid", parameters.valid_dataset_size)):
        raw = module.get_raw_dataset(size, rng)
        assert set(raw) == set(keys.values())
        for short, key in keys.items():
            recorded = g[f"{name}_{split}_{short}"]
            assert raw[key].numpy().dtype == recorded.dtype and np.array_equal(raw[key].numpy(), recorded), (split, key)
        x = raw[RELATIVE_COORDINATES]
        assert x.shape == (size, 2, parameters.spatial_dimension) and bool(((x >= 0) & (x < 1)).all())


def test_the_time_index_is_in_range_by_construction(oracle):
    for T in (1, 2, 12, 1000):
        drawn = [time_index(oracle, INDEX_SEED, call, 0, row, T) for call in (0, 7) for row in range(512)]
        assert min(drawn) >= 0 and max(drawn) < T
        assert T > 12 or set(drawn) == set(range(T))
    # the formula at the ends of the word: 0 -> 0, 2^32 - 1 -> T - 1, never T
    for T in (1, 2, 12, 1000, 2**31 - 1):
        assert (0 * T) >> 32 == 0 and ((2**32 - 1) * T) >> 32 == T - 1


def test_the_time_index_is_uniform_within_five_sigma(oracle):
    """4096 rows at T = 16, seed 20251021, call 0, draw 0: every count within 256 +- 5 sqrt(4096 x 1/16 x 15/16) = 256 +- 77.5,
    the binomial's five standard deviations (a bound from the distribution, not from a measurement)."""
    T, rows = 16, 4096
    counts = np.bincount([time_index(oracle, INDEX_SEED, 0, 0, row, T) for row in range(rows)], minlength=T)
    bound = 5.0 * math.sqrt(rows * (1 / T) * (1 - 1 / T))
    print("time-index counts", counts.tolist(), "bound", bound)
    assert counts.sum() == rows and counts.shape == (T,)
    assert np.all(np.abs(counts - rows / T) <= bound)


def test_optimal_transport_and_host_tensors_are_refused():
    with pytest.raises(NotImplementedError, match="use_optimal_transport=True"):
        training.GaussianDataModule(gaussian_parameters(use_optimal_transport=True))
    T, classes = 4, 2
    vector, matrix = torch.zeros(T), torch.zeros(T, classes, classes)
    host_schedule = kernels.DeviceSchedule(T, classes, 1e-3, *([vector] * 9), *([matrix] * 3))
    x0, a0, l0 = torch.zeros(3, 2, 1), torch.zeros(3, 2, dtype=torch.int64), torch.ones(3, 1)
    with pytest.raises(MdxError, match="no CPU fallback"):
        kernels.noise_training_batch(host_schedule, x0, a0, l0, 3, rng=_hip.Rng(0, 0, 1, 0))
    with pytest.raises(MdxError, match="schedule tables are built on the GPU"):
        training.BatchNoiser(NoiseParameters(total_time_steps=4), num_atom_types=1, spatial_dimension=1, device="cpu")
