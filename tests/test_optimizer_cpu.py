"""The optimizer step without a GPU: the fixtures against a float64 restatement of the closed form (and controls that show the
fixtures see what they are meant to see), the header / Makefile / binding of the new unit, the reference's `optimizer:` and
`scheduler:` surface on host models, the reference's own tests of it, the refusals and the per-block table."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import optimizer_cases as oc
from conftest import GOLDEN, ROOT
from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd.models import optimizer as optimizer_module
from diffusion_for_multi_scale_molecular_dynamics_amd.models import scheduler as scheduler_module

REFERENCE = "/root/reference"
RECORDS = [(case, i) for case in oc.TEACHER_FORCED for i in oc.records(case)]


@pytest.mark.parametrize("case, i", RECORDS)
def test_closed_form_in_float64_reproduces_every_record(case, i):
    """The closed form of include/mdx_hip.h, restated in float64 numpy, stays below 1e-3 of the derived bound on every element of
    every record: the form is the reference's arithmetic, and the bound leaves the kernel its one rounding."""
    g = oc.fixture(case)
    p64, m64, v64 = oc.restatement(g, i)
    worst = dict(p=oc.excess(p64, g[f"r{i}_p64"], g[f"r{i}_p"]), m=oc.excess(m64, g[f"r{i}_m64"]), v=oc.excess(v64, g[f"r{i}_v64"]))
    if float(g["max_norm"]) > 0.0:
        worst["norm"] = oc.excess(np.array([oc.norm64(g, i)]), g[f"r{i}_norm64"].reshape(1))
    print(case, i, worst)
    assert all(value < 1e-3 for value in worst.values()), worst
    assert np.array_equal(g[f"r{i}_step"], g[f"r{i}_step_before"] + g[f"r{i}_has_gradient"].astype(np.int32))


def _beyond(g, i, **switches):
    p64, m64, v64 = oc.restatement(g, i, **switches)
    return max(oc.excess(p64, g[f"r{i}_p64"], g[f"r{i}_p"]), oc.excess(m64, g[f"r{i}_m64"]), oc.excess(v64, g[f"r{i}_v64"]))


@pytest.mark.parametrize("case", ["adamw_decay", "adam_l2"])
def test_control_the_fixtures_see_the_weight_decay_mode(case):
    g = oc.fixture(case)
    assert all(_beyond(g, i, flip_decoupled=True) > 1.0 for i in oc.records(case))


@pytest.mark.parametrize("case", ["adamw_decay", "adam_l2", "adam_default"])
def test_control_the_fixtures_see_the_bias_correction(case):
    g = oc.fixture(case)
    assert all(_beyond(g, i, bias_correction=False) > 1.0 for i in oc.records(case))


def test_control_the_fixtures_see_the_clipping_and_only_where_it_acts():
    g = oc.fixture("adamw_clip")
    assert oc.clip_of(g, 0) < 1.0 and oc.clip_of(g, 1) == 1.0
    assert float(g["r0_norm64"]) > float(g["max_norm"]) > float(g["r1_norm64"])
    assert _beyond(g, 0, clip=1.0) > 1.0
    big = oc.fixture("big")
    assert all(oc.clip_of(big, i) < 1.0 and _beyond(big, i, clip=1.0) > 1.0 for i in oc.records("big"))


def test_control_the_fixtures_see_a_counter_that_did_not_lag():
    g = oc.fixture("missing_gradient")
    i = oc.MISSING_RECORD + 1
    assert g[f"r{i}_step_before"][oc.MISSING_TENSOR] == g[f"r{i}_step_before"][0] - 1
    assert _beyond(g, i) < 1e-3 and _beyond(g, i, advance=oc.MISSING_TENSOR) > 1.0
    # at the record without a gradient nothing of the tensor moves
    j = oc.MISSING_RECORD
    lo, hi = np.cumsum([0] + list(g["counts"]))[oc.MISSING_TENSOR:oc.MISSING_TENSOR + 2]
    assert not g[f"r{j}_has_gradient"][oc.MISSING_TENSOR]
    assert np.array_equal(g[f"r{j}_p64"][lo:hi], g[f"r{j}_p"][lo:hi].astype(np.float64))
    assert np.array_equal(g[f"r{j}_m64"][lo:hi], g[f"r{j}_m"][lo:hi].astype(np.float64))


def test_fixture_shapes():
    for case in ("adamw_decay", "adam_l2", "adam_default", "adamw_clip", "missing_gradient", "free_running"):
        assert oc.shapes(oc.fixture(case)) == list(oc.SMALL_SHAPES)
    chunk = _hip.ADAM_CHUNK_ELEMENTS
    assert list(oc.fixture("big")["counts"]) == [chunk + 1, 2 * chunk]
    assert [int(oc.fixture("adamw_decay")[f"r{i}_step"][0]) for i in range(4)] == [1, 2, 3, 1000]
    zero = oc.split(oc.fixture("adam_default")["r0_g"], oc.fixture("adam_default")["counts"])[1]
    assert zero.size == 63 and not zero.any()
    assert sorted(os.listdir(oc.DIRECTORY)) == sorted(oc.FILES)
    assert all(os.path.getsize(os.path.join(oc.DIRECTORY, name)) < 600 * 1024 for name in oc.FILES)


def test_header_makefile_and_binding_of_the_optimizer_unit():
    header = open(_hip.HEADER_PATH).read()
    assert _hip.ABI_VERSION == 14 and _hip.STATUS_OPTIMIZER_NONFINITE == 524288
    assert re.search(r"#define\s+MDX_ADAM_CHUNK_ELEMENTS\s+%d\b" % _hip.ADAM_CHUNK_ELEMENTS, header)
    assert _hip.ADAM_CHUNK_ELEMENTS % 1024 == 0 and kernels.ADAM_CHUNK_ELEMENTS == _hip.ADAM_CHUNK_ELEMENTS
    for name in ("mdx_adam_step", "mdx_gradient_norm", "mdx_adam_hyper_fill"):
        function = _hip.ABI.functions[name]
        assert function.streamed and function.tensors is not None, name
    step = _hip.ABI.functions["mdx_adam_step"]
    assert [p for _, p in step.params][-2:] == ["status", "stream"]
    assert dict((name, dtype) for _, dtype, name in step.tensors)["hyper"] == torch.float64
    assert [p for _, p in _hip.ABI.functions["mdx_adam_hyper_fill"].params][:7] == list(kernels.ADAM_HYPER_NAMES)
    assert [getattr(_hip, "ADAM_HYPER_" + name.upper()) for name in kernels.ADAM_HYPER_NAMES] == list(range(7))
    makefile = open(os.path.join(_hip.CSRC, "Makefile")).read()
    objects = re.search(r"^OBJS\s*=(.*?)(?<!\\)\n", makefile, flags=re.S | re.M).group(1)
    assert "mdx_optimizer.o" in objects.split()
    assert "case MDX_STATUS_OPTIMIZER_NONFINITE" in open(os.path.join(_hip.CSRC, "mdx_hip.hip")).read()
    assert os.path.isfile(os.path.join(_hip.CSRC, "mdx_optimizer.hip"))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.linear_layer = torch.nn.Linear(4, 1)


@pytest.mark.parametrize("name, expected", [("adam", torch.optim.Adam), ("adamw", torch.optim.AdamW), ("None", torch.optim.Adam)])
@pytest.mark.parametrize("weight_decay", [None, 1e-6])
def test_load_optimizer_on_a_host_model_is_torchs_own_class(name, expected, weight_decay):
    keywords = {} if weight_decay is None else dict(weight_decay=weight_decay)
    parameters = optimizer_module.OptimizerParameters(name=name, learning_rate=0.01, **keywords)
    optimizer = optimizer_module.load_optimizer(parameters, _Net())
    assert type(optimizer) is expected
    assert optimizer.defaults == expected(_Net().parameters(), lr=0.01, weight_decay=parameters.weight_decay).defaults
    assert optimizer_module.check_if_optimizer_is_none(parameters) == (name == "None")
    double = optimizer_module.load_optimizer(parameters, _Net().double())
    assert type(double) is expected
    with pytest.raises(AssertionError, match="Optimizer 'sgd' is not defined."):
        optimizer_module.load_optimizer(optimizer_module.OptimizerParameters(name="sgd", learning_rate=0.1), _Net())
    assert issubclass(optimizer_module.FusedAdam, torch.optim.Adam)


REFERENCE_TEST_FILES = {"tests/models/test_optimizer.py": 4, "tests/models/test_scheduler.py": 2}


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
@pytest.mark.parametrize("test_file", list(REFERENCE_TEST_FILES))
def test_the_references_own_optimizer_and_scheduler_tests_pass_here(test_file, tmp_path):
    """The reference's own test files, unmodified, against this package (the import alias of tests/golden/reference_import_alias.py,
    as tests/test_reference_yaml_surface.py runs its list): every test passes, and the count is the file's."""
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    env["PYTHONPATH"] = os.pathsep.join([GOLDEN, ROOT])
    run = subprocess.run([sys.executable, "-m", "pytest", "-p", "reference_import_alias", os.path.join(REFERENCE, test_file), "-q",
                          "--no-header", "-p", "no:cacheprovider", "--rootdir", str(tmp_path)],
                         env=env, cwd=REFERENCE, capture_output=True, text=True, timeout=600)
    tail = run.stdout.strip().splitlines()[-1] if run.stdout.strip() else run.stderr[-500:]
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-1000:]
    assert f"{REFERENCE_TEST_FILES[test_file]} passed" in tail and "failed" not in tail and "error" not in tail, tail


def _orion_configuration():
    """The reference's template (tests/golden/optimizer/: settings only) with the orion string replaced by a number."""
    with open(os.path.join(oc.DIRECTORY, oc.YAML)) as stream:
        configuration = yaml.safe_load(stream)
    assert str(configuration["optimizer"]["learning_rate"]).startswith("orion~")
    configuration["optimizer"]["learning_rate"] = 1.0e-4
    return configuration


def test_optimizer_and_scheduler_blocks_of_the_references_template():
    from diffusion_for_multi_scale_molecular_dynamics_amd.loss import configure_optimizers
    configuration = _orion_configuration()
    parameters = optimizer_module.create_optimizer_parameters(configuration["optimizer"])
    assert parameters == optimizer_module.OptimizerParameters(name="adamw", learning_rate=1.0e-4, weight_decay=1.0e-6)
    scheduling = scheduler_module.create_scheduler_parameters(configuration)
    assert scheduling == scheduler_module.ReduceLROnPlateauSchedulerParameters(name="ReduceLROnPlateau", factor=0.1, patience=3)
    assert scheduling.monitor == "validation_epoch_loss"
    assert scheduler_module.create_scheduler_parameters(dict(optimizer=configuration["optimizer"])) is None
    net = _Net()
    configured = configure_optimizers(configuration, net)
    assert set(configured) == {"optimizer", "lr_scheduler", "monitor"} and configured["monitor"] == "validation_epoch_loss"
    assert type(configured["optimizer"]) is torch.optim.AdamW
    assert configured["optimizer"].defaults["lr"] == 1.0e-4 and configured["optimizer"].defaults["weight_decay"] == 1.0e-6
    scheduler = configured["lr_scheduler"]
    assert type(scheduler) is torch.optim.lr_scheduler.ReduceLROnPlateau and scheduler.factor == 0.1 and scheduler.patience == 3
    assert scheduler.optimizer is configured["optimizer"]

    class HyperParameters:          # the reference's AXLDiffusionParameters carry the two as attributes
        optimizer_parameters = parameters
        scheduler_parameters = scheduler_module.CosineAnnealingLRSchedulerParameters(T_max=7, eta_min=1e-5)

    other = configure_optimizers(HyperParameters(), net)
    assert set(other) == {"optimizer", "lr_scheduler"} and type(other["lr_scheduler"]) is torch.optim.lr_scheduler.CosineAnnealingLR
    HyperParameters.scheduler_parameters = None
    assert set(configure_optimizers(HyperParameters(), net)) == {"optimizer"}
    with pytest.raises(AssertionError, match="The option field 'sgd' is missing"):
        optimizer_module.create_optimizer_parameters(dict(name="sgd", learning_rate=0.1))
    with pytest.raises(AssertionError, match="The identifier field 'name' is missing"):
        optimizer_module.create_optimizer_parameters(dict(learning_rate=0.1))


class _DeviceTensor:
    """What adam_plan looks at, for a tensor that claims to live on a device: the checks come before any upload or launch."""

    def __init__(self, count=8, dtype=torch.float32, contiguous=True, address=4096):
        self.is_cuda, self.dtype, self._count, self._contiguous, self._address = True, dtype, count, contiguous, address
        self.device, self.grad = "cuda:0", None

    def numel(self):
        return self._count

    def is_contiguous(self):
        return self._contiguous

    def data_ptr(self):
        return self._address


def test_refusals_come_before_any_upload_or_launch(monkeypatch):
    monkeypatch.setattr(kernels, "_adam_upload", lambda *a: pytest.fail("a table was uploaded"))
    monkeypatch.setattr(kernels, "call", lambda *a: pytest.fail("a kernel was launched"))
    host = [torch.zeros(5)]
    with pytest.raises(_hip.MdxError, match=r"parameters\[0\] lives on cpu: the optimizer step runs on the GPU only"):
        kernels.adam_plan(host, [torch.zeros(5)], [torch.zeros(5)], [torch.zeros(5)])
    fine = lambda: _DeviceTensor()
    with pytest.raises(ValueError, match=r"weights\.1 has dtype torch\.float64"):
        kernels.adam_plan([fine(), _DeviceTensor(dtype=torch.float64)], [fine(), fine()], [fine(), fine()], [fine(), fine()],
                          names=["weights.0", "weights.1"])
    with pytest.raises(ValueError, match=r"parameters\[0\] is not contiguous"):
        kernels.adam_plan([_DeviceTensor(contiguous=False)], [fine()], [fine()], [fine()])
    with pytest.raises(ValueError, match=r"parameters\[0\]\.exp_avg has 3 elements, parameters\[0\] has 8"):
        kernels.adam_plan([fine()], [fine()], [_DeviceTensor(count=3)], [fine()])
    with pytest.raises(_hip.MdxError, match=r"parameters\[0\]\.grad lives on cpu"):
        kernels.adam_plan([fine()], [torch.zeros(8)], [fine()], [fine()])
    with pytest.raises(ValueError, match="left out of the plan"):
        kernels.adam_plan([fine()], [None], [fine()], [fine()])
    # load_optimizer does not hand a host or float64 model to the fused step at all; FusedAdam on host tensors refuses at step()
    optimizer = optimizer_module.FusedAdam([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    optimizer.param_groups[0]["params"][0].grad = torch.ones(3)
    with pytest.raises(_hip.MdxError, match="the optimizer step runs on the GPU only"):
        optimizer.step()


def test_table_builder_on_the_big_shapes(monkeypatch):
    chunk = kernels.ADAM_CHUNK_ELEMENTS
    counts = [int(c) for c in oc.fixture("big")["counts"]]
    block_tensor, block_offset = kernels.adam_chunk_table(counts)
    assert block_tensor == [0, 0, 1, 1] and block_offset == [0, chunk, 0, chunk]
    assert kernels.adam_chunk_table([1, chunk, chunk + 1]) == ([0, 1, 2, 2], [0, 0, 0, chunk])
    with pytest.raises(ValueError, match="without elements"):
        kernels.adam_chunk_table([4, 0])
    # the step counters: one entry per chunk, in the order of the tensors
    assert kernels.adam_counter_slots([chunk + 1, 0, 2 * chunk, 5]) == ([0, 2, 2, 4], 5)
    # the plan: the tensor without elements is absent, slots follow the tensors kept; the cache key is pointers, counts, slots
    uploads = []
    monkeypatch.setattr(kernels, "_adam_upload", lambda values, dtype, device: uploads.append((values, dtype)) or values)
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    monkeypatch.setattr(kernels, "_ADAM_PLANS", {})
    tensors = lambda base: [_DeviceTensor(chunk + 1, address=base), _DeviceTensor(0, address=base + 64),
                            _DeviceTensor(2 * chunk, address=base + (1 << 20))]
    p, g, m, v = tensors(1 << 24), tensors(2 << 24), tensors(3 << 24), tensors(4 << 24)
    plan = kernels.adam_plan(p, g, m, v)
    assert plan.number_of_blocks == 4 and plan.counts == [chunk + 1, 2 * chunk] and plan.slots == [0, 2]
    assert plan.block_tensor == [0, 0, 1, 1] and plan.block_offset == [0, chunk, 0, chunk]
    assert plan.addresses == [(1 << 24, 2 << 24, 3 << 24, 4 << 24), tuple((k << 24) + (1 << 20) for k in (1, 2, 3, 4))]
    assert plan.key == ((1 << 24, 2 << 24, 3 << 24, 4 << 24, chunk + 1, 0),
                        tuple((k << 24) + (1 << 20) for k in (1, 2, 3, 4)) + (2 * chunk, 2))
    assert len(uploads) == 5 and plan.counters == 4
    assert kernels.adam_plan(p, g, m, v) is plan and len(uploads) == 5          # cached: nothing uploaded again
