"""The host side of the optimal torus translation (csrc/mdx_optimal_translation.hip, kernels.optimal_translation): the C entry and
its status bit in the binding, the refusal of host tensors and of sizes beyond the transport unit's limits before any launch, and
the fixtures' own records (tests/golden/optimal_translation/, made by tests/golden/make_golden_optimal_translation.py).

The reference's public module transport/optimal_translation.py is NOT in this package: tests/test_transport_cpu.py pins that the
file is absent, and that test stays as it is.  The kernel is reached through `kernels.optimal_translation`."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

FAMILIES = [("uniform", n) for n in (1, 2, 3, 8, 63, 64, 65, 255, 256)] + [("shift", n) for n in (1, 8, 64, 256)] + \
    [("shiftnoise", n) for n in (1, 8, 64, 256)] + [("unbounded", n) for n in (3, 64)] + [("equal", n) for n in (8, 65)] + \
    [("duplicates", n) for n in (8, 65)] + [("shared", n) for n in (8, 64)]
CASES = [f"{family}_n{n}" for family, n in FAMILIES] + ["boundary_n1", "boundary_n2"]
FILES = [name + ".npz" for name in CASES]


def fixture(name):
    return np.load(os.path.join(GOLDEN, "optimal_translation", name + ".npz"))


def test_the_binding_declares_the_entry():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    assert "mdx_optimal_translation" in _hip.ABI_SYMBOLS and _hip.STATUS_TRANSLATION_NO_CANDIDATE == 32768
    assert _hip.ABI_VERSION == 14
    assert callable(kernels.optimal_translation)
    header = open(os.path.join(ROOT, "include", "mdx_hip.h")).read()
    assert re.search(r"#define MDX_STATUS_TRANSLATION_NO_CANDIDATE 32768u", header) and "#define MDX_ABI_VERSION 14" in header
    assert re.search(r"MDX_API int mdx_optimal_translation\(const float\* x, int64_t x_batch_stride, const float\* y, int64_t batch,", header)
    makefile = open(os.path.join(os.path.dirname(_hip.__file__), "csrc", "Makefile")).read()
    assert "mdx_optimal_translation.o" in makefile.split("OBJS =")[1].split("\n\n")[0]
    bits = [getattr(_hip, name) for name in dir(_hip) if name.startswith("STATUS_")]
    assert len(bits) == len(set(bits)) and all(bit & (bit - 1) == 0 for bit in bits)       # one bit each, none shared


def test_host_tensors_are_refused():
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
    x = torch.rand(2, 5, 3)
    for call in (lambda: kernels.optimal_translation(x, x), lambda: kernels.optimal_translation(x[0], x, with_details=True),
                 lambda: kernels.optimal_translation(x, x, status=torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(MdxError, match="lives on cpu: the optimal translation runs on the GPU only \\(no CPU fallback\\)"):
            call()


def test_sizes_beyond_the_limits_are_refused_before_any_launch():
    """The C entry checks the sizes before it looks at a pointer, so with NULL pointers (and no GPU) the answer is the refusal."""
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    lib = _hip.lib()

    def call(batch, N, D, stride=0):
        return lib.mdx_optimal_translation(None, stride, None, batch, N, D, None, None, None, None, None)
    unsupported, invalid = -2, -1
    assert call(4, 257, 3) == unsupported and call(4, 8, 4) == unsupported and call(4, 257, 3, 257 * 3) == unsupported
    assert call(2**31 // 3 + 1, 8, 3) == unsupported
    assert call(4, 0, 3) == invalid and call(4, 8, 0) == invalid and call(-1, 8, 3) == invalid
    assert call(4, 8, 3, 8) == invalid                          # a stride that is neither 0 nor N D
    assert call(4, 256, 3) == invalid and call(4, 8, 3, 24) == invalid        # within the limits: the NULL pointers are seen
    assert call(0, 256, 3) == _hip.MDX_OK
    with pytest.raises(_hip.MdxError, match="mdx_optimal_translation: unsupported size or option"):
        _hip.check(call(4, 257, 3), "mdx_optimal_translation")
    assert lib.mdx_optimal_translation.argtypes[1] is ctypes.c_int64 and len(lib.mdx_optimal_translation.argtypes) == 11


def test_the_fixtures_hold_what_their_maker_asserts():
    assert sorted(os.listdir(os.path.join(GOLDEN, "optimal_translation"))) == sorted(FILES)
    gaps, roundings = [], []
    for name in CASES:
        case = fixture(name)
        for D in case["dimensions"]:
            tau64, count = case[f"d{D}_tau64"], case[f"d{D}_count64"]
            y = case[f"d{D}_y"]
            assert y.dtype == np.float32 and case[f"d{D}_x"].dtype == np.float32 and y.shape[2] == D and tau64.shape == (y.shape[0], D)
            assert case[f"d{D}_tau32"].dtype == np.float32 and tau64.dtype == np.float64
            assert np.array_equal(np.isinf(tau64), count == 0) and np.array_equal(np.isinf(tau64), np.isinf(case[f"d{D}_tau32"]))
            assert np.isinf(tau64).any() == name.startswith("boundary")
            assert np.array_equal(count.ravel(), np.bincount(case[f"d{D}_batch64"] * D + case[f"d{D}_alpha64"], minlength=count.size))
            gaps.append(float(case[f"d{D}_cost_gap64"]))
            roundings.append(float(case[f"d{D}_tau_rounding"]))
            if name.split("_")[0] in ("uniform", "shift", "shiftnoise", "unbounded"):
                assert float(case[f"d{D}_rhs_margin64"]) >= 1e-5
            if name.startswith("equal"):
                assert (tau64 == 0).all() and (case[f"d{D}_cost64"] == 0).all()
    assert min(gaps) > 1e-6
    print(f"smallest cost gap {min(gaps):.2e}, largest |tau32 - tau64| {max(roundings):.2e}")
    assert np.array_equal(fixture("boundary_n1")["d1_tau64"], [[np.inf], [-0.25]])
    second = fixture("boundary_n2")["d2_tau64"]
    assert np.isinf(second[0, 0]) and abs(second[0, 1] + 0.2) < 1e-7
