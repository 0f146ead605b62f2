"""The denoising-loss fixtures (tests/golden/denoising_loss/*.npz, made by tests/golden/make_golden_denoising_loss.py) as the
tests read them: the file list, the bound, and the kernel's operands of a case."""
import os

import numpy as np
import torch

from conftest import GOLDEN

CASES = ("c2_n1_d1_p1", "c3_n5_d3_p6", "c8_n65_d2_p3", "clip", "placed", "sigma0_control")
FILES = [name + ".npz" for name in CASES]
ALGORITHMS = ("mse", "weighted_mse")
DIRECTORY = os.path.join(GOLDEN, "denoising_loss")
_LOADED = {}


def fixture(name):
    if name not in _LOADED:
        with np.load(os.path.join(DIRECTORY, name + ".npz")) as data:
            _LOADED[name] = {key: data[key] for key in data.files}
    return _LOADED[name]


def excess(got, reference64):
    """The largest |got - reference| - (2^-23 |reference| + 1e-12): <= 0 when `got` is one binary32 rounding of a binary64
    evaluation that agrees with the reference's to well below that rounding (terms of at most -log(1e-8) = 18.4)."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    reference64 = np.asarray(reference64, dtype=np.float64)
    assert got.shape == reference64.shape, (got.shape, reference64.shape)
    return float((np.abs(got - reference64) - (2.0**-23 * np.abs(reference64) + 1e-12)).max())


def fraction(got, reference64):
    """The largest |got - reference| as a fraction of its bound (the figure the tests print)."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    reference64 = np.asarray(reference64, dtype=np.float64)
    return float((np.abs(got - reference64) / (2.0**-23 * np.abs(reference64) + 1e-12)).max())


def distance(got, reference64):
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float64)
    return float(np.abs(got - np.asarray(reference64, dtype=np.float64)).max())


def binary32(value):
    return float(np.float32(value))


def scalars(case, algorithm, rounded=True):
    """The kernel's scalar arguments of a case: sigma0 and exponent as the reference's binary32 buffers hold them."""
    g = fixture(case)
    out = dict(kmax=int(g["kmax"]), ce_weight=float(g["ce_weight"]), eps=float(g["eps"]), lambda_weights=tuple(float(w) for w in g["lambda"]))
    for prefix in ("x_", "l_"):
        out[prefix + "algorithm"] = algorithm
        if algorithm == "weighted_mse":
            out[prefix + "sigma0"] = binary32(g["sigma0"]) if rounded else float(g["sigma0"])
            out[prefix + "exponent"] = binary32(g["exponent"]) if rounded else float(g["exponent"])
    return out


def tensors(case, device, **replaced):
    """The kernel's tensor arguments of a case: the recorded operands and the recorded [T, C, C] tables."""
    g = fixture(case)
    names = dict(x0="x0", xt="xt", predicted_x="predicted_x", a0="a0", at="at", logits="logits", time_indices="time_indices",
                 q_matrices="table_q", q_bar_matrices="table_q_bar", q_bar_tm1_matrices="table_q_bar_tm1", l0="l0", lt="lt",
                 predicted_l="predicted_l", sigma_n="sigma_n")
    out = {argument: torch.from_numpy(np.ascontiguousarray(g[key])).to(device) for argument, key in names.items()}
    out["sigma"] = torch.from_numpy(np.ascontiguousarray(g["noise"][:, 0])).to(device)
    out.update(replaced)
    return out
