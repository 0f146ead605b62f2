"""The denoising-gradient fixtures (tests/golden/denoising_gradient/*.npz, made by
tests/golden/make_golden_denoising_gradient.py) as the tests read them, and `closed_form`: the gradient's closed form of
include/mdx_hip.h (mdx_denoising_loss_gradient) restated in float64 numpy, in matrix form -- another operation order than the
kernel's per-atom loops and than torch's autograd chain."""
import os

import numpy as np

import denoising_loss_cases as loss_cases
from conftest import GOLDEN

LARGE = "c4_n300_d3_p6"               # more atoms than the workgroup has threads; its file holds its own operands
CASES = loss_cases.CASES + (LARGE,)
FILES = [name + ".npz" for name in CASES]
ALGORITHMS = loss_cases.ALGORITHMS
DIRECTORY = os.path.join(GOLDEN, "denoising_gradient")
GRADIENTS = ("gradient_x", "gradient_a", "gradient_l")
_LOADED = {}


def gradient_fixture(case):
    """The gradient file of a case.  The large case's operands are handed to denoising_loss_cases' cache, so that its
    `fixture`, `tensors` and `scalars` serve all seven cases."""
    if case not in _LOADED:
        with np.load(os.path.join(DIRECTORY, case + ".npz")) as data:
            _LOADED[case] = {key: data[key] for key in data.files}
        if case == LARGE:
            loss_cases._LOADED[case] = _LOADED[case]
    return _LOADED[case]


def operands(case):
    gradient_fixture(case)
    return loss_cases.fixture(case)


def tensors(case, device, **replaced):
    operands(case)
    return loss_cases.tensors(case, device, **replaced)


def scalars(case, algorithm):
    operands(case)
    return loss_cases.scalars(case, algorithm)


def closed_form(case, algorithm, batch_divisor=None):
    """gradient_x, gradient_a, gradient_l and loss of a case in float64 from the recorded operands and binary64 targets."""
    g = operands(case)
    f64 = lambda key: g[key].astype(np.float64)
    C, N, D, P = (int(v) for v in g["shape"])
    B = g["x0"].shape[0]
    divisor = float(B if batch_divisor is None else batch_divisor)
    lambda_a, lambda_x, lambda_l = (float(w) for w in g["lambda"])
    sigma = f64("noise")[:, 0]
    weights = np.ones(B)
    if algorithm == "weighted_mse":       # sigma0 and exponent as the reference's binary32 buffers hold them
        weights = np.exp(loss_cases.binary32(g["exponent"]) * (sigma - loss_cases.binary32(g["sigma0"]))) + 1.0
    error_x, error_l = f64("predicted_x") - g["target_x64"], f64("predicted_l") - g["target_l64"]
    gradient_x = (2.0 * lambda_x / (divisor * N * D)) * weights[:, None, None] * error_x
    gradient_l = (2.0 * lambda_l / (divisor * P)) * weights[:, None] * error_l

    eps, ce_weight = float(g["eps"]), float(g["ce_weight"])
    a0, at, rows = g["a0"], g["at"], g["time_indices"]
    Q, Qbar, Qbar_tm1 = (f64(key)[rows] for key in ("table_q", "table_q_bar", "table_q_bar_tm1"))      # [B, C, C]
    structure = np.arange(B)[:, None]
    with np.errstate(over="ignore"):
        z = f64("logits")
        e = np.exp(z - z.max(axis=-1, keepdims=True))
    r = e / e.sum(axis=-1, keepdims=True)
    u = np.maximum(r, eps)
    S = u.sum(axis=-1, keepdims=True)
    p = u / S
    step, column = Q[structure, :, at], Qbar[structure, :, at]                  # [B, N, C]: Q[i, a_t] and Qbar[j, a_t]
    Dn = (p * column).sum(axis=-1, keepdims=True)
    pi = step * np.einsum("bnj,bji->bni", p, Qbar_tm1) / Dn
    one_hot_a0 = np.eye(C)[a0]
    q = Qbar_tm1[structure, a0, :] * step / Qbar[structure, a0, at][..., None]
    kept = np.where((rows == 0)[:, None, None], one_hot_a0, q)
    with np.errstate(invalid="ignore", divide="ignore"):       # a posterior of 0 is below eps: the select drops its quotient
        gvec = np.where(pi >= eps, -kept / pi, 0.0)
    h = (np.einsum("bni,bji->bnj", gvec * step, Qbar_tm1) - (gvec * pi).sum(axis=-1, keepdims=True) * column) / Dn
    v = np.where(r >= eps, (h - (h * p).sum(axis=-1, keepdims=True)) / S, 0.0)
    to_logits = r * (v - (r * v).sum(axis=-1, keepdims=True))
    to_logits = to_logits + ce_weight * (r - one_hot_a0) * (a0 != C - 1)[..., None]
    gradient_a = (lambda_a / (divisor * N * C)) * to_logits

    means = g[f"{algorithm}_per_structure64"]
    mean_x = (weights[:, None, None] * error_x**2).mean(axis=(1, 2))
    mean_l = (weights[:, None] * error_l**2).mean(axis=1)
    loss = float((lambda_x * mean_x + lambda_l * mean_l + lambda_a * means[:, 0]).sum() / divisor)
    return dict(gradient_x=gradient_x, gradient_a=gradient_a, gradient_l=gradient_l, loss=np.array(loss))
