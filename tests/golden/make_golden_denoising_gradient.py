"""Generate the denoising-gradient fixtures tests/golden/denoising_gradient/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_denoising_gradient.py

The derivative of the loss the reference's training_step optimises -- _generic_step's `loss`, the mean over the batch of
lambda_x mean_x + lambda_l mean_l + lambda_a mean_a -- with respect to the network's three predictions, by the reference's own
functions under torch's float64 autograd: make_golden_denoising_loss._step on that maker's operands (case_arrays), the three
predictions promoted to binary64 LEAVES, `out["loss"].backward()`.

Cases: the six operand sets of make_golden_denoising_loss.py, whose files hold the operands, and c4_n300_d3_p6, (C, N, D, P) =
(4, 300, 3, 6) with a seed of its own -- more atoms than the kernel's workgroup has threads -- whose file here holds what
case_arrays makes for it and the tests need (LARGE_KEEPS: the operands, the two binary64 targets, the per-structure means)
beside the gradients.  Arrays of a file, for <algorithm> in mse,
weighted_mse (X and L both):
  <algorithm>_gradient_x64 [B, N, D], _gradient_a64 [B, N, C], _gradient_l64 [B, P], _loss64 []
  softmax_clip_margin, posterior_clip_margin     the smallest relative distance |v - eps| / eps of a clipped value v from eps
                                                 among the elements where the side of the clip changes the gradient
Asserted here, for every element of every case: every gradient is finite; the MASK column of gradient_a is exactly 0; and on
both clips (the softmax at eps, the posterior p(a_{t-1} | a_t) at eps) either the decision has a relative margin of at least
1e-6, or both sides give the same gradient (the posterior's weight is 0: q_i = 0 above time index 0, i != a_0 at it).  A
binary64 evaluation in another operation order then takes the reference's side of every clip.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)
import make_golden_denoising_loss as loss_maker  # noqa: E402

DIRECTORY = "denoising_gradient"
ALGORITHMS = loss_maker.ALGORITHMS
LARGE = "c4_n300_d3_p6"
CASES = tuple(loss_maker.CASES) + (LARGE,)
FILES = [name + ".npz" for name in CASES]
CLIP_MARGIN = 1e-6
PREDICTIONS = ("predicted_x", "logits", "predicted_l")
# what the large case's own file keeps of case_arrays: the operands, the two binary64 targets and the per-structure means (the
# unreduced records, the draws and the binary32 records would take the file past the size a committed file may have)
LARGE_KEEPS = ("shape", "kmax", "ce_weight", "eps", "sigma0", "exponent", "lambda", "table_q", "table_q_bar", "table_q_bar_tm1",
               "x0", "l0", "a0", "time", "noise", "time_indices", "xt", "at", "lt", "sigma_n", "sigma_n_divisor", "predicted_x",
               "logits", "predicted_l", "target_x64", "target_l64", "mse_per_structure64", "weighted_mse_per_structure64")


def _operands(arrays):
    """_step's operands from what case_arrays recorded."""
    t = {key: torch.from_numpy(np.ascontiguousarray(arrays[key])) for key in (
        "x0", "xt", "l0", "lt", "a0", "at", "noise", "sigma_n", "predicted_x", "predicted_l", "logits", "time_indices")}
    for key in ("q", "q_bar", "q_bar_tm1"):
        t[key] = torch.from_numpy(arrays["table_" + key])[t["time_indices"]]
    return t


def _clip_margins(out, operands, eps):
    """The smallest relative margin of the two clip decisions among the elements where the decision matters."""
    softmax = torch.softmax(operands["logits"].detach(), dim=-1)
    softmax_margin = float(((softmax - eps).abs() / eps).min())
    C = softmax.shape[-1]
    first = (operands["time_indices"] == 0).reshape(-1, 1, 1)
    kept = torch.nn.functional.one_hot(operands["a0"], C).double()
    weight = torch.where(first, kept, out["q"].detach())
    decisive = weight != 0.0
    margins = ((out["p"].detach() - eps).abs() / eps)[decisive]
    return softmax_margin, float(margins.min()) if margins.numel() else float("inf")


def case_gradients(name, arrays):
    C = int(arrays["shape"][0])
    recorded = {}
    for algorithm in ALGORITHMS:
        parameters = loss_maker._loss_parameters(algorithm, name)
        operands = _operands(arrays)
        for key in PREDICTIONS:
            operands[key] = operands[key].double().requires_grad_(True)
        out = loss_maker._step(operands, parameters, lambda t: t.double())
        assert out["loss"].dtype == torch.float64 and all(out[key] is not None for key in ("p", "q"))
        out["loss"].backward()
        gradients = dict(gradient_x=operands["predicted_x"].grad, gradient_a=operands["logits"].grad,
                         gradient_l=operands["predicted_l"].grad)
        for key, value in gradients.items():
            assert value.dtype == torch.float64 and bool(torch.isfinite(value).all()), (name, algorithm, key)
            recorded[f"{algorithm}_{key}64"] = mg._np(value)
        assert bool((gradients["gradient_a"][..., C - 1] == 0.0).all()), (name, algorithm)
        recorded[f"{algorithm}_loss64"] = mg._np(out["loss"])
        margins = _clip_margins(out, operands, parameters.A.eps)
        assert min(margins) >= CLIP_MARGIN, (name, algorithm, margins)
        if "softmax_clip_margin" in recorded:       # the atom types' part is the same for both algorithms
            assert margins == (float(recorded["softmax_clip_margin"]), float(recorded["posterior_clip_margin"]))
        recorded["softmax_clip_margin"], recorded["posterior_clip_margin"] = np.array(margins[0]), np.array(margins[1])
    return recorded


def golden_denoising_gradient():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    loss_maker.CASES[LARGE] = ((4, 300, 3, 6), 1417)       # case_arrays looks its shape and seed up there
    for name in CASES:
        arrays = loss_maker.case_arrays(name)
        gradients = case_gradients(name, arrays)
        for algorithm in ALGORITHMS:       # the forward's record of the same number
            assert np.array_equal(arrays[f"{algorithm}_loss64"], gradients[f"{algorithm}_loss64"]), (name, algorithm)
        own = {key: arrays[key] for key in LARGE_KEEPS} if name == LARGE else {}
        mg.save(os.path.join(DIRECTORY, name + ".npz"), **own, **gradients)


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_denoising_gradient()
