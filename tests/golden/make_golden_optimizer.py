"""Generate the optimizer-step fixtures tests/golden/optimizer/*.npz by IMPORTING the reference (container-only).

    PYTHONPATH=<the reference checkout>/src python tests/golden/make_golden_optimizer.py

The reference's load_optimizer (models/optimizer.py:60-82) builds the optimizer on float64 parameters; clipping is torch's
clip_grad_norm_, which is what Lightning's default gradient_clip_algorithm="norm" calls.

Records are TEACHER-FORCED: the operands p, g, m, v of a step are binary32 values, `step` is given, and the record is the float64
result of ONE reference step on their float64 copies -- so rounding errors do not accumulate across steps, and a record may start
anywhere (t = 1000).  The operands come from numpy's generator (the same draws on every host); the arithmetic is float64 torch.

A file holds, with all tensors of the list concatenated flat in list order (counts int64 [tensors]):
  optimizer ("adam" | "adamw"), lr, weight_decay, beta1, beta2, eps, max_norm (0: no clipping), steps (the number of records)
  per record i:  r{i}_p, r{i}_g, r{i}_m, r{i}_v f32 [total]   the operands
                 r{i}_has_gradient bool [tensors]             False: grad None, the tensor is left out of the step
                 r{i}_step_before int32 [tensors]             the counters given
                 r{i}_p64, r{i}_m64, r{i}_v64 f64 [total]     the reference's results
                 r{i}_step int32 [tensors]                    the counters after
                 r{i}_norm64 f64                              with clipping: what clip_grad_norm_ returned

    adamw_decay       adamw, lr 1e-3, weight_decay 1e-2; t = 1, 2, 3 and 1000
    adam_l2           adam, weight_decay 1e-2 (coupled); t = 1, 2
    adam_default      adam, weight_decay 0 (the reference's default); t = 1, 2; tensor 1's gradient is all zeros
    adamw_clip        adamw, weight_decay 1e-6, max_norm 0.1: a record whose norm exceeds 0.1, one whose norm is below it
    missing_gradient  adamw; tensor 2 has grad None at the second of three records: nothing of it changes, t lags afterwards
    unaligned_view    adamw; the lists 257, 65, 6: the test makes the parameter and its state views at element offset 1
    big               adamw, max_norm 1; CHUNK + 1 and 2 CHUNK elements, CHUNK = MDX_ADAM_CHUNK_ELEMENTS of include/mdx_hip.h; t = 1, 2
    free_running      adamw, the small list, 20 consecutive float64 steps WITHOUT teacher forcing: p0 f32 [total], g f32 [20, total],
                      p64 f64 [20, total] (the float64 parameters after each step), m64, v64 f64 [total] (after the last)
Beside them config_diffusion_mlp_orion.yaml, the reference's template (settings only), for its `optimizer:` / `scheduler:` blocks.
The small list: 1, 63, 64, 65, (65, 3), 257 elements and one tensor without elements.  Gradient magnitudes are spread per tensor
from 1e-6 to 10; parameters are drawn from N(0, 1).
"""
import os
import re
import shutil
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stubs and imports the reference)

import diffusion_for_multi_scale_molecular_dynamics as reference_package  # noqa: E402
from diffusion_for_multi_scale_molecular_dynamics.models.optimizer import OptimizerParameters, load_optimizer  # noqa: E402

DIRECTORY = "optimizer"
HEADER = os.path.join(os.path.dirname(os.path.dirname(mg.HERE)), "include", "mdx_hip.h")
CHUNK = int(re.search(r"#define\s+MDX_ADAM_CHUNK_ELEMENTS\s+(\d+)", open(HEADER).read()).group(1))
SMALL = (1, 63, 64, 65, 65 * 3, 257, 0)
CASES = {      # name -> (optimizer name, lr, weight_decay, max_norm, counts, seed, the records' t)
    "adamw_decay": ("adamw", 1e-3, 1e-2, 0.0, SMALL, 2101, (1, 2, 3, 1000)),
    "adam_l2": ("adam", 1e-3, 1e-2, 0.0, SMALL, 2102, (1, 2)),
    "adam_default": ("adam", 1e-3, 0.0, 0.0, SMALL, 2103, (1, 2)),
    "adamw_clip": ("adamw", 1e-3, 1e-6, 0.1, SMALL, 2104, (1, 2)),
    "missing_gradient": ("adamw", 1e-3, 1e-2, 0.0, SMALL, 2105, (1, 2, 3)),
    "unaligned_view": ("adamw", 1e-3, 1e-2, 0.0, (257, 65, 6), 2106, (3,)),
    "big": ("adamw", 1e-3, 1e-2, 1.0, (CHUNK + 1, 2 * CHUNK), 2107, (1, 2))}
FREE_RUNNING_STEPS, FREE_RUNNING_SEED = 20, 2108
YAML = "config_diffusion_mlp_orion.yaml"
YAML_SOURCE = ("configuration_templates", "diffusion_config_files", YAML)
FILES = [name + ".npz" for name in list(CASES) + ["free_running"]] + [YAML]
MISSING_TENSOR, MISSING_RECORD, ZERO_GRADIENT_TENSOR = 2, 1, 1


class _Holder(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.tensors = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


def _magnitudes(counts):
    live = [k for k, c in enumerate(counts) if c]
    spread = np.logspace(-6.0, 1.0, len(live))
    return {k: spread[i] for i, k in enumerate(live)}


def _split(flat, counts):
    bounds = np.cumsum([0] + list(counts))
    return [flat[bounds[k]:bounds[k + 1]] for k in range(len(counts))]


def _operands(rng, counts, t, gradient_factor=1.0):
    """p, g, m, v f32 [total]: m = v = 0 at t = 1 (a first step), plausible moments of the gradient's magnitude later."""
    magnitudes = _magnitudes(counts)
    p, g, m, v = [], [], [], []
    for k, count in enumerate(counts):
        scale = magnitudes.get(k, 1.0) * gradient_factor
        p.append(rng.standard_normal(count))
        g.append(scale * rng.standard_normal(count))
        m.append(np.zeros(count) if t == 1 else 0.5 * scale * rng.standard_normal(count))
        v.append(np.zeros(count) if t == 1 else scale**2 * rng.uniform(0.1, 1.0, count))
    return [np.concatenate(a).astype(np.float32) for a in (p, g, m, v)]


def _reference_step(name, lr, weight_decay, max_norm, counts, p, g, m, v, step_before, has_gradient):
    """One step of the reference's optimizer on float64 copies: p64, m64, v64 [total], step [tensors], norm64 or None."""
    tensors = [torch.from_numpy(a.astype(np.float64)) for a in _split(p, counts)]
    holder = _Holder(tensors)
    optimizer = load_optimizer(OptimizerParameters(name=name, learning_rate=lr, weight_decay=weight_decay), holder)
    parameters = list(holder.tensors)
    for k, q in enumerate(parameters):
        if step_before[k] > 0 or not has_gradient[k]:
            optimizer.state[q] = dict(step=torch.tensor(float(step_before[k])),
                                      exp_avg=torch.from_numpy(_split(m, counts)[k].astype(np.float64)),
                                      exp_avg_sq=torch.from_numpy(_split(v, counts)[k].astype(np.float64)))
        q.grad = torch.from_numpy(_split(g, counts)[k].astype(np.float64)) if has_gradient[k] else None
    norm64 = None
    if max_norm > 0.0:
        norm64 = torch.nn.utils.clip_grad_norm_(parameters, max_norm)
        assert norm64.dtype == torch.float64
    optimizer.step()
    p64 = np.concatenate([mg._np(q).reshape(-1) for q in parameters])
    m64, v64, step = [], [], []
    for k, q in enumerate(parameters):
        state = optimizer.state.get(q, {})
        if "exp_avg" in state:
            m64.append(mg._np(state["exp_avg"]).reshape(-1))
            v64.append(mg._np(state["exp_avg_sq"]).reshape(-1))
            step.append(int(state["step"]))
        else:           # (never stepped and no state forced: nothing to read)
            m64.append(_split(m, counts)[k].astype(np.float64))
            v64.append(_split(v, counts)[k].astype(np.float64))
            step.append(int(step_before[k]))
    assert p64.dtype == np.float64
    return p64, np.concatenate(m64), np.concatenate(v64), np.array(step, dtype=np.int32), norm64, optimizer.defaults


def teacher_forced_case(case):
    name, lr, weight_decay, max_norm, counts, seed, ts = CASES[case]
    rng = np.random.default_rng(seed)
    arrays = dict(optimizer=np.array(name), lr=np.array(lr), weight_decay=np.array(weight_decay), max_norm=np.array(max_norm),
                  counts=np.array(counts, dtype=np.int64), steps=np.array(len(ts)), seed=np.array(seed))
    lag = 0
    for i, t in enumerate(ts):
        # adamw_clip: the first record's norm is far above max_norm, the second's below it
        factor = 1e-4 if (case == "adamw_clip" and i == 1) else 1.0
        p, g, m, v = _operands(rng, counts, t, factor)
        has_gradient = np.array([True] * len(counts))
        step_before = np.full(len(counts), t - 1, dtype=np.int32)
        if case == "adam_default":
            bounds = np.cumsum([0] + list(counts))
            g[bounds[ZERO_GRADIENT_TENSOR]:bounds[ZERO_GRADIENT_TENSOR + 1]] = 0.0
        if case == "missing_gradient":
            if i == MISSING_RECORD:
                has_gradient[MISSING_TENSOR], lag = False, 1
            step_before[MISSING_TENSOR] -= lag if i > MISSING_RECORD else 0
        p64, m64, v64, step, norm64, defaults = _reference_step(name, lr, weight_decay, max_norm, counts, p, g, m, v, step_before,
                                                                has_gradient)
        arrays.update({f"r{i}_p": p, f"r{i}_g": g, f"r{i}_m": m, f"r{i}_v": v, f"r{i}_has_gradient": has_gradient,
                       f"r{i}_step_before": step_before, f"r{i}_p64": p64, f"r{i}_m64": m64, f"r{i}_v64": v64, f"r{i}_step": step})
        if norm64 is not None:
            arrays[f"r{i}_norm64"] = mg._np(norm64)
            assert (float(norm64) > max_norm) == (not (case == "adamw_clip" and i == 1)), (case, i, float(norm64))
        assert np.isfinite(p64).all() and np.isfinite(m64).all() and np.isfinite(v64).all()
    if case == "missing_gradient":
        bounds = np.cumsum([0] + list(counts))
        lo, hi = bounds[MISSING_TENSOR], bounds[MISSING_TENSOR + 1]
        i = MISSING_RECORD
        assert np.array_equal(arrays[f"r{i}_p64"][lo:hi], arrays[f"r{i}_p"][lo:hi].astype(np.float64))
        assert arrays[f"r{i}_step"][MISSING_TENSOR] == arrays[f"r{i}_step_before"][MISSING_TENSOR]
        assert arrays[f"r{i + 1}_step"][MISSING_TENSOR] == arrays[f"r{i + 1}_step"][0] - 1
    arrays.update(beta1=np.array(defaults["betas"][0]), beta2=np.array(defaults["betas"][1]), eps=np.array(defaults["eps"]))
    return arrays


def free_running_case():
    name, lr, weight_decay, counts = "adamw", 1e-3, 1e-2, SMALL
    rng = np.random.default_rng(FREE_RUNNING_SEED)
    p0 = _operands(rng, counts, 1)[0]
    gradients = np.stack([_operands(rng, counts, 1)[1] for _ in range(FREE_RUNNING_STEPS)])
    holder = _Holder([torch.from_numpy(a.astype(np.float64)) for a in _split(p0, counts)])
    optimizer = load_optimizer(OptimizerParameters(name=name, learning_rate=lr, weight_decay=weight_decay), holder)
    parameters = list(holder.tensors)
    trajectory = []
    for s in range(FREE_RUNNING_STEPS):
        for q, g in zip(parameters, _split(gradients[s], counts)):
            q.grad = torch.from_numpy(g.astype(np.float64))
        optimizer.step()
        trajectory.append(np.concatenate([mg._np(q).reshape(-1).copy() for q in parameters]))
    m64 = np.concatenate([mg._np(optimizer.state[q]["exp_avg"]).reshape(-1) for q in parameters])
    v64 = np.concatenate([mg._np(optimizer.state[q]["exp_avg_sq"]).reshape(-1) for q in parameters])
    defaults = optimizer.defaults
    return dict(optimizer=np.array(name), lr=np.array(lr), weight_decay=np.array(weight_decay), max_norm=np.array(0.0),
                counts=np.array(counts, dtype=np.int64), steps=np.array(FREE_RUNNING_STEPS), seed=np.array(FREE_RUNNING_SEED),
                beta1=np.array(defaults["betas"][0]), beta2=np.array(defaults["betas"][1]), eps=np.array(defaults["eps"]),
                p0=p0, g=gradients, p64=np.stack(trajectory), m64=m64, v64=v64)


def golden_optimizer():
    os.makedirs(os.path.join(mg.OUT, DIRECTORY), exist_ok=True)
    for case in CASES:
        mg.save(os.path.join(DIRECTORY, case + ".npz"), **teacher_forced_case(case))
    mg.save(os.path.join(DIRECTORY, "free_running.npz"), **free_running_case())
    # the reference's own `optimizer:` and `scheduler:` blocks: a file that holds only settings
    checkout = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(reference_package.__file__))))
    shutil.copyfile(os.path.join(checkout, *YAML_SOURCE), os.path.join(mg.OUT, DIRECTORY, YAML))


if __name__ == "__main__":
    torch.set_num_threads(1)
    golden_optimizer()
