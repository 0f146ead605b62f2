"""The optimizer-step fixtures (tests/golden/optimizer/*, made by tests/golden/make_golden_optimizer.py) as the tests read them:
the file list, the loaders, the derived bound, a float64 numpy restatement of the closed form of include/mdx_hip.h, and the
device operands of a record."""
import os

import numpy as np
import torch

from conftest import GOLDEN

TEACHER_FORCED = ("adamw_decay", "adam_l2", "adam_default", "adamw_clip", "missing_gradient", "unaligned_view", "big")
YAML = "config_diffusion_mlp_orion.yaml"
FILES = [name + ".npz" for name in TEACHER_FORCED + ("free_running",)] + [YAML]
DIRECTORY = os.path.join(GOLDEN, "optimizer")
SMALL_SHAPES = ((1,), (63,), (64,), (65,), (65, 3), (257,), (0,))
MISSING_TENSOR, MISSING_RECORD = 2, 1           # missing_gradient: tensor 2 has grad None at record 1
_LOADED = {}


def fixture(name):
    if name not in _LOADED:
        with np.load(os.path.join(DIRECTORY, name + ".npz")) as data:
            _LOADED[name] = {key: data[key] for key in data.files}
    return _LOADED[name]


def records(case):
    return range(int(fixture(case)["steps"]))


def shapes(g):
    counts = [int(c) for c in g["counts"]]
    return list(SMALL_SHAPES) if counts == [int(np.prod(s)) for s in SMALL_SHAPES] else [(c,) for c in counts]


def split(flat, counts):
    bounds = np.cumsum([0] + [int(c) for c in counts])
    return [flat[bounds[k]:bounds[k + 1]] for k in range(len(counts))]


def hyper(g):
    return dict(lr=float(g["lr"]), beta1=float(g["beta1"]), beta2=float(g["beta2"]), eps=float(g["eps"]),
                weight_decay=float(g["weight_decay"]), max_norm=float(g["max_norm"]))


def decoupled(g):
    return str(g["optimizer"]) == "adamw"


def bound(reference64, parameter=None):
    """|got - ref64| <= 2^-23 |ref64| + 2^-149: one binary32 rounding of a binary64 evaluation, one denormal step as the floor;
    for p' also 2^-50 |p|: a binary64 evaluation in another operation order moves q - delta by a few 2^-53 |p|."""
    reference64 = np.asarray(reference64, dtype=np.float64)
    limit = 2.0**-23 * np.abs(reference64) + 2.0**-149
    if parameter is not None:
        limit = limit + 2.0**-50 * np.abs(np.asarray(parameter, dtype=np.float64))
    return limit


def closed_form64(p, g, m, v, t, *, lr, beta1, beta2, eps, weight_decay, decoupled_weight_decay, clip=1.0, gradient_scale=1.0,
                  bias_correction=True):
    """The closed form of include/mdx_hip.h (mdx_adam_step) in float64 numpy for one tensor at counter t: p', m', v'."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g = (gradient_scale * clip) * g
    if decoupled_weight_decay:
        q = p * (1.0 - lr * weight_decay)
    else:
        g = g + weight_decay * p
        q = p
    m1 = m + (g - m) * (1.0 - beta1)
    v1 = beta2 * v + (1.0 - beta2) * g * g
    correction1 = 1.0 - beta1**int(t) if bias_correction else 1.0
    correction2 = 1.0 - beta2**int(t) if bias_correction else 1.0
    p1 = q - (lr / correction1) * m1 / (np.sqrt(v1) / np.sqrt(correction2) + eps)
    return p1, m1, v1


def norm64(g, i):
    """The global 2-norm of the gradients of record i that are not None, in float64."""
    pieces = [piece.astype(np.float64) for piece, has in zip(split(g[f"r{i}_g"], g["counts"]), g[f"r{i}_has_gradient"]) if has]
    return float(np.sqrt(sum(float(np.sum(piece * piece)) for piece in pieces)))


def clip_of(g, i):
    max_norm = float(g["max_norm"])
    return min(1.0, max_norm / (norm64(g, i) + 1.0e-6)) if max_norm > 0.0 else 1.0


def restatement(g, i, flip_decoupled=False, bias_correction=True, clip=None, advance=None):
    """closed_form64 over record i: (p64, m64, v64) flat, as the record holds them.  The switches are the controls: the
    decoupled flag flipped, no bias correction, a given clip factor, `advance` = a tensor whose counter is taken one too far."""
    counts = g["counts"]
    clip = clip_of(g, i) if clip is None else clip
    flag = decoupled(g) != flip_decoupled
    out = ([], [], [])
    parts = [split(g[f"r{i}_{key}"], counts) for key in ("p", "g", "m", "v")]
    for k in range(len(counts)):
        p, gradient, m, v = (part[k] for part in parts)
        if not g[f"r{i}_has_gradient"][k]:
            result = (p.astype(np.float64), m.astype(np.float64), v.astype(np.float64))
        else:
            t = int(g[f"r{i}_step_before"][k]) + 1 + (1 if advance == k else 0)
            values = hyper(g)
            values.pop("max_norm")
            result = closed_form64(p, gradient, m, v, t, decoupled_weight_decay=flag, clip=clip, bias_correction=bias_correction,
                                   **values)
        for collected, value in zip(out, result):
            collected.append(value)
    return tuple(np.concatenate(collected) for collected in out)


def excess(got, reference64, parameter=None):
    """max over the elements of |got - ref64| / bound: <= 1 is within the bound."""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - np.asarray(reference64, dtype=np.float64)) / bound(reference64, parameter)))


def device_operands(g, i, device, offset=0):
    """The operands of record i as lists of device tensors in the list's shapes: (p, gradients, m, v); a gradient None where the
    record has none.  offset > 0: every tensor is a view at that element offset of a larger buffer."""
    counts = g["counts"]

    def tensors(key):
        out = []
        for piece, shape in zip(split(g[f"r{i}_{key}"], counts), shapes(g)):
            if offset:
                buffer = torch.zeros(piece.size + offset + 3, dtype=torch.float32, device=device)
                buffer[offset:offset + piece.size] = torch.from_numpy(np.ascontiguousarray(piece)).to(device)
                out.append(buffer[offset:offset + piece.size].view(shape))
            else:
                out.append(torch.from_numpy(np.ascontiguousarray(piece)).to(device).view(shape))
        return out

    p, gradients, m, v = tensors("p"), tensors("g"), tensors("m"), tensors("v")
    gradients = [gradient if has else None for gradient, has in zip(gradients, g[f"r{i}_has_gradient"])]
    return p, gradients, m, v


def flat(tensors):
    return np.concatenate([t.detach().cpu().numpy().reshape(-1) for t in tensors]) if tensors else np.zeros(0, np.float32)


def torch64_step(p, gradients, m, v, steps_before, *, lr, weight_decay, decoupled_weight_decay, max_norm=0.0, betas=(0.9, 0.999),
                 eps=1e-8):
    """One step of torch's own Adam / AdamW on the CPU in float64 -- the fixtures' reference -- on float64 copies of the given
    operands (lists; a gradient None leaves its tensor out; steps_before per tensor; m, v may be None before a first step).
    Returns (p64, m64, v64, norm64 or None): lists of float64 numpy arrays, the operands' own where a tensor took no step."""
    parameters = [torch.nn.Parameter(x.detach().cpu().double().clone()) for x in p]
    optimizer_class = torch.optim.AdamW if decoupled_weight_decay else torch.optim.Adam
    optimizer = optimizer_class(parameters, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
    wide = lambda x, like: torch.zeros_like(like) if x is None else x.detach().cpu().double().clone()
    for k, q in enumerate(parameters):
        if gradients[k] is None:
            continue
        q.grad = gradients[k].detach().cpu().double().clone()
        if int(steps_before[k]) > 0:
            optimizer.state[q] = dict(step=torch.tensor(float(steps_before[k])), exp_avg=wide(m[k], q), exp_avg_sq=wide(v[k], q))
    norm = None
    if max_norm > 0.0:
        norm = float(torch.nn.utils.clip_grad_norm_([q for q in parameters if q.grad is not None], max_norm))
    optimizer.step()
    p64 = [q.detach().numpy().reshape(-1) for q in parameters]
    m64, v64 = [], []
    for k, q in enumerate(parameters):
        state = optimizer.state.get(q, {})
        m64.append((state["exp_avg"] if "exp_avg" in state else wide(None if m is None else m[k], q)).numpy().reshape(-1))
        v64.append((state["exp_avg_sq"] if "exp_avg_sq" in state else wide(None if v is None else v[k], q)).numpy().reshape(-1))
    return p64, m64, v64, norm
