"""The reference's models/optimizer.py: the `optimizer:` block of a training configuration and `load_optimizer`.

For float32 device parameters `load_optimizer` returns FusedAdam, whose step() is the fused multi-tensor kernel of
csrc/mdx_optimizer.hip (one launch per parameter group, three with gradient clipping); for host parameters, or any other dtype,
it returns torch's own class exactly as the reference does."""
import logging
from dataclasses import asdict, dataclass
from typing import Any, Dict, Union

import torch
from torch import optim

from .. import kernels
from ..utils.configuration_parsing import create_parameters_from_configuration_dictionary

logger = logging.getLogger(__name__)


@dataclass(kw_only=True)
class OptimizerParameters:
    """Parameters for the optimizer."""

    name: str
    learning_rate: float
    weight_decay: float = 0.0


OPTIMIZERS_BY_NAME = {'adam': optim.Adam, 'adamw': optim.AdamW, 'None': optim.Adam}
OPTIMIZER_PARAMETERS_BY_NAME = {'adam': OptimizerParameters, 'adamw': OptimizerParameters, 'None': OptimizerParameters}


def check_if_optimizer_is_none(optimizer_parameters: Union[OptimizerParameters, None]) -> bool:
    """Whether the optimizer's name is 'None': the reference's switch for turning optimization off  (:27-38)."""
    return optimizer_parameters.name == 'None'


def create_optimizer_parameters(optimizer_configuration_dictionary: Dict[str, Any]) -> OptimizerParameters:
    """The parameters of an `optimizer:` block  (:41-57)."""
    return create_parameters_from_configuration_dictionary(configuration=optimizer_configuration_dictionary, identifier="name",
                                                           options=OPTIMIZER_PARAMETERS_BY_NAME)


class FusedAdam(optim.Adam):
    """torch's Adam / AdamW (amsgrad off, maximize off) whose step() is mdx_adam_step: one launch per parameter group updates
    every float32 device parameter that has a gradient, in binary64 from the binary32 operands, each result rounded once.

    Attributes a trainer sets:
      gradient_clip_val = 0.0   > 0: clip by the group's global gradient norm as torch's clip_grad_norm_ does, inside the step
                                (two more launches for the norm).  `.grad` is NOT rewritten with the clipped values, whereas
                                clip_grad_norm_ scales it in place: after a step `.grad` is untouched, or all zeros with
                                zero_gradients.
      gradient_scale = 1.0      a factor on every gradient (an accumulated sum's 1 / number of batches)
      zero_gradients = False    the step stores +0.0 over each gradient it has consumed: the zero_grad pass, at stable addresses
      last_gradient_norm        f64 [2] on the device after a clipped step (the norm and its square), else None; no host read
      status                    int32 [1] on the device: STATUS_OPTIMIZER_NONFINITE after a gradient that is not finite

    With several parameter groups the norm, and so the clipping, is per group.  The step counters (one per chunk of
    kernels.ADAM_CHUNK_ELEMENTS elements of a parameter), learning rate and the other hyper-parameters live in device memory,
    so a captured step() follows a scheduler: step() compares each group's host values with what it last wrote and refreshes
    the buffer by one tiny launch when they differ -- which must happen outside a stream capture (prepare()), and raises
    inside one.  state_dict() / load_state_dict() use
    torch's layout (`step` a 0-dim float32 tensor per parameter, `exp_avg`, `exp_avg_sq`, torch's param_groups keys), so a
    Lightning checkpoint's optimizer_states[0] loads here and this class's state loads into torch.optim.Adam / AdamW."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *, decoupled_weight_decay=False):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                         foreach=False, capturable=False, differentiable=False, fused=False,
                         decoupled_weight_decay=decoupled_weight_decay)
        self.gradient_clip_val = 0.0
        self.gradient_scale = 1.0
        self.zero_gradients = False
        self.last_gradient_norm = None
        self.status = None
        self._device_state = {}         # group index -> the group's device buffers, what was last written and the last plan

    def _group_state(self, index, group):
        held = self._device_state.get(index)
        if held is None or len(held["slots"]) != len(group["params"]):
            device = next(p.device for p in group["params"])
            # one counter per chunk of every parameter, and a last entry that stays 0 for the parameters without elements
            slots, total = kernels.adam_counter_slots([p.numel() for p in group["params"]])
            first = [slot if p.numel() else total for slot, p in zip(slots, group["params"])]
            held = dict(steps=torch.zeros(total + 1, dtype=torch.int32, device=device), slots=slots,
                        first=torch.tensor(first, dtype=torch.int64, device=device),
                        hyper=torch.zeros(kernels._hip.ADAM_HYPER_COUNT, dtype=torch.float64, device=device), written=None,
                        seen=None, plan=None)
            self._device_state[index] = held
            if self.status is None:
                self.status = torch.zeros(1, dtype=torch.int32, device=device)
        return held

    def _refresh_hyper(self, held, group):
        for refused in ("amsgrad", "maximize"):
            if group.get(refused):
                raise ValueError(f"FusedAdam does not serve {refused}=True")
        values = (float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                  float(group["weight_decay"]), float(self.gradient_clip_val), float(self.gradient_scale))
        if values != held["written"]:
            kernels._device_only("the optimizer step", hyper=held["hyper"])
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("a hyper-parameter of FusedAdam changed inside a stream capture: its refresh launch belongs "
                                   "outside the captured region (call optimizer.prepare() before capturing, and after changing one)")
            kernels.adam_hyper_fill(held["hyper"], *values)
            held["written"] = values

    def _plan(self, index, group, held):
        """The tables of the group's parameters that have a gradient now, their state made.  The addresses of the parameters
        and gradients are compared with the last call's: unchanged, the plan is the last one (the moments are this
        optimizer's own and change only through load_state_dict, which starts afresh)."""
        seen = [(p.data_ptr(), 0 if p.grad is None else p.grad.data_ptr()) for p in group["params"]]
        if seen == held["seen"]:
            return held["plan"]
        served, slots = [], []
        for slot, p in zip(held["slots"], group["params"]):
            if p.grad is None:
                continue
            if p.grad.is_sparse:
                raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
            state = self.state[p]
            if "exp_avg" not in state:
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            served.append(p)
            slots.append(slot)
        names = [f"param_groups[{index}]['params'][{k}]" for k, p in enumerate(group["params"]) if p.grad is not None]
        plan = kernels.adam_plan(served, [p.grad for p in served], [self.state[p]["exp_avg"] for p in served],
                                 [self.state[p]["exp_avg_sq"] for p in served], slots, names=names) if served else None
        held["seen"], held["plan"] = seen, plan
        return plan

    @torch.no_grad()
    def prepare(self):
        """Everything of a step but its launches: the state of every parameter that has a gradient, the tables uploaded, the
        hyper-parameters written where they differ from what was last written.  What a caller runs once before capturing step()
        into a graph (with static gradient buffers) -- the captured step then allocates nothing, uploads nothing and is the
        step's launches alone -- and again, outside the captured region, after a scheduler or the caller changed a
        hyper-parameter: then it is the one fill launch."""
        for index, group in enumerate(self.param_groups):
            if group["params"]:
                held = self._group_state(index, group)
                self._refresh_hyper(held, group)
                self._plan(index, group, held)

    @torch.no_grad()
    def step(self, closure=None):
        """One step of every group: per group one mdx_adam_step launch, after the two of mdx_gradient_norm with
        gradient_clip_val > 0 (the norm is then per group: torch's clip_grad_norm_ over one group's parameters)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.last_gradient_norm = None
        for index, group in enumerate(self.param_groups):
            if not group["params"]:
                continue
            held = self._group_state(index, group)
            self._refresh_hyper(held, group)
            plan = self._plan(index, group, held)
            if plan is None:
                continue
            norm = kernels.adam_step(plan, held["steps"], held["hyper"],
                                     decoupled_weight_decay=bool(group.get("decoupled_weight_decay", False)),
                                     zero_gradients=self.zero_gradients, clip=self.gradient_clip_val > 0.0, status=self.status)
            if norm is not None:
                self.last_gradient_norm = norm
        return loss

    def steps_taken(self) -> list:
        """Per group, a device int32 tensor of the steps each parameter has taken (no host read); 0 for one without elements."""
        return [held["steps"][held["first"]] for held in
                (self._group_state(index, group) for index, group in enumerate(self.param_groups) if group["params"])]

    def state_dict(self):
        """torch's layout: each parameter with state gets `step`, a 0-dim float32 tensor made from the device counter."""
        for index, group in enumerate(self.param_groups):
            if not group["params"]:
                continue
            held = self._device_state.get(index)
            steps = None if held is None else held["steps"][held["first"]].to(torch.float32)
            for k, p in enumerate(group["params"]):
                if "exp_avg" in self.state.get(p, {}):
                    self.state[p]["step"] = steps[k].clone()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        # a torch that kept AdamW as a class of its own wrote no `decoupled_weight_decay` key: this optimizer's own flag stays
        own_flags = [bool(group.get("decoupled_weight_decay", False)) for group in self.param_groups]
        super().load_state_dict(state_dict)
        self._device_state = {}
        for index, group in enumerate(self.param_groups):
            if "decoupled_weight_decay" not in state_dict["param_groups"][index]:
                group["decoupled_weight_decay"] = own_flags[index]
            if not group["params"]:
                continue
            held = self._group_state(index, group)
            for k, p in enumerate(group["params"]):
                state = self.state.get(p, {})
                if "step" in state and p.numel():
                    chunks = -(-p.numel() // kernels.ADAM_CHUNK_ELEMENTS)
                    step = torch.as_tensor(state["step"]).to(device=held["steps"].device).to(torch.int32)
                    held["steps"][held["slots"][k]:held["slots"][k] + chunks] = step
                for name in ("exp_avg", "exp_avg_sq"):
                    if name in state:
                        state[name] = state[name].to(device=p.device, dtype=torch.float32).contiguous()


def _fused_step_serves(model: torch.nn.Module) -> bool:
    parameters = list(model.parameters())
    return bool(parameters) and all(p.is_cuda and p.dtype == torch.float32 for p in parameters)


def load_optimizer(optimizer_parameters: OptimizerParameters, model: torch.nn.Module) -> optim.Optimizer:
    """The optimizer of `model`  (:60-82): torch's Adam / AdamW with the reference's arguments for host parameters or a dtype
    other than float32; FusedAdam -- the same class with the same defaults, step() on the fused kernel -- for float32 device
    parameters."""
    assert optimizer_parameters.name in OPTIMIZERS_BY_NAME.keys(), f"Optimizer '{optimizer_parameters.name}' is not defined."
    optimizer_class = OPTIMIZERS_BY_NAME[optimizer_parameters.name]

    # Adapt the input configurations to the optimizer constructor expectations.
    parameters_dict = asdict(optimizer_parameters)
    parameters_dict.pop("name")
    parameters_dict["lr"] = parameters_dict.pop("learning_rate")

    if _fused_step_serves(model):
        # torch.optim.AdamW's own defaults differ from Adam's in weight_decay alone (1e-2), which the reference always passes
        return FusedAdam(model.parameters(), decoupled_weight_decay=optimizer_class is optim.AdamW, **parameters_dict)
    return optimizer_class(model.parameters(), **parameters_dict)
