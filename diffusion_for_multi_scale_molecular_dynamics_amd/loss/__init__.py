"""The loss calculators' factory (src/.../loss/__init__.py:7-41) and `denoising_loss`, the loss of a score network on a noised
batch: what the reference's AXLDiffusionLightningModel._generic_step (models/axl_diffusion_lightning_model.py:186-381) returns
for a test or validation batch, made by ONE launch of the fused loss kernel after the network's forward; and `training_loss`,
what its training_step optimises: the same with the gradient from the same launch, plus the weighted regularizer loss; and the
driver around it, `configure_optimizers` and `optimisation_step`: what Lightning does around training_step with the reference's
`optimizer:` / `scheduler:` blocks and the trainer's gradient_clipping and accumulate_grad_batches; and
`FusedMlpTrainingStep`, the same step of an MLPScoreNetwork without autograd, on the fused training kernels."""
from typing import Any, Dict, Optional

import torch

from .. import kernels
from ..namespace import (ATOM_TYPES, AXL, AXL_COMPOSITION, CARTESIAN_FORCES, LATTICE_PARAMETERS, NOISE, NOISY_ATOM_TYPES,
                         NOISY_AXL_COMPOSITION, NOISY_LATTICE_PARAMETERS, NOISY_RELATIVE_COORDINATES, Q_BAR_MATRICES,
                         Q_BAR_TM1_MATRICES, Q_MATRICES, RELATIVE_COORDINATES, TIME, TIME_INDICES)
from .atom_type_loss_calculator import D3PMLossCalculator
from .coordinates_loss_calculator import MSELossCalculator, WeightedMSELossCalculator
from .loss_parameters import create_loss_parameters
from ..models.optimizer import FusedAdam, create_optimizer_parameters, load_optimizer
from ..models.scheduler import create_scheduler_parameters, load_scheduler_dictionary

LOSS_BY_ALGO = dict(mse=MSELossCalculator, weighted_mse=WeightedMSELossCalculator)


def create_loss_calculator(loss_parameters: AXL) -> AXL:
    """The calculators of the atom types, coordinates and lattice parameters in an AXL  (:10-41)."""
    coordinates_algorithm = loss_parameters.X.algorithm
    assert coordinates_algorithm in LOSS_BY_ALGO.keys(), \
        f"Algorithm {coordinates_algorithm} is not implemented. Possible choices are {LOSS_BY_ALGO.keys()}"
    lattice_algorithm = loss_parameters.L.algorithm
    assert lattice_algorithm in LOSS_BY_ALGO.keys(), \
        f"Algorithm {lattice_algorithm} is not implemented. Possible choices are {LOSS_BY_ALGO.keys()}"
    return AXL(A=D3PMLossCalculator(loss_parameters.A), X=LOSS_BY_ALGO[coordinates_algorithm](loss_parameters.X),
               L=LOSS_BY_ALGO[lattice_algorithm](loss_parameters.L))


def _per_structure_rows(matrices: torch.Tensor) -> torch.Tensor:
    """[batch, classes, classes] of a noised batch's [batch, atoms, classes, classes] matrices: the rows NoisingTransform's
    expand() views share (no copy), else the first atom's -- the matrices are the same for all atoms of a structure
    (data/diffusion/noising_transform.py:160-162)."""
    return matrices if matrices.dim() == 3 else matrices[:, 0].contiguous()


def _weighted_scalars(prefix: str, parameters) -> dict:
    if parameters.algorithm not in LOSS_BY_ALGO:
        raise AssertionError(f"Algorithm {parameters.algorithm} is not implemented. Possible choices are {LOSS_BY_ALGO.keys()}")
    scalars = {prefix + "algorithm": parameters.algorithm}
    if parameters.algorithm == "weighted_mse":       # 0-dim float32 buffers in the reference: their binary32 values
        scalars[prefix + "sigma0"] = kernels.binary32(parameters.sigma0)
        scalars[prefix + "exponent"] = kernels.binary32(parameters.exponent)
    return scalars


_STATUS = {}


def _status_word(device: torch.device) -> torch.Tensor:
    if device not in _STATUS:
        _STATUS[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return _STATUS[device]


def denoising_loss(axl_network, noised_batch: Dict[str, Any], loss_parameters: Optional[AXL] = None, kmax_target_score: int = 4,
                   conditional: Optional[bool] = None, differentiable: bool = False) -> dict:
    """The denoising loss of `axl_network` on a batch NoisingTransform noised (device tensors only).

    Returns _generic_step's dictionary: `unreduced_loss` (AXL of [B, N, C], [B, N, D], [B, P]), `loss` (0-dim), `sigmas`
    [B, N, D], `model_predictions` (AXL), `target_coordinates_normalized_conditional_scores`,
    `target_lattice_normalized_conditional_scores`, AXL_COMPOSITION, NOISY_AXL_COMPOSITION and TIME; and beside them
    `per_structure_loss` [B], the weighted aggregate of every structure (`loss` is its mean), and `status`, the device word
    the kernel reports the reference's value assertions into: nothing here reads it; kernels.raise_loss_status(status) does.
    The weights are the three lambda_weight of `loss_parameters` (default: create_loss_parameters({})).  `conditional` goes to
    the network's forward as it is.

    `differentiable`: the predictions are not detached before the loss, the launch is mdx_denoising_loss_gradient (the same
    kernel body, writing d loss / d prediction beside the loss) and `loss` is its binary64 total over the batch divided by B,
    with a grad_fn whose backward hands the three gradient buffers to the network's autograd graph -- the loss the reference's
    training_step optimises.  `model_predictions` and `unreduced_loss` stay detached, as in the reference (:343-352);
    `prediction_gradients` (AXL) holds the kernel's three buffers, d loss / d prediction."""
    return _denoising_step(axl_network, noised_batch, loss_parameters, kmax_target_score, conditional, differentiable)[0]


def _loss_arguments(noised_batch, predictions: AXL, parameters: AXL, kmax_target_score: int, status) -> dict:
    """The keyword arguments of kernels.denoising_loss / denoising_loss_and_gradient for a noised batch and a network's
    predictions on it."""
    a0, x0, l0 = noised_batch[ATOM_TYPES], noised_batch[RELATIVE_COORDINATES], noised_batch[LATTICE_PARAMETERS]
    at, xt, lt = noised_batch[NOISY_ATOM_TYPES], noised_batch[NOISY_RELATIVE_COORDINATES], noised_batch[NOISY_LATTICE_PARAMETERS]
    noise, time_indices = noised_batch[NOISE], noised_batch[TIME_INDICES]
    tables = [noised_batch[key] for key in (Q_MATRICES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES)]
    B, N, _ = x0.shape
    # sigma_n = sigma / N^(1/P) inside the kernel: the reference scales by the number of lattice parameters here
    # (models/axl_diffusion_lightning_model.py:275-277), not by the spatial dimension
    return dict(
        x0=x0.contiguous(), xt=xt.contiguous(), predicted_x=predictions.X.contiguous(), sigma=noise.reshape(B).contiguous(),
        a0=a0.contiguous(), at=at.contiguous(), logits=predictions.A.contiguous(), time_indices=time_indices.contiguous(),
        q_matrices=_per_structure_rows(tables[0]), q_bar_matrices=_per_structure_rows(tables[1]),
        q_bar_tm1_matrices=_per_structure_rows(tables[2]), tables_per_structure=True,
        l0=l0.contiguous(), lt=lt.contiguous(), predicted_l=predictions.L.contiguous(),
        sigma_n_divisor=kernels.root_of_atom_count(N, l0.shape[-1]), kmax=kmax_target_score,
        **_weighted_scalars("x_", parameters.X), **_weighted_scalars("l_", parameters.L), ce_weight=parameters.A.ce_weight,
        eps=parameters.A.eps, lambda_weights=(parameters.A.lambda_weight, parameters.X.lambda_weight, parameters.L.lambda_weight),
        status=status)


def _denoising_step(axl_network, noised_batch, loss_parameters, kmax_target_score, conditional, differentiable):
    """denoising_loss's dictionary, and the augmented batch the network saw (what a regularizer is given)."""
    parameters = create_loss_parameters({}) if loss_parameters is None else loss_parameters
    a0, x0, l0 = noised_batch[ATOM_TYPES], noised_batch[RELATIVE_COORDINATES], noised_batch[LATTICE_PARAMETERS]
    at, xt, lt = noised_batch[NOISY_ATOM_TYPES], noised_batch[NOISY_RELATIVE_COORDINATES], noised_batch[NOISY_LATTICE_PARAMETERS]
    noise, time_indices = noised_batch[NOISE], noised_batch[TIME_INDICES]
    tables = [noised_batch[key] for key in (Q_MATRICES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES)]
    kernels._device_only("the denoising loss", atom_types=a0, relative_coordinates=x0, lattice_parameters=l0, noisy_atom_types=at,
                         noisy_relative_coordinates=xt, noisy_lattice_parameters=lt, noise_parameter=noise,
                         time_indices=time_indices, q_matrices=tables[0], q_bar_matrices=tables[1], q_bar_tm1_matrices=tables[2])
    composition, noisy_composition = AXL(A=a0, X=x0, L=l0), AXL(A=at, X=xt, L=lt)
    B, N, D = x0.shape
    forces = noised_batch[CARTESIAN_FORCES] if CARTESIAN_FORCES in noised_batch else torch.zeros_like(x0)
    augmented_batch = {NOISY_AXL_COMPOSITION: noisy_composition, TIME: noised_batch[TIME], NOISE: noise, CARTESIAN_FORCES: forces}
    predictions = axl_network(augmented_batch, conditional=conditional)
    attached = predictions
    predictions = AXL(A=predictions.A.detach(), X=predictions.X.detach(), L=predictions.L.detach())
    status = _status_word(x0.device)
    launch, given = (kernels.denoising_loss_and_gradient, attached) if differentiable else (kernels.denoising_loss, predictions)
    out = launch(**_loss_arguments(noised_batch, given, parameters, kmax_target_score, status))
    per_structure_loss = out.per_structure[:, 3]
    output = dict(unreduced_loss=AXL(A=out.loss_a, X=out.loss_x, L=out.loss_l),
                  loss=out.loss if differentiable else per_structure_loss.mean(dtype=torch.float64).to(torch.float32),
                  sigmas=noise.reshape(B, 1, 1).expand(B, N, D), model_predictions=predictions,
                  target_coordinates_normalized_conditional_scores=out.target_x,
                  target_lattice_normalized_conditional_scores=out.target_l, per_structure_loss=per_structure_loss, status=status)
    if differentiable:
        output["prediction_gradients"] = AXL(A=out.gradient_a, X=out.gradient_x, L=out.gradient_l)
    output[AXL_COMPOSITION] = composition
    output[NOISY_AXL_COMPOSITION] = noisy_composition
    output[TIME] = augmented_batch[TIME]
    return output, augmented_batch


def training_loss(axl_network, noised_batch: Dict[str, Any], loss_parameters: Optional[AXL] = None, regularizer=None,
                  current_epoch: int = 0, kmax_target_score: int = 4, conditional: Optional[bool] = None) -> dict:
    """The loss the reference's training_step optimises (models/axl_diffusion_lightning_model.py:363-375, :447): the
    differentiable denoising_loss, and -- with a `regularizer` whose can_regularizer_run() holds -- its weighted loss on the
    same augmented batch added to `loss` and kept under `regularizer_loss`.  `loss.backward()` runs through both."""
    output, augmented_batch = _denoising_step(axl_network, noised_batch, loss_parameters, kmax_target_score, conditional, True)
    if regularizer and regularizer.can_regularizer_run():
        weighted_regularizer_loss = regularizer.compute_weighted_regularizer_loss(
            score_network=axl_network, augmented_batch=augmented_batch, current_epoch=current_epoch)
        output["loss"] = output["loss"] + weighted_regularizer_loss
        output["regularizer_loss"] = weighted_regularizer_loss
    return output


def configure_optimizers(hyper_params, axl_network) -> dict:
    """dict(optimizer=..., [lr_scheduler=..., monitor=...]) as the reference's Lightning model returns it
    (models/axl_diffusion_lightning_model.py:147-167).  `hyper_params`: an object with `optimizer_parameters` and
    `scheduler_parameters` (the reference's AXLDiffusionParameters, also as a checkpoint's pickle gives them), or a configuration
    dictionary with an `optimizer` block and, optionally, a `scheduler` block."""
    if isinstance(hyper_params, dict):
        optimizer_parameters = create_optimizer_parameters(dict(hyper_params["optimizer"]))
        scheduler_parameters = create_scheduler_parameters(hyper_params)
    else:
        optimizer_parameters = hyper_params.optimizer_parameters
        scheduler_parameters = getattr(hyper_params, "scheduler_parameters", None)
    optimizer = load_optimizer(optimizer_parameters, axl_network)
    output = dict(optimizer=optimizer)
    if scheduler_parameters is not None:
        output.update(load_scheduler_dictionary(scheduler_parameters=scheduler_parameters, optimizer=optimizer))
    return output


def optimisation_step(axl_network, noised_batch: Dict[str, Any], optimizer, loss_parameters: Optional[AXL] = None, regularizer=None,
                      current_epoch: int = 0, batch_index: int = 0, gradient_clipping: float = 0.0,
                      accumulate_grad_batches: int = 1, kmax_target_score: int = 4, conditional: Optional[bool] = None) -> dict:
    """What Lightning does around the reference's training_step for one batch: training_loss, the backward of
    loss / accumulate_grad_batches, and -- on every accumulate_grad_batches-th batch (by `batch_index`) -- the optimizer's step
    with the gradients clipped at the global norm `gradient_clipping` (0: off, as in train_diffusion.py:192), then gradients of
    zero.  Returns training_loss's dictionary, with `gradient_norm` (0-dim, device) when a norm was computed.

    With a FusedAdam the step, the clipping and the zeroing are its launches (the clipped values are used, `.grad` is never
    rewritten with them); any other optimizer gets torch's clip_grad_norm_, step() and zero_grad(set_to_none=False).  Nothing
    is read from the device.  The epoch loop and the data modules around it are training.fit's; logging and checkpoint writing
    are the caller's."""
    if accumulate_grad_batches < 1:
        raise ValueError(f"accumulate_grad_batches is {accumulate_grad_batches}: it counts batches, so at least 1")
    output = training_loss(axl_network, noised_batch, loss_parameters, regularizer, current_epoch, kmax_target_score, conditional)
    (output["loss"] / accumulate_grad_batches).backward()
    if (batch_index + 1) % accumulate_grad_batches != 0:
        return output
    if isinstance(optimizer, FusedAdam):
        optimizer.gradient_clip_val, optimizer.zero_gradients = float(gradient_clipping), True
        optimizer.step()
        if optimizer.last_gradient_norm is not None:
            output["gradient_norm"] = optimizer.last_gradient_norm[0].clone()
    else:
        if gradient_clipping > 0.0:
            parameters = [p for group in optimizer.param_groups for p in group["params"]]
            output["gradient_norm"] = torch.nn.utils.clip_grad_norm_(parameters, gradient_clipping)
        optimizer.step()
        optimizer.zero_grad(set_to_none=False)
    return output


_STEP_BATCH_KEYS = (ATOM_TYPES, RELATIVE_COORDINATES, LATTICE_PARAMETERS, NOISY_ATOM_TYPES, NOISY_RELATIVE_COORDINATES,
                    NOISY_LATTICE_PARAMETERS, NOISE, TIME, TIME_INDICES, Q_MATRICES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES)


class FusedMlpTrainingStep:
    """One whole optimisation step of an MLPScoreNetwork without autograd -- what optimisation_step does with
    accumulate_grad_batches = 1 and no regularizer, as five calls:
      1. kernels.mlp_train_forward on the module's own parameters (raw outputs and the activation record),
      2. the MASK class of the logits filled with -inf,
      3. kernels.denoising_loss_and_gradient, whose three gradient buffers are used as they are,
      4. kernels.mlp_train_backward into a flat gradient buffer this object keeps (the parameters' .grad are its views),
      5. the FusedAdam's step, whose tables name those views; with `gradient_clipping` > 0 its norm launches before it.

    step(noised_batch) runs them eagerly.  step(noised_batch, captured=True) copies the batch into device buffers kept here and
    replays ONE hipGraph of those launches on one stream (captured at the first call, again when the batch's shapes change);
    the optimizer's hyper-parameter fill stays outside the graph (FusedAdam.prepare before every replay: a launch only when a
    value changed), so a scheduler's learning rate is followed.  Nothing is read from the device.  Both return a dictionary with
    `loss` (0-dim, device) and, when clipping, `gradient_norm` (0-dim f64, device); the captured step's are the graph's own
    tensors, which the next replay overwrites.

    Refused at construction, with the reason: a network the kernels do not cover (permutation symmetrisation, time prefactor,
    too many hidden layers or classes), a network with conditional_prob > 0 (the fused forward is unconditional), host
    parameters, an optimizer that is not a FusedAdam or does not hold the network's parameters."""

    def __init__(self, network, optimizer: FusedAdam, loss_parameters: Optional[AXL] = None, gradient_clipping: float = 0.0,
                 kmax_target_score: int = 4):
        reason = kernels.mlp_train_refusal(network)
        if reason:
            raise kernels._hip.MdxError(reason)
        if network.conditional_prob > 0:
            raise kernels._hip.MdxError(f"the fused MLP training step is unconditional: the network's conditional_prob is "
                                        f"{network.conditional_prob}, so some of its forwards would be conditional")
        if not isinstance(optimizer, FusedAdam):
            raise TypeError(f"FusedMlpTrainingStep steps through FusedAdam's launches, got {type(optimizer).__name__}")
        self.network, self.optimizer = network, optimizer
        self.loss_parameters = create_loss_parameters({}) if loss_parameters is None else loss_parameters
        self.gradient_clipping, self.kmax_target_score = float(gradient_clipping), int(kmax_target_score)
        plan = kernels.mlp_train_plan(network)
        held = {id(p) for group in optimizer.param_groups for p in group["params"]}
        missing = [name for name, p in zip(plan.names, plan.parameters) if id(p) not in held]
        if missing:
            raise ValueError(f"the optimizer does not hold the network's parameters {missing}")
        self.flat = torch.zeros(plan.parameter_count, dtype=torch.float32, device=plan.device)
        self.workspace = None
        self._graph, self._graph_key, self._static, self._graph_out = None, None, None, None

    def _prepare(self, batch_size: int):
        """Everything of a step that is not a launch of the five calls: the plan, the workspace, the parameters' .grad bound to
        the flat buffer, the optimizer's state, tables and hyper-parameters."""
        plan = kernels.mlp_train_plan(self.network)
        needed = plan.workspace_doubles(batch_size)
        if self.workspace is None or self.workspace.numel() < needed:
            self.workspace = torch.empty(max(needed, 1), dtype=torch.float64, device=plan.device)
        for p, view in zip(plan.parameters, plan.views(self.flat)):
            if p.grad is None or p.grad.data_ptr() != view.data_ptr():
                p.grad = view
        self.optimizer.gradient_clip_val, self.optimizer.zero_gradients = self.gradient_clipping, False
        self.optimizer.prepare()
        return plan

    def _launches(self, plan, batch, flat=None) -> dict:
        """The five calls; with `flat` (a scratch gradient buffer) the first four alone: nothing of the network or the optimizer
        changes (what runs once, eagerly, before a capture, so that the capture meets no kernel for the first time)."""
        forward = kernels.mlp_train_forward(plan, batch[NOISY_ATOM_TYPES], batch[NOISY_RELATIVE_COORDINATES],
                                            batch[NOISY_LATTICE_PARAMETERS], batch[TIME], batch[NOISE])
        forward.logits[..., plan.num_classes - 1] = -torch.inf
        out = kernels.denoising_loss_and_gradient(**_loss_arguments(
            batch, AXL(A=forward.logits, X=forward.score_x, L=forward.score_l), self.loss_parameters, self.kmax_target_score,
            _status_word(plan.device)))
        kernels.mlp_train_backward(plan, forward.record, out.gradient_a, out.gradient_x, out.gradient_l,
                                   out=self.flat if flat is None else flat, workspace=self.workspace)
        if flat is not None:
            return dict(loss=out.loss)
        self.optimizer.step()
        output = dict(loss=out.loss)
        if self.optimizer.last_gradient_norm is not None:
            output["gradient_norm"] = self.optimizer.last_gradient_norm[0]
        return output

    def step(self, noised_batch: Dict[str, Any], captured: bool = False) -> dict:
        batch = {key: noised_batch[key] for key in _STEP_BATCH_KEYS}
        kernels._device_only("the fused MLP training step", **batch)
        batch[NOISY_ATOM_TYPES] = batch[NOISY_ATOM_TYPES].long()
        for key in (Q_MATRICES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES):
            batch[key] = _per_structure_rows(batch[key])
        batch = {key: t.contiguous() for key, t in batch.items()}
        plan = self._prepare(batch[RELATIVE_COORDINATES].shape[0])
        _status_word(plan.device)
        if not captured:
            return self._launches(plan, batch)
        key = (plan.key,) + tuple((name, tuple(t.shape), t.dtype) for name, t in batch.items())
        if self._graph_key != key:
            self._static = {name: t.clone() for name, t in batch.items()}
            self._launches(plan, self._static, flat=torch.empty_like(self.flat))
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._graph_out = self._launches(plan, self._static)
            self._graph_key = key
        else:
            for name, t in batch.items():
                self._static[name].copy_(t)
        self._graph.replay()
        return dict(self._graph_out)
