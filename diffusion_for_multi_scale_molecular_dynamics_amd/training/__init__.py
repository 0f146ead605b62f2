"""Training on the device: a dataset that lives in HBM, its batches gathered and noised by ONE launch each
(mdx_noise_training_batch), and `fit`, the epoch loop around the optimisation steps of `loss`.

What the reference spreads over its Lightning data modules (data/diffusion/gaussian_data_module.py:26-187, the collate-time
NoisingTransform of lammps_for_diffusion_data_module.py), its Lightning model's training / validation steps
(models/axl_diffusion_lightning_model.py:383-470) and the Lightning trainer of train_diffusion.py:

  BatchNoiser                  NoisingTransform.transform for rows of a device-resident dataset: one launch, no host read
  GaussianDataModuleParameters, GaussianDataModule
                               the reference's Gaussian data source; the raw datasets are the reference's (a CPU generator seeded
                               with random_seed), moved to the device once
  DeviceDataModule             the same service for clean tensors the caller brings
  fit                          epochs of training batches, validation and the scheduler; ONE hipGraph per full batch where
                               FusedMlpTrainingStep serves the network, loss.optimisation_step otherwise

Not here: checkpoint writing, loggers, callbacks and early stopping; sampling and metrics at the end of validation;
optimal-transport noising; the LAMMPS / parquet reader; the order of torch's DataLoader sampler (the shuffle is torch.randperm on
a device generator seeded by the seed and the epoch).
"""
import warnings
from dataclasses import dataclass
from typing import Any, Dict, Iterator, List, Optional

import torch

from .. import kernels, loss
from .._hip import MdxError, Rng
from ..data.diffusion.noising_transform import NoisingTransform
from ..data.element_types import ElementTypes
from ..models.optimizer import FusedAdam
from ..models.score_networks.mlp_score_network import MLPScoreNetwork
from ..namespace import (ATOM_TYPES, CARTESIAN_FORCES, LATTICE_PARAMETERS, NOISE, NOISY_ATOM_TYPES, NOISY_LATTICE_PARAMETERS,
                         NOISY_RELATIVE_COORDINATES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES, Q_MATRICES, RELATIVE_COORDINATES, TIME,
                         TIME_INDICES)
from ..noise_schedulers.noise_parameters import NoiseParameters
from ..noise_schedulers.noise_scheduler import NoiseScheduler

TRAIN_DRAW, VALID_DRAW = 0, 1          # the Philox draw ids of the two datasets: their rows share no stream


def noised_batch_dictionary(buffers: kernels.NoisedTrainingBatch, forces: torch.Tensor) -> Dict[str, torch.Tensor]:
    """NoisingTransform.transform's dictionary over the kernel's buffers: views, no copy.  The three matrices are expand() views
    [B, N, C, C] of the per-structure rows [B, C, C]."""
    B, N = buffers.a0.shape
    expand = lambda rows: rows.unsqueeze(1).expand(B, N, -1, -1)      # noqa: E731
    return {RELATIVE_COORDINATES: buffers.x0, ATOM_TYPES: buffers.a0, LATTICE_PARAMETERS: buffers.l0, CARTESIAN_FORCES: forces,
            TIME: buffers.time.reshape(-1, 1), TIME_INDICES: buffers.time_indices, NOISE: buffers.sigma.reshape(-1, 1),
            Q_MATRICES: expand(buffers.q), Q_BAR_MATRICES: expand(buffers.q_bar), Q_BAR_TM1_MATRICES: expand(buffers.q_bar_tm1),
            NOISY_ATOM_TYPES: buffers.at, NOISY_RELATIVE_COORDINATES: buffers.xt, NOISY_LATTICE_PARAMETERS: buffers.lt}


class BatchNoiser:
    """NoisingTransform.transform (data/diffusion/noising_transform.py:82-200) for rows of a dataset that lives on the device.

    The time index and the three noises of a row are Philox draws keyed by (seed, epoch, the row): they do not depend on the
    batch the row sits in, and the same `epoch` gives the same noise again."""

    def __init__(self, noise_parameters: NoiseParameters, num_atom_types: int, spatial_dimension: int,
                 use_fixed_lattice_parameters: bool = False, seed: int = 0, device="cuda"):
        self.num_atom_types, self.spatial_dimension = num_atom_types, spatial_dimension
        self.use_fixed_lattice_parameters, self.seed = bool(use_fixed_lattice_parameters), int(seed)
        self.noise_scheduler = NoiseScheduler(noise_parameters, num_classes=num_atom_types + 1, device=device)
        self.device = self.noise_scheduler.tables.device
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.epoch_word = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._zeros = {}

    def rng(self, epoch, draw: int = TRAIN_DRAW) -> Rng:
        """The request of one launch; `epoch` an int, or None: the device word `epoch_word` (captured launches)."""
        if epoch is None:
            return Rng(self.seed & 0xFFFFFFFFFFFFFFFF, 0, 1, int(draw), 0, self.epoch_word.data_ptr())
        return Rng(self.seed & 0xFFFFFFFFFFFFFFFF, int(epoch), 1, int(draw), 0, None)

    def _forces(self, dataset, rows, cursor, row_offset, batch_size, like) -> torch.Tensor:
        if CARTESIAN_FORCES not in dataset:
            key = tuple(like.shape)
            if key not in self._zeros:
                self._zeros[key] = torch.zeros_like(like)
            return self._zeros[key]
        positions = torch.arange(batch_size, device=self.device) + row_offset
        if cursor is not None:
            positions = positions + cursor.to(torch.int64) * batch_size
        return dataset[CARTESIAN_FORCES].index_select(0, positions if rows is None else rows.index_select(0, positions))

    def noise(self, dataset: Dict[str, torch.Tensor], rows: Optional[torch.Tensor] = None, cursor: Optional[torch.Tensor] = None,
              batch_size: Optional[int] = None, epoch=0, out: Optional[kernels.NoisedTrainingBatch] = None, row_offset: int = 0,
              draw: int = TRAIN_DRAW) -> Dict[str, torch.Tensor]:
        """One batch of `dataset` (RELATIVE_COORDINATES [M, N, d], ATOM_TYPES [M, N], LATTICE_PARAMETERS [M, d(d+1)/2] on the
        device, CARTESIAN_FORCES optional), gathered and noised in one launch: rows[p] (None: p) for p = row_offset + cursor x
        batch_size + 0 .. batch_size - 1; `cursor` an int32 device word or None (0); batch_size None: every position.  Returns
        NoisingTransform.transform's dictionary, over `out`'s buffers when given.  CARTESIAN_FORCES: one kept buffer of zeros when
        the dataset has none (the data modules leave all-zero forces out), so the batch is the one launch; a dataset that does
        carry forces has them gathered beside it by torch (an arange, an add, one or two index_select).  Nothing is read from
        the device: kernels.raise_noising_status(noiser.status) reports an index out of range."""
        for key in (RELATIVE_COORDINATES, ATOM_TYPES, LATTICE_PARAMETERS):
            assert key in dataset, f"The field '{key}' is missing from the input."
        x0 = dataset[RELATIVE_COORDINATES]
        if batch_size is None:
            batch_size = (x0.shape[0] if rows is None else rows.numel()) - row_offset
        buffers = kernels.noise_training_batch(
            self.noise_scheduler.tables, x0, dataset[ATOM_TYPES], dataset[LATTICE_PARAMETERS], batch_size, rows=rows,
            row_offset=row_offset, cursor=cursor, rng=self.rng(epoch, draw),
            use_fixed_lattice_parameters=self.use_fixed_lattice_parameters, out=out, status=self.status)
        return noised_batch_dictionary(buffers, self._forces(dataset, rows, cursor, row_offset, batch_size, buffers.x0))


# ----------------------------------------------------------------------------------------------------------------
# data modules
# ----------------------------------------------------------------------------------------------------------------
@dataclass(kw_only=True)
class DataModuleParameters:
    """What every data module of a training configuration's `data:` block is told (the reference's
    data/diffusion/data_module_parameters.py).  The batch size comes either as `batch_size`, for both loaders, or as the pair
    `train_batch_size` / `valid_batch_size`; `num_workers` and `max_atom` are read from the block and serve no purpose here (the
    datasets live on the device, nothing is padded).  A subclass names its `data_source`."""

    data_source = None          # a plain class attribute, not a field: the concrete class sets it

    batch_size: Optional[int] = None
    train_batch_size: Optional[int] = None
    valid_batch_size: Optional[int] = None
    num_workers: int = 0
    max_atom: int = 64
    spatial_dimension: int = 3
    use_fixed_lattice_parameters: bool = False      # True: the lattice parameters pass through the noising unchanged
    elements: list[str]

    def __post_init__(self):
        if not self.use_fixed_lattice_parameters:
            warnings.warn("use_fixed_lattice_parameters is False: the lattice parameters are diffused too, which the reference "
                          "calls experimental and not fully tested")
        assert self.data_source is not None, "The data source must be set."
        both_loaders = self.batch_size is not None
        if not both_loaders:
            assert self.valid_batch_size is not None, "If batch_size is None, valid_batch_size must be specified."
            assert self.train_batch_size is not None, "If batch_size is None, train_batch_size must be specified."
        if both_loaders:
            assert self.valid_batch_size is None, "If batch_size is specified, valid_batch_size must be None."
            assert self.train_batch_size is None, "If batch_size is specified, train_batch_size must be None."


@dataclass(kw_only=True)
class GaussianDataModuleParameters(DataModuleParameters):
    """The `data:` block of `data_source: gaussian` (the reference's data/diffusion/gaussian_data_module.py): `number_of_atoms`
    atoms of one element in a unit box, atom n drawn from an isotropic Gaussian of width `sigma_d` around row n of
    `equilibrium_relative_coordinates` and wrapped into the cell; `train_dataset_size` + `valid_dataset_size` such structures
    from one host generator seeded with `random_seed`.  Like the reference's, this __post_init__ stands alone: the base
    class's checks are not run."""
    data_source = "gaussian"

    noise_parameters: NoiseParameters
    use_optimal_transport: bool          # True is refused when the module is built (GaussianDataModule)
    random_seed: int
    number_of_atoms: int
    sigma_d: float = 0.01
    equilibrium_relative_coordinates: List[List[float]]          # [number_of_atoms][spatial_dimension]
    train_dataset_size: int = 8_192
    valid_dataset_size: int = 1_024

    def __post_init__(self):
        assert self.sigma_d > 0.0, "the sigma_d parameter should be positive."
        assert len(self.equilibrium_relative_coordinates) == self.number_of_atoms, \
            "There should be exactly one list of equilibrium coordinates per atom."
        for x in self.equilibrium_relative_coordinates:
            assert len(x) == self.spatial_dimension, "The equilibrium coordinates should be consistent with the spatial dimension."
        assert len(self.elements) == 1, "There can only be one element type for the gaussian data module."


class DeviceDataModule:
    """Training and validation datasets of clean structures on the device, served as noised batches by a BatchNoiser.

    `train` and `valid`: dictionaries with RELATIVE_COORDINATES [M, N, d], ATOM_TYPES int64 [M, N] and LATTICE_PARAMETERS
    [M, d(d+1)/2] (CARTESIAN_FORCES optional); they are moved to `device` once.  Both are required.

    noise_once_at_setup (an attribute, not a configuration field; default True): every sample keeps its time index and its noise
    for the whole run, as the reference's Gaussian module noises its datasets in setup(); False draws fresh noise every epoch, as
    the reference's on-the-fly transform does.  Either way nothing noised is stored: the draws are functions of (seed, call, row),
    call = 0 or the epoch."""

    noise_once_at_setup = True

    def __init__(self, train: Optional[Dict[str, torch.Tensor]], valid: Optional[Dict[str, torch.Tensor]],
                 noise_parameters: NoiseParameters, num_atom_types: int, spatial_dimension: int, batch_size: int,
                 valid_batch_size: Optional[int] = None, use_fixed_lattice_parameters: bool = False, seed: int = 0, device="cuda"):
        assert batch_size, "batch_size must be specified"
        self.train_size, self.valid_size = int(batch_size), int(valid_batch_size or batch_size)
        self.seed = int(seed)
        self._noiser_arguments = (noise_parameters, num_atom_types, spatial_dimension, use_fixed_lattice_parameters, seed, device)
        self.device = torch.device(device)
        self.noiser = self.train_dataset = self.valid_dataset = None        # made when the datasets arrive (setup)
        self._permutation = self._generator = None
        if train is not None or valid is not None:
            self._take(train, valid)

    def _on_device(self, dataset):
        """The fields the noiser reads, moved once.  Forces that are all zero (one host read here, at setup) are left out: the
        noiser then hands every batch one kept buffer of zeros and gathers nothing beside its launch."""
        kept = {key: t.to(self.device).contiguous() for key, t in dataset.items()
                if key in (RELATIVE_COORDINATES, ATOM_TYPES, LATTICE_PARAMETERS, CARTESIAN_FORCES)}
        if CARTESIAN_FORCES in kept and not bool(kept[CARTESIAN_FORCES].any()):
            del kept[CARTESIAN_FORCES]
        return kept

    def _take(self, train, valid):
        if train is None or valid is None:
            raise ValueError("a data module serves a training AND a validation dataset (fit validates every epoch): got None")
        self.noiser = BatchNoiser(*self._noiser_arguments)
        self.device = self.noiser.device
        self.train_dataset, self.valid_dataset = self._on_device(train), self._on_device(valid)
        self._permutation = torch.empty(self.train_dataset[RELATIVE_COORDINATES].shape[0], dtype=torch.int64, device=self.device)
        self._generator = torch.Generator(device=self.device)

    def setup(self, stage: Optional[str] = None):
        """Nothing to make: the datasets came with the constructor."""

    def call_of_epoch(self, epoch: int) -> int:
        """The Philox call index of an epoch's noise."""
        return 0 if self.noise_once_at_setup else int(epoch)

    def shuffle(self, epoch: int) -> torch.Tensor:
        """The epoch's permutation of the training rows, written into the module's persistent device buffer."""
        self._generator.manual_seed((self.seed * 1_000_003 + int(epoch)) % 2**63)
        return torch.randperm(self._permutation.numel(), generator=self._generator, device=self.device, out=self._permutation)

    def _batches(self, dataset, rows, size, call, draw) -> Iterator[Dict[str, torch.Tensor]]:
        count = dataset[RELATIVE_COORDINATES].shape[0]
        for start in range(0, count, size):
            yield self.noiser.noise(dataset, rows=rows, row_offset=start, batch_size=min(size, count - start), epoch=call, draw=draw)

    def train_batches(self, epoch: int) -> Iterator[Dict[str, torch.Tensor]]:
        """The epoch's training batches: shuffled, the tail batch kept (drop_last=False)."""
        return self._batches(self.train_dataset, self.shuffle(epoch), self.train_size, self.call_of_epoch(epoch), TRAIN_DRAW)

    def valid_batches(self, epoch: int) -> Iterator[Dict[str, torch.Tensor]]:
        """The validation batches, in order."""
        return self._batches(self.valid_dataset, None, self.valid_size, self.call_of_epoch(epoch), VALID_DRAW)


class GaussianDataModule(DeviceDataModule):
    """Gaussian Data Module (data/diffusion/gaussian_data_module.py:66-187): an in-memory dataset of relative coordinates that
    follow a Gaussian distribution around equilibrium sites, one element, a unit box."""

    def __init__(self, hyper_params: GaussianDataModuleParameters, device="cuda"):
        p = hyper_params
        if p.use_optimal_transport:        # refused with NoisingTransform's reason
            NoisingTransform(p.noise_parameters, len(p.elements), p.spatial_dimension, use_optimal_transport=True, device=device)
        self.hyper_params = p
        self.element_types = ElementTypes(p.elements)
        self.sites = torch.tensor(p.equilibrium_relative_coordinates, dtype=torch.float32)          # [N, d], on the host
        super().__init__(None, None, p.noise_parameters, len(p.elements), p.spatial_dimension, p.batch_size or p.train_batch_size,
                         valid_batch_size=p.valid_batch_size, use_fixed_lattice_parameters=p.use_fixed_lattice_parameters,
                         seed=p.random_seed, device=device)

    def get_raw_dataset(self, batch_size: int, rng: torch.Generator):
        """`batch_size` clean structures as HOST tensors, drawn from `rng`: the one draw is torch.normal on [batch_size, N, d]
        tensors of means and widths, so a generator seeded like the reference's gives the reference's numbers
        (tests/golden/training/gaussian_raw.npz).  Keys: the three clean fields, zero CARTESIAN_FORCES, and the reference's
        `natom` and `potential_energy` columns."""
        p = self.hyper_params
        shape = (batch_size, p.number_of_atoms, p.spatial_dimension)
        drawn = torch.normal(mean=self.sites.expand(shape).contiguous(), std=torch.full(shape, p.sigma_d), generator=rng)
        wrapped = torch.remainder(drawn.to(torch.float32), 1.0)
        wrapped = torch.where(wrapped == 1.0, torch.zeros_like(wrapped), wrapped)       # remainder's 1.0 of a tiny negative number
        angles = p.spatial_dimension * (p.spatial_dimension - 1) // 2
        unit_box = torch.cat([torch.ones(batch_size, p.spatial_dimension), torch.zeros(batch_size, angles)], dim=1)
        return {RELATIVE_COORDINATES: wrapped, ATOM_TYPES: torch.zeros(shape[:2], dtype=torch.int64), LATTICE_PARAMETERS: unit_box,
                CARTESIAN_FORCES: torch.zeros(shape), "natom": torch.full((batch_size,), float(p.number_of_atoms)),
                "potential_energy": torch.zeros(batch_size)}

    def setup(self, stage: Optional[str] = None):
        """The two raw datasets from one CPU generator seeded with random_seed, training first, then moved to the device."""
        rng = torch.Generator()
        rng.manual_seed(self.hyper_params.random_seed)
        train = self.get_raw_dataset(self.hyper_params.train_dataset_size, rng)
        valid = self.get_raw_dataset(self.hyper_params.valid_dataset_size, rng)
        self._take(train, valid)


# ----------------------------------------------------------------------------------------------------------------
# the epoch loop
# ----------------------------------------------------------------------------------------------------------------
def captured_route_refusal(axl_network, optimizer, regularizer, accumulate_grad_batches: int) -> Optional[str]:
    """Why `fit` cannot run its captured route on these, or None."""
    if regularizer is not None:
        return "the captured route has no regularizer"
    if accumulate_grad_batches != 1:
        return "the captured route steps on every batch (accumulate_grad_batches = 1)"
    if not isinstance(optimizer, FusedAdam):
        return f"the captured route steps through FusedAdam's launches, got {type(optimizer).__name__}"
    if not isinstance(axl_network, MLPScoreNetwork):
        return f"the fused MLP training kernels evaluate an MLPScoreNetwork, not a {type(axl_network).__name__}"
    reason = kernels.mlp_train_refusal(axl_network)
    if reason:
        return reason
    if axl_network.conditional_prob > 0:
        return "the fused MLP training step is unconditional and the network's conditional_prob is positive"
    return None


class _CapturedEpoch:
    """The captured route's device state: ONE hipGraph = the noising launch (writing into the buffers the step reads), the five
    calls of FusedMlpTrainingStep, loss_sum += loss x batch and cursor += 1."""

    def __init__(self, step: loss.FusedMlpTrainingStep, data_module: DeviceDataModule):
        self.step, self.data, self.noiser = step, data_module, data_module.noiser
        device = data_module.device
        self.cursor = torch.zeros(1, dtype=torch.int32, device=device)
        self.loss_sum = torch.zeros(1, dtype=torch.float64, device=device)
        self.graph, self.full, self.tail = None, None, None

    def _buffers(self, count: int):
        x0 = self.data.train_dataset[RELATIVE_COORDINATES]
        buffers = kernels.noised_training_batch_buffers(count, x0.shape[1], x0.shape[2], self.noiser.num_atom_types + 1, x0.device)
        batch = noised_batch_dictionary(buffers, None)
        static = {key: loss._per_structure_rows(batch[key]) if key in (Q_MATRICES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES) else batch[key]
                  for key in loss._STEP_BATCH_KEYS}
        return buffers, static

    def launches(self, plan, buffers, static, count: int, row_offset: int, cursor, flat=None) -> dict:
        dataset = self.data.train_dataset
        kernels.noise_training_batch(self.noiser.noise_scheduler.tables, dataset[RELATIVE_COORDINATES], dataset[ATOM_TYPES],
                                     dataset[LATTICE_PARAMETERS], count, rows=self.data._permutation, row_offset=row_offset,
                                     cursor=cursor, rng=self.noiser.rng(None, TRAIN_DRAW),
                                     use_fixed_lattice_parameters=self.noiser.use_fixed_lattice_parameters, out=buffers,
                                     status=self.noiser.status)
        out = self.step._launches(plan, static, flat=flat)
        self.loss_sum.add_(out["loss"].to(torch.float64), alpha=float(count))
        if cursor is not None:
            cursor.add_(1)
        return out

    def run(self, epoch: int) -> torch.Tensor:
        """One epoch's training batches; returns the device sum of loss x batch size."""
        size, rows = self.data.train_size, self.data._permutation.numel()
        full, left = divmod(rows, size)
        self.data.shuffle(epoch)
        self.noiser.epoch_word.fill_(self.data.call_of_epoch(epoch))
        if full:
            plan = self.step._prepare(size)       # (the optimizer's hyper-parameter fill: outside the graph, once per epoch)
            if self.graph is None:
                # every launch of the graph once eagerly, on a scratch gradient buffer and without the optimizer's step: the
                # capture meets no kernel for the first time, and nothing of the network changes
                self.full = self._buffers(size)
                self.launches(plan, *self.full, size, 0, self.cursor, flat=torch.empty_like(self.step.flat))
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self.launches(plan, *self.full, size, 0, self.cursor)
        self.cursor.zero_()
        self.loss_sum.zero_()
        for _ in range(full):
            self.graph.replay()
        if left:
            plan = self.step._prepare(left)
            if self.tail is None:
                self.tail = self._buffers(left)
            self.launches(plan, *self.tail, left, full * size, None)
        return self.loss_sum


def _validation_sum(axl_network, data_module, loss_parameters, epoch: int) -> torch.Tensor:
    """Sum over the validation batches of loss x batch size, on the device: the reference's validation_step
    (models/axl_diffusion_lightning_model.py:449-470), unconditional, under no_grad and in eval mode."""
    total = torch.zeros(1, dtype=torch.float64, device=data_module.device)
    was_training = axl_network.training
    axl_network.eval()
    try:
        with torch.no_grad():
            for batch in data_module.valid_batches(epoch):
                out = loss.denoising_loss(axl_network, batch, loss_parameters, conditional=False)
                total.add_(out["loss"].to(torch.float64), alpha=float(batch[RELATIVE_COORDINATES].shape[0]))
    finally:
        axl_network.train(was_training)
    return total


class TrainingHistory(dict):
    """fit's result: a dictionary of three lists with one entry per epoch -- train_epoch_loss, validation_epoch_loss,
    learning_rate -- and, as attributes beside them, `optimizer` and `lr_scheduler` (None without one): the objects
    loss.configure_optimizers made, whose state a caller may want to keep."""

    def __init__(self, optimizer, lr_scheduler):
        super().__init__(train_epoch_loss=[], validation_epoch_loss=[], learning_rate=[])
        self.optimizer, self.lr_scheduler = optimizer, lr_scheduler


def fit(axl_network, data_module: DeviceDataModule, hyper_params: Any, max_epochs: int, loss_parameters=None, regularizer=None,
        gradient_clipping: float = 0.0, accumulate_grad_batches: int = 1, captured: Optional[bool] = None) -> TrainingHistory:
    """Train `axl_network` for `max_epochs` epochs of `data_module`'s batches.  `hyper_params`: what loss.configure_optimizers
    accepts.  Per epoch: the training batches, the validation batches (denoising_loss, unconditional), then the scheduler --
    ReduceLROnPlateau is stepped on its `monitor` value (train_epoch_loss or validation_epoch_loss), any other once per epoch.

    Returns a TrainingHistory: train_epoch_loss, validation_epoch_loss, learning_rate, one entry per epoch -- the
    batch-size-weighted means of the batches' losses (added in binary64 on the device) and the learning rate the epoch ran
    with.  ONE host read per epoch brings the two sums and the noiser's status word: a dataset row or atom type out of range
    (the kernel clamps it) raises IndexError at the end of the epoch it was met in.

    Two routes, decided once.  Captured (`captured` True, or None where it applies: a network and optimizer FusedMlpTrainingStep
    accepts, no regularizer, accumulate_grad_batches 1): every full batch is one replay of one hipGraph that holds the noising
    launch, the step's five calls and the two device counters; nothing is copied from the host and nothing is read; the tail
    batch runs the same launches eagerly.  General: per batch one noising launch, then loss.optimisation_step."""
    if data_module.train_dataset is None:
        data_module.setup()
    configured = loss.configure_optimizers(hyper_params, axl_network)
    optimizer, scheduler, monitor = configured["optimizer"], configured.get("lr_scheduler"), configured.get("monitor")
    refusal = captured_route_refusal(axl_network, optimizer, regularizer, accumulate_grad_batches)
    if captured and refusal:
        raise MdxError(f"fit(captured=True): {refusal}")
    captured = refusal is None if captured is None else bool(captured)
    epoch_runner = None
    if captured:
        epoch_runner = _CapturedEpoch(loss.FusedMlpTrainingStep(axl_network, optimizer, loss_parameters, gradient_clipping), data_module)
    train_rows = data_module.train_dataset[RELATIVE_COORDINATES].shape[0]
    valid_rows = data_module.valid_dataset[RELATIVE_COORDINATES].shape[0]
    history = TrainingHistory(optimizer, scheduler)
    for epoch in range(max_epochs):
        history["learning_rate"].append(float(optimizer.param_groups[0]["lr"]))
        if captured:
            train_sum = epoch_runner.run(epoch)
        else:
            train_sum = torch.zeros(1, dtype=torch.float64, device=data_module.device)
            for batch_index, batch in enumerate(data_module.train_batches(epoch)):
                out = loss.optimisation_step(axl_network, batch, optimizer, loss_parameters, regularizer, current_epoch=epoch,
                                             batch_index=batch_index, gradient_clipping=gradient_clipping,
                                             accumulate_grad_batches=accumulate_grad_batches)
                train_sum.add_(out["loss"].detach().to(torch.float64), alpha=float(batch[RELATIVE_COORDINATES].shape[0]))
        valid_sum = _validation_sum(axl_network, data_module, loss_parameters, epoch)
        status = data_module.noiser.status
        sums = torch.cat([train_sum, valid_sum, status.to(torch.float64)]).tolist()                  # the epoch's one host read
        if int(sums[2]) & kernels._hip.STATUS_NOISING_INDEX:
            kernels.raise_noising_status(status)
        metrics = dict(train_epoch_loss=sums[0] / train_rows, validation_epoch_loss=sums[1] / valid_rows)
        for name, value in metrics.items():
            history[name].append(value)
        if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            scheduler.step(metrics[monitor])
        elif scheduler is not None:
            scheduler.step()
    return history
