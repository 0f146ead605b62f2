"""What AnalyticalScoreNetwork and EquivariantAnalyticalScoreNetwork share around their one-kernel forward.  A mixin in front of
ScoreNetwork; the class sets `natoms`, `number_of_atomic_classes`, `spatial_dimension` and, in its __init__, `graph_status`,
`_constants` and its cache slot to None."""
from typing import AnyStr, Dict

import torch

from ... import kernels
from ...namespace import AXL, NOISY_AXL_COMPOSITION


class _ExactScoreOutputs:
    _device_copies_slot: str        # the attribute that holds the device copies (the name it had before the classes shared this)

    # ---- what the samplers look for (generators/network_hooks.py)
    def capture_safe(self, batch_size: int, number_of_atoms: int, device) -> bool:
        """No host read in the forward: the forward can always be captured into a hipGraph."""
        return True

    def check_status(self):
        """One host read of the status word: the reference's assertion for an invalid sigma or coordinate; the word is cleared."""
        if self.graph_status is not None:
            kernels.raise_analytical_status(self.graph_status)

    def _status_on(self, device) -> torch.Tensor:
        if self.graph_status is None or self.graph_status.device != device:
            self.graph_status = torch.zeros(1, dtype=torch.int32, device=device)
        return self.graph_status

    def _copies_on(self, device, *parameters: torch.Tensor):
        """`parameters` as contiguous f32 on `device`, copied there once (a forward inside a captured loop must not upload) and
        again only after one of them was replaced or written in place."""
        key = (device, *(item for p in parameters for item in (p.data_ptr(), p._version)))
        cached = getattr(self, self._device_copies_slot)
        if cached is None or cached[0] != key:
            cached = (key, *(p.detach().to(device=device, dtype=torch.float32).contiguous() for p in parameters))
            setattr(self, self._device_copies_slot, cached)
        return cached[1:]

    def _check_batch(self, batch: Dict[AnyStr, torch.Tensor]):
        super()._check_batch(batch)
        assert batch[NOISY_AXL_COMPOSITION].X.shape[1] == self.natoms, \
            "The dimension corresponding to the number of atoms is not consistent with the configuration."

    def _constant_outputs(self, batch_size: int, device):
        """The logits (0, .., 0, -inf) [batch, natoms, classes] and the zero lattice output [batch, natoms, d]: constants, made
        once per (batch size, device) and returned by every forward (read-only by contract: the samplers only read them), so
        that a forward inside the loop is the kernel and nothing else of this class's."""
        key = (batch_size, device)
        if self._constants is None or self._constants[0] != key:
            atomic_logits = torch.zeros(batch_size, self.natoms, self.number_of_atomic_classes, device=device)
            atomic_logits[..., -1] = -torch.inf
            self._constants = (key, atomic_logits, torch.zeros(batch_size, self.natoms, self.spatial_dimension, device=device))
        return self._constants[1], self._constants[2]

    def _as_axl(self, scores: torch.Tensor, batch_size: int, device) -> AXL:
        """AXL(A = the constant logits: one possible atom type, X = scores, L = zeros in the reference's shape)."""
        atomic_logits, zeros = self._constant_outputs(batch_size, device)
        return AXL(A=atomic_logits, X=scores, L=zeros)
