"""Force-field augmented score network (src/.../models/score_networks/force_field_augmented_score_network.py:20-236).

Wraps any ScoreNetwork and adds a short-range repulsive pseudo-force to the coordinate score.  Inputs that do not require
grad (the sampler's) go through ONE HIP kernel (mdx_force_field_pseudo_force: the radius graph's tile and pair test, the sum
per atom in place, no edge list, no host read), fused with the add to the inner network's score in forward(): the wrapper can
then be captured into a hipGraph with the network it wraps.  Inputs that require grad take the torch formulation below, over
the full HIP radius graph (kernel N1: every (src, dst, image) edge with its lattice shift, sorted by source atom).
"""
from dataclasses import dataclass
from typing import AnyStr, Dict, Optional

import torch

from ... import kernels
from ...namespace import AXL, NOISY_AXL_COMPOSITION
from ...utils import neighbors
from ...utils.neighbors import get_periodic_adjacency_information
from .score_network import ScoreNetwork

MIN_BOX_SIZE = 1.0      # map_noisy_axl_lattice_parameters_to_unit_cell_vectors(..., min_box_size=1.0) (:147-150)


@dataclass(kw_only=True)
class ForceFieldParameters:
    """phi(r) = strength * (r - radial_cutoff)^2 for r < radial_cutoff  (:20-41)."""

    radial_cutoff: float
    strength: float

    def __post_init__(self):
        assert self.radial_cutoff > 0.0, "the radial cutoff should be greater than zero."
        assert self.strength > 0.0, "the repulsive strength should be greater than zero."


class ForceFieldAugmentedScoreNetwork(torch.nn.Module):
    def __init__(self, score_network: ScoreNetwork, force_field_parameters: ForceFieldParameters):
        super().__init__()
        self._score_network = score_network
        self._force_field_parameters = force_field_parameters
        self._own_status = None         # the kernel's status word when the wrapped network has none
        self._status_used = None        # the word the last kernel launch reported into

    @property
    def force_field_parameters(self) -> ForceFieldParameters:
        return self._force_field_parameters

    # What the generators look for on a score network (generators/network_hooks.py is the contract).  The names below go
    # straight through to the wrapped network, reads and sets alike.  One rule for all of them: a name the wrapped network
    # lacks is absent here too (hasattr is false, and a set is dropped), so that the hooks' defaults for an absent name --
    # None, "off", a no-op -- mean what they would mean on the wrapped network.  graph_status, check_status and capture_safe
    # are written out below: they also answer for the pseudo-force kernel.
    FORWARDED = ("edge_chain_precision", "sigma_uniform_hint", "logits_unread_hint", "first_layer_table", "adapt_f16_range",
                 "begin_f16_range_fallback", "reset_f16_range")

    def __getattr__(self, name):
        if name in self.FORWARDED:
            return getattr(self._score_network, name)
        return super().__getattr__(name)

    def __setattr__(self, name, value):
        if name not in self.FORWARDED:
            super().__setattr__(name, value)
        elif hasattr(self._score_network, name):
            setattr(self._score_network, name, value)

    @property
    def graph_status(self):
        """The status word of the last pseudo-force launch (the wrapped network's word when it has one), else the wrapped
        network's."""
        if self._status_used is not None:
            return self._status_used
        return getattr(self._score_network, "graph_status", None)

    def check_status(self):
        """Raise for any MDX_STATUS_* bit collected by the wrapped network's kernels or the pseudo-force kernel (the
        reference's "radial cutoff is so large" assertion among them): one host read per word, every word cleared."""
        words = []
        for word in (getattr(self._score_network, "graph_status", None), self._own_status):
            if word is not None and all(word is not w for w in words):
                words.append(word)
        held = [w.clone() for w in words]
        for w in words:
            w.zero_()
        for w in held:
            neighbors._raise_if_cutoff_too_large(w)

    def capture_safe(self, batch_size: int, number_of_atoms: int, device) -> bool:
        """The pseudo-force kernel needs no host synchronisation: the wrapped network's answer decides (True without one)."""
        ask = getattr(self._score_network, "capture_safe", None)
        return True if ask is None else bool(ask(batch_size, number_of_atoms, device))

    def forward(self, batch: Dict[AnyStr, torch.Tensor], conditional: Optional[bool] = None) -> AXL:
        raw = self._score_network(batch, conditional)
        comp = batch[NOISY_AXL_COMPOSITION]
        if not self._on_kernel(comp):
            return AXL(A=raw.A, X=raw.X + self._torch_pseudo_force(comp), L=raw.L)
        if raw.X.requires_grad:         # (autograd through the wrapped network: the add stays a torch operation, same bits)
            return AXL(A=raw.A, X=raw.X + self._kernel_pseudo_force(comp), L=raw.L)
        return AXL(A=raw.A, X=self._kernel_pseudo_force(comp, score_in=raw.X.contiguous()), L=raw.L)

    def get_relative_coordinates_pseudo_force(self, batch: Dict[AnyStr, torch.Tensor]) -> torch.Tensor:
        """F_i = sum_j 2 s (r_ij - r0)/r_ij * (p_j + shift - p_i), converted to relative coordinates (:86-236)."""
        comp = batch[NOISY_AXL_COMPOSITION]
        if self._on_kernel(comp):
            return self._kernel_pseudo_force(comp)
        return self._torch_pseudo_force(comp)

    @staticmethod
    def _on_kernel(comp: AXL) -> bool:
        """The HIP kernel computes the pseudo-force unless autograd has to see through it."""
        return not (comp.X.requires_grad or comp.L.requires_grad)

    def _status_word(self, device) -> torch.Tensor:
        word = getattr(self._score_network, "graph_status", None)
        if word is None or word.device != device:
            if self._own_status is None or self._own_status.device != device:
                self._own_status = torch.zeros(1, dtype=torch.int32, device=device)
            word = self._own_status
        return word

    def _kernel_pseudo_force(self, comp: AXL, score_in: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = comp.X
        self._status_used = self._status_word(x.device)
        p = self._force_field_parameters
        return kernels.force_field_pseudo_force(x.contiguous(), comp.L.contiguous(), MIN_BOX_SIZE, p.radial_cutoff, p.strength,
                                                score_in=score_in, status=self._status_used)

    def _torch_pseudo_force(self, comp: AXL) -> torch.Tensor:
        """The same sum in torch operations over the full radius graph's edge list (one host read sizes it): the path for
        inputs that require grad."""
        x = comp.X
        bsz, n, d = x.shape
        s, r0 = self._force_field_parameters.strength, self._force_field_parameters.radial_cutoff
        lengths = comp.L[:, :d].clip(min=MIN_BOX_SIZE)
        cell = torch.diag_embed(lengths)
        cart = torch.matmul(x, cell)
        info = get_periodic_adjacency_information(cart, cell, radial_cutoff=r0)      # d = 3 only, as the reference (:131-135)
        src, dst = info.adjacency_matrix
        node = info.edge_batch_indices * n + src                    # sorted: edges are grouped by source atom
        flat = cart.reshape(bsz * n, d)
        disp = flat.index_select(0, info.edge_batch_indices * n + dst) - flat.index_select(0, node) + info.shifts
        r = torch.linalg.norm(disp, dim=1)
        contrib = (2.0 * s * (r - r0) / (r + 1.0e-8)).unsqueeze(1) * disp
        degree = torch.bincount(node, minlength=bsz * n)
        forces = torch.segment_reduce(contrib, "sum", lengths=degree, axis=0, unsafe=True).reshape(bsz, n, d)
        return forces / lengths.unsqueeze(1)                        # cartesian -> relative for a diagonal cell
