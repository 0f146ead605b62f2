"""Excise and repaint (src/.../active_learning_loop/sample_maker/excise_and_repaint_sample_maker.py:28-242): the environments of
the uncertain atoms are cut out of a frame, moved into a small box, and the rest of that box is repainted around each of them
by the constrained generator.

batch_environments = True (this package's own switch; an attribute, not a configuration field) runs the samples of ALL
environments of a frame through ONE PerSampleConstrainedLangevinGenerator, built once per maker and reused: E x S
trajectories in one captured loop instead of E loops one after another.  False is the reference's flow, one
ConstrainedLangevinGenerator per environment in order, drawing from torch's one global stream.

The sample edit's distances are binary64 on the widened float32 samples (mdx_edit_keep_mask); the reference computes them in
the samples' own binary32, so an atom within ~1e-6 Angstrom of the edit radius may fall on the other side."""
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from ... import kernels
from ...generators.axl_generator import SamplingParameters
from ...generators.constrained_langevin_generator import (ConstrainedLangevinGenerator,
                                                          PerSampleConstrainedLangevinGenerator)
from ...generators.noise_sources import PerEnvironmentNoise
from ...generators.sampling_constraint import SamplingConstraint
from ...models.score_networks.score_network import ScoreNetwork
from ...namespace import AXL
from ...noise_schedulers.noise_parameters import NoiseParameters
from ...sampling.diffusion_sampling import create_batch_of_samples
from ..atom_selector.base_atom_selector import BaseAtomSelector
from ..excisor.base_excisor import BaseEnvironmentExcision
from .base_sample_maker import BaseExciseSampleMaker, BaseExciseSampleMakerArguments


@dataclass(kw_only=True)
class ExciseAndRepaintSampleMakerArguments(BaseExciseSampleMakerArguments):
    algorithm: str = "excise_and_repaint"
    sample_edit_radius: Optional[float] = None      # Angstrom: generated atoms this close to the central atom are removed


def environments_per_chunk(number_of_environments: int, samples_per_environment: int, sample_batchsize: Optional[int]) -> List[int]:
    """How many WHOLE environments each sample() call of the batched maker takes: max(1, sample_batchsize // S) of them, all at
    once without a sample_batchsize."""
    if number_of_environments == 0:
        return []
    per_call = number_of_environments if not sample_batchsize else max(1, int(sample_batchsize) // samples_per_environment)
    full, rest = divmod(number_of_environments, per_call)
    return [per_call] * full + ([rest] if rest else [])


class ExciseAndRepaintSampleMaker(BaseExciseSampleMaker):
    batch_environments: bool = True

    def __init__(self, sample_maker_arguments: ExciseAndRepaintSampleMakerArguments, atom_selector: BaseAtomSelector,
                 environment_excisor: BaseEnvironmentExcision, noise_parameters: NoiseParameters,
                 sampling_parameters: SamplingParameters, diffusion_model: ScoreNetwork, device: str = "cpu"):
        super().__init__(sample_maker_arguments=sample_maker_arguments, atom_selector=atom_selector,
                         environment_excisor=environment_excisor)
        assert sample_maker_arguments.number_of_samples_per_substructure == sampling_parameters.number_of_samples, \
            ("ExciseAndRepaint uses a generative model to generates samples. The number of samples requested in "
             "the sampling_parameters (ie, 'number_of_samples') should be identical to the number of samples per "
             "substructure requested in the sample_maker configuration (ie 'number_of_samples_per_substructure'). "
             "The configuration currently asks for inconsistent things. Review input.")
        self.samples_should_be_edited = False
        if sample_maker_arguments.sample_edit_radius is not None:
            self.samples_should_be_edited = True
            self.sample_edit_radius = sample_maker_arguments.sample_edit_radius
        self.sample_noise_parameters = noise_parameters
        self.sampling_parameters = sampling_parameters
        self.diffusion_model = diffusion_model
        self.device = torch.device(device)
        self._batched_generator = None

    def create_sampling_constraints(self, constrained_structure: AXL) -> SamplingConstraint:
        """The excised structure (numpy) as the generator's constraint: its atoms are the sample's FIRST atoms, in order, so the
        active atom keeps its index; coordinates rounded to float32 once (:101-110)."""
        return SamplingConstraint(elements=self.arguments.element_list,
                                  constrained_relative_coordinates=torch.FloatTensor(constrained_structure.X),
                                  constrained_atom_types=torch.LongTensor(constrained_structure.A),
                                  constrained_indices=torch.arange(len(constrained_structure.X)))

    @staticmethod
    def torch_batch_axl_to_list_of_numpy_axl(axl_structure: AXL):
        """AXL of batched torch tensors -> one numpy AXL per structure (:122-133)."""
        return [AXL(A=a, X=x, L=lattice) for a, x, lattice in zip(axl_structure.A.cpu().numpy(), axl_structure.X.cpu().numpy(),
                                                                  axl_structure.L.cpu().numpy())]

    # -----------------------------------------------------------------------------------------------------------
    # the sample edit
    # -----------------------------------------------------------------------------------------------------------
    @staticmethod
    def _keep_masks(axl_structure: AXL, sample_environment: torch.Tensor, active_atoms, counts, radius: float) -> np.ndarray:
        """bool [B,N]: one launch of mdx_edit_keep_mask for a batch on the device."""
        device = axl_structure.X.device
        as_words = lambda v: v.to(device=device, dtype=torch.int32) if isinstance(v, torch.Tensor) else \
            torch.tensor(np.asarray(v), dtype=torch.int32, device=device)       # noqa: E731
        active_atoms, counts = as_words(active_atoms), as_words(counts)
        assert bool(((active_atoms >= 0) & (active_atoms < axl_structure.X.shape[1])).all()), "an active atom outside the sample"
        keep = kernels.edit_keep_mask(axl_structure.X.contiguous(), axl_structure.L.to(torch.float32).contiguous(),
                                      as_words(sample_environment), active_atoms, counts, radius)
        return keep.cpu().numpy().astype(bool)

    @staticmethod
    def _compact(samples: List[AXL], keep: np.ndarray) -> List[AXL]:
        """The ragged result of the edit: every sample keeps its own number of atoms (host)."""
        return [AXL(A=sample.A[mask], X=sample.X[mask], L=sample.L) for sample, mask in zip(samples, keep)]

    @staticmethod
    def edit_generated_structure(sampled_structure: AXL, active_atom_index: int, number_of_constrained_atoms: int,
                                 sample_edit_radius: float) -> AXL:
        """Remove the GENERATED atoms (those after the first number_of_constrained_atoms) within sample_edit_radius of the
        active atom (:224-242); one numpy structure, through the same kernel as a batch."""
        if not torch.cuda.is_available():
            raise kernels._hip.MdxError("the sample edit runs on the GPU only (mdx_edit_keep_mask; there is no CPU fallback)")
        device = torch.device("cuda", torch.cuda.current_device())
        batch = AXL(A=None, X=torch.from_numpy(np.asarray(sampled_structure.X, dtype=np.float32))[None].to(device),
                    L=torch.from_numpy(np.asarray(sampled_structure.L, dtype=np.float32))[None].to(device))
        keep = ExciseAndRepaintSampleMaker._keep_masks(batch, torch.zeros(1, dtype=torch.int32), [active_atom_index],
                                                       [number_of_constrained_atoms], sample_edit_radius)
        return ExciseAndRepaintSampleMaker._compact([sampled_structure], keep)[0]

    # -----------------------------------------------------------------------------------------------------------
    # one environment at a time (the reference's flow)
    # -----------------------------------------------------------------------------------------------------------
    def make_samples_from_constrained_substructure(self, substructure: AXL, active_atom_index: int, num_samples: int = 1
                                                   ) -> Tuple[List[AXL], List[int], List[Dict[str, Any]]]:
        """`num_samples` repaints around one substructure already in the new box, with a generator of its own (:157-197)."""
        number_of_constrained_atoms = len(substructure.X)
        assert active_atom_index < number_of_constrained_atoms, \
            ("The active atom index is larger than the number of constrained atoms: "
             "this should be impossible, something is wrong. Review code!")
        generator = ConstrainedLangevinGenerator(noise_parameters=self.sample_noise_parameters,
                                                 sampling_parameters=self.sampling_parameters,
                                                 axl_network=self.diffusion_model,
                                                 sampling_constraints=self.create_sampling_constraints(substructure))
        with torch.no_grad():
            generated = create_batch_of_samples(generator=generator, sampling_parameters=self.sampling_parameters,
                                                device=self.device)["original_axl"]
        new_structures = self.torch_batch_axl_to_list_of_numpy_axl(generated)
        if self.samples_should_be_edited:
            keep = self._keep_masks(generated, torch.zeros(len(new_structures), dtype=torch.int32), [active_atom_index],
                                    [number_of_constrained_atoms], self.sample_edit_radius)
            new_structures = self._compact(new_structures, keep)
        infos = [self._create_sample_info_dictionary(substructure) for _ in new_structures]
        return new_structures, num_samples * [active_atom_index], infos

    def filter_made_samples(self, structures: List[AXL]) -> List[AXL]:
        return structures

    # -----------------------------------------------------------------------------------------------------------
    # all environments of a frame in one batch
    # -----------------------------------------------------------------------------------------------------------
    def make_samples(self, structure: AXL, uncertainty_per_atom: np.array
                     ) -> Tuple[List[AXL], List[np.array], List[Dict[str, Any]]]:
        if not self.batch_environments:
            return super().make_samples(structure, uncertainty_per_atom)
        environments, in_new_box, central_indices, tables = self._excise_tables(structure, uncertainty_per_atom)
        if not environments:
            return [], [], []
        S = self.arguments.number_of_samples_per_substructure
        generated = self._sample_batched(tables, S)
        samples = self.torch_batch_axl_to_list_of_numpy_axl(generated)
        if self.samples_should_be_edited:
            sample_environment = torch.arange(len(environments), dtype=torch.int32).repeat_interleave(S)
            keep = self._keep_masks(generated, sample_environment, central_indices, tables[3], self.sample_edit_radius)
            samples = self._compact(samples, keep)
        active_indices, infos = [], []
        for environment, embedded, central in zip(environments, in_new_box, central_indices):
            active_indices += [np.array([central]) for _ in range(S)]
            infos += [self._with_structures(self._create_sample_info_dictionary(embedded), environment, embedded)
                      for _ in range(S)]
        return samples, active_indices, infos

    def _sample_batched(self, tables, samples_per_environment: int) -> AXL:
        """The E x S samples, `environments_per_chunk` environments per sample() call.  rng_mode "device": a call is one call
        index of the Philox source.  rng_mode "reference": environment e (counted over the whole frame) draws from a host
        generator of its own seeded torch.initial_seed() + e, whatever chunk it falls in."""
        if self._batched_generator is None:
            self._batched_generator = PerSampleConstrainedLangevinGenerator(
                noise_parameters=self.sample_noise_parameters, sampling_parameters=self.sampling_parameters,
                axl_network=self.diffusion_model, elements=self.arguments.element_list)
        generator = self._batched_generator
        cx, ca, cidx, counts = tables
        S, parts, first = samples_per_environment, [], 0
        with torch.no_grad():
            for size in environments_per_chunk(len(counts), S, self.sampling_parameters.sample_batchsize):
                chunk = slice(first, first + size)
                generator.set_environments((cx[chunk], ca[chunk], None if cidx is None else cidx[chunk], counts[chunk]), S)
                if generator.rng_mode == "reference":
                    generator.noise_source = PerEnvironmentNoise([torch.initial_seed() + e for e in range(first, first + size)], S)
                parts.append(generator.sample(size * S, self.device))
                first += size
        lattice = torch.concat([p.L for p in parts])
        lattice[..., generator.spatial_dimension:] = 0          # as create_batch_of_samples: the angle entries are zeroed
        return AXL(A=torch.concat([p.A for p in parts]), X=torch.concat([p.X for p in parts]), L=lattice)
