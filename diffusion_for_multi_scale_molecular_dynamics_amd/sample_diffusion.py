"""Entry point: draw samples with the MI355X hot path (drop-in for src/.../sample_diffusion.py:52-274).

Same flags, YAML surface (`noise:`, `sampling:`, optional `elements:`), and output files (`samples.pt` =
{"cartesian_positions", "original_axl"}, `trajectories.pt`, `config_backup.yaml`, `console.log`).
Differences, all additive:
  * the score network comes from `--checkpoint` as in the reference -- the trainer's Lightning checkpoint: rebuilt from the
    hyper-parameters pickled inside it, weights under the prefix `axl_network.` (read without Lightning and without the
    reference package: utils/lightning_checkpoint.py) -- or, additionally, from a bare state_dict together with a `model:
    score_network:` block in the config, or is randomly initialised with `--random_init_seed` (synthetic benchmarks); an exact
    network (`architecture: analytical`: no trained weights) is built from the `model: score_network:` block alone when no
    `--checkpoint` is given;
  * under `torchrun` (one process per GPU) the sub-batches are sharded over the ranks and gathered once (RCCL);
    rank 0 writes the files (`trajectories.pt` holds every rank's recorded sub-batches, in sub-batch order);
  * `oracle: {name: stillinger_weber, sw_coeff_filename: <a LAMMPS .sw file, absolute or relative to the configuration>}` writes
    `energies.pt` (the Stillinger-Weber energy of every sample, CPU float64, as the reference's :243-251) from a HIP kernel;
    `name: lammps` is reported as out of scope (no LAMMPS here: samples.pt is written, energies.pt is not), Orion reporting
    is absent;
  * `--reference_samples PATH` (a torch pickle of reference structures in the sample contract, with `potential_energy` when the
    data set has it) together with a `metrics:` block that asks for something writes `metrics.pt`: the reference's validation
    metrics of the samples against those structures (metrics.compute_sampling_metrics: Kolmogorov-Smirnov distances of
    interatomic distances, energies and lattice parameters, from HIP kernels).  Without the flag the block is ignored, as in
    the reference.
"""
import argparse
import logging
import os
import shutil
import socket
import sys
from pathlib import Path
from typing import Any, AnyStr, Dict, Optional

import torch
import yaml

from .generators.instantiate_generator import instantiate_generator
from .generators.load_sampling_parameters import load_sampling_parameters
from .generators.sampling_constraint import read_sampling_constraint
from .generators.trajectory_initializer import instantiate_trajectory_initializer
from .models.score_networks.score_network import ScoreNetwork
from .data.element_types import ElementTypes
from .models.score_networks.score_network_factory import (EXACT_SCORE_NETWORKS_BY_ARCH, create_score_network,
                                                          create_score_network_parameters)
from .noise_schedulers.noise_parameters import NoiseParameters
from .namespace import AXL, AXL_COMPOSITION
from .sampling.diffusion_sampling import create_batch_of_samples_sharded
from .utils.structure_utils import (StillingerWeberParameters, compute_stillinger_weber_energies_and_forces,
                                    read_stillinger_weber_coefficients)

logger = logging.getLogger(__name__)


def extract_and_validate_parameters(hyper_params: Dict[AnyStr, Any]):
    """:168-188"""
    assert "noise" in hyper_params, "The noise parameters must be defined to draw samples."
    assert "sampling" in hyper_params, "The sampling parameters must be defined to draw samples."
    return NoiseParameters(**hyper_params["noise"]), load_sampling_parameters(hyper_params["sampling"])


def global_parameters_of(hyper_params: Dict[AnyStr, Any]) -> Optional[Dict[AnyStr, Any]]:
    """What the reference hands to create_score_network_parameters beside the `model: score_network:` block: for a TRAINING
    configuration (top-level `elements` and `data: max_atom`) exactly its dict(max_atom, spatial_dimension -- 3 when the file
    does not say --, elements) (models/instantiate_diffusion_model.py:34-41: a block that contradicts it is refused, as there);
    otherwise whichever of `elements` / `spatial_dimension` the file has; None when it has neither (a sampling configuration
    that spells its block out)."""
    data = hyper_params.get("data")
    if "elements" in hyper_params and isinstance(data, dict) and "max_atom" in data:
        return dict(max_atom=data["max_atom"], spatial_dimension=hyper_params.get("spatial_dimension", 3),
                    elements=hyper_params["elements"])
    out = {key: hyper_params[key] for key in ("elements", "spatial_dimension") if key in hyper_params}
    return out or None


def exact_score_network_block(hyper_params: Dict[AnyStr, Any]) -> Optional[Dict[AnyStr, Any]]:
    """The configuration's `model: score_network:` block when it names an exact architecture (one with no trained weights, which
    can therefore be built without a checkpoint); None otherwise."""
    model = hyper_params.get("model")
    block = model.get("score_network") if isinstance(model, dict) else None
    if isinstance(block, dict) and block.get("architecture") in EXACT_SCORE_NETWORKS_BY_ARCH:
        return block
    return None


def get_axl_network(checkpoint_path, hyper_params: Optional[Dict[AnyStr, Any]] = None) -> ScoreNetwork:
    """:191-205.  The reference rebuilds the network from the hyper-parameters INSIDE the Lightning checkpoint
    (`load_from_checkpoint`), so its sampling configurations hold no `model:` block; so does this -- without Lightning and
    without the reference package (utils/lightning_checkpoint.py) -- and loads the `axl_network.*` weights.  A `model:
    score_network:` block in the configuration, when there is one, takes precedence (a bare state_dict has nothing else)."""
    from .utils.lightning_checkpoint import load_checkpoint, score_network_parameters_of, state_dict_of
    checkpoint = load_checkpoint(checkpoint_path)
    hyper_params = hyper_params or {}
    if "model" in hyper_params and "score_network" in hyper_params["model"]:
        parameters = create_score_network_parameters(hyper_params["model"]["score_network"], global_parameters_of(hyper_params))
    else:
        parameters = score_network_parameters_of(checkpoint)
        assert parameters is not None, \
            "the checkpoint holds no hyper-parameters (not a Lightning checkpoint of the reference's trainer): the config " \
            "must contain the `model: score_network:` block that describes its network"
    network = create_score_network(parameters)
    network.load_state_dict(state_dict_of(checkpoint))
    return network.eval()


def _init_distributed(device: torch.device):
    if "RANK" not in os.environ:            # (under torchrun the group is set up at any world size, 1 included)
        return 0, 1, device
    import torch.distributed as dist
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if device.type == "cuda":
        device = torch.device("cuda", local_rank)
        torch.cuda.set_device(device)
    if not dist.is_initialized():
        dist.init_process_group(backend="nccl" if device.type == "cuda" else "gloo")
    return dist.get_rank(), dist.get_world_size(), device


def main(args: Optional[Any] = None, axl_network: Optional[ScoreNetwork] = None) -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", required=True, help="config file with sampling parameters in yaml format.")
    parser.add_argument("--checkpoint", default=None, help="path to checkpoint model to be loaded.")
    parser.add_argument("--output", required=True, help="path to outputs - will store files here")
    parser.add_argument("--path_to_starting_configuration_data_pickle", default=None)
    parser.add_argument("--path_to_sampling_constraint_data_pickle", default=None)
    parser.add_argument("--device", default="cuda", help="Device to use. Defaults to cuda.")
    parser.add_argument("--reference_pickles", action="store_true",
                        help="write samples.pt / trajectories.pt naming the REFERENCE's AXL class, so that the reference's own "
                             "tools read them with a plain torch.load (default: this package's class)")
    parser.add_argument("--random_init_seed", type=int, default=None,
                        help="build the network of `model.score_network` with random weights (synthetic runs)")
    parser.add_argument("--reference_samples", default=None,
                        help="torch pickle of reference structures (the sample contract; `potential_energy` optional): with a "
                             "`metrics:` block in the configuration, metrics.pt is written beside samples.pt")
    args = parser.parse_args(args)

    rank, world, device = _init_distributed(torch.device(args.device))
    os.makedirs(args.output, exist_ok=True)
    if rank == 0:
        logging.basicConfig(level=logging.INFO, force=True,
                            handlers=[logging.StreamHandler(sys.stdout),
                                      logging.FileHandler(os.path.join(args.output, "console.log"))])
        shutil.copyfile(args.config, os.path.join(args.output, "config_backup.yaml"))
    with open(args.config) as fd:
        hyper_params = yaml.safe_load(fd)
    logger.info("Sampling Experiment info:\n  Hostname : %s\n  Checkpoint : %s\n  Device   : %s\n  Ranks    : %d",
                socket.gethostname(), args.checkpoint, device, world)

    noise_parameters, sampling_parameters = extract_and_validate_parameters(hyper_params)
    if "elements" in hyper_params:
        ElementTypes.validate_elements(hyper_params["elements"])
    if getattr(sampling_parameters, "rng_mode", "reference") == "reference":
        logger.info("Sampling in the reference's mode (draws from torch's CPU generator in the reference's order, uploaded every step, "
                    "eager launches: reproduces the reference's run for a given torch.manual_seed).  `rng_mode: device` and "
                    "`use_hip_graph: true` in the `sampling:` block select the throughput modes (INTEGRATION.md).")
    oracle_parameters = oracle_parameters_of(hyper_params, args.config)
    metrics_parameters = metrics_parameters_of(hyper_params, args.reference_samples, oracle_parameters)
    if axl_network is None:
        if args.random_init_seed is not None:
            torch.manual_seed(args.random_init_seed)
            axl_network = create_score_network(
                create_score_network_parameters(hyper_params["model"]["score_network"], global_parameters_of(hyper_params))).eval()
        elif args.checkpoint is None and exact_score_network_block(hyper_params) is not None:
            # an exact network (`architecture: analytical`) has no trained weights: the `model: score_network:` block is all of it
            axl_network = create_score_network(
                create_score_network_parameters(exact_score_network_block(hyper_params), global_parameters_of(hyper_params))).eval()
        else:
            assert args.checkpoint is not None and os.path.exists(args.checkpoint), \
                f"The path {args.checkpoint} does not exist. Cannot go on."
            axl_network = get_axl_network(args.checkpoint, hyper_params)
    axl_network = axl_network.to(device)
    if "force_field" in hyper_params:                                  # src/sample_diffusion.py:132-139
        from .models.score_networks.force_field_augmented_score_network import (ForceFieldAugmentedScoreNetwork,
                                                                                 ForceFieldParameters)
        force_field_parameters = ForceFieldParameters(**hyper_params["force_field"])
        if force_field_parameters.radial_cutoff > 0.0:
            logger.info("Augmenting the AXL_network with an excluding Force Field.")
            axl_network = ForceFieldAugmentedScoreNetwork(axl_network, force_field_parameters)
        else:
            logger.info("Force field parameters are present, but the radial cutoff is zero. Using original AXL network")

    trajectory_initializer = instantiate_trajectory_initializer(
        sampling_parameters=sampling_parameters,
        path_to_starting_configuration_data_pickle=args.path_to_starting_configuration_data_pickle)
    sampling_constraints = None
    if args.path_to_sampling_constraint_data_pickle is not None:
        sampling_constraints = read_sampling_constraint(args.path_to_sampling_constraint_data_pickle)
    generator = instantiate_generator(sampling_parameters=sampling_parameters, noise_parameters=noise_parameters,
                                      axl_network=axl_network, trajectory_initializer=trajectory_initializer,
                                      sampling_constraints=sampling_constraints)
    create_samples_and_write_to_disk(generator, sampling_parameters, oracle_parameters, device, args.output, rank,
                                     for_reference=args.reference_pickles, metrics_parameters=metrics_parameters,
                                     reference_samples=args.reference_samples)


def metrics_parameters_of(hyper_params: Dict[AnyStr, Any], reference_samples, oracle_parameters):
    """The `metrics:` block as SamplingMetricsParameters when `--reference_samples` is given and the block asks for anything;
    None otherwise (the block is then ignored, as in the reference's sample_diffusion).  Refused HERE, before sampling: a file
    that does not exist, and `compute_energies` without a Stillinger-Weber `oracle:` block."""
    if reference_samples is None or "metrics" not in hyper_params:
        return None
    from .metrics import as_sampling_metrics_parameters, asks_for_anything, check_energy_oracle
    parameters = as_sampling_metrics_parameters(hyper_params["metrics"])
    if not asks_for_anything(parameters):
        return None
    assert os.path.isfile(reference_samples), f"The reference samples '{reference_samples}' do not exist."
    check_energy_oracle(parameters, oracle_parameters)
    return parameters


def oracle_parameters_of(hyper_params: Dict[AnyStr, Any], config_path) -> Optional[StillingerWeberParameters]:
    """The `oracle:` block (:141-147).  `name: stillinger_weber` needs the configuration's `elements` and a coefficient file
    that exists and parses (absolute, or relative to the configuration file): anything else is refused HERE, before sampling.
    Every other oracle (`lammps`) is reported as out of scope: None."""
    if "oracle" not in hyper_params:
        return None
    block = dict(hyper_params["oracle"])
    if block.get("name") != "stillinger_weber":
        logger.warning("The configuration has an `oracle:` block: the energy oracle (LAMMPS) is outside this package's scope; "
                       "samples.pt is written, energies.pt is not.")
        return None
    assert "elements" in hyper_params, "elements are needed to define the energy oracle."
    assert "sw_coeff_filename" in block, "`oracle: name: stillinger_weber` needs `sw_coeff_filename`, a LAMMPS .sw file"
    path = Path(block["sw_coeff_filename"])
    if not path.is_absolute():
        path = Path(config_path).resolve().parent / path
    parameters = StillingerWeberParameters(**dict(block, sw_coeff_filename=str(path)), elements=hyper_params["elements"])
    read_stillinger_weber_coefficients(parameters.sw_coeff_filename, parameters.elements)       # refusals come now
    return parameters


def create_samples_and_write_to_disk(generator, sampling_parameters, oracle_parameters, device, output_path, rank: int = 0,
                                     for_reference: bool = False, metrics_parameters=None, reference_samples=None):
    """:208-270.  oracle_parameters: the reference's third argument, the energy oracle to evaluate the samples with: None or
    StillingerWeberParameters (rank 0 then writes energies.pt); LAMMPS and anything else is outside this package's scope and
    refused; Orion reporting likewise absent.  metrics_parameters (SamplingMetricsParameters) and reference_samples (the path
    of a pickled reference batch), both or neither: rank 0 then writes metrics.pt."""
    if oracle_parameters is not None and not isinstance(oracle_parameters, StillingerWeberParameters):
        raise NotImplementedError("energy oracles other than StillingerWeberParameters (LAMMPS) are outside this package's scope: "
                                  "pass oracle_parameters=None")
    logger.info("Generating samples...")
    with torch.no_grad():
        samples_batch = create_batch_of_samples_sharded(generator=generator, sampling_parameters=sampling_parameters,
                                                        device=device)
    logger.info("Done Generating Samples.")
    fallbacks = getattr(generator, "f16_range_fallbacks", 0)
    if fallbacks:
        logger.warning("%d sampler iteration(s) were recomputed with the exact-f32 MFMA kernels: the split-f16 edge chain met "
                       "values beyond the f16 range (set edge_chain_precision='f32' on the network to avoid the retries)",
                       fallbacks)
    output_directory = Path(output_path)
    if sampling_parameters.record_samples:
        write_trajectories(generator.sample_trajectory_recorder, sampling_parameters, output_directory, for_reference)
    if rank != 0:
        return
    if for_reference:
        from .utils import reference_pickles
        reference_pickles.save_for_reference(samples_batch, output_directory / "samples.pt")
    else:
        with open(output_directory / "samples.pt", "wb") as fd:
            torch.save(samples_batch, fd)
    if oracle_parameters is not None:
        logger.info("Compute energy from Oracle...")
        axl = samples_batch[AXL_COMPOSITION]
        chunks = []
        for start in range(0, axl.X.shape[0], sampling_parameters.sample_batchsize):
            chunk = {AXL_COMPOSITION: AXL(*(t[start:start + sampling_parameters.sample_batchsize] for t in axl))}
            chunks.append(compute_stillinger_weber_energies_and_forces(chunk, oracle_parameters)[0].cpu())
        logger.info("Writing energies to disk...")
        with open(output_directory / "energies.pt", "wb") as fd:
            torch.save(torch.cat(chunks), fd)
    if metrics_parameters is not None and reference_samples is not None:
        from .metrics import compute_sampling_metrics
        from .utils import reference_pickles
        logger.info("Compute sampling metrics...")
        metrics = compute_sampling_metrics(samples_batch, reference_pickles.load(reference_samples), metrics_parameters,
                                           oracle_parameters, sampling_parameters.sample_batchsize)
        for name, value in metrics.items():
            logger.info("  %s : %.6g", name, value)
        with open(output_directory / "metrics.pt", "wb") as fd:
            torch.save(metrics, fd)
    logger.info("Done!")


def write_trajectories(recorder, sampling_parameters, output_directory: Path, for_reference: bool = False):
    """`trajectories.pt` of the WHOLE run (src/sample_diffusion.py:253-257).  Under several ranks every rank has recorded its own
    sub-batches: each writes `trajectories.rank{r}.pt` into the (shared, single-node) output directory, and after a barrier
    rank 0 puts the entries back in sub-batch order -- the file a single process would have written -- and removes the
    per-rank files.  No collective carries the records: they are T x (1 + M) compositions per sub-batch."""
    import torch.distributed as dist
    from .sampling.diffusion_sampling import split_sizes
    from .utils.sample_trajectory import merge_sharded_entries
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        recorder.write_to_pickle(output_directory / "trajectories.pt", for_reference=for_reference)
        return
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.save(recorder.entries(), output_directory / f"trajectories.rank{rank}.pt")
    dist.barrier()
    if rank == 0:
        paths = [output_directory / f"trajectories.rank{r}.pt" for r in range(world)]
        per_rank = [torch.load(path, weights_only=False) for path in paths]
        sizes = split_sizes(sampling_parameters.number_of_samples, sampling_parameters.sample_batchsize)
        merge_sharded_entries(per_rank, sizes, world).write_to_pickle(output_directory / "trajectories.pt", for_reference=for_reference)
        for path in paths:
            os.remove(path)
    dist.barrier()


if __name__ == "__main__":
    main()
