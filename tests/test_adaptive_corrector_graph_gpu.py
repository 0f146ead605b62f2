"""AdaptiveCorrectorGenerator on the device-resident loop: captured into a hipGraph (use_hip_graph, rng_mode="device"), equal to
its eager steps bit for bit, against the CPU oracle, with the score network's reports handled per iteration, through the CLI,
and with the batch totals all-reduced over RCCL in a one-rank process group."""
import copy
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import adaptive_cases
import cases
import nets
from conftest import ROOT, torus_rel_l2
from oracle import reference_sampler as RS

pytestmark = pytest.mark.gpu

SEED = 17
# traj_egnn_rc's network and shape (N 64, cell 10.86, M 2, radius graph) under the adaptive algorithm
EGNN = (cases.noise_ns(4, **cases.LIN),
        dict(cases.sampling_ns(64, 1, M=2, one=False, greedy=False, cell=[10.86] * 3), algorithm="adaptive_corrector"),
        lambda eb: nets.egnn_net(1, "radial_cutoff", 7.5, edge_builder=eb))
CASES = dict(adaptive_cases.ALL, adaptive_egnn_rc=EGNN)


def _pkg():
    from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.adaptive_corrector import AdaptiveCorrectorGenerator
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
        PredictorCorrectorSamplingParameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    return AdaptiveCorrectorGenerator, PredictorCorrectorSamplingParameters, NoiseParameters, MdxError


def _build(name, cuda, **extra):
    """(generator, noise parameters, sampling parameters, CPU copy of the network)"""
    Generator, Sampling, Noise, _ = _pkg()
    noise_kw, sampling_kw, netf = CASES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        npar, spar = Noise(**noise_kw), Sampling(**dict(sampling_kw, rng_mode="device", seed=SEED, **extra))
    torch.manual_seed(1234)
    net = nets.fake_net(spar.num_atom_types) if netf is None else netf(None)
    net_cpu = copy.deepcopy(net) if "egnn" not in name else None
    return Generator(npar, spar, net.to(cuda)), npar, spar, net_cpu


def _np(axl):
    return RS.AXL(A=axl.A.cpu().numpy(), X=axl.X.cpu().numpy(), L=axl.L.cpu().numpy())


def _same_bits(a, b):
    return (np.array_equal(a.A, b.A) and np.array_equal(a.X.view(np.int32), b.X.view(np.int32))
            and np.array_equal(a.L.view(np.int32), b.L.view(np.int32)))


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


@pytest.mark.parametrize("name", list(CASES))
def test_captured_loop_equals_eager_steps(cuda, name):
    """use_hip_graph=True constructs (it raised MdxError before the batch statistics ran on the device), samples on a captured
    IterationLoop without an eager-launch warning, and equals the eager generator bit for bit in A, X and L.  The EGNN case
    additionally: finite outputs, no status bit, three sample() calls on ONE capture."""
    outs = {}
    for use_graph in (False, True):
        gen, *_ = _build(name, cuda, use_hip_graph=use_graph)
        with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            calls = [gen.sample(6, cuda) for _ in range(3)]
        assert not [w for w in caught if "launched eagerly" in str(w.message)]
        if use_graph:
            loop = gen._buffers["graph_loop"]
            assert loop.graph is not None
            with torch.no_grad():
                gen.sample(6, cuda)
            assert gen._buffers["graph_loop"] is loop
        else:
            assert "graph_loop" not in gen._buffers
        if "egnn" in name:
            assert all(torch.isfinite(c.X).all() and torch.isfinite(c.L).all() for c in calls)
            assert int(gen._status.item()) == 0 and gen.f16_range_fallbacks == 0 and gen.table_fallbacks == 0
        outs[use_graph] = [_np(c) for c in calls]
    for eager, captured in zip(outs[False], outs[True]):
        assert _same_bits(eager, captured), name
    assert not np.array_equal(outs[True][0].X, outs[True][1].X)
    if not CASES[name][1]["use_fixed_lattice_parameters"]:
        assert not np.array_equal(outs[True][0].L, outs[True][1].L)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("name", list(adaptive_cases.ALL))
def test_against_the_oracle(cuda, name, use_graph):
    """A exact, X torus rel-L2 < 1e-5, L rel-L2 < 1e-5 against OracleAdaptiveCorrectorGenerator on the CPU copy of the network
    with the Philox specification (the bars of test_adaptive_corrector_against_golden_and_oracle)."""
    gen, npar, spar, net_cpu = _build(name, cuda, use_hip_graph=use_graph)
    with torch.no_grad():
        out = _np(gen.sample(6, cuda))
    ora = RS.OracleAdaptiveCorrectorGenerator(npar, spar, net_cpu, noise=RS.PhiloxNoise(SEED, 0)).sample(6)
    x_err, l_err = torus_rel_l2(out.X, ora.X), _rel_l2(out.L, ora.L)
    print(f"{name} graph {use_graph}: X {x_err:.2e} L {l_err:.2e}")
    assert np.array_equal(out.A, ora.A)
    assert x_err < 1e-5
    assert l_err < 1e-5


def test_step_size_the_loop_used(cuda):
    """One eagerly launched device-index iteration: the weights left on the device equal the float64 formula evaluated on that
    iteration's own last predictions and draws, within the kernel test's derived bar."""
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    from test_adaptive_corrector_kernel_gpu import _formula, _sigmas, eps_bar
    name = "traj_adaptive_free_lattice"
    gen, npar, spar, _ = _build(name, cuda)
    B, N, d, M, T = 5, spar.number_of_atoms, 3, spar.number_of_corrector_steps, npar.total_time_steps
    seen = []
    inner = gen._get_model_predictions
    gen._get_model_predictions = lambda *a, **k: (seen.append(inner(*a, **k)), seen[-1])[1]
    with torch.no_grad():
        sched = gen._prepare(cuda)
        gen._begin_call(cuda)
        comp = gen.initialize(B, cuda)
        comp = RS.AXL(A=comp.A.clone(), X=comp.X.clone(), L=comp.L.clone())
        d_index = torch.tensor([T - 1], dtype=torch.int32, device=cuda)
        gen._iteration_on_device_index(comp, torch.zeros_like(comp.X), d_index)
    assert int(d_index.item()) == T - 2 and len(seen) == 1 + M
    _, _, weights = gen._buffers[("adaptive", B)]
    src, index = gen.noise_source, T - 1
    draw = index * (M + 1) + M                                     # the last corrector: offset 1 + (M - 1)
    zx = kernels.rng_fill(kernels.RNG_NORMAL, src.seed, src.call, draw, _hip.TAG_COORD, B * N, d, cuda).view(B, N, d)
    zl = kernels.rng_fill(kernels.RNG_NORMAL, src.seed, src.call, draw, _hip.TAG_LATTICE, B, 6, cuda)
    sigma, sigma_n = _sigmas(sched, index, N, d)
    _, want = _formula(seen[-1].X, seen[-1].L, zx, zl, sigma, sigma_n, False, r=npar.corrector_r, small=spar.small_epsilon)
    got = weights.double().cpu().numpy()
    bar = eps_bar(N, d)
    assert abs(got[0] - want[0]) / want[0] <= bar and abs(got[3] - want[3]) / want[3] <= bar
    assert got[2] == want[2] and got[5] == want[5]
    assert abs(got[1] - want[1]) / want[1] <= bar / 2 + 2.0 ** -24 and abs(got[4] - want[4]) / want[4] <= bar / 2 + 2.0 ** -24


class _RangeReportAt(torch.nn.Module):
    """Test plugin around an EGNN (as tests/test_egnn_chain_gpu.py's): at ONE time value it raises the f16-range bit in the
    network's status word -- what the split-f16 kernels do when an activation overflows -- and spoils the scores of that
    forward.  Device operations only (the iteration is captured); silent when the network runs the exact-f32 kernels.  It sets a
    status bit; it provokes no fault."""

    def __init__(self, net, time_value):
        super().__init__()
        self.net = net
        self.register_buffer("time_values", torch.as_tensor(time_value, dtype=torch.float32).reshape(-1))

    graph_status = property(lambda self: self.net.graph_status)
    edge_chain_precision = property(lambda self: self.net.edge_chain_precision,
                                    lambda self, value: setattr(self.net, "edge_chain_precision", value))

    def forward(self, batch, conditional=None):
        from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
        from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL, TIME
        out = self.net(batch, conditional)
        if self.net.edge_chain_precision in ("f16x3", "f16x3_32x32"):
            hit = (batch[TIME][:1, 0:1] == self.time_values).any().reshape(1)
            self.net.graph_status.bitwise_or_(hit.to(torch.int32) * _hip.STATUS_EGNN_F16_RANGE)
            out = AXL(A=out.A, X=out.X + hit.to(out.X.dtype) * 1.0e3, L=out.L)
        return out


@pytest.mark.parametrize("use_graph", [True, False])
def test_forced_f16_range_report_costs_the_flagged_iterations(cuda, use_graph):
    """A network that reports the f16-range bit at one time value: seen by the predictor of iteration k and by the correctors of
    iteration k + 1 (they share time[k]), so exactly two iterations are recomputed in f32 by the inherited _recover -- on the
    same draws, which depend on the time index only -- and the result equals, bit for bit, the run with the precision switched
    by hand for exactly those iterations."""
    Generator, Sampling, Noise, _ = _pkg()
    T, B, k, precision = 9, 5, 4, "f16x3"
    noise_kw, sampling_kw, _ = EGNN

    def build(wrap):
        torch.manual_seed(21)
        net = nets.egnn_net(1, "radial_cutoff", 7.5, hidden=32, n_layers=2, n_hidden=2).to(cuda)
        net.edge_chain_precision = precision
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            npar = Noise(**dict(noise_kw, total_time_steps=T))
            spar = Sampling(**dict(sampling_kw, rng_mode="device", seed=5, use_hip_graph=use_graph and wrap))
        gen = Generator(npar, spar, net)
        gen._prepare(cuda)
        if wrap:
            gen.axl_network = _RangeReportAt(net, float(gen.noise.time[k])).to(cuda)
        return gen, net

    gen, net = build(wrap=True)
    with torch.no_grad(), pytest.warns(UserWarning, match="f16 range"):
        got = gen.sample(B, cuda)
    assert gen.f16_range_fallbacks == 2 and net.edge_chain_precision == precision
    if use_graph:
        assert gen._buffers["graph_loop"].graph is not None
    ref, ref_net = build(wrap=False)
    with torch.no_grad():
        ref._begin_call(cuda)
        comp = ref.initialize(B, cuda)
        forces = torch.zeros_like(comp.X)
        for i in range(T - 1, -1, -1):
            ref_net.edge_chain_precision = "f32" if i in (k, k + 1) else precision
            comp = ref._iteration(comp, i, forces)
        ref.check_status()
    assert torch.equal(got.A, comp.A) and torch.equal(got.X, comp.X) and torch.equal(got.L, comp.L)
    assert torch.isfinite(got.X).all() and (got.A == 0).all()


def test_refusals_and_fallbacks(cuda):
    """fused_score_network is still refused (the persistent MLP kernel has no batch-wide reduction); recording launches eagerly
    and records, as for every generator."""
    Generator, Sampling, Noise, MdxError = _pkg()
    noise_kw, sampling_kw, netf = CASES["traj_adaptive_mlp"]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        npar = Noise(**noise_kw)
        fused = Sampling(**dict(sampling_kw, rng_mode="device", seed=SEED, fused_score_network=True))
    with pytest.raises(MdxError, match="use_hip_graph / fused_score_network do not apply"):
        Generator(npar, fused, netf(None).to(cuda))
    outs = []
    for record in (True, False):
        extra = dict(record_samples=True, record_samples_corrector_steps=True) if record else {}
        gen, npar, spar, _ = _build("traj_adaptive_mlp", cuda, use_hip_graph=True, **extra)
        with torch.no_grad():
            outs.append(_np(gen.sample(4, cuda)))
        if record:
            assert "graph_loop" not in gen._buffers
            data = gen.sample_trajectory_recorder._internal_data
            T, M = npar.total_time_steps, spar.number_of_corrector_steps
            assert len(data["predictor_step"]) == T and len(data["corrector_step"]) == T * M
            for entry in data["predictor_step"]:
                assert torch.equal(entry["composition_i"].X, entry["composition_im1"].X)
        else:
            assert gen._buffers["graph_loop"].graph is not None
    assert _same_bits(outs[0], outs[1])


def test_cli_end_to_end(cuda, tmp_path):
    """sample_diffusion with `algorithm: adaptive_corrector, rng_mode: device, use_hip_graph: true` -- a YAML that failed at
    construction -- writes samples.pt equal to the generator's own output."""
    import yaml
    from diffusion_for_multi_scale_molecular_dynamics_amd import sample_diffusion
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.adaptive_corrector import AdaptiveCorrectorGenerator
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.instantiate_generator import instantiate_generator
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.load_sampling_parameters import load_sampling_parameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.score_network_factory import (
        create_score_network, create_score_network_parameters)
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.sampling.diffusion_sampling import create_batch_of_samples_sharded
    cfg = dict(noise=dict(total_time_steps=10, sigma_min=1e-3, sigma_max=0.2, schedule_type="linear", corrector_r=0.17),
               sampling=dict(algorithm="adaptive_corrector", spatial_dimension=3, number_of_atoms=8, number_of_samples=12,
                             sample_batchsize=5, num_atom_types=1, number_of_corrector_steps=2,
                             use_fixed_lattice_parameters=False, rng_mode="device", use_hip_graph=True, seed=11),
               elements=["Si"],
               model=dict(score_network=dict(architecture="mlp", number_of_atoms=8, num_atom_types=1, n_hidden_dimensions=2,
                                             hidden_dimensions_size=16, relative_coordinates_embedding_dimensions_size=8,
                                             noise_embedding_dimensions_size=4, time_embedding_dimensions_size=4,
                                             atom_type_embedding_dimensions_size=1,
                                             lattice_parameters_embedding_dimensions_size=1)))
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    out = tmp_path / "out"
    sample_diffusion.main(["--config", str(tmp_path / "config.yaml"), "--output", str(out), "--device", "cuda",
                           "--random_init_seed", "3"])
    samples = torch.load(out / "samples.pt", weights_only=False)
    assert samples["original_axl"].X.shape == (12, 8, 3) and samples["original_axl"].L.shape == (12, 6)
    torch.manual_seed(3)
    net = create_score_network(create_score_network_parameters(cfg["model"]["score_network"],
                                                               sample_diffusion.global_parameters_of(cfg))).eval().to(cuda)
    spar = load_sampling_parameters(cfg["sampling"])
    gen = instantiate_generator(sampling_parameters=spar, noise_parameters=NoiseParameters(**cfg["noise"]), axl_network=net,
                                trajectory_initializer=None)
    assert type(gen) is AdaptiveCorrectorGenerator and gen.use_hip_graph
    with torch.no_grad():
        own = create_batch_of_samples_sharded(generator=gen, sampling_parameters=spar, device=cuda)
    assert gen._buffers["graph_loop"].graph is not None
    for got, want in zip(samples["original_axl"], own["original_axl"]):
        assert torch.equal(got.cpu(), want.cpu())


_WORKER = r'''
import os, sys, warnings
import torch, torch.distributed as dist
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import adaptive_cases, nets
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.adaptive_corrector import AdaptiveCorrectorGenerator
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
    PredictorCorrectorSamplingParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters

assert os.environ["WORLD_SIZE"] == "1" and os.environ["RANK"] == "0"
device = torch.device("cuda", int(os.environ["LOCAL_RANK"]))
torch.cuda.set_device(device)
dist.init_process_group(backend="nccl", device_id=device)               # RCCL
reduced = []
inner = dist.all_reduce
dist.all_reduce = lambda t, *a, **k: (reduced.append((t.dtype, tuple(t.shape))), inner(t, *a, **k))[1]

for name in ("traj_adaptive_free_lattice", "traj_adaptive_fake"):
    noise_kw, sampling_kw, netf = adaptive_cases.ALL[name]
    outs = {{}}
    for sync in (True, False):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            spar = PredictorCorrectorSamplingParameters(**dict(sampling_kw, rng_mode="device", seed=606, use_hip_graph=True,
                                                               sync_batch_statistics=sync))
        torch.manual_seed(1234)
        net = nets.fake_net(spar.num_atom_types) if netf is None else netf(None)
        gen = AdaptiveCorrectorGenerator(NoiseParameters(**noise_kw), spar, net.to(device))
        del reduced[:]
        with torch.no_grad(), warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            outs[sync] = [gen.sample(5, device) for _ in range(2)]
        eager = [w for w in caught if "launched eagerly" in str(w.message)]
        steps = 2 * NoiseParameters(**noise_kw).total_time_steps * spar.number_of_corrector_steps
        if sync:       # the eager branch, ONE all-reduce of the double[8] totals per corrector step, one warning
            assert len(eager) == 1 and "graph_loop" not in gen._buffers, name
            assert reduced == [(torch.float64, (8,))] * steps, (name, reduced[:4], len(reduced))
        else:          # captured
            assert not eager and not reduced and gen._buffers["graph_loop"].graph is not None, name
    for a, b in zip(outs[True], outs[False]):      # a one-rank sum changes nothing
        assert torch.equal(a.A, b.A) and torch.equal(a.X, b.X) and torch.equal(a.L, b.L), name

dist.barrier()
dist.destroy_process_group()
print("worker ok")
'''


def test_synchronised_statistics_over_rccl_in_a_one_rank_group(cuda, tmp_path):
    """One child process under torchrun --nproc-per-node 1: with sync_batch_statistics the run takes the eager branch with the
    RCCL all-reduce of the totals, and equals the captured un-synchronised run bit for bit."""
    script = tmp_path / "adaptive_rccl_worker.py"
    script.write_text(_WORKER.format(root=ROOT))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29581", str(script)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    run = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0 and "worker ok" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])
