"""The sampler with and without the per-node work whose result is a constant per class:
  * EGNNScoreNetwork.first_layer_class_rows -- on the distance table the first graph layer's h is one row per class, read by its
    node kernel through the nodes' classes; h [n_nodes, H] and the first projections are not made;
  * with ONE atom type the predictor's forward runs without its logits path too (network_hooks.logits_unread), and the type
    update takes no logits (mdx_pc_step_update, logits == NULL).
The final composition is the same bit for bit with both on and off, eager and captured, and across a table fallback; two atom
types, a recorder or a forward hook keep the predictor's logits.  T = 6, M = 2, B = 4, N = 8, device RNG, radius graph, 2 graph
layers of width 32, first_layer_table = "on"."""
import warnings

import pytest
import torch

import cases
import nets
from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MDX_PREDICTOR
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.langevin_generator import IterationLoop, LangevinGenerator
from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
    PredictorCorrectorSamplingParameters
from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters

pytestmark = pytest.mark.gpu

T, M, B, N = 6, 2, 4, 8


def _net(device, num_atom_types, switches, precision="f16x3", table="on", steep=False):
    net = nets.egnn_net(num_atom_types, "radial_cutoff", 7.5, hidden=32, n_layers=2, n_hidden=2, seed=17).to(device)
    net.edge_chain_precision = precision
    if steep:       # every first-layer neuron a kink in r^2 narrower than a grid cell: the table fails its midpoint check
        with torch.no_grad():
            first = net.egnn.graph_layers[0].message_mlp[0]
            first.weight[:, 2 * 32] *= 1.0e4
            first.bias.copy_(-first.weight[:, 2 * 32] * torch.linspace(0.5, 11.5, 32, device=device))
    net.first_layer_table = table                     # ("auto" declines grids this small)
    net.first_layer_class_rows = net.skip_unread_logits = switches
    return net


def _generator(device, net, num_atom_types, use_graph, **record):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        npar = NoiseParameters(**cases.noise_ns(T, **cases.LIN))
        spar = PredictorCorrectorSamplingParameters(
            **cases.sampling_ns(N, num_atom_types, M=M, greedy=False, one=False, cell=[10.86] * 3),
            rng_mode="device", seed=11, use_hip_graph=use_graph, **record)
    return LangevinGenerator(npar, spar, net)


@pytest.fixture
def seen(monkeypatch):
    """What the run did: forwards that returned A = None (they end in kernels.egnn_scores), node kernels that read class rows,
    and per step update (mode, were logits passed)."""
    log = dict(hinted=0, indexed=0, steps=[])
    scores, rows, step = kernels.egnn_scores, kernels.node_mlp_rows, kernels.pc_step_update

    def node_mlp_rows(*a, **k):
        log["indexed"] += k.get("row_class") is not None
        return rows(*a, **k)

    def pc_step_update(sched, mode, index_i, d_index, flags, atom_types, x, l, logits, *rest):
        log["steps"].append((mode, logits is not None))
        return step(sched, mode, index_i, d_index, flags, atom_types, x, l, logits, *rest)

    monkeypatch.setattr(kernels, "egnn_scores", lambda *a, **k: (log.__setitem__("hinted", log["hinted"] + 1), scores(*a, **k))[1])
    monkeypatch.setattr(kernels, "node_mlp_rows", node_mlp_rows)
    monkeypatch.setattr(kernels, "pc_step_update", pc_step_update)
    return log


def _device_loop(gen, device, log, iterations=T):
    gen._prepare(device)
    gen._begin_call(device)
    loop = IterationLoop(gen, gen.initialize(B, device), T, use_graph=False)
    log.update(hinted=0, indexed=0, steps=[])
    loop.advance(iterations)
    gen.check_status()
    return loop.composition


def test_final_composition_is_the_same(cuda, seen):
    outs = []
    with torch.no_grad():
        for switches in (True, False):
            for how in ("graph", "eager", "device_loop"):
                net = _net(cuda, 1, switches)
                gen = _generator(cuda, net, 1, how == "graph")
                seen.update(hinted=0, indexed=0, steps=[])
                outs.append(_device_loop(gen, cuda, seen) if how == "device_loop" else gen.sample(B, cuda))
                assert gen.table_fallbacks == 0 and gen.f16_range_fallbacks == 0 and net.table_builds() > 0
                if how == "device_loop":
                    # every forward of the device loop runs without its logits path and on the class rows; no step gets logits
                    assert seen["hinted"] == ((M + 1) * T if switches else 0)
                    assert seen["indexed"] == ((M + 1) * T if switches else 0)
                    assert len(seen["steps"]) == (M + 1) * T
                    assert all(has_logits == (mode == MDX_PREDICTOR and not switches) for mode, has_logits in seen["steps"])
                elif how == "graph":
                    assert (seen["indexed"] > 0) == switches and (seen["hinted"] > 0) == switches
                else:       # sample()'s eager loop hands its predictions back: whole forwards, but still on the class rows
                    assert seen["hinted"] == 0 and (seen["indexed"] > 0) == switches
    for out in outs[1:]:
        assert torch.equal(out.A, outs[0].A) and torch.equal(out.X, outs[0].X) and torch.equal(out.L, outs[0].L)


@pytest.mark.parametrize("use_graph", [True, False])
def test_across_a_table_fallback(cuda, use_graph):
    """The table fails its check in the first iteration: that iteration is recomputed on the per-edge chain -- which needs h per
    node again -- and the run equals one with first_layer_table = 'off' from the start."""
    with torch.no_grad():
        net = _net(cuda, 1, True, precision="f32", steep=True)            # (f32: no f16-range report can join the table's)
        gen = _generator(cuda, net, 1, use_graph)
        with pytest.warns(UserWarning, match="distance table"):
            got = gen.sample(B, cuda)
        assert gen.table_fallbacks == 1 and net.first_layer_table == "off"
        ref_gen = _generator(cuda, _net(cuda, 1, False, precision="f32", table="off", steep=True), 1, use_graph)
        ref = ref_gen.sample(B, cuda)
        assert ref_gen.table_fallbacks == 0
    assert torch.equal(got.A, ref.A) and torch.equal(got.X, ref.X) and torch.equal(got.L, ref.L)


def test_two_atom_types_keep_the_predictors_logits(cuda, seen):
    with torch.no_grad():
        gen = _generator(cuda, _net(cuda, 2, True), 2, False)
        _device_loop(gen, cuda, seen)
    assert seen["hinted"] == M * T and seen["indexed"] == (M + 1) * T           # the correctors alone leave their logits out
    assert all(has_logits == (mode == MDX_PREDICTOR) for mode, has_logits in seen["steps"])


@pytest.mark.parametrize("watcher", ["recorder", "forward_hook"])
def test_a_recorder_or_a_hook_sees_the_predictors_logits(cuda, watcher, seen):
    outs = []
    with torch.no_grad():
        for switches in (True, False):
            net = _net(cuda, 1, switches)
            if watcher == "recorder":
                gen = _generator(cuda, net, 1, False, record_samples=True)
                gen.sample(B, cuda)
                torch.cuda.synchronize()
                steps = gen.sample_trajectory_recorder._internal_data["predictor_step"]
                assert len(steps) == T
                outs.append([step["model_predictions_i"] for step in steps])
            else:
                outs.append([])
                net.register_forward_hook(lambda module, args, out, kept=outs[-1]: kept.append(out))
                _device_loop(_generator(cuda, net, 1, False), cuda, seen, iterations=2)
                torch.cuda.synchronize()
                assert len(outs[-1]) == 2 * (M + 1)
    assert seen["hinted"] == 0
    for on, off in zip(*outs):
        assert on.A is not None and torch.equal(torch.as_tensor(on.A), torch.as_tensor(off.A))
        assert torch.equal(torch.as_tensor(on.X), torch.as_tensor(off.X))
