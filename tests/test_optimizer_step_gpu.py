"""The fused optimizer step on the GPU (csrc/mdx_optimizer.hip through kernels.adam_step, models/optimizer.py::FusedAdam and
loss.optimisation_step) against the float64 records of tests/golden/optimizer/ and float64 torch steps on the CPU.

The bound is derived, not measured (optimizer_cases.bound): |got - ref64| <= 2^-23 |ref64| + 2^-149 for m', v' and the norm -- one
binary32 rounding of a binary64 evaluation -- and 2^-50 |p| more for p'."""
import copy

import numpy as np
import pytest
import torch

import nets
import optimizer_cases as oc
from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd.loss import configure_optimizers, optimisation_step
from diffusion_for_multi_scale_molecular_dynamics_amd.models.optimizer import FusedAdam, OptimizerParameters, load_optimizer

pytestmark = pytest.mark.gpu
RECORDS = [(case, i) for case in oc.TEACHER_FORCED for i in oc.records(case)]


def bits(tensors):
    return oc.flat(tensors).view(np.int32)


def run_record(g, i, device, offset=0, zero_gradients=False, clip=None, groups=None):
    """Record i through kernels.adam_step: one plan over the tensors that have a gradient (or one per entry of `groups`, lists
    of tensor indices).  Returns the tensors after, the counters, the norm buffer's copy and the status word."""
    p, gradients, m, v = oc.device_operands(g, i, device, offset)
    values = oc.hyper(g)
    clip = values["max_norm"] > 0.0 if clip is None else clip
    served = [k for k in range(len(p)) if gradients[k] is not None]
    # the counters: one entry per chunk, every chunk of a tensor at the tensor's given step
    slots, total = kernels.adam_counter_slots(g["counts"])
    chunks = [-(-int(count) // kernels.ADAM_CHUNK_ELEMENTS) for count in g["counts"]]
    steps = torch.from_numpy(np.repeat(g[f"r{i}_step_before"].astype(np.int32), chunks)).to(device)
    assert steps.numel() == total
    hyper = torch.zeros(_hip.ADAM_HYPER_COUNT, dtype=torch.float64, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    kernels.adam_hyper_fill(hyper, values["lr"], values["beta1"], values["beta2"], values["eps"], values["weight_decay"],
                            values["max_norm"], 1.0)
    norm = None
    for group in ([served] if groups is None else groups):
        group = [k for k in group if k in served]
        plan = kernels.adam_plan([p[k] for k in group], [gradients[k] for k in group], [m[k] for k in group],
                                 [v[k] for k in group], slots=[slots[k] for k in group])
        out = kernels.adam_step(plan, steps, hyper, oc.decoupled(g), zero_gradients=zero_gradients, clip=clip,
                                status=status)
        norm = None if out is None else out.clone()
    torch.cuda.synchronize()
    per_chunk = np.split(steps.cpu().numpy(), np.cumsum(chunks)[:-1])
    assert all(len(set(entries.tolist())) <= 1 for entries in per_chunk)           # every chunk of a tensor at the same step
    per_tensor = np.array([entries[0] if len(entries) else 0 for entries in per_chunk], dtype=np.int32)
    return dict(p=p, g=[x for x in gradients if x is not None], m=m, v=v, steps=per_tensor, norm=norm, status=int(status.item()))


@pytest.mark.parametrize("case, i", RECORDS)
def test_teacher_forced_records_within_the_derived_bound(case, i, cuda):
    g = oc.fixture(case)
    out = run_record(g, i, cuda)
    worst = dict(p=oc.excess(oc.flat(out["p"]), g[f"r{i}_p64"], g[f"r{i}_p"]), m=oc.excess(oc.flat(out["m"]), g[f"r{i}_m64"]),
                 v=oc.excess(oc.flat(out["v"]), g[f"r{i}_v64"]))
    if float(g["max_norm"]) > 0.0:
        worst["norm"] = oc.excess(out["norm"][:1].cpu().numpy(), g[f"r{i}_norm64"].reshape(1))
        assert float(out["norm"][1]) == float(out["norm"][0])**2 or abs(float(out["norm"][1]) - float(out["norm"][0])**2) <= \
            4e-16 * float(out["norm"][1])
    print(case, i, worst)
    assert all(value <= 1.0 for value in worst.values()), worst
    live = g["counts"] > 0           # a tensor without elements takes no row of the tables: its counter is not served
    assert np.array_equal(out["steps"][live], g[f"r{i}_step"][live])
    assert out["status"] == 0
    # the gradients: bit-unchanged without zero_gradients, exactly +0.0 with it -- and the same p', m', v' bits either way
    _, recorded, _, _ = oc.device_operands(g, i, cuda)
    assert np.array_equal(bits(out["g"]), bits([x for x in recorded if x is not None]))
    zeroed = run_record(g, i, cuda, zero_gradients=True)
    assert not bits(zeroed["g"]).any()
    assert all(np.array_equal(bits(zeroed[key]), bits(out[key])) for key in ("p", "m", "v"))


def test_unaligned_views_give_the_bits_of_aligned_copies(cuda):
    g = oc.fixture("unaligned_view")
    aligned, views = run_record(g, 0, cuda), run_record(g, 0, cuda, offset=1)
    assert all(t.data_ptr() % 16 == 0 for t in aligned["p"]) and all(t.data_ptr() % 16 == 4 for t in views["p"])
    assert all(np.array_equal(bits(views[key]), bits(aligned[key])) for key in ("p", "m", "v"))
    assert np.array_equal(views["steps"], aligned["steps"]) and views["status"] == 0
    # with clipping the norm kernel takes the dword path as well: the same bits
    a, b = run_record(g, 0, cuda, clip=True), run_record(g, 0, cuda, offset=1, clip=True)
    assert torch.equal(a["norm"], b["norm"]) and np.array_equal(bits(a["p"]), bits(b["p"]))


def test_big_tensors_split_across_two_groups_give_the_bits_of_one(cuda):
    g = oc.fixture("big")
    for i in oc.records("big"):
        one, two = run_record(g, i, cuda, clip=False), run_record(g, i, cuda, clip=False, groups=[[0], [1]])
        assert all(np.array_equal(bits(one[key]), bits(two[key])) for key in ("p", "m", "v"))
        assert np.array_equal(one["steps"], two["steps"]) and np.array_equal(one["steps"], g[f"r{i}_step"])


def test_a_gradient_that_is_not_finite_sets_the_status_bit_and_nothing_raises(cuda):
    g = oc.fixture("adamw_decay")
    parameters = [torch.nn.Parameter(t) for t in oc.device_operands(g, 0, cuda)[0]]
    optimizer = FusedAdam(parameters, lr=1e-3, weight_decay=1e-2, decoupled_weight_decay=True)
    for q, gradient in zip(parameters, oc.device_operands(g, 0, cuda)[1]):
        q.grad = gradient
    optimizer.step()
    assert int(optimizer.status.item()) == 0
    parameters[3].grad[7] = float("nan")
    before = bits(parameters)
    optimizer.step()
    assert int(optimizer.status.item()) == _hip.STATUS_OPTIMIZER_NONFINITE
    after = oc.flat(parameters)
    assert np.isnan(after).sum() == 1 and np.isnan(oc.flat([parameters[3]])[7])          # it propagates, as in torch
    assert not np.array_equal(after.view(np.int32), before)


def small_optimizer(device, case="adamw_decay", record=0, **keywords):
    """FusedAdam on the small list with record's parameters and gradients (static gradient buffers)."""
    g = oc.fixture(case)
    p, gradients, _, _ = oc.device_operands(g, record, device)
    parameters = [torch.nn.Parameter(t) for t in p]
    for q, gradient in zip(parameters, gradients):
        q.grad = gradient
    settings = dict(lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), decoupled_weight_decay=oc.decoupled(g))
    settings.update(keywords)
    return FusedAdam(parameters, **settings), parameters


@pytest.fixture
def launches(monkeypatch):
    """The names of the entry points called and of the tables uploaded, in order."""
    seen = []
    call, upload = _hip.call, kernels._adam_upload
    monkeypatch.setattr(kernels, "call", lambda name, *args: (seen.append(name), call(name, *args))[1])
    monkeypatch.setattr(kernels, "_adam_upload", lambda *args: (seen.append("upload"), upload(*args))[1])
    return seen


def test_launch_counts(cuda, launches):
    optimizer, parameters = small_optimizer(cuda)
    optimizer.step()
    assert launches == ["mdx_adam_hyper_fill"] + ["upload"] * 5 + ["mdx_adam_step"]
    del launches[:]
    optimizer.step()
    assert launches == ["mdx_adam_step"]                    # no table upload, no fill: one launch
    del launches[:]
    optimizer.gradient_clip_val = 0.1
    optimizer.step()
    assert launches == ["mdx_adam_hyper_fill", "mdx_gradient_norm", "mdx_adam_step"]
    del launches[:]
    optimizer.step()
    assert launches == ["mdx_gradient_norm", "mdx_adam_step"]
    assert optimizer.last_gradient_norm.is_cuda and optimizer.last_gradient_norm.dtype == torch.float64
    optimizer.gradient_clip_val = 0.0
    optimizer.step()
    del launches[:]
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=10, eta_min=1e-5)
    optimizer.step()
    assert launches == ["mdx_adam_step"]
    scheduler.step()
    del launches[:]
    optimizer.step()
    assert launches == ["mdx_adam_hyper_fill", "mdx_adam_step"]          # exactly one fill, no upload


def optimizer_operands(optimizer, parameters):
    """What the next step reads: clones of p, .grad, exp_avg, exp_avg_sq and the counters (host)."""
    steps = optimizer.steps_taken()[0].cpu().numpy()
    state = lambda q, key: optimizer.state[q][key].clone() if key in optimizer.state.get(q, {}) else None
    return ([q.detach().clone() for q in parameters], [None if q.grad is None else q.grad.clone() for q in parameters],
            [state(q, "exp_avg") for q in parameters], [state(q, "exp_avg_sq") for q in parameters], steps)


def assert_step_within_bound(before, parameters, optimizer, lr, max_norm=0.0, what=""):
    group = optimizer.param_groups[0]
    p, gradients, m, v, steps = before
    p64, m64, v64, norm = oc.torch64_step(p, gradients, m, v, steps, lr=lr, weight_decay=group["weight_decay"],
                                          decoupled_weight_decay=group["decoupled_weight_decay"], max_norm=max_norm,
                                          betas=group["betas"], eps=group["eps"])
    stepped = [k for k, gradient in enumerate(gradients) if gradient is not None and gradient.numel()]
    worst = dict(
        p=oc.excess(oc.flat(parameters), np.concatenate(p64), oc.flat(p)),
        m=oc.excess(oc.flat([optimizer.state[parameters[k]]["exp_avg"] for k in stepped]), np.concatenate([m64[k] for k in stepped])),
        v=oc.excess(oc.flat([optimizer.state[parameters[k]]["exp_avg_sq"] for k in stepped]), np.concatenate([v64[k] for k in stepped])))
    print(what, worst)
    assert all(value <= 1.0 for value in worst.values()), (what, worst)
    return norm


def test_the_step_after_a_scheduler_changed_the_learning_rate(cuda):
    optimizer, parameters = small_optimizer(cuda)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=4, eta_min=1e-6)
    optimizer.step()
    scheduler.step()
    lr = optimizer.param_groups[0]["lr"]
    assert lr != float(oc.fixture("adamw_decay")["lr"])
    before = optimizer_operands(optimizer, parameters)
    optimizer.step()
    assert_step_within_bound(before, parameters, optimizer, lr, what="after CosineAnnealingLR.step()")
    # a float64 step at the OLD learning rate is beyond the bound: the comparison sees the rate
    p64_old = oc.torch64_step(*before, lr=float(oc.fixture("adamw_decay")["lr"]), weight_decay=1e-2, decoupled_weight_decay=True)[0]
    assert oc.excess(oc.flat(parameters), np.concatenate(p64_old), oc.flat(before[0])) > 1.0


def test_state_dict_crosses_to_torch_and_back(cuda):
    optimizer, parameters = small_optimizer(cuda)
    optimizer.step()
    optimizer.step()
    state = optimizer.state_dict()
    assert set(state) == {"state", "param_groups"}
    reference_keys = set(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0])
    assert set(state["param_groups"][0]) == reference_keys
    entry = state["state"][0]
    assert set(entry) == {"step", "exp_avg", "exp_avg_sq"} and entry["step"].dtype == torch.float32 and entry["step"].dim() == 0
    # this class's state into torch.optim.AdamW on a copy of the parameters
    copies = [torch.nn.Parameter(q.detach().clone()) for q in parameters]
    theirs = torch.optim.AdamW(copies, lr=1e-3, weight_decay=1e-2)
    theirs.load_state_dict(copy.deepcopy(state))
    live = [k for k, q in enumerate(parameters) if q.numel()]
    assert all(float(theirs.state[copies[k]]["step"]) == 2.0 for k in live)
    assert all(torch.equal(theirs.state[copies[k]]["exp_avg"], optimizer.state[parameters[k]]["exp_avg"]) for k in live)
    # torch's state after two steps into FusedAdam
    g = oc.fixture("adamw_decay")
    twins = [torch.nn.Parameter(t) for t in oc.device_operands(g, 0, cuda)[0]]
    torchs = torch.optim.AdamW(twins, lr=float(g["lr"]), weight_decay=float(g["weight_decay"]))
    for _ in range(2):
        for q, gradient in zip(twins, oc.device_operands(g, 0, cuda)[1]):
            q.grad = gradient
        torchs.step()
    mine, mine_parameters = small_optimizer(cuda)
    with torch.no_grad():
        for q, twin in zip(mine_parameters, twins):
            q.copy_(twin)
    mine.load_state_dict(copy.deepcopy(torchs.state_dict()))
    assert np.array_equal(mine.steps_taken()[0].cpu().numpy()[live], np.full(len(live), 2))
    assert mine.param_groups[0]["decoupled_weight_decay"] is True
    # both optimizers' third steps against the float64 reference
    before = optimizer_operands(optimizer, parameters)
    optimizer.step()
    assert_step_within_bound(before, parameters, optimizer, 1e-3, what="third step, own state")
    before = optimizer_operands(mine, mine_parameters)
    assert all(int(s) == 2 for s in before[4][live])
    mine.step()
    assert_step_within_bound(before, mine_parameters, mine, 1e-3, what="third step, torch's state")


def test_captured_step_replays_as_eager_steps_and_follows_the_learning_rate(cuda, launches, monkeypatch):
    g = oc.fixture("free_running")
    gradients = [oc.split(g["g"][s], g["counts"]) for s in range(4)]

    def refill(parameters, s):
        with torch.no_grad():
            for q, piece, shape in zip(parameters, gradients[s], oc.shapes(g)):
                q.grad.copy_(torch.from_numpy(np.ascontiguousarray(piece)).view(shape))

    captured, parameters = small_optimizer(cuda)
    twin, twin_parameters = small_optimizer(cuda)
    captured.gradient_clip_val = twin.gradient_clip_val = 0.1
    captured.prepare()
    del launches[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured.step()
    assert launches == ["mdx_gradient_norm", "mdx_adam_step"]       # one stream's chain: nothing else was enqueued or uploaded
    assert int(captured.steps_taken()[0].max().item()) == 0           # capturing ran nothing
    for s in range(3):
        refill(parameters, s), refill(twin_parameters, s)
        graph.replay()
        twin.step()
    torch.cuda.synchronize()
    assert np.array_equal(bits(parameters), bits(twin_parameters))
    assert torch.equal(captured.steps_taken()[0], twin.steps_taken()[0]) and int(twin.steps_taken()[0][0].item()) == 3
    assert torch.equal(captured.last_gradient_norm, twin.last_gradient_norm)
    # a new learning rate: written by the fill launch outside the captured region, honoured by the next replay
    captured.param_groups[0]["lr"] = twin.param_groups[0]["lr"] = 2.5e-4
    del launches[:]
    captured.prepare()
    assert launches == ["mdx_adam_hyper_fill"]
    refill(parameters, 3), refill(twin_parameters, 3)
    stale = bits(parameters)
    graph.replay()
    twin.step()
    torch.cuda.synchronize()
    assert np.array_equal(bits(parameters), bits(twin_parameters)) and not np.array_equal(bits(parameters), stale)
    # a hyper-parameter that changes inside a capture raises before anything is launched
    captured.param_groups[0]["lr"] = 1e-4
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    del launches[:]
    with pytest.raises(RuntimeError, match="outside the captured region"):
        captured.step()
    assert launches == []


def training_setup(device):
    from test_denoising_loss_gpu import noised_batch
    net = nets.mlp_net(5, 2, hidden=32, seed=11).to(device)
    net.register_parameter("never_used", torch.nn.Parameter(torch.full((3,), 0.5, device=device)))
    configured = configure_optimizers(dict(optimizer=dict(name="adamw", learning_rate=1e-3, weight_decay=1e-2)), net)
    assert set(configured) == {"optimizer"} and type(configured["optimizer"]) is FusedAdam
    seen = {}
    for q in net.parameters():
        q.register_post_accumulate_grad_hook(lambda q: seen.__setitem__(q, q.grad.detach().clone()))
    return net, configured["optimizer"], noised_batch("c3_n5_d3_p6", device), seen


def test_optimisation_step_end_to_end(cuda):
    net, optimizer, batch, seen = training_setup(cuda)
    parameters = list(net.parameters())
    assert load_optimizer(OptimizerParameters(name="adam", learning_rate=1e-3), net).defaults["decoupled_weight_decay"] is False
    start = [q.detach().clone() for q in parameters]
    out = optimisation_step(net, batch, optimizer, gradient_clipping=0.1)
    gradients = [seen.get(q) for q in parameters]
    assert len(seen) >= 8 and net.never_used not in seen
    before = (start, gradients, [None] * len(parameters), [None] * len(parameters), np.zeros(len(parameters), dtype=np.int32))
    norm = assert_step_within_bound(before, parameters, optimizer, 1e-3, max_norm=0.1, what="one optimisation_step")
    assert oc.excess(out["gradient_norm"].reshape(1).cpu().numpy(), np.array([norm])) <= 1.0
    assert out["gradient_norm"].is_cuda and out["loss"].is_cuda
    # the gradients were consumed and are zeros; the parameter without a gradient keeps its bits and has no state
    assert all(q.grad is None or not q.grad.view(-1).view(torch.int32).any() for q in parameters)
    assert net.never_used.grad is None and torch.equal(net.never_used.detach(), torch.full((3,), 0.5, device=cuda))
    assert net.never_used not in optimizer.state
    stepped = torch.tensor([gradient is not None for gradient in gradients])
    assert np.array_equal(optimizer.steps_taken()[0].cpu().numpy(), stepped.numpy().astype(np.int32))
    # a second step sees counters 2
    seen.clear()
    before = optimizer_operands(optimizer, parameters)
    optimisation_step(net, batch, optimizer, gradient_clipping=0.1, batch_index=1)
    assert np.array_equal(optimizer.steps_taken()[0].cpu().numpy(), 2 * stepped.numpy().astype(np.int32))
    before = (before[0], [seen.get(q) for q in parameters]) + before[2:]
    assert_step_within_bound(before, parameters, optimizer, 1e-3, max_norm=0.1, what="second optimisation_step")
    assert int(optimizer.status.item()) == 0


def test_optimisation_step_accumulates_over_two_batches(cuda):
    net, optimizer, batch, seen = training_setup(cuda)
    parameters = list(net.parameters())
    start = [q.detach().clone() for q in parameters]
    out = optimisation_step(net, batch, optimizer, gradient_clipping=0.1, accumulate_grad_batches=2, batch_index=0)
    assert "gradient_norm" not in out
    assert np.array_equal(bits(parameters), bits(start))                    # no parameter bit changed
    first = {q: gradient.clone() for q, gradient in seen.items()}
    assert all(torch.equal(q.grad, first[q]) and bool(q.grad.any()) for q in first)          # the gradients are kept
    optimisation_step(net, batch, optimizer, gradient_clipping=0.1, accumulate_grad_batches=2, batch_index=1)
    gradients = [seen.get(q) for q in parameters]          # what the second backward left: the sum of the two halved gradients
    before = (start, gradients, [None] * len(parameters), [None] * len(parameters), np.zeros(len(parameters), dtype=np.int32))
    assert_step_within_bound(before, parameters, optimizer, 1e-3, max_norm=0.1, what="accumulated step")
    assert all(q.grad is None or not q.grad.view(-1).view(torch.int32).any() for q in parameters)
    assert int(optimizer.steps_taken()[0].max().item()) == 1


def test_trajectory_guard_against_a_drifting_state(cuda):
    """free_running's 20 steps through FusedAdam and through torch.optim.AdamW in float32 on the same GPU with the same gradients:
    the kernel's largest distance to the float64 record must not exceed twice torch's own.  Both are chains of binary32 roundings
    that differ only in how many roundings a step has; a guard against a drifting state, not a precision claim."""
    g = oc.fixture("free_running")
    counts, shapes = g["counts"], oc.shapes(g)
    make = lambda: [torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(piece)).to(cuda).view(shape))
                    for piece, shape in zip(oc.split(g["p0"], counts), shapes)]
    mine_parameters, torch_parameters = make(), make()
    settings = dict(lr=float(g["lr"]), weight_decay=float(g["weight_decay"]), betas=(float(g["beta1"]), float(g["beta2"])),
                    eps=float(g["eps"]))
    mine = FusedAdam(mine_parameters, decoupled_weight_decay=True, **settings)
    theirs = torch.optim.AdamW(torch_parameters, **settings)
    distance = dict(mine=0.0, torch=0.0)
    for s in range(int(g["steps"])):
        for group in (mine_parameters, torch_parameters):
            for q, piece, shape in zip(group, oc.split(g["g"][s], counts), shapes):
                q.grad = torch.from_numpy(np.ascontiguousarray(piece)).to(cuda).view(shape)
        mine.step()
        theirs.step()
        distance["mine"] = max(distance["mine"], float(np.max(np.abs(oc.flat(mine_parameters).astype(np.float64) - g["p64"][s]))))
        distance["torch"] = max(distance["torch"], float(np.max(np.abs(oc.flat(torch_parameters).astype(np.float64) - g["p64"][s]))))
    print("trajectory distances", distance, "ratio", distance["mine"] / distance["torch"])
    assert distance["torch"] > 0.0 and distance["mine"] <= 2.0 * distance["torch"], distance
