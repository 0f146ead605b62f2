"""The training epoch on the GPU: BatchNoiser's dictionary against NoisingTransform.transform's, `fit`'s captured route against
a hand-written loop of the eager launches (bit for bit), noise_once_at_setup, the general route against
loss.optimisation_step, the two schedulers, a learning sanity condition, and the host work of a captured epoch."""
import numpy as np
import pytest
import torch

from training_cases import gaussian_parameters, same_bits

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels, loss, training
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import Rng
from diffusion_for_multi_scale_molecular_dynamics_amd.data.diffusion.noising_transform import NoisingTransform
from diffusion_for_multi_scale_molecular_dynamics_amd.models.score_networks.mlp_score_network import (MLPScoreNetwork,
                                                                                                       MLPScoreNetworkParameters)
from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (ATOM_TYPES, CARTESIAN_FORCES, LATTICE_PARAMETERS,
                                                                        NOISY_RELATIVE_COORDINATES, Q_BAR_MATRICES,
                                                                        Q_BAR_TM1_MATRICES, Q_MATRICES, RELATIVE_COORDINATES,
                                                                        TIME_INDICES)

pytestmark = pytest.mark.gpu

ADAMW = dict(optimizer=dict(name="adamw", learning_rate=2e-3, weight_decay=1e-2))


def network(cuda, seed=11, **keywords):
    torch.manual_seed(seed)
    return MLPScoreNetwork(MLPScoreNetworkParameters(
        number_of_atoms=2, num_atom_types=1, spatial_dimension=3, n_hidden_dimensions=2, hidden_dimensions_size=32,
        relative_coordinates_embedding_dimensions_size=16, noise_embedding_dimensions_size=8, time_embedding_dimensions_size=8,
        atom_type_embedding_dimensions_size=4, lattice_parameters_embedding_dimensions_size=4, **keywords)).to(cuda)


def module(cuda, once=True, **changes):
    made = training.GaussianDataModule(gaussian_parameters(**changes), device=cuda)
    made.noise_once_at_setup = once
    made.setup()
    return made


def parameter_bits(net):
    return [p.detach().view(torch.int32).clone() for p in net.parameters()]


def same_parameters(a, b):
    return all(torch.equal(x, y) for x, y in zip(parameter_bits(a), parameter_bits(b)))


def validation_loss(net, data, epoch):
    total = torch.zeros(1, dtype=torch.float64, device=data.device)
    with torch.no_grad():
        for batch in data.valid_batches(epoch):
            out = loss.denoising_loss(net, batch, None, conditional=False)
            total.add_(out["loss"].to(torch.float64), alpha=float(batch[RELATIVE_COORDINATES].shape[0]))
    return float(total) / data.valid_dataset[RELATIVE_COORDINATES].shape[0]


def test_the_loaders_dictionary_is_the_transforms(cuda, monkeypatch):
    data = module(cuda)
    noiser, dataset = data.noiser, data.train_dataset
    ours = noiser.noise(dataset, batch_size=12, epoch=0)
    assert CARTESIAN_FORCES not in dataset            # the Gaussian module's forces are all zero: left out at setup
    clean = {key: dataset[key][:12].clone() for key in (RELATIVE_COORDINATES, ATOM_TYPES, LATTICE_PARAMETERS)}
    clean[CARTESIAN_FORCES] = torch.zeros_like(clean[RELATIVE_COORDINATES])
    transform = NoisingTransform(gaussian_parameters().noise_parameters, num_atom_types=1, spatial_dimension=3,
                                 use_optimal_transport=False, device=cuda)
    theirs = transform.transform(clean)
    assert set(ours) == set(theirs) and len(ours) == 13
    for key in theirs:
        assert ours[key].shape == theirs[key].shape and ours[key].dtype == theirs[key].dtype and ours[key].is_cuda, key
    for key in (Q_MATRICES, Q_BAR_MATRICES, Q_BAR_TM1_MATRICES):
        assert ours[key].shape == (12, 2, 2, 2) and ours[key].stride(1) == 0 == theirs[key].stride(1)
        assert torch.equal(ours[key][:, 1], getattr(noiser.noise_scheduler.tables, {Q_MATRICES: "q_matrix", Q_BAR_MATRICES: "q_bar_matrix",
                                                                                    Q_BAR_TM1_MATRICES: "q_bar_tm1_matrix"}[key])[ours[TIME_INDICES]])
    for key in (RELATIVE_COORDINATES, ATOM_TYPES, LATTICE_PARAMETERS):
        assert same_bits(ours[key], dataset[key][:12])
    # without forces in the dataset: one kept buffer of zeros and ONE launch; with forces: the rows' own, gathered beside it
    assert not bool(ours[CARTESIAN_FORCES].any()) and noiser.noise(dataset, batch_size=12)[CARTESIAN_FORCES] is ours[CARTESIAN_FORCES]
    launches = []
    call = _hip.call
    monkeypatch.setattr(kernels, "call", lambda name, *args: (launches.append(name), call(name, *args))[1])
    noiser.noise(dataset, batch_size=12)
    monkeypatch.undo()
    assert launches == ["mdx_noise_training_batch"]
    forces = torch.rand(160, 2, 3, generator=torch.Generator().manual_seed(1)).to(cuda)
    rows = torch.tensor([7, 3, 159, 0, 64], device=cuda)
    with_forces = noiser.noise({**dataset, CARTESIAN_FORCES: forces}, rows=rows, row_offset=1, batch_size=3)
    assert same_bits(with_forces[CARTESIAN_FORCES], forces[rows[1:4]]) and same_bits(with_forces[RELATIVE_COORDINATES],
                                                                                    dataset[RELATIVE_COORDINATES][rows[1:4]])
    # the consumers take it unchanged
    net = network(cuda)
    out = loss.denoising_loss(net, ours, conditional=False)
    assert out["loss"].dim() == 0 and bool(torch.isfinite(out["loss"]))
    optimizer = loss.configure_optimizers(ADAMW, net)["optimizer"]
    before = parameter_bits(net)
    stepped = loss.FusedMlpTrainingStep(net, optimizer).step(ours)
    assert bool(torch.isfinite(stepped["loss"])) and not all(torch.equal(a, b) for a, b in zip(before, parameter_bits(net)))
    kernels.raise_loss_status(out["status"])
    kernels.raise_noising_status(noiser.status)


@pytest.mark.parametrize("once", (True, False))
def test_the_captured_fit_is_the_hand_written_eager_loop(once, cuda):
    epochs, clipping = 2, 0.5
    data, net = module(cuda, once), network(cuda)
    history = training.fit(net, data, ADAMW, epochs, gradient_clipping=clipping, captured=True)

    twin_data, twin = module(cuda, once), network(cuda)
    optimizer = loss.configure_optimizers(ADAMW, twin)["optimizer"]
    step = loss.FusedMlpTrainingStep(twin, optimizer, gradient_clipping=clipping)
    dataset, tables = twin_data.train_dataset, twin_data.noiser.noise_scheduler.tables
    x0, a0, l0 = dataset[RELATIVE_COORDINATES], dataset[ATOM_TYPES], dataset[LATTICE_PARAMETERS]
    train_losses, valid_losses = [], []
    for epoch in range(epochs):
        permutation = twin_data.shuffle(epoch)
        call = 0 if once else epoch
        total = torch.zeros(1, dtype=torch.float64, device=cuda)
        for start in range(0, 160, 64):
            count = min(64, 160 - start)
            buffers = kernels.noise_training_batch(tables, x0, a0, l0, count, rows=permutation, row_offset=start,
                                                   rng=Rng(1234, call, 1, training.TRAIN_DRAW))
            out = step.step(training.noised_batch_dictionary(buffers, torch.zeros_like(buffers.x0)))
            total.add_(out["loss"].to(torch.float64), alpha=float(count))
        train_losses.append(float(total) / 160)
        valid_losses.append(validation_loss(twin, twin_data, epoch))
    assert same_parameters(net, twin)
    trained = list(zip(kernels.mlp_train_plan(net).parameters, kernels.mlp_train_plan(twin).parameters))
    assert len(trained) > 10          # (the conditional layers take no part in the unconditional step and hold no state)
    for p, q in trained:
        for key in ("exp_avg", "exp_avg_sq"):
            assert same_bits(history.optimizer.state[p][key], optimizer.state[q][key]), key
    assert torch.equal(history.optimizer.steps_taken()[0], optimizer.steps_taken()[0])
    assert int(optimizer.steps_taken()[0].max()) == 3 * epochs
    assert history["train_epoch_loss"] == train_losses and history["validation_epoch_loss"] == valid_losses
    assert history["learning_rate"] == [2e-3] * epochs
    kernels.raise_noising_status(data.noiser.status)


def _by_row(data, epoch, key):
    """A field of an epoch's training batches, put back in dataset order."""
    batches = list(data.train_batches(epoch))
    stacked = torch.cat([batch[key] for batch in batches])
    out = torch.empty_like(stacked)
    out[data._permutation] = stacked
    return out


def test_noise_once_at_setup(cuda):
    once, fresh = module(cuda, True), module(cuda, False)
    for key in (TIME_INDICES, NOISY_RELATIVE_COORDINATES):
        assert same_bits(_by_row(once, 0, key), _by_row(once, 3, key))
        assert not same_bits(_by_row(fresh, 0, key), _by_row(fresh, 3, key))
        assert same_bits(_by_row(once, 0, key), _by_row(fresh, 0, key))
        first, again = list(once.valid_batches(0)), list(once.valid_batches(3))
        assert all(same_bits(a[key], b[key]) for a, b in zip(first, again))
    # the shuffle is another one every epoch, the same one for the same epoch, and a permutation
    p0, p3 = once.shuffle(0).clone(), once.shuffle(3).clone()
    assert not torch.equal(p0, p3) and torch.equal(once.shuffle(0), p0) and torch.equal(p0.sort().values, torch.arange(160, device=cuda))
    assert [batch[RELATIVE_COORDINATES].shape[0] for batch in once.train_batches(0)] == [64, 64, 32]      # the tail is kept


def test_the_general_route_is_the_loop_of_optimisation_steps(cuda):
    hyper = dict(optimizer=dict(name="adam", learning_rate=1e-3))
    data, net = module(cuda), network(cuda)
    history = training.fit(net, data, hyper, 1, gradient_clipping=0.5, accumulate_grad_batches=2)      # accumulation: general
    twin_data, twin = module(cuda), network(cuda)
    optimizer = loss.configure_optimizers(hyper, twin)["optimizer"]
    total = torch.zeros(1, dtype=torch.float64, device=cuda)
    permutation = twin_data.shuffle(0)
    for index, start in enumerate(range(0, 160, 64)):
        batch = twin_data.noiser.noise(twin_data.train_dataset, rows=permutation, row_offset=start, batch_size=min(64, 160 - start),
                                       epoch=0)
        out = loss.optimisation_step(twin, batch, optimizer, batch_index=index, gradient_clipping=0.5, accumulate_grad_batches=2)
        total.add_(out["loss"].detach().to(torch.float64), alpha=float(batch[RELATIVE_COORDINATES].shape[0]))
    assert same_parameters(net, twin) and not same_parameters(net, network(cuda))
    assert history["train_epoch_loss"] == [float(total) / 160]
    assert history["validation_epoch_loss"] == [validation_loss(twin, twin_data, 0)]
    with pytest.raises(_hip.MdxError, match="accumulate_grad_batches"):
        training.fit(network(cuda), data, hyper, 1, accumulate_grad_batches=2, captured=True)


def test_the_schedulers_are_followed(cuda, monkeypatch):
    graphs = []
    graph_class = torch.cuda.CUDAGraph
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda *a, **k: (graphs.append(1), graph_class(*a, **k))[1])
    plateau = dict(optimizer=dict(name="adam", learning_rate=0.05), scheduler=dict(name="ReduceLROnPlateau", factor=0.5, patience=0))
    data, net = module(cuda, once=False), network(cuda)
    history = training.fit(net, data, plateau, 6, captured=True)
    rates = history["learning_rate"]
    print("ReduceLROnPlateau:", rates, history["validation_epoch_loss"])
    assert len(graphs) == 1                                        # one capture serves every learning rate
    # torch's own scheduler on the recorded metric gives the recorded rates
    dummy = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=0.05)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(dummy, factor=0.5, patience=0)
    expected = []
    for value in history["validation_epoch_loss"]:
        expected.append(dummy.param_groups[0]["lr"])
        scheduler.step(value)
    assert rates == expected and len(set(rates)) > 1
    # the captured route followed them: the general route on the same kernels (fused_training) ends with the same bits
    twin = network(cuda)
    twin.fused_training = True
    again = training.fit(twin, module(cuda, once=False), plateau, 6, captured=False)
    assert again["learning_rate"] == rates and same_parameters(net, twin)

    cosine = dict(optimizer=dict(name="adamw", learning_rate=1e-2), scheduler=dict(name="CosineAnnealingLR", T_max=4, eta_min=1e-4))
    history = training.fit(network(cuda), module(cuda), cosine, 5)
    dummy = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=1e-2)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(dummy, T_max=4, eta_min=1e-4)
    expected = []
    for _ in range(5):
        expected.append(dummy.param_groups[0]["lr"])
        dummy.step()
        scheduler.step()
    assert history["learning_rate"] == expected and expected[4] == 1e-4


def test_ten_epochs_learn(cuda):
    data, net = module(cuda), network(cuda)
    before = validation_loss(net, data, 0)
    history = training.fit(net, data, ADAMW, 10)
    print("validation loss before", before, "after", history["validation_epoch_loss"])
    assert history["validation_epoch_loss"][-1] < before and all(np.isfinite(history["train_epoch_loss"]))


def test_a_captured_epoch_does_no_host_work_between_its_batches(cuda, monkeypatch):
    data, net = module(cuda, train_dataset_size=288), network(cuda)        # 4 full batches and a tail of 32
    events = []
    call = _hip.call
    monkeypatch.setattr(kernels, "call", lambda name, *args: (events.append(name), call(name, *args))[1])
    for name in ("copy_", "item", "tolist", "cpu", "numpy"):
        original = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda original, name: lambda self, *a, **k: (events.append(name), original(self, *a, **k))[1])(original, name))
    replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (events.append("replay"), replay(self))[1])
    training.fit(net, data, ADAMW, 2, captured=True)
    assert events.count("replay") == 8 and events.count("mdx_noise_training_batch") >= 2
    replays = [k for k, name in enumerate(events) if name == "replay"]
    for epoch_replays in (replays[:4], replays[4:]):
        assert events[epoch_replays[0]:epoch_replays[-1] + 1] == ["replay"] * 4          # nothing between the first and the last
    # one host read per epoch, and it is the epoch's sums; no copy from the host anywhere in the second epoch
    assert events.count("tolist") == 2 and events.count("item") == 0 and events.count("cpu") == 0 and events.count("numpy") == 0
    assert "copy_" not in events[replays[4]:]


def test_fit_reports_a_dataset_out_of_range_and_a_module_needs_both_datasets(cuda):
    parameters = gaussian_parameters()
    good = module(cuda)
    train = {key: t.clone() for key, t in good.train_dataset.items()}
    train[ATOM_TYPES][5, 1] = 1                    # MASK: not an atom type of a clean structure
    data = training.DeviceDataModule(train, good.valid_dataset, parameters.noise_parameters, num_atom_types=1, spatial_dimension=3,
                                     batch_size=64, seed=3, device=cuda)
    for captured in (True, False):
        with pytest.raises(IndexError, match="outside its range"):
            training.fit(network(cuda), data, ADAMW, 2, captured=captured)
        assert int(data.noiser.status.item()) == 0          # raised once, cleared
    history = training.fit(network(cuda), good, ADAMW, 1)
    assert set(history) == {"train_epoch_loss", "validation_epoch_loss", "learning_rate"} and all(len(v) == 1 for v in history.values())
    assert history.lr_scheduler is None and history.optimizer.param_groups[0]["lr"] == 2e-3
    with pytest.raises(ValueError, match="a training AND a validation dataset"):
        training.DeviceDataModule(train, None, parameters.noise_parameters, num_atom_types=1, spatial_dimension=3, batch_size=64,
                                  device=cuda)
    # a 64-bit seed: the shuffle's own seed stays inside what a generator takes
    big = training.DeviceDataModule(good.train_dataset, good.valid_dataset, parameters.noise_parameters, num_atom_types=1,
                                    spatial_dimension=3, batch_size=64, seed=2**63 - 1, device=cuda)
    assert torch.equal(big.shuffle(2).sort().values, torch.arange(160, device=cuda))
