"""The first layer's distance table kept on the device under a sigma key (kernels.EgnnTableMemo): reuse
on (EGNNScoreNetwork.first_layer_table_reuse, the default) against off -- every forward builds -- bit for bit, and the device's
own build counter for what was and was not rebuilt.  Small shapes: B = 3, N = 8, radius graph, 2 graph layers of width 32, 4 and 9
class pairs, both arithmetic modes; one case at the benchmarked width 256."""
import pytest
import torch

import nets

pytestmark = pytest.mark.gpu

CASES = [(32, 1, "f16x3"), (32, 1, "f32"), (32, 2, "f16x3"), (32, 2, "f32"), (256, 1, "f16x3")]


def _batch(device, num_atom_types, sigma, seed, B=3, N=8):
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import (AXL, CARTESIAN_FORCES, NOISE,
                                                                              NOISY_AXL_COMPOSITION, TIME)
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(B, N, 3, generator=g)
    A = torch.randint(0, num_atom_types + 1, (B, N), generator=g)            # MASK included
    L = torch.tensor([10.86, 10.86, 10.86, 0.0, 0.0, 0.0]).repeat(B, 1)
    sig = sigma.reshape(B, 1) if isinstance(sigma, torch.Tensor) else torch.full((B, 1), float(sigma))
    return {NOISY_AXL_COMPOSITION: AXL(A=A.to(device), X=X.to(device), L=L.to(device)), TIME: torch.full((B, 1), 0.5).to(device),
            NOISE: sig.to(device), CARTESIAN_FORCES: torch.zeros(B, N, 3, device=device)}


def _net(device, hidden, num_atom_types, precision, reuse, seed=11):
    net = nets.egnn_net(num_atom_types, "radial_cutoff", 7.5, hidden=hidden, n_layers=2, n_hidden=2, seed=seed).to(device)
    net.edge_chain_precision = precision
    net.first_layer_table = "on"                      # ("auto" declines grids this small)
    net.first_layer_table_reuse = reuse
    return net


def _forward(net, batch):
    with torch.no_grad():
        out = net(batch, conditional=False)
    word = int(net.graph_status.item())
    net.graph_status.zero_()
    return out, word


def _same(a, b):
    return torch.equal(a.X, b.X) and torch.equal(a.A, b.A)


@pytest.mark.parametrize("hidden,num_atom_types,precision", CASES)
def test_reuse_at_equal_sigma_and_rebuild_at_a_new_one(cuda, hidden, num_atom_types, precision):
    on, off = (_net(cuda, hidden, num_atom_types, precision, reuse) for reuse in (True, False))
    first, second, third = (_batch(cuda, num_atom_types, s, seed) for s, seed in ((0.05, 1), (0.05, 2), (0.11, 3)))
    assert on.table_builds() == 0
    _, word = _forward(on, first)
    assert word == 0 and on.table_builds() == 1
    got, word = _forward(on, second)                      # equal sigma, other coordinates and types: the table is reused
    assert word == 0 and on.table_builds() == 1
    for batch in (first, second):
        want, word = _forward(off, batch)
        assert word == 0
    assert off.table_builds() == 2                        # reuse off: every forward builds
    assert _same(got, want)
    got, word = _forward(on, third)                       # another sigma: one more build
    assert word == 0 and on.table_builds() == 2
    want, _ = _forward(off, third)
    assert _same(got, want)
    got, _ = _forward(on, second)                         # and back: a key holds one sigma
    assert on.table_builds() == 3
    want, _ = _forward(off, second)
    assert _same(got, want)


@pytest.mark.parametrize("hidden,num_atom_types,precision", [(32, 2, "f16x3"), (32, 1, "f32")])
def test_whatever_else_the_table_depends_on_resets_the_key(cuda, hidden, num_atom_types, precision):
    """After each change the next forward builds again (the counter) and equals a freshly made network in the same state."""
    net = _net(cuda, hidden, num_atom_types, precision, True)
    batch, other = _batch(cuda, num_atom_types, 0.07, 5), _batch(cuda, num_atom_types, 0.07, 6)
    _forward(net, batch)
    builds = net.table_builds()
    assert builds == 1

    def fresh(change):
        made = _net(cuda, hidden, num_atom_types, precision, True)
        change(made)
        return _forward(made, other)[0]

    def scale_first_weight(n):
        with torch.no_grad():
            n.egnn.graph_layers[0].message_mlp[0].weight.mul_(1.25)      # in place: the parameter's version moves

    def scale_embedding(n):
        with torch.no_grad():
            n.egnn.embedding_in.weight.mul_(0.75)

    changes = []
    for change in (scale_first_weight, scale_embedding):
        changes.append(change)
        change(net)
        got, word = _forward(net, other)
        assert word == 0 and net.table_builds() == builds + 1
        builds += 1
        assert _same(got, fresh(lambda n: [c(n) for c in changes]))
        _forward(net, batch)
        assert net.table_builds() == builds               # (and the new table is kept in its turn)

    # the other precision and back (what the generator does around an f16-range report)
    elsewhere = "f32" if precision != "f32" else "f16x3"
    net.edge_chain_precision = elsewhere
    _forward(net, other)
    assert net.table_builds() == builds + 1
    net.edge_chain_precision = precision
    got, _ = _forward(net, other)
    assert net.table_builds() == builds + 2
    builds += 2
    assert _same(got, fresh(lambda n: [c(n) for c in changes]))

    # the activation exponents
    for call in ("begin_f16_range_fallback", "adapt_f16_range", "reset_f16_range"):
        getattr(net, call)()
        got, _ = _forward(net, other)
        assert net.table_builds() == builds + 1, call
        builds += 1
    assert _same(got, fresh(lambda n: [c(n) for c in changes]))            # (reset_f16_range: a fresh network's exponents)

    # the table mode
    net.first_layer_table = "off"
    _forward(net, other)
    assert net.table_builds() == builds
    net.first_layer_table = "on"
    got, _ = _forward(net, other)
    assert net.table_builds() == builds + 1
    assert _same(got, fresh(lambda n: [c(n) for c in changes]))


@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_nonuniform_sigma_on_a_reused_table_is_reported(cuda, precision):
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    net = _net(cuda, 32, 1, precision, True)
    _, word = _forward(net, _batch(cuda, 1, 0.05, 1))
    assert word == 0 and net.table_builds() == 1
    sigma = torch.tensor([0.05, 0.05, 0.2])                # sigma[0] is the key's: nothing is built, the check still runs
    _, word = _forward(net, _batch(cuda, 1, sigma, 2))
    assert word & _hip.STATUS_EGNN_TABLE and net.table_builds() == 1
    _, word = _forward(net, _batch(cuda, 1, 0.05, 3))      # the table itself was never in doubt
    assert word == 0 and net.table_builds() == 1


def test_a_failed_build_leaves_no_key(cuda):
    """The steep first layer of tests/test_egnn_first_layer_table_gpu.py::test_steep_first_layer_falls_back_once at width 32:
    the midpoint check fails, nothing counts as built, and the next forward at the same sigma builds and reports again."""
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    net = _net(cuda, 32, 1, "f32", True)
    with torch.no_grad():
        first = net.egnn.graph_layers[0].message_mlp[0]
        first.weight[:, 2 * 32] *= 1.0e4                   # w_radial
        first.bias.copy_(-first.weight[:, 2 * 32] * torch.linspace(0.5, 11.5, 32, device=cuda))
    for seed in (1, 2):
        _, word = _forward(net, _batch(cuda, 1, 0.05, seed))
        assert word & _hip.STATUS_EGNN_TABLE
        assert net.table_builds() == 0
        memos = list(net.egnn.graph_layers[0]._table_memos.values())
        assert len(memos) == 1 and int(memos[0].key[0].item()) == kernels.TABLE_NO_KEY
        assert float(memos[0].worst.item()) > kernels.TABLE_TOLERANCE          # (each forward ran the midpoint check)
        memos[0].worst.zero_()
