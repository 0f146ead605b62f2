"""mdx_node_mlp_rows_indexed: the whole node MLP on rows whose h half is class_rows[row_class[r]] -- the operand and the residual
read through the index -- against mdx_node_mlp_rows_split on the materialised h = class_rows[row_class]: the same bits in out
and in the next layer's projections.  130 rows = one full 128-row tile and a remainder of 2."""
import pytest
import torch

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "f16x3", "f16x3_32x32"]


def _pack(device, H, precision, project, seed):
    torch.manual_seed(seed)
    layers = [torch.nn.Linear(2 * H, H), torch.nn.Linear(H, H), torch.nn.Linear(H, H)]
    mods = [m.to(device) for m in layers]
    assert kernels.NodeMlpPack.supported(mods)
    proj_w = (torch.randn(2 * H, H) * (1.5 / H ** 0.5)).to(device) if project else None
    pack = kernels.NodeMlpPack(mods, precision, next_projection=proj_w)
    assert pack.projects == project
    return pack, mods


def _both(pack, class_rows, row_class, agg, residual):
    status = torch.zeros(1, dtype=torch.int32, device=agg.device)
    want = kernels.node_mlp_rows(pack, class_rows[row_class].contiguous(), residual, status=status, agg=agg)
    got = kernels.node_mlp_rows(pack, class_rows, residual, status=status, agg=agg, row_class=row_class)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return (want, got) if pack.projects else ((want,), (got,))


def _classes(kind, M, g):
    if kind == "all_present":
        row_class = torch.randint(0, 3, (M,), generator=g)
        row_class[:3] = torch.arange(3)
        row_class[-2:] = torch.tensor([2, 1])             # the remainder rows read other classes than row 0
        return row_class
    return torch.cat([torch.full((128,), 1), torch.tensor([0, 2])])      # the full tile entirely of one class


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("project", [True, False])
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("kind", ["all_present", "one_class_tile"])
def test_indexed_equals_materialised(cuda, precision, project, residual, kind):
    H, M = 32, 130
    g = torch.Generator().manual_seed(7)
    pack, _ = _pack(cuda, H, precision, project, seed=5)
    class_rows = torch.randn(3, H, generator=g).to(cuda)
    agg = torch.randn(M, H, generator=g).to(cuda)
    row_class = _classes(kind, M, g).to(cuda)
    want, got = _both(pack, class_rows, row_class, agg, residual)
    for w, t in zip(want, got):
        assert w.shape == t.shape and torch.equal(w, t)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_indexed_equals_materialised_at_hidden_256(cuda, precision):
    H, M = 256, 130
    g = torch.Generator().manual_seed(9)
    pack, _ = _pack(cuda, H, precision, True, seed=6)
    class_rows = torch.randn(2, H, generator=g).to(cuda)
    agg = torch.randn(M, H, generator=g).to(cuda)
    row_class = torch.randint(0, 2, (M,), generator=g).to(cuda)
    want, got = _both(pack, class_rows, row_class, agg, True)
    for w, t in zip(want, got):
        assert torch.equal(w, t)


@pytest.mark.parametrize("bad", [3, -1])
def test_class_outside_the_rows_reads_row_0_and_reports(cuda, bad):
    H, M = 32, 130
    g = torch.Generator().manual_seed(11)
    pack, _ = _pack(cuda, H, "f16x3", True, seed=5)
    class_rows = torch.randn(3, H, generator=g).to(cuda)
    agg = torch.randn(M, H, generator=g).to(cuda)
    row_class = torch.randint(0, 3, (M,), generator=g)
    row_class[129] = bad                                   # in the ragged last tile
    status = torch.zeros(1, dtype=torch.int32, device=cuda)
    got, proj = kernels.node_mlp_rows(pack, class_rows, True, status=status, agg=agg, row_class=row_class.to(cuda))   # MDX_OK
    torch.cuda.synchronize()
    assert int(status.item()) == _hip.STATUS_EGNN_TABLE
    row_class[129] = 0
    status.zero_()
    want, want_proj = kernels.node_mlp_rows(pack, class_rows[row_class.to(cuda)].contiguous(), True, status=status, agg=agg)
    assert int(status.item()) == 0 and torch.equal(got, want) and torch.equal(proj, want_proj)
