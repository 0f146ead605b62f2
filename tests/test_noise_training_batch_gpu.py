"""mdx_noise_training_batch on the GPU: the reference's recorded transform bit for bit (tests/golden/denoising_loss/*.npz), the
device RNG against the same draws made by mdx_rng_fill and the oracle's Philox, the gather by rows and cursor, the fixed lattice,
the ends of the time axis, batch sizes 1 and 8192, a captured launch, and the refusals.  Everything is compared bit for bit."""
import numpy as np
import pytest
import torch

from denoising_loss_cases import CASES, fixture
from training_cases import fixture_dataset, fixture_schedule, random_dataset, same_bits, time_index

from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
from diffusion_for_multi_scale_molecular_dynamics_amd._hip import MdxError, Rng

pytestmark = pytest.mark.gpu

SEED = 20251021
FIELDS = kernels.NoisedTrainingBatch._fields


def _status(cuda):
    return torch.zeros(1, dtype=torch.int32, device=cuda)


def _equal(a: kernels.NoisedTrainingBatch, b: kernels.NoisedTrainingBatch, skip=()):
    for name in FIELDS:
        if name not in skip:
            assert same_bits(getattr(a, name), getattr(b, name)), name


def _rows_of(out: kernels.NoisedTrainingBatch, index) -> kernels.NoisedTrainingBatch:
    return kernels.NoisedTrainingBatch(*(t[index] for t in out))


@pytest.mark.parametrize("case", CASES)
def test_the_recorded_transform_bit_for_bit(case, cuda):
    g = fixture(case)
    sched, (x0, a0, l0) = fixture_schedule(case, cuda), fixture_dataset(case, cuda)
    t = lambda key: torch.from_numpy(np.ascontiguousarray(g[key])).to(cuda)       # noqa: E731
    status = _status(cuda)
    out = kernels.noise_training_batch(sched, x0, a0, l0, x0.shape[0], time_indices=t("time_indices"), z=t("draw_x"), u=t("draw_a"),
                                       z_lattice=t("draw_l"), status=status)
    C = sched.num_classes
    assert int(status.item()) == (_hip.STATUS_NOISING_INDEX if bool((a0 >= C - 1).any()) else 0)
    assert same_bits(out.xt, t("transform_xt")) and same_bits(out.at, t("transform_at")) and same_bits(out.lt, t("transform_lt"))
    assert same_bits(out.time, t("time")[:, 0]) and same_bits(out.sigma, t("noise")[:, 0])
    indices = t("time_indices")
    assert same_bits(out.time_indices, indices)
    assert same_bits(out.q, sched.q_matrix[indices]) and same_bits(out.q_bar, sched.q_bar_matrix[indices])
    assert same_bits(out.q_bar_tm1, sched.q_bar_tm1_matrix[indices])
    assert same_bits(out.x0, x0) and same_bits(out.a0, a0) and same_bits(out.l0, l0)


def _predrawn(oracle, sched, call, draw, rows, atoms, dimension, dataset_rows, cuda):
    """The four draws of the device path, made as arrays: mdx_rng_fill at the items of every dataset row, the time index on the
    oracle's Philox; then picked at `rows`."""
    C, nl = sched.num_classes, dimension * (dimension + 1) // 2
    z = kernels.rng_fill(kernels.RNG_NORMAL, SEED, call, draw, _hip.TAG_TRAIN_Z, dataset_rows * atoms, dimension, cuda)
    u = kernels.rng_fill(kernels.RNG_UNIFORM, SEED, call, draw, _hip.TAG_TRAIN_U, dataset_rows * atoms, C, cuda)
    z_lattice = kernels.rng_fill(kernels.RNG_NORMAL, SEED, call, draw, _hip.TAG_TRAIN_LATTICE, dataset_rows, nl, cuda)
    indices = torch.tensor([time_index(oracle, SEED, call, draw, int(r), sched.total_time_steps) for r in rows.tolist()],
                           dtype=torch.int64, device=cuda)
    return dict(time_indices=indices, z=z.reshape(dataset_rows, atoms, dimension)[rows].contiguous(),
                u=u.reshape(dataset_rows, atoms, C)[rows].contiguous(), z_lattice=z_lattice[rows].contiguous())


@pytest.mark.parametrize("case", ["c2_n1_d1_p1", "c3_n5_d3_p6", "c8_n65_d2_p3"])
def test_the_device_rng_is_the_predrawn_path_on_the_same_draws(case, cuda, oracle):
    sched, (x0, a0, l0) = fixture_schedule(case, cuda), fixture_dataset(case, cuda)
    M, N, d = x0.shape
    rows = torch.randperm(M, generator=torch.Generator().manual_seed(3)).to(cuda)
    call, draw = 3, 1
    device_path = kernels.noise_training_batch(sched, x0, a0, l0, M, rows=rows, rng=Rng(SEED, call, 1, draw))
    predrawn = kernels.noise_training_batch(sched, x0, a0, l0, M, rows=rows, **_predrawn(oracle, sched, call, draw, rows, N, d, M, cuda))
    _equal(device_path, predrawn)
    other_call = kernels.noise_training_batch(sched, x0, a0, l0, M, rows=rows, rng=Rng(SEED, call + 1, 1, draw))
    assert not same_bits(other_call.xt, device_path.xt)          # a negative control: another call, other noise


def _small(cuda, T=16, C=3, M=37, N=5, d=3):
    sched = kernels.noise_schedule_build(T, "exponential", 1e-5, 1e-3, 0.5, 2e-7, C, cuda)
    return sched, random_dataset(M, N, d, C, cuda)


def test_gather_and_cursor_give_each_row_its_own_bits(cuda):
    sched, (x0, a0, l0) = _small(cuda)
    M, B, rng = 37, 12, Rng(SEED, 2, 1, 0)
    whole = kernels.noise_training_batch(sched, x0, a0, l0, M, rng=rng)          # un-gathered: structure r is row r
    permutation = torch.randperm(M, generator=torch.Generator().manual_seed(11)).to(cuda)
    cursor, status = torch.zeros(1, dtype=torch.int32, device=cuda), _status(cuda)
    for c in (0, 1, 2):
        cursor.fill_(c)
        out = kernels.noise_training_batch(sched, x0, a0, l0, B, rows=permutation, cursor=cursor, rng=rng, status=status)
        _equal(out, _rows_of(whole, permutation[c * B:(c + 1) * B]))
    tail = kernels.noise_training_batch(sched, x0, a0, l0, 1, rows=permutation, row_offset=3 * B, rng=rng, status=status)
    _equal(tail, _rows_of(whole, permutation[3 * B:]))
    # another batch size and another order: the same bits per dataset row
    cursor.fill_(3)
    five = kernels.noise_training_batch(sched, x0, a0, l0, 5, rows=permutation, cursor=cursor, rng=rng, status=status)
    _equal(five, _rows_of(whole, permutation[15:20]))
    backwards = permutation.flip(0).contiguous()
    out = kernels.noise_training_batch(sched, x0, a0, l0, M, rows=backwards, rng=rng, status=status)
    _equal(out, _rows_of(whole, backwards))
    assert int(status.item()) == 0
    # the draws are real ones: rows differ from one another, indices cover more than one value
    assert len(set(whole.time_indices.tolist())) > 4 and not same_bits(whole.xt[0], whole.xt[1])


def test_a_fixed_lattice_passes_the_lattice_through(cuda):
    sched, (x0, a0, l0) = _small(cuda)
    rows = torch.arange(36, -1, -3, device=cuda)
    free = kernels.noise_training_batch(sched, x0, a0, l0, rows.numel(), rows=rows, rng=Rng(SEED, 0, 1, 0))
    fixed = kernels.noise_training_batch(sched, x0, a0, l0, rows.numel(), rows=rows, rng=Rng(SEED, 0, 1, 0),
                                         use_fixed_lattice_parameters=True)
    assert same_bits(fixed.lt, l0[rows]) and not same_bits(free.lt, l0[rows])
    _equal(fixed, free, skip=("lt",))
    # without any lattice draw: the pre-drawn path needs no z_lattice
    predrawn = kernels.noise_training_batch(sched, x0, a0, l0, rows.numel(), rows=rows, time_indices=free.time_indices,
                                            z=torch.zeros_like(free.xt), u=torch.full((rows.numel(), 5, 3), 0.5, device=cuda),
                                            use_fixed_lattice_parameters=True)
    assert same_bits(predrawn.lt, l0[rows]) and same_bits(predrawn.xt, x0[rows])


def test_the_ends_of_the_time_axis(cuda, oracle):
    sched, (x0, a0, l0) = _small(cuda)
    T = sched.total_time_steps
    indices = torch.tensor([0, T - 1] * 6, dtype=torch.int64, device=cuda)
    g = torch.Generator().manual_seed(2)
    z, u, zl = torch.randn(12, 5, 3, generator=g).to(cuda), torch.rand(12, 5, 3, generator=g).to(cuda), torch.randn(12, 6, generator=g).to(cuda)
    status = _status(cuda)
    out = kernels.noise_training_batch(sched, x0, a0, l0, 12, time_indices=indices, z=z, u=u, z_lattice=zl, status=status)
    assert int(status.item()) == 0
    assert same_bits(out.time, sched.time[indices]) and same_bits(out.sigma, sched.sigma[indices])
    assert same_bits(out.q, sched.q_matrix[indices]) and same_bits(out.q_bar_tm1, sched.q_bar_tm1_matrix[indices])
    # the stand-alone noisers on the same operands (the reference's own signatures): the same bits
    sigmas = sched.sigma[indices]
    assert same_bits(out.xt, kernels.noise_relative_coordinates(x0[:12].contiguous(), z, sigmas.reshape(-1, 1, 1).expand(12, 5, 3).contiguous()))
    q_bar = sched.q_bar_matrix[indices].unsqueeze(1).expand(12, 5, 3, 3).contiguous()
    assert same_bits(out.at, kernels.noise_atom_types(a0[:12].contiguous(), q_bar, u))
    sigmas_n = (sigmas.reshape(-1, 1) / torch.full((12, 6), kernels.root_of_atom_count(5, 3), device=cuda)).contiguous()
    assert same_bits(out.lt, kernels.noise_lattice_parameters(l0[:12].contiguous(), zl, sigmas_n))
    # the device draw reaches both ends of [0, T) over the rows of a larger dataset, and never leaves it
    big = random_dataset(4096, 1, 1, 3, cuda)
    drawn = kernels.noise_training_batch(sched, *big, 4096, rng=Rng(SEED, 0, 1, 0)).time_indices
    assert int(drawn.min()) == 0 and int(drawn.max()) == T - 1
    assert drawn[:64].tolist() == [time_index(oracle, SEED, 0, 0, r, T) for r in range(64)]


def test_batch_sizes_one_and_8192_against_twelve_at_a_time(cuda):
    M, N, d, C = 8192, 2, 1, 3
    sched = kernels.noise_schedule_build(16, "exponential", 1e-5, 1e-3, 0.5, 2e-7, C, cuda)
    x0, a0, l0 = random_dataset(M, N, d, C, cuda)
    rng, status = Rng(SEED, 1, 1, 0), _status(cuda)
    whole = kernels.noise_training_batch(sched, x0, a0, l0, M, rng=rng, status=status)
    pieces = kernels.noised_training_batch_buffers(M, N, d, C, cuda)
    for start in range(0, M, 12):
        count = min(12, M - start)
        kernels.noise_training_batch(sched, x0, a0, l0, count, row_offset=start, rng=rng, status=status,
                                     out=kernels.NoisedTrainingBatch(*(t[start:start + count] for t in pieces)))
    _equal(whole, pieces)
    one = kernels.noise_training_batch(sched, x0, a0, l0, 1, row_offset=4097, rng=rng, status=status)
    _equal(one, _rows_of(pieces, slice(4097, 4098)))
    assert int(status.item()) == 0


def test_captured_and_replayed_with_the_words_rewritten(cuda):
    sched, (x0, a0, l0) = _small(cuda)
    B = 12
    permutation = torch.randperm(37, generator=torch.Generator().manual_seed(4)).to(cuda)
    cursor = torch.zeros(1, dtype=torch.int32, device=cuda)
    epoch = torch.zeros(1, dtype=torch.int32, device=cuda)
    out = kernels.noised_training_batch_buffers(B, 5, 3, 3, cuda)
    request = Rng(SEED, 0, 1, 0, 0, epoch.data_ptr())
    kernels.noise_training_batch(sched, x0, a0, l0, B, rows=permutation, cursor=cursor, rng=request, out=out)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kernels.noise_training_batch(sched, x0, a0, l0, B, rows=permutation, cursor=cursor, rng=request, out=out)
    for c, e in ((0, 0), (2, 0), (1, 5), (0, 5)):
        cursor.fill_(c)
        epoch.fill_(e)
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = kernels.noise_training_batch(sched, x0, a0, l0, B, rows=permutation, row_offset=c * B, rng=Rng(SEED, e, 1, 0))
        _equal(out, eager)


def test_negative_controls(cuda):
    sched, (x0, a0, l0) = _small(cuda)
    M, rng = 37, Rng(SEED, 0, 1, 0)
    good = kernels.noise_training_batch(sched, x0, a0, l0, 4, rng=rng)
    # a row index equal to M: reported, clamped to the last row
    status = _status(cuda)
    rows = torch.tensor([0, M, 2, 3], dtype=torch.int64, device=cuda)
    out = kernels.noise_training_batch(sched, x0, a0, l0, 4, rows=rows, rng=rng, status=status)
    assert int(status.item()) == _hip.STATUS_NOISING_INDEX
    assert same_bits(out.x0[1], x0[M - 1]) and same_bits(out.x0[0], good.x0[0]) and same_bits(out.xt[2:], good.xt[2:])
    with pytest.raises(IndexError, match="outside its range"):
        kernels.raise_noising_status(status)
    assert int(status.item()) == 0
    # a position past the end of `rows` (a cursor that ran on): reported too, nothing read past the array
    cursor = torch.full((1,), 9, dtype=torch.int32, device=cuda)
    kernels.noise_training_batch(sched, x0, a0, l0, 4, rows=rows, cursor=cursor, rng=rng, status=status)
    assert int(status.item()) == _hip.STATUS_NOISING_INDEX
    status.zero_()
    # an atom type equal to C - 1 (MASK) in the dataset: reported; the MASK row of Qbar is a row of the table
    masked = a0.clone()
    masked[1, 2] = 2
    out = kernels.noise_training_batch(sched, x0, masked, l0, 4, rng=rng, status=status)
    assert int(status.item()) == _hip.STATUS_NOISING_INDEX and int(out.at[1, 2]) == 2 and same_bits(out.at[0], good.at[0])
    status.zero_()
    masked[1, 2] = 7                    # outside the table altogether: clamped, reported
    kernels.noise_training_batch(sched, x0, masked, l0, 4, rng=rng, status=status)
    assert int(status.item()) == _hip.STATUS_NOISING_INDEX
    # a given time index equal to T
    status.zero_()
    indices = torch.tensor([0, 16, 1, 2], dtype=torch.int64, device=cuda)
    z, u, zl = torch.zeros(4, 5, 3, device=cuda), torch.full((4, 5, 3), 0.5, device=cuda), torch.zeros(4, 6, device=cuda)
    out = kernels.noise_training_batch(sched, x0, a0, l0, 4, time_indices=indices, z=z, u=u, z_lattice=zl, status=status)
    assert int(status.item()) == _hip.STATUS_NOISING_INDEX and int(out.time_indices[1]) == 15
    # M N >= 2^32 is refused; called with an EMPTY batch, so that nothing can be launched whatever the entry answers (the
    # size check comes before the empty batch's MDX_OK); host tensors are refused too
    import ctypes as C
    p = C.c_void_p(64)
    entry = _hip.lib().mdx_noise_training_batch
    arguments = lambda rows_total, atoms: (C.byref(sched.c_struct), p, p, p, rows_total, None, 0, 0, None, None, None, None, None, rng,  # noqa: E731
                                           0, atoms, 3, 1.0, 0, p, p, p, p, p, p, p, p, p, p, p, p, None, None)
    assert entry(*arguments(2**29, 8)) == _hip.ERR_INVALID_ARG and entry(*arguments(2**32, 1)) == _hip.ERR_INVALID_ARG
    assert entry(*arguments(2**29 - 1, 8)) == _hip.MDX_OK
    with pytest.raises(MdxError, match="no CPU fallback"):
        kernels.noise_training_batch(sched, x0.cpu(), a0, l0, 4, rng=rng)
    with pytest.raises(MdxError, match="no CPU fallback"):
        kernels.noise_training_batch(sched, x0, a0, l0, 4, rows=rows.cpu(), rng=rng)
    with pytest.raises(ValueError, match="needs the device RNG"):
        kernels.noise_training_batch(sched, x0, a0, l0, 4)
