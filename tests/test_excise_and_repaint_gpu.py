"""GPU tests of the excise-and-repaint path: the excision kernel against the reference's recorded environments and against the
numpy restatement of tests/excise_cases.py, the per-sample repaint kernel against mdx_repaint_constrained_rows, the batched
generator against one ConstrainedLangevinGenerator per environment, and the sample maker against the reference's samples
(tests/golden/excise_and_repaint/, made by tests/golden/make_golden_excise_and_repaint.py).

Bars.  Indices, counts, atom types and keep masks: exact.  Constrained coordinates: 2^-23 absolute (one float32 ulp at 1; both
sides compute in binary64 in the same order and round once, so 0 is expected).  Trajectories: 1e-5 relative L2 on the torus, the
project's parity bar.  The observed maxima are printed (run with -s) and recorded in profiles/r10_excise_and_repaint.md."""
import numpy as np
import pytest
import torch

import excise_cases as ec
import nets
from conftest import load_golden, torus_rel_l2

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
PARITY = 1e-5


def _kernels():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip, kernels
    return kernels, _hip


def _axl():
    from diffusion_for_multi_scale_molecular_dynamics_amd.namespace import AXL
    return AXL


def _launch(cuda, x, sides, central, new_sides=None, capacity=None, status=None, **mode):
    """kernels.excise_environments on numpy inputs -> numpy (source, constrained x, counts)."""
    kernels, _ = _kernels()
    dev = lambda v, dtype: torch.tensor(np.asarray(v), dtype=dtype, device=cuda)      # noqa: E731
    source, cx, counts = kernels.excise_environments(
        dev(x, torch.float64), dev(sides, torch.float64), dev(central, torch.int64),
        new_box_sides=None if new_sides is None else dev(new_sides, torch.float64), capacity=capacity, status=status, **mode)
    return source.cpu().numpy(), cx.cpu().numpy(), counts.cpu().numpy()


MODES = {"spherical": dict(radial_cutoff=ec.RADIAL_CUTOFF), "nearest_neighbors": dict(number_of_neighbors=ec.NUMBER_OF_NEIGHBORS)}


# ------------------------------------------------------------------------------------------------------------------
# 1. the excision kernel against the reference
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(MODES))
def test_excision_against_the_reference(cuda, name):
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.excisor import excisor_factory as ef
    g, frame = load_golden(f"excise_and_repaint/{name}.npz"), load_golden("excise_and_repaint/frame.npz")
    count = g["count"]
    assert list(count) == ([4, 4, 5] if name == "spherical" else [5, 5, 5])
    source, cx, counts = _launch(cuda, frame["X"], frame["L"][:3], ec.CENTRAL_ATOMS, new_sides=[ec.NEW_BOX] * 3, capacity=8,
                                 **MODES[name])
    assert np.array_equal(counts, count) and counts.dtype == np.int32 and cx.dtype == np.float32
    worst = 0.0
    for e, k in enumerate(count):
        assert np.array_equal(source[e, :k], g["source"][e, :k]), (name, e)
        assert not source[e, k:].any() and not cx[e, k:].any()                        # zero padding up to the capacity
        worst = max(worst, float(np.abs(cx[e, :k].astype(np.float64) - g["X_constraint"][e, :k].astype(np.float64)).max()))
    print(f"excision vs the reference, {name}: max |x - x_ref| = {worst:.3e}")
    assert worst <= ULP
    # the excisor objects: numpy structures, as the reference returns them
    algorithm = dict(spherical=dict(algorithm="spherical_cutoff", radial_cutoff=ec.RADIAL_CUTOFF),
                     nearest_neighbors=dict(algorithm="nearest_neighbors", number_of_neighbors=ec.NUMBER_OF_NEIGHBORS))[name]
    excisor = ef.create_excisor(ef.create_excisor_parameters(algorithm))
    structure = _axl()(A=frame["A"], X=frame["X"], L=frame["L"])
    centred, indices = excisor.excise_environments(structure, np.array(ec.CENTRAL_ATOMS))
    raw, _ = excisor.excise_environments(structure, np.array(ec.CENTRAL_ATOMS), center_atoms=False)
    assert indices == [0, 0, 0] and len(centred) == 3
    for e, k in enumerate(count):
        assert np.array_equal(centred[e].X, g["X_centred"][e, :k]) and centred[e].X.dtype == np.float64
        assert np.array_equal(raw[e].X, g["X_raw"][e, :k]) and np.array_equal(raw[e].A, g["A"][e, :k])
        assert np.array_equal(centred[e].L, frame["L"])
    one, index = excisor._excise_one_environment(structure, ec.CENTRAL_ATOMS[1])
    assert index == 0 and np.array_equal(one.X, g["X_raw"][1, :count[1]])
    assert excisor.excise_environments(structure, np.array([], dtype=np.int64)) == ([], [])


# ------------------------------------------------------------------------------------------------------------------
# 2. the excision kernel against the restatement
# ------------------------------------------------------------------------------------------------------------------
def _compare_with_restatement(cuda, x, sides, central, new_sides=None, **mode):
    n = len(x)
    source, cx, counts = _launch(cuda, x, sides, central, new_sides=new_sides, **mode)
    worst = 0.0
    for e, c in enumerate(central):
        order, want, outside = ec.excise(x, sides, c, new_sides=new_sides, **mode)
        assert not outside
        assert counts[e] == len(order) and np.array_equal(source[e, :len(order)], order), (n, mode, e)
        assert not source[e, len(order):].any() and not cx[e, len(order):].any()
        worst = max(worst, float(np.abs(cx[e, :len(order)].astype(np.float64) - want.astype(np.float32).astype(np.float64)).max()))
    assert worst <= ULP, worst
    return worst


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("n", [1, 5, 63, 300])
def test_excision_against_the_restatement(cuda, n, d):
    rng = np.random.default_rng(100 * n + d)
    x = rng.random((n, d))
    x[0] = 0.98                                           # the first central atom's environment straddles the cell boundary
    sides = np.array([9.0, 10.0, 11.0])[:d]
    central = sorted({0, n // 2, n - 1})
    radius = 0.3 * sides.min() if n < 300 else 2.0
    new_sides = 2.0 * radius + 0.5 + np.zeros(d)          # every member lies within `radius` of the centre: inside
    worst = _compare_with_restatement(cuda, x, sides, central, new_sides=new_sides, radial_cutoff=radius)
    for k in (1, max(1, n - 1), n + 3):                   # k >= N - 1: the whole structure, whatever k
        worst = max(worst, _compare_with_restatement(cuda, x, sides, central, number_of_neighbors=k))
    print(f"excision vs the restatement, N = {n}, d = {d}: max |x - x_ref| = {worst:.3e}")


def test_excision_status_codes(cuda):
    kernels, _hip = _kernels()
    frame = load_golden("excise_and_repaint/frame.npz")
    x, sides = frame["X"], frame["L"][:3]

    def word(**kw):
        status = torch.zeros(1, dtype=torch.int32, device=cuda)
        out = _launch(cuda, x, sides, status=status, **kw)
        return int(status.item()), out

    bits, (source, cx, counts) = word(central=[40], radial_cutoff=3.0, capacity=3)
    assert bits == _hip.STATUS_EXCISE_CAPACITY and counts[0] == 5 and source.shape == (1, 3)         # the true count
    assert np.array_equal(source[0], load_golden("excise_and_repaint/spherical.npz")["source"][2, :3])
    bits, (_, _, counts) = word(central=[40], radial_cutoff=3.0, new_sides=[2.0, 8.0, 8.0], capacity=8)
    assert bits == _hip.STATUS_EXCISE_OUTSIDE_BOX and counts[0] == 5
    bits, (source, cx, counts) = word(central=[63, 20, -1], radial_cutoff=3.0, capacity=8)
    assert bits == _hip.STATUS_EXCISE_CENTRAL_INDEX and list(counts) == [0, 4, 0] and not source[0].any() and not cx[2].any()
    bits, _ = word(central=[20, 54, 40], radial_cutoff=3.0, new_sides=[ec.NEW_BOX] * 3, capacity=8)
    assert bits == 0
    # without a caller's status word the wrapper reads it and raises; the limits are refused on the host
    with pytest.raises(kernels.ExcisionCapacityError):
        _launch(cuda, x, sides, [40], radial_cutoff=3.0, capacity=3)
    with pytest.raises(AssertionError, match="Excised atoms are outside the new box"):
        _launch(cuda, x, sides, [40], radial_cutoff=3.0, new_sides=[2.0, 8.0, 8.0])
    with pytest.raises(IndexError):
        _launch(cuda, x, sides, [63], radial_cutoff=3.0)
    with pytest.raises(_hip.MdxError, match="at most 3 spatial dimensions"):
        _launch(cuda, np.zeros((5, 4)), np.ones(4), [0], radial_cutoff=1.0)
    with pytest.raises(_hip.MdxError, match="at most 3 spatial dimensions"):
        _launch(cuda, np.zeros((_hip.EXCISE_MAX_ATOMS + 1, 3)), np.ones(3), [0], radial_cutoff=1.0)
    with pytest.raises(_hip.MdxError, match="no CPU fallback"):
        kernels.excise_environments(torch.zeros(5, 3, dtype=torch.float64), torch.ones(3, dtype=torch.float64),
                                    torch.zeros(1, dtype=torch.int64), radial_cutoff=1.0)


def test_excision_tie_rule_on_the_crystal(cuda):
    """The unperturbed crystal: whole shells at equal distance.  Equal distances go to the lower atom index."""
    x, sides = ec.diamond_sites(2), np.array([ec.BOX] * 3)
    central = [0, 5, 31, 63]
    for mode in (dict(number_of_neighbors=4), dict(number_of_neighbors=9), dict(radial_cutoff=2.4), dict(radial_cutoff=3.9)):
        _compare_with_restatement(cuda, x, sides, central, **mode)
    source, _, counts = _launch(cuda, x, sides, central, radial_cutoff=3.9)
    assert list(counts) == [17] * 4                      # the atom, its 4 first and 12 second neighbours
    distance = ec.distances(x, x[0], sides)
    assert any(distance[a] == distance[b] for a, b in zip(source[0, 1:16], source[0, 2:17]))       # (ties were met)


# ------------------------------------------------------------------------------------------------------------------
# 3. the per-sample repaint kernel against mdx_repaint_constrained_rows
# ------------------------------------------------------------------------------------------------------------------
N, D, TYPES = 8, 3, 2
COUNTS, S = [1, 4, 5, N], 2


def _schedule(cuda):
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_scheduler import NoiseScheduler
    return NoiseScheduler(NoiseParameters(**ec.NOISE), num_classes=TYPES + 1, device=cuda).tables


def _repaint_tables(cuda, counts, seed=3):
    g = torch.Generator().manual_seed(seed)
    E = len(counts)
    cx = torch.rand(E, N, D, generator=g)
    ca = torch.randint(0, TYPES, (E, N), generator=g)
    cidx = torch.stack([torch.randperm(N, generator=g) for _ in range(E)])
    return cx.to(cuda), ca.to(cuda), cidx.to(cuda), torch.tensor(counts, dtype=torch.int32, device=cuda)


def _batch(cuda, B, seed=4):
    g = torch.Generator().manual_seed(seed)
    x, a = torch.rand(B, N, D, generator=g), torch.randint(0, TYPES + 1, (B, N), generator=g)
    z, u = torch.randn(B, N, D, generator=g), torch.rand(B, N, TYPES + 1, generator=g)
    return x.to(cuda), a.to(cuda), z.to(cuda), u.to(cuda)


def _bits(t):
    return t.cpu().numpy().view(np.int32) if t.dtype == torch.float32 else t.cpu().numpy()


@pytest.mark.parametrize("index", [0, 3])
def test_per_sample_repaint_equals_the_shared_entry_per_environment(cuda, index):
    kernels, _hip = _kernels()
    sched = _schedule(cuda)
    cx, ca, cidx, counts = _repaint_tables(cuda, COUNTS)
    B = len(COUNTS) * S
    x, a, z, u = _batch(cuda, B)
    environment = torch.arange(len(COUNTS), dtype=torch.int32, device=cuda).repeat_interleave(S)
    rng = _hip.Rng(0, 0, 2, 2)
    got_x, got_a = x.clone(), a.clone()
    kernels.repaint_rows_per_sample(sched, index, None, cx, ca, cidx, counts, environment, z, u, rng, got_x, got_a)
    for e, k in enumerate(COUNTS):
        rows = slice(e * S, (e + 1) * S)
        want_x, want_a = x[rows].clone(), a[rows].clone()
        kernels.repaint_constrained_rows(sched, index, None, cx[e, :k].contiguous(), ca[e, :k].contiguous(),
                                         cidx[e, :k].contiguous(), z[rows].contiguous(), u[rows].contiguous(), rng, want_x, want_a)
        assert np.array_equal(_bits(got_x[rows]), _bits(want_x)) and np.array_equal(_bits(got_a[rows]), _bits(want_a)), (index, e)
        untouched = cidx[e, k:]
        assert torch.equal(got_x[rows][:, untouched], x[rows][:, untouched])          # the rows past count[e] stay
        if index == 0:
            assert torch.equal(got_x[rows][:, cidx[e, :k]], cx[e, :k].expand(S, k, D))     # the hard constraint: unnoised
    # the loop variable on the device gives the same bits
    d_index = torch.tensor([index], dtype=torch.int32, device=cuda)
    dev_x, dev_a = x.clone(), a.clone()
    kernels.repaint_rows_per_sample(sched, 0, d_index, cx, ca, cidx, counts, environment, z, u, rng, dev_x, dev_a)
    assert np.array_equal(_bits(dev_x), _bits(got_x)) and torch.equal(dev_a, got_a)


@pytest.mark.parametrize("device_rng", [False, True])
def test_per_sample_repaint_with_equal_environments_is_the_shared_entry(cuda, device_rng):
    kernels, _hip = _kernels()
    sched = _schedule(cuda)
    E, K, index = 3, 4, 5
    cx, ca, cidx, counts = _repaint_tables(cuda, [K])
    tables = (cx.expand(E, N, D).contiguous(), ca.expand(E, N).contiguous(), cidx.expand(E, N).contiguous(), counts.expand(E).contiguous())
    x, a, z, u = _batch(cuda, E * S)
    if device_rng:
        z = u = None
    environment = torch.arange(E, dtype=torch.int32, device=cuda).repeat_interleave(S)
    rng = _hip.Rng(77, 2, 2, 3)
    got_x, got_a, want_x, want_a = x.clone(), a.clone(), x.clone(), a.clone()
    kernels.repaint_rows_per_sample(sched, index, None, *tables, environment, z, u, rng, got_x, got_a)
    kernels.repaint_constrained_rows(sched, index, None, cx[0, :K].contiguous(), ca[0, :K].contiguous(), cidx[0, :K].contiguous(),
                                     z, u, rng, want_x, want_a)
    assert np.array_equal(_bits(got_x), _bits(want_x)) and torch.equal(got_a, want_a)
    assert not torch.equal(got_x, x)


def test_per_sample_repaint_device_rng_is_the_documented_stream(cuda):
    kernels, _hip = _kernels()
    sched = _schedule(cuda)
    cx, ca, cidx, counts = _repaint_tables(cuda, COUNTS)
    B, index, seed, call, stride, offset = len(COUNTS) * S, 4, 20250815, 3, 2, 2
    x, a, _, _ = _batch(cuda, B)
    environment = torch.arange(len(COUNTS), dtype=torch.int32, device=cuda).repeat_interleave(S)
    rng = _hip.Rng(seed, call, stride, offset)
    draw = index * stride + offset
    z = kernels.rng_fill(kernels.RNG_NORMAL, seed, call, draw, _hip.TAG_REPAINT_Z, B * N, D, cuda).view(B, N, D)
    u = kernels.rng_fill(kernels.RNG_UNIFORM, seed, call, draw, _hip.TAG_REPAINT_U, B * N, TYPES + 1, cuda).view(B, N, TYPES + 1)
    got_x, got_a, want_x, want_a = x.clone(), a.clone(), x.clone(), a.clone()
    kernels.repaint_rows_per_sample(sched, index, None, cx, ca, cidx, counts, environment, None, None, rng, got_x, got_a)
    kernels.repaint_rows_per_sample(sched, index, None, cx, ca, cidx, counts, environment, z, u, rng, want_x, want_a)
    assert np.array_equal(_bits(got_x), _bits(want_x)) and torch.equal(got_a, want_a)


# ------------------------------------------------------------------------------------------------------------------
# 4. the generator
# ------------------------------------------------------------------------------------------------------------------
def _parameters(**extra):
    import warnings

    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.predictor_corrector_axl_generator import \
        PredictorCorrectorSamplingParameters
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_parameters import NoiseParameters
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return NoiseParameters(**ec.NOISE), PredictorCorrectorSamplingParameters(**dict(ec.SAMPLING, **extra))


@pytest.fixture(scope="module")
def network(cuda):
    return nets.load_fixture_weights(nets.mlp_net(ec.N_ATOMS, 1), load_golden("excise_and_repaint/samples.npz")).to(cuda)


def _golden_tables(name="spherical"):
    g = load_golden(f"excise_and_repaint/{name}.npz")
    return (torch.from_numpy(g["X_constraint"]), torch.from_numpy(g["A"]), None, torch.from_numpy(g["count"].astype(np.int32)))


def _per_sample_generator(network, **extra):
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.constrained_langevin_generator import \
        PerSampleConstrainedLangevinGenerator
    noise, sampling = _parameters(**extra)
    return PerSampleConstrainedLangevinGenerator(noise, sampling, network, elements=["Si"])


def test_batched_generator_against_one_generator_per_environment(cuda, network):
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.constrained_langevin_generator import \
        ConstrainedLangevinGenerator
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.noise_sources import PerEnvironmentNoise
    from diffusion_for_multi_scale_molecular_dynamics_amd.generators.sampling_constraint import SamplingConstraint
    cx, ca, _, counts = _golden_tables()
    S, E = ec.SAMPLES_PER_ENVIRONMENT, len(counts)
    noise, sampling = _parameters()
    singles = []
    with torch.no_grad():
        for e in range(E):
            k = int(counts[e])
            constraint = SamplingConstraint(elements=["Si"], constrained_relative_coordinates=cx[e, :k].clone(),
                                            constrained_atom_types=ca[e, :k].clone(), constrained_indices=torch.arange(k))
            torch.manual_seed(ec.BASE_SEED + e)
            singles.append(ConstrainedLangevinGenerator(noise, sampling, network, constraint).sample(S, cuda))
        generator = _per_sample_generator(network)
        generator.set_environments((cx, ca, None, counts), S)
        generator.noise_source = PerEnvironmentNoise([ec.BASE_SEED + e for e in range(E)], S)
        batched = generator.sample(E * S, cuda)
    want_a, want_x = torch.cat([s.A for s in singles]).cpu().numpy(), torch.cat([s.X for s in singles]).cpu().numpy()
    assert np.array_equal(batched.A.cpu().numpy(), want_a)
    error = torus_rel_l2(batched.X.cpu().numpy(), want_x)
    print(f"batched generator vs one generator per environment: rel-L2 = {error:.3e}")
    assert error <= PARITY
    for e in range(E):                                   # the hard constraint at the end of the trajectory
        k = int(counts[e])
        assert torch.equal(batched.X[e * S:(e + 1) * S, :k].cpu(), cx[e, :k].expand(S, k, 3))
    with pytest.raises(Exception, match="fused_score_network"):
        fused = _per_sample_generator(network, rng_mode="device", seed=1, fused_score_network=True)
        fused.set_environments((cx, ca, None, counts), S)
        fused.sample(E * S, cuda)


def test_batched_generator_graph_replay_and_rewritten_tables(cuda, network):
    S = ec.SAMPLES_PER_ENVIRONMENT
    first, second = _golden_tables("spherical"), _golden_tables("nearest_neighbors")
    outs = {}
    with torch.no_grad():
        for use_graph in (False, True):
            generator = _per_sample_generator(network, rng_mode="device", seed=9, use_hip_graph=use_graph)
            generator.set_environments(first, S)
            a = generator.sample(3 * S, cuda)
            kept = generator._buffers.get("graph_loop")
            generator.set_environments(second, S)                  # other tables, the same shapes: rewritten in place
            b = generator.sample(3 * S, cuda)
            assert generator._buffers.get("graph_loop") is kept and (kept is not None) == use_graph
            outs[use_graph] = (a, b)
            if use_graph:
                generator.set_environments(tuple(t if t is None else t[:2] for t in second), S)      # another E: the graph goes
                assert "graph_loop" not in generator._buffers
                assert generator.sample(2 * S, cuda).X.shape == (2 * S, ec.N_ATOMS, 3)
    for eager, graph in zip(outs[False], outs[True]):
        assert torch.equal(eager.A, graph.A) and np.array_equal(_bits(eager.X), _bits(graph.X))
    assert not torch.equal(outs[True][0].X, outs[True][1].X)
    counts = second[3]
    for e in range(3):
        assert torch.equal(outs[True][1].X[e * S:(e + 1) * S, :int(counts[e])].cpu(), second[0][e, :int(counts[e])].expand(S, -1, 3))


# ------------------------------------------------------------------------------------------------------------------
# 5. the maker
# ------------------------------------------------------------------------------------------------------------------
def _maker(cuda, network, radius, batch_environments, **sampling_extra):
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.atom_selector import atom_selector_factory as sf
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.excisor import excisor_factory as ef
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker.excise_and_repaint_sample_maker import (
        ExciseAndRepaintSampleMaker, ExciseAndRepaintSampleMakerArguments)
    arguments = ExciseAndRepaintSampleMakerArguments(element_list=["Si"], sample_box_size=[ec.NEW_BOX] * 3,
                                                     number_of_samples_per_substructure=ec.SAMPLES_PER_ENVIRONMENT,
                                                     sample_edit_radius=radius)
    selector = sf.create_atom_selector(sf.create_atom_selector_parameters(
        dict(algorithm="threshold", uncertainty_threshold=ec.UNCERTAINTY_THRESHOLD)))
    excisor = ef.create_excisor(ef.create_excisor_parameters(dict(algorithm="spherical_cutoff", radial_cutoff=ec.RADIAL_CUTOFF)))
    noise, sampling = _parameters(**sampling_extra)
    maker = ExciseAndRepaintSampleMaker(arguments, selector, excisor, noise, sampling, network, device=str(cuda))
    maker.batch_environments = batch_environments
    return maker


@pytest.mark.parametrize("sample_batchsize", [None, ec.SAMPLES_PER_ENVIRONMENT])
@pytest.mark.parametrize("edited", [False, True])
@pytest.mark.parametrize("batch_environments", [False, True])
def test_sample_maker_against_the_reference(cuda, network, batch_environments, edited, sample_batchsize):
    """batch_environments=False against the reference's maker after one torch.manual_seed (`seq`), True against the reference
    reseeded per environment (`per_env`); sample_batchsize = S runs the batched maker one environment per call."""
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker.namespace import (
        AXL_STRUCTURE_IN_NEW_BOX, AXL_STRUCTURE_IN_ORIGINAL_BOX)
    g, frame, excised = (load_golden("excise_and_repaint/" + name + ".npz") for name in ("samples", "frame", "spherical"))
    run = "per_env" if batch_environments else "seq"
    structure = _axl()(A=frame["A"], X=frame["X"], L=frame["L"])
    S, E = ec.SAMPLES_PER_ENVIRONMENT, 3
    extra = {} if sample_batchsize is None else dict(sample_batchsize=sample_batchsize)
    torch.manual_seed(ec.BASE_SEED)
    plain, active, infos = _maker(cuda, network, None, batch_environments, **extra).make_samples(structure, frame["uncertainty"])
    assert len(plain) == len(active) == len(infos) == E * S
    assert np.array_equal(np.stack([s.A for s in plain]), g[run + "_A"])
    error = torus_rel_l2(np.stack([s.X for s in plain]), g[run + "_X"])
    print(f"sample maker, batch_environments = {batch_environments}, sample_batchsize = {sample_batchsize}: rel-L2 = {error:.3e}")
    assert error <= PARITY
    np.testing.assert_allclose(np.stack([s.L for s in plain]), g[run + "_L"], rtol=0, atol=0)
    for b, (sample, index, info) in enumerate(zip(plain, active, infos)):
        e, k = b // S, int(excised["count"][b // S])
        assert sample.A.dtype == g[run + "_A"].dtype and sample.X.dtype == g[run + "_X"].dtype and sample.L.dtype == g[run + "_L"].dtype
        assert isinstance(index, np.ndarray) and index.shape == (1,) and index[0] == g[run + "_active"][b] == 0
        assert set(info) == {"constrained_atom_indices", AXL_STRUCTURE_IN_ORIGINAL_BOX, AXL_STRUCTURE_IN_NEW_BOX}
        assert info["constrained_atom_indices"] == list(range(k)) and k == g[run + "_constrained"][b]
        assert np.array_equal(info[AXL_STRUCTURE_IN_ORIGINAL_BOX].X, excised["X_centred"][e, :k])
        assert np.array_equal(info[AXL_STRUCTURE_IN_NEW_BOX].X, excised["X_embedded"][e, :k])
        assert info[AXL_STRUCTURE_IN_NEW_BOX].X.dtype == np.float64
        assert np.array_equal(info[AXL_STRUCTURE_IN_NEW_BOX].L, [ec.NEW_BOX] * 3 + [0.0] * 3)
        pinned = np.abs(sample.X[:k].astype(np.float64) - excised["X_constraint"][e, :k].astype(np.float64)).max()
        assert pinned <= ULP                                                            # the constrained atoms come first, pinned
    if not edited:
        return
    torch.manual_seed(ec.BASE_SEED)
    after, active, _ = _maker(cuda, network, ec.SAMPLE_EDIT_RADIUS, batch_environments, **extra).make_samples(
        structure, frame["uncertainty"])
    keep = g[run + "_keep"]
    assert not keep.all() and len(after) == E * S
    for b, (sample, before) in enumerate(zip(after, plain)):
        count = int(g[run + "_edited_count"][b])
        assert len(sample.X) == len(sample.A) == count                                  # the keep mask is the reference's ...
        assert np.array_equal(sample.X, before.X[keep[b]]) and np.array_equal(sample.A, before.A[keep[b]])     # ... atom for atom
        assert np.array_equal(sample.A, g[run + "_edited_A"][b, :count])
        assert np.array_equal(sample.L, before.L) and active[b][0] == 0
    assert torus_rel_l2(np.concatenate([s.X for s in after]),
                        np.concatenate([g[run + "_edited_X"][b, :int(g[run + "_edited_count"][b])] for b in range(E * S)])) <= PARITY


def test_sample_maker_limits_and_static_edit(cuda, network):
    from diffusion_for_multi_scale_molecular_dynamics_amd.active_learning_loop.sample_maker.excise_and_repaint_sample_maker import \
        ExciseAndRepaintSampleMaker
    g, frame = load_golden("excise_and_repaint/samples.npz"), load_golden("excise_and_repaint/frame.npz")
    structure = _axl()(A=frame["A"], X=frame["X"], L=frame["L"])
    maker = _maker(cuda, network, None, True)
    maker.arguments.max_constrained_substructure = 2
    torch.manual_seed(ec.BASE_SEED)
    samples, active, infos = maker.make_samples(structure, frame["uncertainty"])
    assert len(samples) == 2 * ec.SAMPLES_PER_ENVIRONMENT                              # the two most uncertain atoms
    assert torus_rel_l2(np.stack([s.X for s in samples]), g["per_env_X"][:len(samples)]) <= PARITY
    assert maker.make_samples(structure, np.zeros(63)) == ([], [], [])                  # nothing above the threshold
    small = _maker(cuda, network, None, True)
    small.arguments.new_box_lattice_parameters = np.array([2.0, 6.5, 6.5, 0.0, 0.0, 0.0])
    with pytest.raises(AssertionError, match="Excised atoms are outside the new box"):
        small.make_samples(structure, frame["uncertainty"])
    with pytest.raises(AssertionError, match="Excised atoms are outside the new box"):
        ExciseAndRepaintSampleMaker.embed_structure_in_new_box(infos[0]["axl_structure_in_original_box"],
                                                                 np.array([2.0, 6.5, 6.5, 0.0, 0.0, 0.0]))
    b = int(np.flatnonzero(~g["seq_keep"].all(axis=1))[0])
    sample = _axl()(A=g["seq_A"][b], X=g["seq_X"][b], L=g["seq_L"][b])
    edited = ExciseAndRepaintSampleMaker.edit_generated_structure(sample, 0, int(g["seq_constrained"][b]), ec.SAMPLE_EDIT_RADIUS)
    assert np.array_equal(edited.X, sample.X[g["seq_keep"][b]]) and np.array_equal(edited.A, sample.A[g["seq_keep"][b]])
