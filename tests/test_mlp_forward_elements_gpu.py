"""The fused MLP score network (csrc/mdx_hip.hip) PER ELEMENT against the float64 restatement of tests/mlp_cases.py on sparse
contractive networks -- see that module's docstring for the construction and for the bar, every constant of which was written
down before any GPU run (tests/test_mlp_cases_cpu.py holds the restatement, the negative controls and the conditions on the inputs
without a GPU):
  * the hardware v_cos_f32 / v_sin_f32 of the folded forwards against float64 on a grid (mdx_math_probe fn 4 / 5);
  * mdx_mlp_forward: logits, score_x, score_l of every shape at which an edge exists, with the packed image and with the in-kernel
    re-layout, with LDS and with global weights;
  * the forwards inside mdx_mlp_pc_sample, every variant, through one predictor step with the caller's zero noise: x' is an
    affine image of score_x and l' (free lattice) of score_l; and through one predictor step from index 1, where a MASK atom
    unmasks to the arg-max of its logits (networks with two or three atom types: with one type no decision reads the logit, and
    the sampler's logits row of those networks is not checked).

Every output is a view inside a guarded buffer (NaN, or a sentinel for the atom types) with 64 guard elements on either side;
every comparison is |got - want| <= bar for every element; each family prints its worst error / bar."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_cases as mc

pytestmark = pytest.mark.gpu

PAD = 64
SENTINEL = -7777
MEASURED = {}


def _hip():
    from diffusion_for_multi_scale_molecular_dynamics_amd import _hip
    return _hip


def _kernels():
    from diffusion_for_multi_scale_molecular_dynamics_amd import kernels
    return kernels


def _dev(array, device):
    return torch.as_tensor(np.ascontiguousarray(array)).to(device)


def _guarded(shape, device, values=None):
    """An output of `shape` inside a larger NaN-filled buffer: (buffer, view); values: what the view holds at the start."""
    count = int(np.prod(shape))
    buffer = torch.full((count + 2 * PAD,), float("nan"), dtype=torch.float32, device=device)
    view = buffer[PAD:PAD + count].view(*shape)
    if values is not None:
        view.copy_(_dev(values, device))
    return buffer, view


def _untouched(buffer):
    return bool(torch.isnan(buffer[:PAD]).all()) and bool(torch.isnan(buffer[-PAD:]).all())


def _guarded_types(a, device):
    buffer = torch.full((a.size + 2 * PAD,), SENTINEL, dtype=torch.int64, device=device)
    view = buffer[PAD:PAD + a.size].view(*a.shape)
    view.copy_(_dev(a, device))
    return buffer, view


def _types_untouched(buffer):
    return bool((buffer[:PAD] == SENTINEL).all()) and bool((buffer[-PAD:] == SENTINEL).all())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _report(family, ratio):
    MEASURED[family] = max(MEASURED.get(family, 0.0), ratio)
    print(f"{family}: worst error / bar {ratio:.3f}")


def _check(family, got, want, bar, where=None, distance=None):
    """|got - want| <= bar for every element (bar 0: equal; -inf: equal), no NaN; reports the worst ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape == bar.shape, (got.shape, want.shape, bar.shape)
    assert not np.any(np.isnan(got)), (family, where, np.argwhere(np.isnan(got))[:4])
    infinite = np.isinf(want)
    assert np.array_equal(got[infinite], want[infinite]), (family, where, "an infinite element")
    got, want, bar = got[~infinite], want[~infinite], bar[~infinite]
    assert np.all(np.isfinite(got)), (family, where)
    error = np.abs(got - want) if distance is None else distance(got, want)
    exact = bar == 0.0
    assert np.all(error[exact] == 0.0), (family, where)
    ratio = float(np.max(error[~exact] / bar[~exact])) if np.any(~exact) else 0.0
    _report(family, ratio)
    assert ratio <= 1.0, (family, where, ratio, int(np.sum(error > bar)))


@functools.lru_cache(maxsize=None)
def _pack(shape, device):
    """(network on the device, its MlpPack built the production way -- the host's binary64 folding included)."""
    import copy
    network = copy.deepcopy(mc.build_network(shape)).to(device)
    return network, _kernels().MlpPack(network, device)


def _image_floats(pack):
    return int(_hip().lib().mdx_mlp_image_floats(C.byref(pack.c_struct)))


def _without_image(struct):
    """A copy of the descriptor with packed_image = NULL: the kernels re-lay the weights out themselves (write_mlp_image)."""
    copy = type(struct)()
    C.memmove(C.byref(copy), C.byref(struct), C.sizeof(struct))
    copy.packed_image = None
    assert struct.packed_image and not copy.packed_image
    return copy


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the hardware sin / cos
def test_hardware_sincos(cuda):
    """v_cos_f32 / v_sin_f32 with the argument in revolutions (mdx_math_probe fn 4 / 5) against float64 cos / sin(2 pi x) on
    mc.sincos_grid(): every k 2^-20 in [0, 1), the 64 binary32 neighbours on either side of 0, 1/4, 1/2, 3/4 and 1, and 2^16 random
    binary32 values, each promoted to float64.  The bound is mc.HW_SINCOS_ABS = 2 x the maximum measured here on an MI355X:
    1.237048e-07 (2.08 u) for both functions (cos at x = 0x1.fe5p-8, sin a quarter turn further); an error of 4 x that figure
    fails.  fn 2 / 3 (the software sequence) stay what they were."""
    grid = mc.sincos_grid()
    x = _dev(grid, cuda)
    angle = 2.0 * np.pi * grid.astype(np.float64)
    worst = {}
    for fn, name, want in ((4, "cos", np.cos(angle)), (5, "sin", np.sin(angle))):
        got = _kernels().math_probe(fn, x).cpu().numpy().astype(np.float64)
        assert np.all(np.isfinite(got))
        error = np.abs(got - want)
        worst[name] = float(error.max())
        print(f"hardware {name}: largest |error| {worst[name]:.6e} at x = {float(grid[int(np.argmax(error))]).hex()}"
              f" ({worst[name] / mc.HW_SINCOS_ABS:.3f} of HW_SINCOS_ABS)")
    _report("hardware sin / cos", max(worst.values()) / mc.HW_SINCOS_ABS)
    assert max(worst.values()) <= mc.HW_SINCOS_ABS, worst
    assert mc.HW_SINCOS_ABS == 2.0 * mc.HW_SINCOS_MEASURED
    with pytest.raises(_hip().MdxError):
        _kernels().math_probe(6, x[:4])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. mdx_mlp_forward
def _forward(device, struct, inputs, shape):
    B, N, d, Cn, nl = inputs.x.shape[0], shape.N, shape.d, shape.types + 1, mc.n_lattice(shape.d)
    buffers, views = zip(*[_guarded(s, device) for s in ((B, N, Cn), (B, N, d), (B, nl))])
    _hip().call("mdx_mlp_forward", C.byref(struct), _dev(inputs.a, device), _dev(inputs.x, device), _dev(inputs.l, device),
                _dev(inputs.time[:, None], device), _dev(inputs.sigma[:, None], device), B, *views)
    got = [v.cpu().numpy() for v in views]
    assert all(_untouched(b) for b in buffers), "mdx_mlp_forward wrote outside its outputs"
    return got


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("shape", mc.FORWARD_SHAPES, ids=mc.shape_id)
def test_mlp_forward_elements(cuda, shape, B):
    """mdx_mlp_forward per element at the smallest shape of every edge (the template; one lane and one hidden layer; nothing a
    multiple of four; d = 2 and d = 1; N d = 60 and 72 around a wavefront; hidden 128, whose image exceeds the LDS limit, so that
    mlp_forward_kernel<false> reads the weights from global memory -- as does 96 x 4 at N = 20), B = 1, 5, 37 (one wavefront,
    two workgroups, a ragged tenth), coordinates 0, 1/4, 1/2, 3/4, 1 - 2^-24 and, the entry point being periodic, -0.25, 1.5, 3.0; the MASK class among the atom
    types; time 0 and 1; sigma 1e-3 ... 0.5; a lattice with off-diagonal entries.  The MASK logit is exactly -inf, nothing outside
    the outputs is written, and the run with packed_image = NULL (the in-kernel re-layout) gives the same bits.
    Measured on an MI355X: logits 0.105, score_x 0.105, score_l 0.100 of the bar with LDS weights; 0.081, 0.102, 0.069 with global
    weights."""
    _, pack = _pack(shape, cuda)
    limit_exceeded = 4 * (_image_floats(pack) + 4 * mc.wave_floats(shape)) > mc.LDS_LIMIT_BYTES
    assert 4 * _image_floats(pack) > mc.LDS_LIMIT_BYTES or shape != mc.GLOBAL, "hidden 128: the image alone exceeds the LDS limit"
    assert limit_exceeded == (shape in (mc.GLOBAL, mc.N20)), "which instantiation runs: image + wavefront regions against the limit"
    inputs = mc.make_inputs(shape, B, True)
    want = mc.forward(shape, mc.weights_of(shape), inputs, "layers")
    got = _forward(cuda, pack.c_struct, inputs, shape)
    again = _forward(cuda, _without_image(pack.c_struct), inputs, shape)
    family = "mdx_mlp_forward, global weights" if limit_exceeded else "mdx_mlp_forward"
    for name, values, relaid in zip(("logits", "score_x", "score_l"), got, again):
        assert np.array_equal(_bits(values), _bits(relaid)), (name, "the packed image and the in-kernel re-layout differ")
        _check(f"{family} {name}", values, want[name], want["bar_" + name], (mc.shape_id(shape), B))
    assert np.all(np.isneginf(got[0][..., -1]))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the forwards inside mdx_mlp_pc_sample, through one predictor step
@functools.lru_cache(maxsize=None)
def _schedule(num_classes, device):
    from diffusion_for_multi_scale_molecular_dynamics_amd.noise_schedulers.noise_scheduler import NoiseScheduler
    return NoiseScheduler(mc.noise_parameters(), num_classes=num_classes, device=device).tables


def _device_scalars(sched, shape, index):
    """The step's scalars from the DEVICE tables, read back (they are bit-exact-tested elsewhere); equal to the oracle's."""
    tables = {k: getattr(sched, k).cpu().numpy() for k in ("time", "sigma", "g", "g_squared")}
    scalars = mc.step_scalars(tables, shape, index)
    oracle = mc.step_scalars(mc.oracle_schedule(shape.types + 1), shape, index)
    assert all(np.float32(scalars[k]).view(np.uint32) == np.float32(oracle[k]).view(np.uint32) for k in ("time", "sigma", "w", "n"))
    assert index != mc.SAMPLER_T or float(scalars["w"]) / float(scalars["sigma"]) >= 0.25
    return scalars


def _predictor_step(device, shape, B, struct, options, fixed_lattice=True, index=mc.SAMPLER_T):
    """One launch of mdx_mlp_pc_sample: one iteration from `index`, M = 0, the caller's records (zero z and Gumbel noise, u = 1/2
    where greedy).  -> (types, x', l', status, the inputs' step scalars)."""
    hip = _hip()
    sched = _schedule(shape.types + 1, device)
    scalars = _device_scalars(sched, shape, index)
    inputs = mc.step_inputs(shape, B, scalars)
    greedy = mc.is_greedy(B)
    a_buffer, a = _guarded_types(inputs.a, device)
    x_buffer, x = _guarded(inputs.x.shape, device, inputs.x)
    l_buffer, lattice = _guarded(inputs.l.shape, device, inputs.l)
    status = torch.zeros(1, dtype=torch.int32, device=device)
    flags = hip.PcFlags(int(greedy), 0, int(fixed_lattice), 1, mc.SMALL_EPSILON)
    rng = hip.Rng(mc.RNG_SEED, mc.RNG_CALL, 1, 0, 0, None)
    records = _dev(mc.records(shape, B, greedy), device)
    hip.call("mdx_mlp_pc_sample", C.byref(sched.c_struct), C.byref(struct), C.byref(flags), 0, 0, int(index), 1, rng, B, a, x,
             lattice, records, records.numel(), int(options) | hip.MLP_SAMPLE_CALLER_NOISE, status)
    got = a.cpu().numpy(), x.cpu().numpy(), lattice.cpu().numpy(), int(status.item())
    assert _types_untouched(a_buffer) and _untouched(x_buffer) and _untouched(l_buffer), "the sampler wrote outside its composition"
    return got + (scalars,)


def _check_types(family, device, shape, B, struct, options, form):
    """The atom-type step: one predictor step from index 1, where a MASK atom unmasks to the arg-max of its real-class logits.  The
    types must equal the oracle's update of the float64 logits for every atom whose margin exceeds 1e-3 (at least 90 % of them,
    MASK atoms among them: tests/test_mlp_cases_cpu.py also shows that wrong logits change these decisions).  One atom type: a
    single real class, no decision reads the logit -- the sampler's logits row of those networks is NOT checked here."""
    if shape.types < 2:
        return
    types, _, _, status, scalars = _predictor_step(device, shape, B, struct, options, index=mc.TYPES_INDEX)
    assert status == 0 and scalars["idx"] == 0
    step = mc.predictor_step(shape, B, form, scalars)
    a = step["inputs"].a
    want, qualifies = mc.type_decisions(step["net"]["logits"], a, mc.oracle_schedule(shape.types + 1), 0, mc.is_greedy(B))
    masked = qualifies & (a == shape.types)
    assert qualifies.mean() >= 0.9 and masked.any()
    assert np.array_equal(want[masked], np.argmax(step["net"]["logits"][..., :-1], axis=-1)[masked])
    wrong = int(np.sum(types[qualifies] != want[qualifies]))
    print(f"{family} types: {int(qualifies.sum())} decided atoms ({int(masked.sum())} unmasked by their logits), {wrong} wrong")
    assert wrong == 0, (family, mc.shape_id(shape), B, np.argwhere(qualifies & (types != want))[:4])


def _check_step(family, device, shape, B, struct, options, form, free_lattice=False):
    """x' (and l') of the step from index T per element, then the atom-type step from index 1 (_check_types).  The types of the
    step from index T do not depend on the logits (mlp_cases' docstring) and are only held to their range."""
    types, x, lattice, status, scalars = _predictor_step(device, shape, B, struct, options, fixed_lattice=not free_lattice)
    assert status == 0
    z_lattice = None
    if free_lattice:        # the in-kernel draw of the predictor at index T: item = structure, draw = T (M + 1), MDX_TAG_LATTICE
        z_lattice = _kernels().rng_fill(_kernels().RNG_NORMAL, mc.RNG_SEED, mc.RNG_CALL, mc.SAMPLER_T, _hip().TAG_LATTICE, B,
                                        mc.n_lattice(shape.d), device).cpu().numpy()
    step = mc.predictor_step(shape, B, form, scalars, z_lattice)
    where = (mc.shape_id(shape), B)
    assert np.all((x >= 0.0) & (x < 1.0)), where
    _check(f"{family} x'", x, step["x"], step["bar_x"], where, distance=mc.torus_distance)
    if free_lattice:
        _check(f"{family} l'", lattice, step["l"], step["bar_l"], where)
    else:
        assert np.array_equal(_bits(lattice), _bits(step["inputs"].l)), "a fixed lattice changed"
    assert types.min() >= 0 and types.max() <= shape.types
    _check_types(family, device, shape, B, struct, options, form)
    return x


def _variant(struct, options):
    return int(_hip().lib().mdx_mlp_pc_sample_variant(C.byref(struct), int(options)))


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("shape", mc.GENERIC_SHAPES, ids=mc.shape_id)
def test_sampler_generic_forwards(cuda, shape, B):
    """SPEC 0, both forms, on the template, the all-odd shape, d = 2 and N = 24 (two passes of the lane loops): layer by layer
    (GENERIC_KERNEL | UNFOLDED, mlp_forward_wave on the LDS image) against the layer-by-layer bar, and folded (GENERIC_KERNEL,
    mlp_forward_wave_folded: the host's folded matrices, hardware sin / cos) against the folded bar.  The generic kernel folds only
    when that pays and the folded matrices fit the LDS next to the image: where mc.generic_folds says no (N = 24: it pays, but does
    not fit) the run must equal the unfolded one bit for bit and is held to the layer-by-layer bar; where it says yes the two
    must differ at B = 37.  With packed_image = NULL: the same bits.
    Measured on an MI355X: x' layer by layer at most 0.172, folded 0.172 of the bar; no wrong type."""
    hip = _hip()
    _, pack = _pack(shape, cuda)
    struct = pack.c_struct
    assert struct.folded_input and struct.folded_output
    plain, folded = hip.MLP_SAMPLE_GENERIC_KERNEL | hip.MLP_SAMPLE_UNFOLDED, hip.MLP_SAMPLE_GENERIC_KERNEL
    assert _variant(struct, plain) == 0 and _variant(struct, folded) == 0
    x_plain = _check_step("sampler SPEC 0, layer by layer", cuda, shape, B, struct, plain, "layers")
    folds = mc.generic_folds(shape, _image_floats(pack))
    assert folds == (shape != mc.N24)
    x_folded = _check_step("sampler SPEC 0, folded" if folds else "sampler SPEC 0, layer by layer", cuda, shape, B, struct, folded,
                           "folded" if folds else "layers")
    same = np.array_equal(_bits(x_plain), _bits(x_folded))
    assert same or folds, "the generic kernel folded where the folded matrices do not fit"
    # (the other direction only where there are enough elements: the two forms differ in the last bits of the score, which the
    # rounding of x' can absorb for a handful of coordinates)
    assert not (same and folds and B == 37), "the folded forward did not run"
    for options in (plain, folded):
        relaid = _predictor_step(cuda, shape, B, _without_image(struct), options)[1]
        assert np.array_equal(_bits(relaid), _bits(x_plain if options == plain else x_folded))


@pytest.mark.parametrize("B", mc.BATCHES)
def test_sampler_template_literals(cuda, B):
    """SPEC 1 (UNFOLDED on the template's dimensions: mlp_forward_regs, every layer's weights in registers) against the
    layer-by-layer bar: score_x through x'.  The template has one atom type, so nothing here reads its logits row.  Measured on an MI355X: x' at most 0.139 of the bar."""
    hip = _hip()
    _, pack = _pack(mc.TEMPLATE, cuda)
    assert _variant(pack.c_struct, hip.MLP_SAMPLE_UNFOLDED) == 1
    _check_step("sampler SPEC 1", cuda, mc.TEMPLATE, B, pack.c_struct, hip.MLP_SAMPLE_UNFOLDED, "layers")


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("shape", mc.FAMILY_SHAPES, ids=mc.shape_id)
def test_sampler_register_resident_family(cuda, shape, B):
    """SPEC 1xx (options 0; N = 8, e_a = e_l = 1, one or two atom types, two to four hidden layers: mlp_forward_folded) against the
    folded bar.  Measured on an MI355X: x' at most 0.186 of the bar; no wrong type (two atom types)."""
    _, pack = _pack(shape, cuda)
    assert _variant(pack.c_struct, 0) == 100 + 10 * (shape.types + 1) + shape.layers
    _check_step("sampler SPEC 1xx", cuda, shape, B, pack.c_struct, 0, "folded")


def _padded_cases():
    import test_generator_gpu as tg
    cases = [(mc.Shape(s[0], s[1], 3, s[2], s[3], *s[4:]), variant) for s, variant in tg.PADDED_FAMILY_SHAPES]
    return cases + [(mc.ALL_ODD, 212), (mc.D2, 213)]


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("shape,variant", _padded_cases(), ids=lambda v: mc.shape_id(v) if isinstance(v, tuple) else str(v))
def test_sampler_padded_family(cuda, shape, variant, B):
    """SPEC 2xx (PADDED_FAMILY: mlp_forward_padded on the zero-padded folded matrices, FQ = 16, 32 and 48 first-layer quads) on the
    shapes of test_generator_gpu.PADDED_FAMILY_SHAPES, the all-odd shape (hidden 50 < 64: the padded neurons stay zero) and d = 2,
    against the folded bar.  A shape outside the family's limits (one hidden layer; more than 192 folded inputs) runs the generic
    kernel layer by layer (asserted bit for bit against the UNFOLDED run) and is held to that bar.
    Measured on an MI355X: x' at most 0.172 of the bar; no wrong type."""
    hip = _hip()
    _, pack = _pack(shape, cuda)
    if mc.folded_inputs(shape) > 192:
        variant = 0
    assert _variant(pack.c_struct, hip.MLP_SAMPLE_PADDED_FAMILY) == variant
    assert bool(pack.c_struct.folded_padded) == (variant >= 200)
    if variant >= 200:
        _check_step("sampler SPEC 2xx", cuda, shape, B, pack.c_struct, hip.MLP_SAMPLE_PADDED_FAMILY, "folded")
    else:       # both such shapes run the layer-by-layer forward: one hidden layer; an image beyond the LDS limit (global weights)
        assert not mc.generic_folds(shape, _image_floats(pack))
        assert shape.layers == 1 or 4 * (_image_floats(pack) + 4 * mc.wave_floats(shape)) > mc.LDS_LIMIT_BYTES
        x = _check_step("sampler SPEC 0, layer by layer", cuda, shape, B, pack.c_struct, hip.MLP_SAMPLE_PADDED_FAMILY, "layers")
        unfolded = _predictor_step(cuda, shape, B, pack.c_struct, hip.MLP_SAMPLE_GENERIC_KERNEL | hip.MLP_SAMPLE_UNFOLDED)[1]
        assert np.array_equal(_bits(x), _bits(unfolded)), "which forward the generic kernel ran"


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("shape", (mc.GLOBAL, mc.GLOBAL_TWO_TYPES), ids=mc.shape_id)
def test_sampler_global_weights(cuda, shape, B):
    """Hidden 128 (options 0): the image exceeds the LDS limit, so mlp_pc_sample_kernel<G, false, 0> reads the caller's tensors from
    global memory, layer by layer; with two atom types as well, for the atom-type step.
    Measured on an MI355X: x' at most 0.171 of the bar; no wrong type."""
    _, pack = _pack(shape, cuda)
    assert 4 * _image_floats(pack) > mc.LDS_LIMIT_BYTES and _variant(pack.c_struct, 0) == 0
    _check_step("sampler global weights", cuda, shape, B, pack.c_struct, 0, "layers")


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("shape", mc.LATTICE_SHAPES, ids=mc.shape_id)
def test_sampler_free_lattice(cuda, shape, B):
    """use_fixed_lattice_parameters = 0 on the template and the all-odd shape, product options: l' = (l + (w s_l) / sigma_n) +
    n z_lat with z_lat drawn in-kernel from the documented Philox stream -- regenerated here with kernels.rng_fill (item = the
    structure, draw = T, MDX_TAG_LATTICE) -- checks score_l per element, x' and the types as before.
    Measured on an MI355X: l' at most 0.312, x' 0.165 of the bar."""
    _, pack = _pack(shape, cuda)
    assert _variant(pack.c_struct, 0) >= 100
    _check_step("sampler free lattice", cuda, shape, B, pack.c_struct, 0, "folded", free_lattice=True)
