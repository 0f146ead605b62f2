"""tests/mlp_cases.py without a GPU: the float64 restatement of the fused MLP forward against the package's own module in float64,
the generators, the inputs' edges, the negative controls (each must leave its bar by more than 4x), and the conditions on the
inputs that the GPU tests (tests/test_mlp_forward_elements_gpu.py) rely on: w / sigma >= 1/4 at the sampler's x' step, and at the
atom-type step at least 90 % of the atoms with a decided type and decisions that change when the logits are wrong."""
import numpy as np
import pytest

import mlp_cases as mc

SHARP = 2.0 ** -15          # the median of bar / |value| over the non-zero outputs of the layer-by-layer form


def _padded_shapes():
    import test_generator_gpu as tg
    return tuple(mc.Shape(s[0], s[1], 3, s[2], s[3], *s[4:]) for s, _ in tg.PADDED_FAMILY_SHAPES)


def _all_shapes():
    seen = []
    for shape in mc.FORWARD_SHAPES + mc.FAMILY_SHAPES + _padded_shapes() + (mc.GLOBAL_TWO_TYPES,):
        if shape not in seen:
            seen.append(shape)
    return seen


def _sampler_shapes():
    seen = []
    for shape in mc.GENERIC_SHAPES + mc.FAMILY_SHAPES + _padded_shapes() + (mc.ALL_ODD, mc.D2, mc.GLOBAL, mc.GLOBAL_TWO_TYPES):
        if shape not in seen:
            seen.append(shape)
    return seen


ALL_SHAPES = _all_shapes()
SAMPLER_SHAPES = _sampler_shapes()


def test_the_issue_table():
    t = mc.TEMPLATE_EMBEDDINGS
    assert [tuple(s) for s in mc.FORWARD_SHAPES] == [
        (8, 1, 3, 64, 3, 32, 16, 16, 1, 1), (1, 1, 3, 16, 1, 4, 1, 1, 1, 1), (5, 3, 3, 50, 2, 7, 3, 5, 3, 2),
        (5, 2, 2, 48, 3, 8, 4, 4, 3, 2), (3, 1, 1, 32, 2, 4, 2, 2, 1, 1), (20, 1, 3, 96, 4) + t, (24, 2, 3, 64, 2) + t,
        (8, 1, 3, 128, 3) + t]
    assert mc.BATCHES == (1, 5, 37)
    assert mc.N20.N * mc.N20.d == 60 and mc.N24.N * mc.N24.d == 72
    odd = mc.ALL_ODD
    assert all(v % 4 for v in (2 * odd.N * odd.d, odd.ec, odd.hidden, mc.outputs(odd), mc.folded_inputs(odd)))
    assert {(s.types, s.layers) for s in mc.FAMILY_SHAPES} == {(t_, n) for t_ in (1, 2) for n in (2, 3, 4)}


def test_sincos_grid():
    grid = mc.sincos_grid()
    assert grid.dtype == np.float32 and grid.size == 2 ** 20 + 5 * 129 + 2 ** 16
    g64 = grid.astype(np.float64)
    for centre in (0.0, 0.25, 0.5, 0.75, 1.0):
        c = np.float32(centre)
        assert np.sum((grid > c) & (grid <= c + 64 * np.spacing(c))) >= 64 and np.sum(grid < c) >= 64
        below = np.sort(np.unique(grid[grid < c]))[-64:]
        assert np.all(np.diff(below.view(np.int32)) == (1 if centre > 0 else -1))
    assert g64.min() < 0.0 and g64.max() > 1.0


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=mc.shape_id)
def test_sparse_network(shape):
    """Every nn.Linear of the forward: r in {1, 2, 4} non-zeros per row (the row's length at the most), sum |w| <= 1/2, biases
    of order one; the kinds and the r walk through the layers; row 0 of hidden layer 0 reads the last input."""
    network = mc.build_network(shape)
    counts = set()
    for name, linear in mc.linears(network):
        w = linear.weight.detach().numpy()
        per_row = (w != 0).sum(axis=1)
        assert per_row.min() == per_row.max() and per_row[0] in (1, 2, 4, w.shape[1]), name
        assert np.all(np.abs(w.astype(np.float64)).sum(axis=1) <= 0.5 * (1 + 1e-6)), name
        assert 0.0 < np.abs(linear.bias.detach().numpy()).max() <= 1.0
        counts.add(int(per_row[0]))
    assert 4 in counts and len(counts) >= 2
    # the global-weights form adds a row's terms behind its last whole quad as a rounded product and a rounded addition: the row
    # rule's one spare rounding covers ONE non-zero there (mlp_cases' docstring), in every matrix of the shapes that run that form
    if shape in (mc.GLOBAL, mc.GLOBAL_TWO_TYPES, mc.N20):
        for name, linear in mc.linears(network):
            if name == "coordinates" or name.startswith(("hidden", "out_")):          # the matrices the row loop runs
                w = linear.weight.detach().numpy()
                assert np.all((w[:, w.shape[1] // 4 * 4:] != 0).sum(axis=1) <= 1), name
    assert network.mlp_layers[0].weight[0, -1] != 0
    assert len(network.mlp_layers) == shape.layers and network.spatial_dimension == shape.d


@pytest.mark.parametrize("B", mc.BATCHES)
@pytest.mark.parametrize("periodic", [False, True])
def test_input_edges(B, periodic):
    for shape in mc.FORWARD_SHAPES:
        inputs = mc.make_inputs(shape, B, periodic)
        x = inputs.x.reshape(-1)
        special = mc.SPECIAL_COORDINATES + (mc.PERIODIC_COORDINATES if periodic else ())
        assert x.dtype == np.float32 and np.all(np.isin(x[0::2], np.array(special, dtype=np.float32)))
        assert len(set(x[0::2].tolist())) == min(len(special), (x.size + 1) // 2)
        if not periodic:
            assert np.all((x >= 0) & (x < 1))
        assert inputs.a[0, 0] == shape.types and inputs.a.min() >= 0 and inputs.a.max() <= shape.types
        assert inputs.time[0] == 0 and (B == 1 or inputs.time[1] == 1) and np.all((inputs.time >= 0) & (inputs.time <= 1))
        assert inputs.sigma.min() == np.float32(1e-3) and (B == 1 or inputs.sigma.max() == np.float32(0.5))
        assert shape.d == 1 or np.all(inputs.l[:, shape.d:] != 0)
    if B == 37:     # every special value appears in every shape with more than a handful of coordinates
        for shape in mc.FORWARD_SHAPES:
            x = mc.make_inputs(shape, B, periodic).x.reshape(-1)
            assert all(np.any(x == np.float32(v)) for v in special)


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=mc.shape_id)
def test_restatement_equals_the_float64_module(shape):
    """The restatement is tied to the module, not to the kernel: 1e-12 relative against network.double() on the same inputs; and
    the folded algebra (checked inside mc.forward) is the same function."""
    for B in mc.BATCHES:
        inputs = mc.make_inputs(shape, B, False)
        forms = ("layers", "folded") if shape.layers >= 2 else ("layers",)
        for form in forms:
            want = mc.forward(shape, mc.weights_of(shape), inputs, form, software_bar=False)
            logits, score_x, score_l = mc.module_forward(shape, inputs)
            assert np.all(np.isneginf(want["logits"][..., -1])) and np.all(np.isneginf(logits[..., -1]))
            for got, ref in ((want["logits"][..., :-1], logits[..., :-1]), (want["score_x"], score_x), (want["score_l"], score_l)):
                assert got.shape == ref.shape and np.all(np.abs(got - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref)))
            for name in ("logits", "score_x", "score_l"):
                bar = want["bar_" + name]
                assert bar.shape == want[name].shape and np.all(np.isfinite(bar)) and np.all(bar >= 0)
                assert np.all(bar[..., :-1] > 0) if name == "logits" else np.all(bar > 0)
            assert np.all(want["bar_logits"][..., -1] == 0)


@pytest.mark.parametrize("shape", mc.FORWARD_SHAPES, ids=mc.shape_id)
def test_the_bar_is_sharp(shape):
    """A bar that is too wide is not a test: the median of bar / |value| stays below 2^-15 (a few hundred u)."""
    want = mc.forward(shape, mc.weights_of(shape), mc.make_inputs(shape, 37, True), "layers")
    values = np.concatenate([want[n][np.isfinite(want[n])].reshape(-1) for n in ("logits", "score_x", "score_l")])
    bars = np.concatenate([want["bar_" + n][np.isfinite(want[n])].reshape(-1) for n in ("logits", "score_x", "score_l")])
    keep = values != 0
    sharp = float(np.median(bars[keep] / np.abs(values[keep])))
    print(f"{mc.shape_id(shape)}: median bar / |value| = {sharp / mc.U:.1f} u")
    assert sharp < SHARP


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=mc.shape_id)
def test_negative_controls_leave_the_bar(shape):
    """Each restated mistake moves at least one element by more than 4x its bar, in both arithmetic forms (the folded bar is
    the wider one).  One atom: there is no next atom to take an embedding from."""
    assert mc.HW_SINCOS_ABS > 0
    inputs = mc.make_inputs(shape, 5, False)
    weights = mc.weights_of(shape)
    for form in (("layers", "folded") if shape.layers >= 2 else ("layers",)):
        want = mc.forward(shape, weights, inputs, form, software_bar=False)
        for name in mc.CONTROLS:
            if name == "atom_embedding_from_next_atom" and shape.N == 1:
                continue
            wrong_weights, keywords = mc.control(shape, weights, inputs, name)
            wrong = mc.forward_layers(shape, wrong_weights, inputs, software_bar=False, **keywords)
            worst = 0.0
            for key in ("logits", "score_x", "score_l"):
                finite = np.isfinite(want[key])
                worst = max(worst, float(np.max(np.abs(wrong[key][finite] - want[key][finite]) / want["bar_" + key][finite])))
            assert worst > 4.0, (form, name, worst)


@pytest.mark.parametrize("shape", SAMPLER_SHAPES, ids=mc.shape_id)
def test_sampler_step_conditions(shape):
    """Conditions on the inputs of the predictor-step tests, from the oracle's schedule: at index T w / sigma >= 1/4 (a smaller
    factor lets the bar of x swallow the score's error), the same for the lattice's w / sigma_n; at index 1, the atom-type step,
    at least 90 % of the atoms have a decision margin above 1e-3 for every batch size (greedy at B = 5), MASK atoms among them."""
    C = shape.types + 1
    tables = mc.oracle_schedule(C)
    scalars = mc.step_scalars(tables, shape)
    assert scalars["idx"] == mc.SAMPLER_T - 1 > 0
    assert float(scalars["w"]) / float(scalars["sigma"]) >= 0.25
    assert float(scalars["w"]) / float(scalars["sigma_n"]) >= 0.25
    assert float(scalars["sigma"]) == np.float32(mc.SAMPLER_SIGMA_MAX)
    first = mc.step_scalars(tables, shape, mc.TYPES_INDEX)
    assert first["idx"] == 0 and np.array_equal(tables["q_bar_tm1_matrix"][0], np.eye(C, dtype=np.float32))
    form = "folded" if shape.layers >= 2 else "layers"
    for B in mc.BATCHES:
        step = mc.predictor_step(shape, B, form, scalars)
        assert np.all(step["bar_x"] > 0) and np.all(np.isfinite(step["x"]))
        step = mc.predictor_step(shape, B, form, first)
        a = step["inputs"].a
        types, qualifies = mc.type_decisions(step["net"]["logits"], a, tables, 0, mc.is_greedy(B))
        assert qualifies.mean() >= 0.9, (B, qualifies.mean())
        assert np.any(qualifies & (a == shape.types)), "no MASK atom with a decided type"
        assert np.all(types[qualifies] != shape.types) and np.all(types[qualifies & (a != shape.types)] == a[qualifies & (a != shape.types)])


@pytest.mark.parametrize("shape", [s for s in SAMPLER_SHAPES if s.types >= 2], ids=mc.shape_id)
def test_the_type_step_reads_the_logits(shape):
    """The atom-type step is a check of the logits rows: on every network with two or three atom types, at B = 37, a head column
    taken from its neighbour (the logit of atom 0, class 0 computed with the weights of the next logits row) and logits replaced by
    noise each change the type of at least one atom that qualifies; a MASK atom's decision is the arg-max of its real-class
    logits.  (One atom type: one real class, nothing to decide -- mlp_cases' docstring.)"""
    C = shape.types + 1
    tables = mc.oracle_schedule(C)
    first = mc.step_scalars(tables, shape, mc.TYPES_INDEX)
    form = "folded" if shape.layers >= 2 else "layers"
    changed_by_column = changed_by_noise = 0
    for B in mc.BATCHES:
        step = mc.predictor_step(shape, B, form, first)
        inputs, logits = step["inputs"], step["net"]["logits"]
        types, qualifies = mc.type_decisions(logits, inputs.a, tables, 0, mc.is_greedy(B))
        masked = qualifies & (inputs.a == shape.types)
        assert np.array_equal(types[masked], np.argmax(logits[..., :-1], axis=-1)[masked])
        wrong = mc.weights_of(shape).copy()
        wrong.w["out_a"][:-1], wrong.b["out_a"][:-1] = wrong.w["out_a"][1:].copy(), wrong.b["out_a"][1:].copy()    # every row from the next
        shifted = mc.forward_layers(shape, wrong, inputs, software_bar=False)["logits"]
        changed_by_column += int(np.sum(mc.type_decisions(shifted, inputs.a, tables, 0, mc.is_greedy(B))[0][qualifies] != types[qualifies]))
        noise = 5.0 * np.random.default_rng(B).standard_normal(logits.shape)
        noise[..., -1] = -np.inf
        changed_by_noise += int(np.sum(mc.type_decisions(noise, inputs.a, tables, 0, mc.is_greedy(B))[0][qualifies] != types[qualifies]))
    assert changed_by_column > 0 and changed_by_noise > 0, (changed_by_column, changed_by_noise)


def test_generic_fold_rule():
    """fold_pays as the header states it; the N = 24 shape pays but (decided with the image size on the GPU) may not fit."""
    assert not mc.fold_pays(mc.ONE_LANE)
    assert all(mc.fold_pays(s) for s in mc.GENERIC_SHAPES)
    assert mc.wave_floats(mc.TEMPLATE) % 4 == 0
