"""tests/transport_cases.py without a GPU: the float64 restatement of the transport alignment kernel against the reference's own
binary64 records (tests/golden/transport/, every stage the fixtures hold), the point groups against the fixtures', and the
conditions on the new cases that tests/test_transport_align_elements_gpu.py relies on -- for the restatement alone."""
import math

import numpy as np
import pytest

import transport_cases as tc
from test_transport_cpu import fixture

DISCRETE = ["d1_n3", "d2_n3", "d3_n5", "d3_n8", "d3_n8_identity", "d3_n64", "d3_n65", "noising_d3_n8"]
SHARED_MU = [name for name in DISCRETE if name != "noising_d3_n8"]
ALL_FIXTURES = DISCRETE + ["d3_n2_ties", "toy1d"]
COSTS_BAR, IMAGE_BAR, MATRIX_BAR = 1e-13, 1e-14, 1e-14


def _mu(record):
    return record["MU"] if "MU" in record.files else record["sites"]


def test_point_groups_are_the_fixtures():
    """2, 8 and 48 signed permutation matrices with the identity first, equal as sets to the operations of every fixture made
    with the symmetries (the identity alone in the others)."""
    for D, count in ((1, 2), (2, 8), (3, 48)):
        group = tc.point_group(D)
        assert group.shape == (count, D, D) and group.dtype == np.float32 and len(tc.as_set(group)) == count
        assert np.array_equal(group[0], np.eye(D)) and np.all(np.abs(group).sum(axis=1) == 1) and np.all(np.abs(group).sum(axis=2) == 1)
    seen = set()
    for name in ALL_FIXTURES:
        record = fixture(name)
        D, operations = int(record["D"]), record["operations"]
        if operations.shape[0] == 1:
            assert np.array_equal(operations[0], tc.point_group(D)[0]), name
        else:
            assert tc.as_set(operations) == tc.as_set(tc.point_group(D)) and operations.shape[0] == len(tc.point_group(D)), name
            seen.add(D)
    assert seen == {1, 2, 3}


@pytest.mark.parametrize("name", DISCRETE)
def test_restatement_reproduces_the_references_binary64_records(name):
    """Every fixture with compare_discrete: the chosen operation and every operation's col_idx are equal; costs64 within 1e-13
    relative, image64 within 1e-14 on the torus, the invariants within 1e-14, cost_matrices64 (N <= 8) within 1e-14.
    Measured: costs at most 2.3e-15, the image and the invariants 2.3e-16, the matrices 3.9e-16."""
    record = fixture(name)
    assert bool(record["compare_discrete"])
    keep = 2 if "cost_matrices64" in record.files else 0
    got = tc.align(record["X"], _mu(record), record["operations"], keep_matrices=keep)
    assert np.array_equal(got.operation, record["operation64"])
    assert np.array_equal(got.col_idx, record["col_idx64"])
    cost_distance = np.abs(got.costs / record["costs64"] - 1.0).max()
    image_distance = tc.torus(got.image, record["image64"]).max()
    invariant_distance = max(tc.torus(got.xt, record["x_invariant64"]).max(),
                             tc.torus(got.mt[:record["mu_invariant64"].shape[0]], record["mu_invariant64"]).max())
    print(f"{name}: costs64 {cost_distance:.2e} relative, image64 {image_distance:.2e}, invariants {invariant_distance:.2e} on the torus")
    assert cost_distance <= COSTS_BAR and image_distance <= IMAGE_BAR and invariant_distance <= IMAGE_BAR
    centre_distance = tc.torus(tc.centre(record["X"]), record["centre64"]).max()
    assert centre_distance <= IMAGE_BAR
    if keep:
        matrix_distance = np.abs(got.matrices - record["cost_matrices64"]).max()
        print(f"{name}: cost_matrices64 {matrix_distance:.2e}")
        assert matrix_distance <= MATRIX_BAR
    # the restatement of an arbitrary choice, given its own: the same image and cost
    for b in range(got.costs.shape[0]):
        o = got.operation[b]
        image, cost = tc.chosen(got.xt[b], got.mt[b], record["operations"], o, got.col_idx[b, o])
        assert np.array_equal(image, got.image[b]) and abs(cost - got.costs[b, o]) <= 1e-15 * cost


def test_score_restatement_reproduces_score64():
    """score64 of the shared-mu fixtures at their three sigmas (both sides of the branch) and their kmax (2 and 4): the largest
    distance, as a fraction of the structure's largest |score64|, is what transport_cases.SCORE_RESTATEMENT_DISTANCE records,
    and SCORE_F is 500 times it.
    Measured: 1.9e-14 (d3_n8_identity at sigma 0.5; 1.7e-14 on d3_n64)."""
    worst, kmaxes, sides = 0.0, set(), set()
    for name in SHARED_MU:
        record = fixture(name)
        got = tc.align(record["X"], record["sites"], record["operations"])
        kmax, sigma_d = int(record["kmax"]), float(record["sigma_d"])
        kmaxes.add(kmax)
        for level, sigma in enumerate(record["sigma"]):
            B = record["X"].shape[0]
            want = record["score64"][level]
            mine = tc.score(got.xt, got.image, np.full(B, sigma, dtype=np.float32), sigma_d ** 2, kmax)
            largest = np.abs(want).reshape(B, -1).max(axis=1)
            distance = float((np.abs(mine - want).reshape(B, -1).max(axis=1) / largest).max())
            sides.add(math.sqrt(sigma_d ** 2 + float(sigma) ** 2) <= tc.SIGMA_THRESHOLD)
            print(f"{name} sigma {float(sigma):g} kmax {kmax}: restatement to score64 {distance:.2e} of the structure's largest")
            worst = max(worst, distance)
    print(f"largest restatement-to-reference distance of the score: {worst:.2e}")
    assert kmaxes == set(tc.KMAX) and sides == {True, False}
    assert worst <= tc.SCORE_RESTATEMENT_DISTANCE
    assert tc.SCORE_F == 500 * tc.SCORE_RESTATEMENT_DISTANCE and tc.SCORE_F <= 1e-3 * tc.EPS32


def test_the_case_list_is_the_issues():
    specs = tc.SPECS
    assert [specs[f"d3_n{n}"] for n in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)] == \
        [(3, n, 48, 4, False) for n in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256)]
    for D, O in ((1, 2), (2, 8)):
        assert [specs[f"d{D}_n{n}"] for n in (65, 129, 256)] == [(D, n, O, 4, False) for n in (65, 129, 256)]
    assert [specs[f"d3_n{n}_o{o}"] for o, n in ((1, 129), (5, 129), (13, 129), (13, 256))] == \
        [(3, n, o, 4, False) for o, n in ((1, 129), (5, 129), (13, 129), (13, 256))]
    assert [specs[f"noising_d3_n{n}"] for n in (65, 129, 256)] == [(3, n, 1, 4, True) for n in (65, 129, 256)]
    assert specs["d3_n129_b1"] == (3, 129, 48, 1, False) and len(specs) == 12 + 6 + 4 + 3 + 1
    assert tc.TIES == ["d3_n1", "d3_n2"] and set(tc.GENERIC) | set(tc.TIES) == set(tc.NAMES)
    # the largest launch: 4 N D + 8 + 48 + waves N doubles, waves N ints, O N bytes of dynamic LDS, below the 64 KiB of a launch
    N, D, O, waves = 256, 3, 48, 8
    assert (4 * N * D + 8 + 48 + waves * N) * 8 + waves * N * 4 + O * N == 61888 < 65536


def test_sigmas():
    """The issue's five -- 0.01, 0.2, the largest binary32 at or below 0x1.988454p-2, the next above it, 0.5 -- and the two
    binary32 neighbours whose s_eff = sqrt(sigma_d^2 + sigma^2), the quantity the kernel compares, lie either side of the
    threshold; every structure count and case start cycles through all of them over the shared-mu cases."""
    s = tc.SIGMAS
    assert s.dtype == np.float32 and len(s) == 7
    assert s[0] == np.float32(0.01) and s[1] == np.float32(0.2) and s[4] == np.float32(0.5)
    assert float(s[2]) <= tc.SIGMA_THRESHOLD < float(s[3]) and s[3] == np.nextafter(s[2], np.float32(1))
    below, above = (math.sqrt(tc.SIGMA_D ** 2 + float(v) ** 2) for v in s[5:])
    assert below <= tc.SIGMA_THRESHOLD < above and s[6] == np.nextafter(s[5], np.float32(1))
    used = set()
    for name in tc.SHARED_MU:
        values = tc.sigmas_of(name)
        assert values.dtype == np.float32 and values.shape == (tc.SPECS[name][3],)
        used.update(values.tolist())
    assert used == set(s.tolist())
    # either side of the branch inside ONE launch, in every case of four structures
    for name in tc.SHARED_MU:
        if tc.SPECS[name][3] == 4:
            sides = {math.sqrt(tc.SIGMA_D ** 2 + float(v) ** 2) <= tc.SIGMA_THRESHOLD for v in tc.sigmas_of(name)}
            assert sides == {True, False}, name


def test_the_three_branches_join():
    """sigma_normalized_score: the two small-sigma forms agree at u = 1/2 and the Ewald form agrees with them across the
    threshold once kmax is large enough for all three truncations to have converged; odd about u = 1/2 on the torus."""
    u = np.array([0.0, 0.1, 0.25, 0.49999, 0.5, 0.50001, 0.75, 0.9])
    low, high = tc.SIGMA_THRESHOLD, float(np.nextafter(np.float32(tc.SIGMA_THRESHOLD), np.float32(1)))
    a, b = tc.sigma_normalized_score(u, low, 8), tc.sigma_normalized_score(u, high, 8)
    assert np.abs(a - b).max() <= 1e-6
    left, right = tc.sigma_normalized_score(np.array([0.5 - 1e-9]), 0.1, 4), tc.sigma_normalized_score(np.array([0.5 + 1e-9]), 0.1, 4)
    assert abs(left[0] + right[0]) <= 1e-9 * abs(left[0]) + 1e-12
    for s in (0.05, 0.3, 0.45):
        assert np.abs(tc.sigma_normalized_score(u[1:], s, 6) + tc.sigma_normalized_score(1.0 - u[1:], s, 6)).max() <= 1e-9


@pytest.mark.parametrize("name", tc.NAMES)
def test_conditions_on_the_new_cases(name):
    """For the restatement alone, no structure left out: binary32 inputs in [0, 1) of the stated shapes, made the same way twice;
    resolved centres (sites >= 0.05, every structure >= 1e-3); every col_idx a permutation; on every generic case (N >= 63) the
    two lowest operation costs of EVERY structure differ by more than 1e-6 relative; on the tie cases (N = 1, 2) the lowest cost
    is shared by an operation and its inverse to rounding.
    Measured: the smallest gap of a generic structure is 1.4e-4 (d3_n256_o13); the smallest |mean exp(2 pi i x)| is 5.9e-3."""
    D, N, O, B, noising = tc.SPECS[name]
    case = tc.case(name)
    again = tc.case.__wrapped__(name)
    assert all(np.array_equal(getattr(case, key), getattr(again, key)) for key in ("x", "mu", "operations"))
    assert case.x.shape == (B, N, D) and case.mu.shape == ((B, N, D) if noising else (N, D)) and case.operations.shape == (O, D, D)
    for a in (case.x, case.mu):
        assert a.dtype == np.float32 and (a >= 0.0).all() and (a < 1.0).all()
    assert np.array_equal(case.operations, tc.point_group(D)[:O]) and case.shared == (not noising) and case.generic == (N >= 63)
    lengths = [np.abs(np.exp(2j * np.pi * a.astype(np.float64)).mean(axis=-2)).min() for a in (case.x, case.mu)]
    assert lengths[0] >= tc.MIN_STRUCTURE_CENTRE and lengths[1] >= (tc.MIN_STRUCTURE_CENTRE if noising else tc.MIN_SITE_CENTRE)
    got = tc.solution(name)
    assert np.array_equal(np.sort(got.col_idx, axis=2), np.broadcast_to(np.arange(N), (B, O, N)))
    assert (got.image >= 0.0).all() and (got.image < 1.0).all() and np.isfinite(got.costs).all()
    gaps = tc.operation_gaps(got.costs)
    print(f"{name}: smallest operation gap {gaps.min():.2e}, smallest centre length {min(lengths):.2e}")
    if case.generic:
        assert (gaps > tc.OPERATION_GAP).all(), gaps
    elif N == 1:
        assert (got.costs <= tc.single_atom_cost_bar(D)).all()
    else:
        assert (gaps <= 1e-12).all(), gaps


def test_the_first_minimum_is_chosen():
    """Operations listed twice tie exactly: the restatement takes the first of the two, as torch.argmin and the kernel do."""
    case = tc.case("d3_n63")
    once = tc.align(case.x, case.mu, case.operations[:6])
    twice = tc.align(case.x, case.mu, np.repeat(case.operations[:6], 2, axis=0))
    assert np.array_equal(twice.costs[:, 0::2], once.costs) and np.array_equal(twice.costs[:, 1::2], once.costs)
    assert np.array_equal(twice.operation, 2 * once.operation) and np.array_equal(twice.image, once.image)
