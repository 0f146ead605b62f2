"""A float64 restatement of the transport alignment kernel (csrc/mdx_transport.hip: transport_align_kernel<1 | 2 | 4>, behind
mdx_transport_align and mdx_equivariant_analytical_score), the cases that reach every instantiation up to 256 atoms, and the bars
of tests/test_transport_align_elements_gpu.py.  tests/test_transport_cases_cpu.py holds the restatement to the reference's own
binary64 records (tests/golden/transport/) and checks the conditions on the cases, without a GPU.

The restatement is plain numpy float64 on the binary32 inputs promoted once, as the kernel does, stage by stage:
  wrap01      y - floor(y), with 1.0 mapped to 0
  centre      atan2(mean sin 2 pi x, mean cos 2 pi x) / 2 pi per dimension;  x~ = wrap01(x - centre(x)), mu~ likewise
  cost        C_o[i, j] = sum_d (delta - rint delta)^2, delta = (R_o mu~)_j - x~_i
  solve       scipy.optimize.linear_sum_assignment per operation (scipy is the tests' alone); cost_o = sum_i C_o[i, col_o[i]]
  choose      the first arg-min of cost_o in operation order
  image       wrap01(R mu~[col])
  score       sigma . s(wrap01(x~ - image), s_eff, kmax) / s_eff, s_eff = sqrt(sigma_d^2 + sigma^2), s the three-branch
              sigma_normalized_score of csrc/mdx_wrapped_score.hpp with its binary32 threshold constant 0x1.988454p-2
`chosen` evaluates the image and the cost of ANY (operation, col_idx), so that a test can hold what the kernel reports to the
restatement's own numbers as well as what scipy chose.

The cases follow the recipe of tests/golden/make_golden_transport.py, seeded: sites drawn until |mean exp(2 pi i site)| >= 0.05 in
every dimension; the first half of a batch uniform in the cell, the second half a random permutation of the sites plus noise of
width sigma_d = 0.02 plus a random global translation, wrapped into [0, 1).  The point groups are the 2, 8 and 48 signed
permutation matrices, generated here with the identity first.  The per-structure-mu cases are the noising transform's use: x
uniform, mu = x noised at 0.1, the identity alone.

Bars (each written down before any GPU run):
  COST_BAR    1e-12 relative: the project's bar between two binary64 evaluations of an optimum (the CPU test shows the
              restatement and the reference 2e-15 apart).
  IMAGE_BAR   2^-24 on the torus per element: one rounding to binary32 of a value in [0, 1) is at most 2^-25.
  score       |got - want| <= 2^-24 |want| (1 + 2^-10) + SCORE_F max_structure |want|: the one rounding to binary32, and
              SCORE_F = 500 SCORE_RESTATEMENT_DISTANCE = 9.5e-12, where SCORE_RESTATEMENT_DISTANCE = 1.9e-14 is the largest distance
              between the restatement and the reference's binary64 score on the fixtures (a fraction of the structure's largest
              |score64|, printed and asserted by the CPU test; 1.9e-14 on d3_n8_identity at sigma 0.5, above the 1.7e-14 of the other
              six fixtures, hence 500 times the record and not a round 1e-11), four orders below the rounding term.
  N = 1       is degenerate for everything but the image: x~ and mu~ are the roundings of x - centre(x), exactly 0 in exact
              arithmetic, so every cost and every score is the square or a multiple of ROUNDING noise and there is nothing to be
              relative to.  The centre carries the roundings of 2 pi x, of the sine and the cosine, of atan2 and of the division, a
              few 2^-53 of a turn: each of x~, mu~ lies within CENTRE_NOISE = 2^-50 of 0 on the torus in either evaluation.  Hence
              at N = 1 a cost is at most D (2 CENTRE_NOISE)^2 (single_atom_cost_bar: an absolute bar, about 1e-29 where a wrong
              cost is of order 0.1), and a score, whose slope in the residual is at most sigma / s_eff^2 near 0, is at most
              2 CENTRE_NOISE sigma / s_eff^2 in either evaluation, so two differ by 4 CENTRE_NOISE sigma / s_eff^2 at most
              (single_atom_score_bar, added to the bar above; it also covers the sums over k = -kmax .. kmax of the score at
              u = 0, which are antisymmetric and cancel only to a few 2^-53 of their largest term, whatever the order of the sum).
              Measured on an MI355X at N = 1: both evaluations give costs of exactly 0 and scores of 1e-17, 0.003 of this bar --
              and 1e70 of the relative bar alone.  Every case with N >= 2 is held to the relative bars alone.
"""
import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np
from scipy.optimize import linear_sum_assignment

TWO_PI = 2.0 * math.pi
SIGMA_THRESHOLD = float.fromhex("0x1.988454p-2")      # 1 / sqrt(2 pi) in binary32, as the reference compares with in either precision
SIGMA_D = 0.02
NOISING_SIGMA = 0.1
MIN_SITE_CENTRE = 0.05

COST_BAR = 1e-12
IMAGE_BAR = 2.0 ** -24
EPS32 = 2.0 ** -24
SCORE_RESTATEMENT_DISTANCE = 1.9e-14     # measured by tests/test_transport_cases_cpu.py, which asserts it is not exceeded
SCORE_F = 500 * SCORE_RESTATEMENT_DISTANCE
CENTRE_NOISE = 2.0 ** -50
OPERATION_GAP = 1e-6                     # the two lowest operation costs of a generic structure differ by more, relative
MIN_STRUCTURE_CENTRE = 1e-3              # |mean exp(2 pi i x)| of every structure: the centre's rounding is amplified by 1 / this

KMAX = (2, 4)
_T32 = np.float32(SIGMA_THRESHOLD)
# s_eff, not sigma, is what the kernel compares with the threshold: the two binary32 sigmas whose s_eff lie either side of it
_AT_BRANCH = np.float32(math.sqrt(SIGMA_THRESHOLD ** 2 - SIGMA_D ** 2))


def _straddle():
    def s_eff(s):
        return math.sqrt(SIGMA_D ** 2 + float(s) ** 2)
    s = _AT_BRANCH
    while s_eff(s) <= SIGMA_THRESHOLD:
        s = np.nextafter(s, np.float32(1))
    while s_eff(s) > SIGMA_THRESHOLD:
        s = np.nextafter(s, np.float32(0))
    return s, np.nextafter(s, np.float32(1))


SIGMAS = np.array([0.01, 0.2, _T32, np.nextafter(_T32, np.float32(1)), 0.5, *_straddle()], dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
def wrap01(y):
    y = np.asarray(y, dtype=np.float64)
    r = y - np.floor(y)
    return np.where(r == 1.0, 0.0, r)


def centre(x):
    """The atan2 centre of x [..., N, D] per dimension: [..., D]."""
    x = np.asarray(x, dtype=np.float64)
    return np.arctan2(np.sin(TWO_PI * x).mean(axis=-2), np.cos(TWO_PI * x).mean(axis=-2)) / TWO_PI


def invariant(x):
    x = np.asarray(x, dtype=np.float64)
    return wrap01(x - centre(x)[..., None, :])


def rotate(operation, m):
    """(R m_j)_d of every atom j of m [N, D]."""
    return np.asarray(m, dtype=np.float64) @ np.asarray(operation, dtype=np.float64).T


def cost_matrix(xt, rotated):
    """C[i, j] = sum_d (delta - rint delta)^2, delta = rotated_j - x~_i, the dimensions added in order."""
    total = np.zeros((xt.shape[0], rotated.shape[0]))
    for d in range(xt.shape[1]):
        delta = rotated[None, :, d] - xt[:, None, d]
        g = delta - np.rint(delta)
        total += g * g
    return total


def chosen(xt, mt, operations, operation, col_idx):
    """(image [N, D], cost) of one structure under operation index `operation` and the assignment col_idx (row i of x takes
    column col_idx[i] of mu), whoever chose them."""
    rotated = rotate(operations[operation], mt)[np.asarray(col_idx, dtype=np.int64)]
    delta = rotated - xt
    g = delta - np.rint(delta)
    return wrap01(rotated), float((g * g).sum(axis=1).sum())


def align(x, mu, operations, keep_matrices=0):
    """Every stage for x f32 [B, N, D], mu f32 [N, D] or [B, N, D], operations [O, D, D]: a namespace of xt, mt [B, N, D], costs
    [B, O], col_idx [B, O, N], operation [B], image [B, N, D] (and `matrices` [keep_matrices, O, N, N])."""
    x = np.asarray(x, dtype=np.float64)
    B, N, D = x.shape
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), x.shape)
    operations = np.asarray(operations, dtype=np.float64)
    O = operations.shape[0]
    xt, mt = invariant(x), invariant(mu)
    costs, col_idx = np.empty((B, O)), np.empty((B, O, N), dtype=np.int64)
    image = np.empty((B, N, D))
    matrices = np.empty((keep_matrices, O, N, N))
    rows = np.arange(N)
    for b in range(B):
        for o in range(O):
            matrix = cost_matrix(xt[b], rotate(operations[o], mt[b]))
            if b < keep_matrices:
                matrices[b, o] = matrix
            col_idx[b, o] = linear_sum_assignment(matrix)[1]
            costs[b, o] = matrix[rows, col_idx[b, o]].sum()
    operation = np.argmin(costs, axis=1)          # the first minimum
    for b in range(B):
        image[b] = chosen(xt[b], mt[b], operations, operation[b], col_idx[b, operation[b]])[0]
    return SimpleNamespace(xt=xt, mt=mt, costs=costs, col_idx=col_idx, operation=operation, image=image, matrices=matrices)


def sigma_normalized_score(u, s, kmax):
    """sigma x score of one wrapped Gaussian of width s at u in [0, 1), truncated at |k| <= kmax: the three branches of
    csrc/mdx_wrapped_score.hpp (small sigma with u < 1/2 and u >= 1/2; the Ewald form above the threshold)."""
    u = np.asarray(u, dtype=np.float64)[..., None]
    k = np.arange(-kmax, kmax + 1, dtype=np.float64)
    if s <= SIGMA_THRESHOLD:
        arg = np.where(u < 0.5, k * k + 2.0 * u * k, (k * k - 1.0) + 2.0 * u * (k + 1.0))
        e = np.exp(-0.5 * arg * (1.0 / (s * s)))
        return (-u[..., 0] - (k * e).sum(axis=-1) / e.sum(axis=-1)) / s
    upk, sg = u + k, s * k
    e_upk = np.exp(-math.pi * upk * upk)
    combination = math.sqrt(TWO_PI) * s * np.exp(-2.0 * math.pi * math.pi * sg * sg) - np.exp(-math.pi * k * k)
    angle = TWO_PI * (u * k)
    z = e_upk.sum(axis=-1) + (combination * np.cos(angle)).sum(axis=-1)
    d = (upk * e_upk).sum(axis=-1) + (k * combination * np.sin(angle)).sum(axis=-1)
    return s * (-TWO_PI * d) / z


def score(xt, image, sigmas, sigma_d_square, kmax):
    """The fused score [B, N, D] of aligned structures, one binary32 sigma per structure."""
    out = np.empty_like(xt)
    for b, sigma in enumerate(np.asarray(sigmas, dtype=np.float32).astype(np.float64)):
        s_eff = math.sqrt(sigma_d_square + sigma * sigma)
        out[b] = sigma * sigma_normalized_score(wrap01(xt[b] - image[b]), s_eff, kmax) / s_eff
    return out


def torus(a, b):
    """|a - b| on the torus, per element."""
    diff = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return np.abs(diff - np.rint(diff))


def score_bar(want, sigmas=None, sigma_d_square=None):
    """The per-element bar of the fused score (module docstring); the N = 1 form when the structures have one atom."""
    largest = np.abs(want).reshape(want.shape[0], -1).max(axis=1)[:, None, None]
    bar = EPS32 * np.abs(want) * (1.0 + 2.0 ** -10) + SCORE_F * largest
    if want.shape[1] == 1:
        bar = bar + single_atom_score_bar(sigmas, sigma_d_square)[:, None, None]
    return bar


def single_atom_score_bar(sigmas, sigma_d_square):
    sigma = np.asarray(sigmas, dtype=np.float32).astype(np.float64)
    return 4.0 * CENTRE_NOISE * sigma / (sigma_d_square + sigma * sigma)


def single_atom_cost_bar(D):
    return D * (2.0 * CENTRE_NOISE) ** 2


# ---------------------------------------------------------------------------------------------------------------------------
# the point groups
@functools.lru_cache(maxsize=None)
def point_group(D):
    """The 2^D D! signed permutation matrices f32 [O, D, D], the identity first."""
    matrices = []
    for permutation in itertools.permutations(range(D)):
        for signs in itertools.product((1.0, -1.0), repeat=D):
            m = np.zeros((D, D), dtype=np.float32)
            for r in range(D):
                m[r, permutation[r]] = signs[r]
            matrices.append(m)
    out = np.stack(matrices)
    out.setflags(write=False)
    return out


def as_set(operations):
    return {tuple(np.asarray(m, dtype=np.int64).reshape(-1).tolist()) for m in operations}


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
SPECS = {}          # name -> (D, N, O, B, per-structure mu)


def _spec(name, D, N, O, B=4, noising=False):
    assert name not in SPECS
    SPECS[name] = (D, N, O, B, noising)


for _n in (1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256):
    _spec(f"d3_n{_n}", 3, _n, 48)
for _d, _o in ((1, 2), (2, 8)):
    for _n in (65, 129, 256):
        _spec(f"d{_d}_n{_n}", _d, _n, _o)
for _o, _n in ((1, 129), (5, 129), (13, 129), (13, 256)):
    _spec(f"d3_n{_n}_o{_o}", 3, _n, _o)
for _n in (65, 129, 256):
    _spec(f"noising_d3_n{_n}", 3, _n, 1, noising=True)
_spec("d3_n129_b1", 3, 129, 48, B=1)

NAMES = list(SPECS)
SHARED_MU = [name for name in NAMES if not SPECS[name][4]]
GENERIC = [name for name in NAMES if SPECS[name][1] >= 63]
TIES = [name for name in NAMES if SPECS[name][1] < 63]
SEEDS = {}          # a case whose default seed (its index) misses a condition of the CPU test gets another here


def _wrapped32(y):
    y = np.remainder(y.astype(np.float32), np.float32(1.0)).astype(np.float32)
    y[y == 1.0] = 0.0
    return y


def _sites(rng, N, D):
    for _ in range(1000):
        sites = rng.random((N, D), dtype=np.float32)
        if (np.abs(np.exp(2j * np.pi * sites.astype(np.float64)).mean(axis=0)) >= MIN_SITE_CENTRE).all():
            return sites
    raise RuntimeError("no sites with a resolved centre in 1000 draws")


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case, made once and never written to: name, D, N, O, B, operations f32 [O, D, D], x f32 [B, N, D], mu f32
    [N, D] (shared) or [B, N, D], shared, generic."""
    D, N, O, B, noising = SPECS[name]
    rng = np.random.default_rng(SEEDS.get(name, 20260000 + NAMES.index(name)))
    operations = np.ascontiguousarray(point_group(D)[:O])
    x = np.empty((B, N, D), dtype=np.float32)
    if noising:
        assert O == 1
        x[:] = rng.random((B, N, D), dtype=np.float32)
        mu = _wrapped32(x + np.float32(NOISING_SIGMA) * rng.standard_normal((B, N, D), dtype=np.float32))
    else:
        mu = _sites(rng, N, D)
        for b in range(B):
            if b < B // 2:
                x[b] = rng.random((N, D), dtype=np.float32)
            else:
                noise = np.float32(SIGMA_D) * rng.standard_normal((N, D), dtype=np.float32)
                x[b] = _wrapped32(mu[rng.permutation(N)] + noise + rng.random((1, D), dtype=np.float32))
    for a in (operations, x, mu):
        assert a.dtype == np.float32
        a.setflags(write=False)
    return SimpleNamespace(name=name, D=D, N=N, O=O, B=B, operations=operations, x=x, mu=mu, shared=not noising, generic=N >= 63,
                           sigma_d=SIGMA_D, sigma_d_square=SIGMA_D ** 2)


@functools.lru_cache(maxsize=None)
def solution(name):
    """align() of a case: made once, shared by the tests that need it, never written to."""
    c = case(name)
    s = align(c.x, c.mu, c.operations)
    for a in vars(s).values():
        a.setflags(write=False)
    return s


def sigmas_of(name):
    """One sigma per structure, cycling through SIGMAS from another start in every case."""
    B = SPECS[name][3]
    return SIGMAS[(np.arange(B) + NAMES.index(name)) % len(SIGMAS)]


def operation_gaps(costs):
    """(second lowest - lowest) / lowest of the operation costs, per structure; infinite with one operation, 0 where the lowest
    cost is 0."""
    if costs.shape[1] < 2:
        return np.full(costs.shape[0], np.inf)
    two = np.sort(costs, axis=1)[:, :2]
    difference = two[:, 1] - two[:, 0]
    return np.divide(difference, two[:, 0], out=np.zeros_like(difference), where=two[:, 0] > 0.0)
