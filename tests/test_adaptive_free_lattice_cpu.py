"""The adaptive corrector with a FREE lattice: the CPU oracle against the reference's recorded trajectories
(tests/golden/make_golden_adaptive.py), and the fixtures themselves regenerated from the reference byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_cases
import nets
from conftest import GOLDEN, ROOT, load_golden, torus_rel_l2
from oracle import reference_sampler as RS
from test_golden_reproducible import REFERENCE

FILES = [name + ".npz" for name in adaptive_cases.FREE_LATTICE]


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))


@pytest.mark.parametrize("name", list(adaptive_cases.FREE_LATTICE))
def test_adaptive_free_lattice_trajectories(oracle, name):
    """tests/test_oracle_golden.py::test_adaptive_corrector_trajectories for the lattice branch: the reference computes the
    lattice step size from one lattice draw and updates with the next, and the oracle consumes exactly those draws."""
    g = load_golden(name + ".npz")
    noise_kw, sampling_kw, netf = adaptive_cases.FREE_LATTICE[name]
    npar, spar = adaptive_cases.cases.as_objects(noise_kw, sampling_kw)
    net = nets.fake_net(spar.num_atom_types) if netf is None else nets.load_fixture_weights(netf(None), g)
    replay = RS.ReplayNoise(g)
    gen = RS.OracleAdaptiveCorrectorGenerator(npar, spar, net, noise=replay)
    gen.record = True
    out = gen.sample(int(g["batch"]))
    assert replay.exhausted()
    assert np.array_equal(out.A, g["final_A"])
    x_err, l_err = torus_rel_l2(out.X, g["final_X"]), _rel_l2(out.L, g["final_L"])
    print(f"{name}: X torus rel-L2 {x_err:.2e}, L rel-L2 {l_err:.2e}")
    assert x_err < 1e-5
    assert l_err < 1e-5
    predictors = [r for r in gen.records if r[0] == "predictor"]
    assert len(predictors) == len(g["pred_index"])
    for k, r in enumerate(predictors):
        assert np.array_equal(r[3].X, r[2].X) and np.array_equal(r[3].L, r[2].L)       # the predictor leaves X and L untouched
        assert np.array_equal(r[3].A, g["pred_composition_im1_A"][k])
    # the reference's own records say the same of its predictor
    assert np.array_equal(g["pred_composition_im1_X"], g["pred_composition_i_X"])
    assert np.array_equal(g["pred_composition_im1_L"], g["pred_composition_i_L"])
    # and its corrector moves the lattice: the fixture exercises the branch
    assert not np.array_equal(g["corr_corrected_composition_i_L"], g["corr_composition_i_L"])


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_adaptive_free_lattice_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_adaptive.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / name).read_bytes() == open(os.path.join(GOLDEN, name), "rb").read(), name
