"""The Stillinger-Weber fixtures are what tests/golden/make_golden_stillinger_weber.py makes from the reference tree today
(container-only), byte for byte, and the coefficient files are the reference's.  Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_reference_yaml_surface import REFERENCE

COEFFICIENTS = os.path.join(REFERENCE, "data", "stillinger_weber_coefficients")


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_stillinger_weber_fixtures_reproduce(tmp_path):
    env = dict(os.environ, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_stillinger_weber.py"), REFERENCE], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == ["lammps_si8_frames.npz"]
    committed = os.path.join(GOLDEN, "stillinger_weber")
    assert sorted(os.listdir(committed)) == ["Si.sw", "SiGe.sw", "lammps_si8_frames.npz"]
    assert (tmp_path / "lammps_si8_frames.npz").read_bytes() == open(os.path.join(committed, "lammps_si8_frames.npz"), "rb").read()
    for name in ("Si.sw", "SiGe.sw"):
        assert open(os.path.join(COEFFICIENTS, name), "rb").read() == open(os.path.join(committed, name), "rb").read(), name
