"""The analytical-score fixtures are what tests/golden/make_golden_analytical.py makes from the reference today (container-only),
byte for byte, as tests/test_golden_force_field_reproducible.py checks the force-field ones.  Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_golden_reproducible import REFERENCE

FILES = [name + ".npz" for name in ("toy1d", "diamond", "perm4", "perm3_2d", "perm5", "perm7", "big", "kmax0", "mixed_sigma", "edges",
                                    "wrapped_gaussian")]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_analytical_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_analytical.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == ["analytical"] and sorted(os.listdir(tmp_path / "analytical")) == sorted(FILES)
    assert sorted(os.listdir(os.path.join(GOLDEN, "analytical"))) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / "analytical" / name).read_bytes() == open(os.path.join(GOLDEN, "analytical", name), "rb").read(), name
