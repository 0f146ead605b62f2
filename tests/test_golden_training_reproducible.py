"""The training fixture is what tests/golden/make_golden_training.py makes from the reference today (container-only), byte for
byte, as tests/test_golden_regression_reproducible.py checks the regression ones.  Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_golden_reproducible import REFERENCE
from training_cases import FILES


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_training_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_training.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == ["training"] and sorted(os.listdir(tmp_path / "training")) == sorted(FILES)
    assert sorted(os.listdir(os.path.join(GOLDEN, "training"))) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / "training" / name).read_bytes() == open(os.path.join(GOLDEN, "training", name), "rb").read(), name
