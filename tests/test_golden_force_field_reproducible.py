"""The force-field fixtures are what tests/golden/make_golden_force_field.py makes from the reference today (container-only),
byte for byte, as tests/test_golden_reproducible.py checks make_golden.py's.  Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_golden_reproducible import REFERENCE

FILES = ["ff_c3.npz", "ff_images.npz", "ff_clipped.npz"]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_force_field_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_force_field.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / name).read_bytes() == open(os.path.join(GOLDEN, name), "rb").read(), name
