"""The excise-and-random fixtures are what tests/golden/make_golden_excise_and_random.py makes from the reference today
(container-only), byte for byte, as tests/test_golden_excise_and_repaint_reproducible.py checks the excise-and-repaint ones.
Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

import excise_random_cases as rc
from conftest import GOLDEN, ROOT
from test_golden_reproducible import REFERENCE

FILES = [name + ".npz" for name in rc.case_names()]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_excise_and_random_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_excise_and_random.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == ["excise_and_random"] and sorted(os.listdir(tmp_path / "excise_and_random")) == sorted(FILES)
    assert sorted(os.listdir(os.path.join(GOLDEN, "excise_and_random"))) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / "excise_and_random" / name).read_bytes() == \
            open(os.path.join(GOLDEN, "excise_and_random", name), "rb").read(), name
