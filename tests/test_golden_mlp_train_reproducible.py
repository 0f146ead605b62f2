"""The MLP-training fixtures are what tests/golden/make_golden_mlp_train.py makes from the reference today (container-only), byte
for byte, as tests/test_golden_optimizer_reproducible.py checks the optimizer ones; each is no larger than the largest optimizer
fixture.  Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from mlp_train_cases import GOLDEN_DIRECTORY, GOLDEN_FILES
from test_golden_reproducible import REFERENCE


def test_fixtures_are_small():
    largest = max(os.path.getsize(os.path.join(GOLDEN, "optimizer", name)) for name in os.listdir(os.path.join(GOLDEN, "optimizer")))
    assert sorted(os.listdir(os.path.join(GOLDEN, GOLDEN_DIRECTORY))) == sorted(GOLDEN_FILES)
    assert all(os.path.getsize(os.path.join(GOLDEN, GOLDEN_DIRECTORY, name)) <= largest for name in GOLDEN_FILES)


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_mlp_train_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_mlp_train.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == [GOLDEN_DIRECTORY] and sorted(os.listdir(tmp_path / GOLDEN_DIRECTORY)) == sorted(GOLDEN_FILES)
    for name in GOLDEN_FILES:
        assert (tmp_path / GOLDEN_DIRECTORY / name).read_bytes() == \
            open(os.path.join(GOLDEN, GOLDEN_DIRECTORY, name), "rb").read(), name
