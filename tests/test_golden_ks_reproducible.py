"""The Kolmogorov-Smirnov fixtures are what tests/golden/make_golden_ks.py makes from the reference today (container-only), byte
for byte, as tests/test_golden_consistency_reproducible.py checks the consistency ones.  Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from ks_cases import FILES
from test_golden_reproducible import REFERENCE


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_ks_fixtures_reproduce(tmp_path):
    pytest.importorskip("scipy.stats")                       # the reference's class calls scipy.stats.ks_2samp
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_ks.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == ["ks"] and sorted(os.listdir(tmp_path / "ks")) == sorted(FILES)
    assert sorted(os.listdir(os.path.join(GOLDEN, "ks"))) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / "ks" / name).read_bytes() == open(os.path.join(GOLDEN, "ks", name), "rb").read(), name
