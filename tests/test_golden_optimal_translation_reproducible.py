"""The optimal-translation fixtures are what tests/golden/make_golden_optimal_translation.py makes from the reference today
(container-only), byte for byte, as tests/test_golden_transport_reproducible.py checks the transport ones.  Skipped where the
reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_golden_reproducible import REFERENCE
from test_optimal_translation_cpu import FILES


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_optimal_translation_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_optimal_translation.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == ["optimal_translation"] and sorted(os.listdir(tmp_path / "optimal_translation")) == sorted(FILES)
    assert sorted(os.listdir(os.path.join(GOLDEN, "optimal_translation"))) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / "optimal_translation" / name).read_bytes() == \
            open(os.path.join(GOLDEN, "optimal_translation", name), "rb").read(), name
