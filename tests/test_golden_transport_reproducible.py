"""The optimal-transport fixtures are what tests/golden/make_golden_transport.py makes from the reference today (container-only),
byte for byte, as tests/test_golden_analytical_reproducible.py checks the analytical ones.  Skipped where the reference is absent."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT
from test_golden_reproducible import REFERENCE

FILES = [name + ".npz" for name in ("d1_n3", "d2_n3", "d3_n5", "d3_n8", "d3_n8_identity", "d3_n2_ties", "toy1d", "d3_n64", "d3_n65",
                                    "noising_d3_n8")]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="the reference is not on this machine")
def test_transport_fixtures_reproduce(tmp_path):
    env = dict(os.environ, PYTHONPATH=REFERENCE, MDX_GOLDEN_OUT=str(tmp_path))
    run = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_transport.py")], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    assert os.listdir(tmp_path) == ["transport"] and sorted(os.listdir(tmp_path / "transport")) == sorted(FILES)
    assert sorted(os.listdir(os.path.join(GOLDEN, "transport"))) == sorted(FILES)
    for name in FILES:
        assert (tmp_path / "transport" / name).read_bytes() == open(os.path.join(GOLDEN, "transport", name), "rb").read(), name
