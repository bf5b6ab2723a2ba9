"""The spectrum estimator's persistent kernel on capped grids: one child process under the diagnostic build, whose COMMS_GRID_CAP =
1, 3 and 7 makes every wave take five or more chunks (tests/spectrum_children.py), at N = 64 and 1024, K = 3 and 97."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "comms_rs_amd", "lib", "libcomms_hip_diag.so")  # build()'s diagnostic build: the only one with the knob

pytestmark = pytest.mark.gpu


def test_spectrum_on_capped_grids():
    assert os.path.exists(DIAG_LIB), "the diagnostic build is part of build(): %s" % DIAG_LIB
    env = dict(os.environ, COMMS_HIP_LIB=DIAG_LIB)
    env.pop("COMMS_GRID_CAP", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "spectrum_children.py")], env=env, capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
