"""Persistent kernels on capped grids.  The diagnostic build's COMMS_GRID_CAP lowers resident_workgroups() (csrc/common.hpp), so
a handle made under cap 1, 3 or 7 walks a call of a few tens of thousands of samples in four or more passes per workgroup, wave
or lane: third and fourth passes over the same LDS image, survivor slot or workspace slot, the grid-dependent steps at residues
the full chip never gives them, and both sides of the rate-matching and Viterbi form seams.  The cases are
tests/grid_cases.py's (tests/test_grid_cases.py holds them to their rules); tests/grid_children.py runs one node family per
child process, against the node's own reference at its own bound and bit for bit against an uncapped handle."""
import os
import subprocess
import sys

import pytest

import grid_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIAG_LIB = os.path.join(ROOT, "comms_rs_amd", "lib", "libcomms_hip_diag.so")  # build()'s diagnostic build: the only one with the knob

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_family_on_capped_grids(family):
    assert os.path.exists(DIAG_LIB), "the diagnostic build is part of build(): %s" % DIAG_LIB
    env = dict(os.environ, COMMS_HIP_LIB=DIAG_LIB)
    env.pop("COMMS_GRID_CAP", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "grid_children.py"), family], env=env, capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]


def test_the_knob_is_the_diagnostic_builds_alone():
    """Under the product library the variable changes nothing: the handle reports the full chip's grid."""
    code = r'''
import os, re, sys
sys.path.insert(0, %r)
import comms_rs_amd as c
os.environ["COMMS_GRID_CAP"] = "3"
k = c.ConvEncoderNode(40, 7, (0o133, 0o171, 0o165)).kernel(10 ** 7)
assert int(re.search(r"max_grid=(\d+)", k).group(1)) == 8 * 256, k
print("ok")
''' % ROOT
    env = dict(os.environ)
    env.pop("COMMS_HIP_LIB", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr
