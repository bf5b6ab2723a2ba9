"""Runs the C++ host-graph test of the spectrum estimator nodes (tests/host/test_spectrum_nodes_gpu.cpp) on the GPU box: SpectrumNode
in a graph over messages of uneven lengths and SpectrumNodeDev, against a direct DFT in double precision."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_cpp_spectrum_nodes():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "comms_rs_amd", "host"), "-s"], timeout=600)
    out = subprocess.run([os.path.join(ROOT, "comms_rs_amd", "lib", "test_spectrum_nodes_gpu")], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all passed" in out.stdout
