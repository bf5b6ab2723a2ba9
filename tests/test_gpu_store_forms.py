"""The 16-byte write-through store forms of the mixer and the decimator (csrc/common.hpp: store16, write_through) against the
plain-store forms, bit for bit.  The product build takes the write-through form only for outputs above 32 MiB; the diagnostic
build's COMMS_WT_MIN_BYTES lowers that threshold (read once per process), so one child process (tests/store_forms_child.py)
loads the diagnostic build with the knob at 0 beside the product build and runs every case on both:

  mixer     n in {2, 3, 511, 512, 513, one grid sweep - 1, one grid sweep + 3}, in place and out of place: two consecutive calls
            of n samples and one call over the 2 n -- both builds equal bit for bit (`-forms`), and the second call's output
            equals the tail of the one call bit for bit (`-carry`: the phase carried over).
  decimate  8-byte elements, rate in {2, 3, 8, 100}, n_out in {1, 2, 3, 1023, 1024, 1025} and one n_out past a grid sweep; n a
            multiple of the rate and n = (n_out - 1) rate + 1 (the last kept sample is the last input sample: the paired load
            reads in[(n_out - 1) rate] at most); output 16-byte aligned and 8 bytes on (the 8-byte kernel): equal to
            oracle.decimate and to the product build, guard bytes around the output untouched.
  elemN     elements of 1, 2, 4 and 16 bytes: the unchanged kernel, still exact.
  chain     mixer -> decimate -> mixer -> decimate twice on the same buffers on one stream without a host synchronisation:
            round 2 repeats round 1 (the oscillators are back at their start phase) and both equal the product build's.

No tolerance anywhere: the mixer's arithmetic is the same in both forms and the decimator copies bytes.

The `-forms` cases compare the two builds under an arbitrary oscillator (dphase 0.2 pi); the `-carry` cases use dphase = T / 1024,
whose advance over one grid sweep is a whole number of turns: only there are the rotor a lane steps from sweep to sweep and the
closed form a second call evaluates the same f64 numbers (tests/store_forms_child.py: mixer_case; NOTES.md, "Store forms")."""
import os
import subprocess
import sys

import pytest

import store_forms_child as child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def results():
    env = dict(os.environ, **{child.KNOB: "0"})
    env.pop("COMMS_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "store_forms_child.py")], env=env, capture_output=True, text=True,
                         timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("done"), out.stdout[-3000:] + out.stderr[-3000:]
    return dict(line.split(" ", 2)[1:3] for line in out.stdout.splitlines() if line.startswith("case "))


@pytest.mark.parametrize("case", child.CASES)
def test_store_form(results, case):
    assert results.get(case, "not run").split(" ")[0] == "ok", results.get(case)
