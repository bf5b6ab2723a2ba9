"""The child process of tests/test_gpu_ofdm.py's capped-grid test: the OFDM modulator and demodulator on handles made under
COMMS_GRID_CAP = 1, then 3 (the diagnostic build, which the parent selects through COMMS_HIP_LIB).  Per case, direction and
cap: kernel() must report max_grid == grid == cap and four or more passes per workgroup; the outputs are within the bounds of
the reference and equal the bytes of an uncapped handle of this process.  The cases are tests/ofdm_ref.py's
(tests/test_ofdm_ref.py holds them to their rules).  The first failure ends the process: nothing is launched behind it.  The
last line is "ok"."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import ofdm_ref as r  # noqa: E402

KNOB = "COMMS_GRID_CAP"


def fields(name):
    return {a: int(b) for a, b in re.findall(r"(\w+)=(\d+)", name)}


def make(factory, cap=None):
    """A handle made under the cap (None: the full chip); the knob is read at create."""
    if cap is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = str(cap)
    try:
        return factory()
    finally:
        os.environ.pop(KNOB, None)


def main():
    import comms_rs_amd as c

    assert c.device_count() >= 1 and c.LIB_PATH.endswith("libcomms_hip_diag.so"), c.LIB_PATH
    for name, frames in r.GRID_CASES:
        f = r.GRID_FORMATS[name]
        args, kw = f.node_args()
        z = r.data_values(f, frames)
        rx = r.through_channel(f, r.ref_mod(f, z), r.symbol_thetas(f))
        for direction, cls, x, want, per, bound in (("mod", c.OfdmModNode, z, r.ref_mod(f, z), f.sym_len, r.FFT_BOUND),
                                                    ("demod", c.OfdmDemodNode, rx, r.ref_demod(f, rx), f.D, r.CHANNEL_BOUND)):
            new = lambda: cls(*args, **kw)  # noqa: E731
            plain = make(new).run(x)
            err = r.symbol_errors(plain, want, per).max()
            assert err <= bound, (name, direction, err)
            for cap in r.CAPS:
                node = make(new, cap)
                k = fields(node.kernel(frames))
                passes = -(-k["items"] // cap)
                assert k["max_grid"] == k["grid"] == cap and k["items"] == r.grid_items(f, direction, frames, cap), k
                assert passes == r.grid_passes(f, direction, frames, cap) >= r.MIN_PASSES, k
                assert node.run(x).tobytes() == plain.tobytes(), (name, direction, cap)
                print("ofdm %s %s cap %d: %d items, %d passes, worst symbol %.3e, bytes equal" % (direction, name, cap, k["items"], passes, err))
    print("ok")


if __name__ == "__main__":
    main()
