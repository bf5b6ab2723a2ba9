"""The child process of tests/test_gpu_spectrum_grids.py: the spectrum estimator on capped grids.  Run under the diagnostic
library (COMMS_HIP_LIB), whose COMMS_GRID_CAP lowers resident_workgroups(): a handle made under cap 1, 3 or 7 walks its chunks in
five or more passes per wave.  Every capped handle is held to the reference's bounds and, byte for byte, to an uncapped handle."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import spectrum_ref as ref  # noqa: E402

CAPS = (1, 3, 7)
SIZES = (64, 1024)
AVGS = (3, 97)
PASSES = 5          # items per wave, at least, under the largest cap
WAVES = 4           # chunks a workgroup takes at a time


def n_segments(avg):
    """Enough segments for PASSES items per wave at cap 7 (an item is a chunk of <= 32 segments, ceil(avg / 32) per row), ending
    inside a row."""
    per_row = -(-avg // ref.CHUNK)
    rows = -(-(PASSES * WAVES * max(CAPS)) // per_row) + 1
    return rows * avg + avg // 2


def main():
    import comms_rs_amd as c

    assert c.device_count() >= 1
    for n_fft in SIZES:
        hop = n_fft // 2
        w = c.window_taps("hann", n_fft)
        for avg in AVGS:
            x = ref.signal(n_fft + (n_segments(avg) - 1) * hop + 5, 1000 + n_fft + avg)
            os.environ.pop("COMMS_GRID_CAP", None)
            full = c.SpectrumNode(n_fft, w, hop, avg)
            want = full.run(x)
            P = ref.ref_rows(x, w, hop, avg, float(np.float32(full.scale)))
            ref.check_rows(want, P, avg, "N=%d K=%d uncapped" % (n_fft, avg))
            for cap in CAPS:
                os.environ["COMMS_GRID_CAP"] = str(cap)
                node = c.SpectrumNode(n_fft, w, hop, avg)
                name = node.kernel(len(x))
                grid, items = (int(re.search(r" %s=(\d+)" % key, name).group(1)) for key in ("grid", "items"))
                assert grid == cap and "max_grid=%d " % cap in name, name
                assert items >= PASSES * WAVES * cap, name
                cut = 2 * n_fft + 1   # (a short first call: the second one keeps nearly every item)
                got = np.concatenate([node.run(x[:cut]), node.run(x[cut:])])
                ref.check_rows(got, P, avg, "N=%d K=%d cap=%d" % (n_fft, avg, cap))
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n_fft, avg, cap)
            os.environ.pop("COMMS_GRID_CAP", None)
    print("ok")


if __name__ == "__main__":
    main()
