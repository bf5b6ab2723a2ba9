"""The child process of tests/test_gpu_symmap.py's capped-grid test: the symbol mapper and the soft demapper on handles made
under COMMS_GRID_CAP = 1, then 3 (the diagnostic build, which the parent selects through COMMS_HIP_LIB).  Per case and cap:
kernel() must report max_grid == grid == cap and four or more passes per lane; the outputs equal the reference and the bytes of
an uncapped handle of this process.  The cases are tests/symmap_ref.py's (tests/test_symmap_ref.py holds them to their rules).
The first failure ends the process: nothing is launched behind it.  The last line is "ok"."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import symmap_ref as sr  # noqa: E402

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
    for m, name, E, P, G, frames in sr.GRID_MAP_CASES:
        table = sr.table_of(name)[1]
        word = sr.noisy_points(sr.QPSK, P, 3) if P else None
        new = lambda: c.SymbolMapNode(m, table, E, word, G)  # noqa: E731
        bits = np.random.default_rng(E).integers(0, 2, (frames, E), dtype=np.uint8)
        records = sr.dirty_records(bits, 1)
        want = sr.ref_map(bits, m, table, word, G)
        plain = make(new).run(records)
        assert plain.tobytes() == want.tobytes(), (name, E)
        for cap in sr.CAPS:
            node = make(new, cap)
            k = fields(node.kernel(frames))
            assert k["max_grid"] == k["grid"] == cap and -(-k["syms"] // (cap * k["wg"])) == sr.map_passes(E, m, P, G, frames, cap) >= sr.MIN_PASSES, k
            assert node.run(records).tobytes() == plain.tobytes(), (name, E, cap)
            print("symmap %s E=%d cap %d: %d passes, exact" % (name, E, cap, sr.map_passes(E, m, P, G, frames, cap)))
    for name, F, frames in sr.GRID_DEMAP_CASES:
        m, table, given, split = sr.table_of(name)
        z = sr.demap_input(table, frames * F, F)
        want = {"llr": sr.ref_llr_records(z, table, F, 0.6), "bits": sr.ref_bits_records(z, table, F)}
        new = lambda: c.DemapNode(m, given, F).set_llr_scale(0.6)  # noqa: E731
        plain = make(new)
        for cap in sr.CAPS:
            node = make(new, cap)
            for fmt in ("llr", "bits"):
                node.set_output_format(fmt)
                plain.set_output_format(fmt)
                k = fields(node.kernel(frames))
                per = k["wg"] // 64 if fmt == "bits" else k["wg"]
                assert k["max_grid"] == k["grid"] == cap and -(-k["items"] // (cap * per)) == sr.demap_passes(F, frames, cap, fmt) >= sr.MIN_PASSES, k
                assert ("form=table" in node.kernel(frames)) == (split is None)
                got, ref = node.run(z), plain.run(z)
                assert got.tobytes() == ref.tobytes(), (name, F, cap, fmt)
                assert sr.same_floats(got, want[fmt]) if fmt == "llr" else got.tobytes() == want[fmt].tobytes(), (name, F, cap, fmt)
                print("demap %s F=%d %s cap %d: %d passes, exact" % (name, F, fmt, cap, sr.demap_passes(F, frames, cap, fmt)))
    print("ok")


if __name__ == "__main__":
    main()
