"""The checks of tests/test_gpu_csi.py that also run on capped grids, and the child process that runs them there:
`python csi_children.py` makes every handle under COMMS_GRID_CAP = 1 and 3 (the diagnostic build, which the parent selects
through COMMS_HIP_LIB, as tests/test_gpu_small_grids.py does), so that a workgroup walks several (frame, block) items and a
lane several symbols.  The first failure ends the process: nothing is launched behind it.  The last line is "ok"."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import csi_ref as cr  # noqa: E402
import ofdm_ref as r  # noqa: E402
import symmap_ref as sr  # noqa: E402

KNOB = "COMMS_GRID_CAP"
CAPS = (1, 3)
GUARD = 256


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


def check_csi(c, kind, name, cpe, n_frames, cap=None):
    """One case of csi_ref.csi_cases(): the record against ref_csi within the bound, the demodulator's records byte for byte,
    the call split in two, and the device form with a guard behind the record."""
    f, rx, want = cr.csi_case(kind, name, cpe, n_frames)
    args, kw = f.node_args()
    dem = make(lambda: c.OfdmDemodNode(*args, **kw), cap)
    k = fields(dem.kernel(n_frames))
    assert cap is None or (k["max_grid"] == cap and k["grid"] == min(k["items"], cap)), k
    rec, g = dem.run(rx, csi=True)
    assert g.dtype == np.float32 and g.shape == (n_frames, f.D) and dem.data_carriers == f.D
    err = float(cr.csi_errors(g, want).max())
    print("%-8s %-16s cpe %d frames %d cap %s: csi off by %.3e, bound %.3e, blocks %d" % (kind, name, cpe, n_frames, cap, err, cr.CSI_BOUND, k["blocks"]))
    assert err <= cr.CSI_BOUND, (kind, name, cpe, n_frames, cap, err)
    assert rec.tobytes() == dem.run(rx).tobytes()
    if n_frames > 2:
        a, b = dem.run(rx[:2], csi=True), dem.run(rx[2:], csi=True)
        assert np.concatenate([a[0], b[0]]).tobytes() == rec.tobytes() and np.concatenate([a[1], b[1]]).tobytes() == g.tobytes()
    # device form: the record is written whole, the guard behind it is not touched
    d_in = c.DeviceBuf(rx.nbytes).upload(rx)
    d_out = c.DeviceBuf(rec.nbytes)
    d_csi = c.DeviceBuf(g.nbytes + GUARD).upload(np.full(g.nbytes + GUARD, 0xFF, np.uint8))
    dem.run_dev(d_in.ptr, n_frames, d_out.ptr, csi_ptr=d_csi.ptr)
    raw = d_csi.download(np.uint8, g.nbytes + GUARD)
    assert np.all(raw[g.nbytes:] == 0xFF), "the guard region was written"
    assert raw[: g.nbytes].tobytes() == g.tobytes() and d_out.download(np.uint8, rec.nbytes).tobytes() == rec.tobytes()
    return k


def demap_node(c, name, F, force_table, cap=None):
    m, table, arg, _ = sr.table_of(name)
    return m, table, make(lambda: c.DemapNode(m, arg, F, force_table=force_table), cap)


def check_weighted(c, name, F, P, n_frames, force_table, cap=None):
    """One shape of the weighted demapper against ref_weighted_llr, byte for byte; all weights 1.0 against DemapNode.run."""
    m, table, node = demap_node(c, name, F, force_table, cap)
    node.set_llr_scale(0.75)
    z = sr.demap_input(table, n_frames * F, 7 + F).reshape(n_frames, F)
    w = cr.weights_for(F, P, n_frames, 9 + F)
    got = node.run(z, weights=w)
    want = cr.ref_weighted_llr(z.ravel(), w, table, F, 0.75)
    k = node.kernel(n_frames)
    assert got.shape == want.shape and sr.same_floats(got, want), (name, F, P, n_frames, force_table, cap, k)
    wj = w[:, np.arange(F) % P].ravel()
    erased = got.reshape(-1, m)[~(np.isfinite(wj) & (wj > 0))]
    assert erased.size and not erased.view(np.uint32).any()
    assert node.run(z, weights=np.ones((n_frames, P), np.float32)).tobytes() == node.run(z).tobytes()
    assert ("form=table" in k) == (force_table or sr.table_of(name)[3] is None)
    return k


def main():
    import comms_rs_amd as c

    assert c.device_count() >= 1
    for cap in CAPS:
        for kind, name, cpe in cr.csi_cases():
            for n_frames in r.FRAME_COUNTS:
                check_csi(c, kind, name, cpe, n_frames, cap)
        passes = 0
        for name in cr.WEIGHT_TABLES:
            for force_table in (False, True):
                for F, P in cr.WEIGHT_SHAPES:
                    for n_frames in cr.WEIGHT_FRAMES:
                        k = fields(check_weighted(c, name, F, P, n_frames, force_table, cap))
                        assert k["max_grid"] == cap and k["grid"] <= cap
                        passes = max(passes, -(-k["items"] // (k["grid"] * k["wg"])))
        print("weighted demapper cap %d: up to %d passes per lane" % (cap, passes))
        assert passes >= (3 if cap == 1 else 1)
    print("ok")


if __name__ == "__main__":
    main()
