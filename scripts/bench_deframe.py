"""The deframer on one MI355X: deframe_kernel on 2^24 symbols with one frame per 2^16 symbols (F = 2048: 256 frames) and one
per 256 symbols (F = 64: 65536 frames), QPSK, BITS and LLR output, beside

  route   what the node replaces: per frame, comms_mixer_run_dev at -arg(corr) on a pointer offset, then
          comms_sym_to_bits_dev: two launches and a host loop per frame, hard bits only (the amplitude is not applied)
  copy    a plain device copy of the bytes the launch moves (8 B read per payload symbol plus the record written), as one
          copy of half that many bytes

The detections are made on the host (index, a rotation), so that the frame synchroniser is not part of the figure.  Every
deframer call ends synchronised, so it is timed twice: an event pair around the call (descriptor upload, launch and the
host's wait included) and the project's KernelTimer (the launch alone); the route and the copy by event pairs.  Median over
ROUNDS rounds of the median of REPS calls (the route: ROUTE_REPS, it takes up to a second per pass), the forms taking turns
round by round, one process, after a warm-up that lets the clocks settle.  Prints one line per cell; `--json` adds a JSON
line.  No pass / fail figure."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS, ROUTE_REPS, ROUNDS = 20, 3, 3
P = 32


def timed_events(fn, reps=REPS, warm=3):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)  # us


def cell(res, x, n, F, spacing, fmt):
    index = np.arange(1000, n - P - F, spacing, dtype=np.uint64)
    dets = np.zeros(index.size, c.FRAME_DETECTION_DTYPE)
    ang = 0.37 * np.arange(index.size)
    dets["index"], dets["corr_re"], dets["corr_im"], dets["metric"], dets["energy"] = index, 64 * np.cos(ang), 64 * np.sin(ang), 1.0, 64.0
    nf = index.size
    node = c.DeframeNode(F, P, P - 2, normalise=True, word_energy=64.0).set_output_format(fmt)
    fb = node.frame_bytes()
    out = torch.empty(nf * fb, dtype=torch.uint8, device="cuda:0")
    timer = c.KernelTimer(REPS).attach(node)
    mixer = c.MixerNode(0.0, 0.0)
    pay = torch.empty(F, dtype=torch.complex64, device="cuda:0")
    bits = torch.empty(nf * (F // 4), dtype=torch.uint8, device="cuda:0")
    moved = nf * (8 * F + fb)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")

    def deframe_once():
        node.set_position(0)
        got = node.run_dev(x.data_ptr(), n, dets, out.data_ptr(), nf, stream=STREAM)
        assert got == nf

    def deframe():
        timer.reset()
        t = timed_events(deframe_once)
        return t, float(np.median(timer.read_ms()) * 1e3)

    def route_once():
        for f in range(nf):
            mixer.phase = -ang[f]
            mixer.run_dev(x.data_ptr() + 8 * (int(index[f]) + P), F, pay.data_ptr(), STREAM)
            c.sym_to_bits_dev(pay.data_ptr(), F, 2, bits.data_ptr() + f * (F // 4), stream=STREAM)

    per = {"deframe": [], "deframe_kernel": [], "route": [], "copy": []}
    order = ["deframe", "route", "copy"]
    for r in range(ROUNDS):
        for k in order[r % 3:] + order[:r % 3]:
            if k == "deframe":
                t, tk = deframe()
                per["deframe"].append(t)
                per["deframe_kernel"].append(tk)
            elif k == "route":
                per["route"].append(timed_events(route_once, ROUTE_REPS, 1))
            else:
                per["copy"].append(timed_events(lambda: dst.copy_(src)))
    row = {k: float(np.median(v)) for k, v in per.items()}
    row["frames"], row["bytes_moved"] = int(nf), int(moved)
    name = "n%d_F%d_%s" % (n, F, fmt)
    print("%-20s deframe %.1f us (kernel alone %.1f) [%s]   route (%d x 2 launches) %.1f us   copy of %.2f MB %.1f us   "
          "route / deframe = %.1f   deframe kernel / copy = %.2f"
          % (name, row["deframe"], row["deframe_kernel"], node.kernel(nf), nf, row["route"], 1e-6 * moved, row["copy"],
             row["route"] / row["deframe"], row["deframe_kernel"] / row["copy"]), flush=True)
    res[name] = row
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    n = 1 << 24
    rng = np.random.default_rng(3)
    y = ((1 - 2 * rng.integers(0, 2, n)) + 1j * (1 - 2 * rng.integers(0, 2, n))) * np.exp(0.37j)
    x = torch.from_numpy((y + 0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)).to("cuda:0")
    res = {}
    for F, spacing in ((2048, 1 << 16), (64, 256)):
        for fmt in ("bits", "llr"):
            cell(res, x, n, F, spacing, fmt)
    if "--json" in sys.argv:
        print(json.dumps(res))
