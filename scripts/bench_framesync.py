"""The frame synchroniser on one MI355X: framesync_kernel at 2^24 symbols, word lengths P = 13, 64 and 512 with guard G = P - 1,
beside

  fir     comms_fir_run_dev with the P conjugated, reversed taps on the same input: the only route to c[k] before this node.
          It writes 8 B per position, normalises nothing and leaves e[k], m[k], the peak search and the threshold to the
          host (not counted)
  copy    a plain device copy of 8 bytes per symbol (4 n read, 4 n written: the footprint of one read of the stream)

The stream is noise with one word per 2^16 symbols (256 detections).  Every frame synchroniser call ends synchronised (the
detections come back to the host), so it is timed twice: an event pair around the call (launch, copy-back and the host's
wait included) and the project's KernelTimer (the launch alone); the FIR and the copy by event pairs.  Median over ROUNDS
rounds of the median of REPS calls, the forms taking turns round by round, one process, after a warm-up that lets the clocks
settle.  Prints one line per cell; `--json` adds a JSON line.  No pass / fail figure."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS, ROUNDS = 20, 5
SPACING = 1 << 16


def timed_events(fn):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)  # us


def cell(res, n, P):
    G = P - 1
    rng = np.random.default_rng(P)
    word = ((1 - 2 * rng.integers(0, 2, P)) + 1j * (1 - 2 * rng.integers(0, 2, P))).astype(np.complex64)
    y = (0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    for k in range(1000, n - P, SPACING):
        y[k: k + P] += word
    x = torch.from_numpy(y).to("cuda:0")
    out = torch.empty_like(x)
    node = c.FrameSyncNode(word, 0.5, G)
    timer = c.KernelTimer(REPS).attach(node)
    fir = c.BatchFirNode(np.conj(word[::-1]))
    src = torch.empty(4 * n, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(4 * n, dtype=torch.uint8, device="cuda:0")

    def frames():
        timer.reset()
        t = timed_events(lambda: node.run_dev(x.data_ptr(), n, stream=STREAM, raw=True))
        return t, float(np.median(timer.read_ms()) * 1e3)

    per = {"framesync": [], "framesync_kernel": [], "fir": [], "copy": []}
    order = ["framesync", "fir", "copy"]
    for r in range(ROUNDS):
        for k in order[r % 3:] + order[:r % 3]:
            if k == "framesync":
                t, tk = frames()
                per["framesync"].append(t)
                per["framesync_kernel"].append(tk)
            elif k == "fir":
                per["fir"].append(timed_events(lambda: fir.run_dev(x.data_ptr(), n, out.data_ptr(), STREAM)))
            else:
                per["copy"].append(timed_events(lambda: dst.copy_(src)))
    row = {k: float(np.median(v)) for k, v in per.items()}
    node.run_dev(x.data_ptr(), n, stream=STREAM, raw=True)
    row["detections"] = node.found
    name = "n%d_P%d_G%d" % (n, P, G)
    print("%-20s framesync %.1f us (kernel alone %.1f) [%s]   fir (algo %s) %.1f us   copy of %.1f MB %.1f us   %d detections   "
          "fir / framesync kernel = %.2f   framesync kernel / copy = %.2f"
          % (name, row["framesync"], row["framesync_kernel"], node.kernel(n), fir.algo_for(n), row["fir"], 8e-6 * n, row["copy"],
             row["detections"], row["fir"] / row["framesync_kernel"], row["framesync_kernel"] / row["copy"]), flush=True)
    res[name] = row
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    res = {}
    for P in (13, 64, 512):
        cell(res, 1 << 24, P)
        torch.cuda.empty_cache()
    if "--json" in sys.argv:
        print(json.dumps(res))
