"""The OFDM synchroniser on one MI355X, both kernels at 2^24 samples.

  detect    ofdmsync_detect_kernel at (L, W, G) = (80, 80, 40), (320, 320, 160), (1280, 1280, 512), beside
            copy        a plain device copy of 8 bytes per sample (4 n read, 4 n written: the footprint of one read of the stream)
            framesync   comms_framesync_run_dev at P = 64, G = 63 on the same input
  correct   ofdmsync_correct_kernel on records of 1280 and of 20480 samples, beside
            copy        a device copy of its bytes (8 n read, 8 n written)
            mixer       comms_mixer_run_dev over the same samples as one stream

The stream is noise with one two-symbol repetition per 2^16 samples.  Calls that end synchronised (detect, framesync, correct)
are timed by the project's KernelTimer (the launch alone) and by an event pair around the call (copy-back and the host's wait
included); the copy and the mixer by event pairs.  Median over ROUNDS rounds of the median of REPS calls, the forms taking
turns round by round, one process, after a warm-up that lets the clocks settle.  Prints one line per cell; `--json` adds a
JSON line.  No pass / fail figure."""
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


def with_timer(timer, fn):
    timer.reset()
    t = timed_events(fn)
    return t, float(np.median(timer.read_ms()) * 1e3)


def rounds(forms):
    """forms: name -> callable returning one figure or a tuple of them; the median over ROUNDS, the order rotating."""
    per = {k: [] for k in forms}
    order = list(forms)
    for r in range(ROUNDS):
        for k in order[r % len(order):] + order[:r % len(order)]:
            per[k].append(forms[k]())
    return {k: np.median(np.array(v, np.float64), axis=0) for k, v in per.items()}


def detect_cell(res, n, L, W, G):
    rng = np.random.default_rng(L)
    y = (0.05 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    sym = (rng.standard_normal(L) + 1j * rng.standard_normal(L)).astype(np.complex64)
    for k in range(5000, n - 2 * L, SPACING):
        y[k: k + L] += sym
        y[k + L: k + 2 * L] += sym
    x = torch.from_numpy(y).to("cuda:0")
    node = c.OfdmSyncNode(L, W, 0.5, G)
    timer = c.KernelTimer(REPS + 3).attach(node)
    word = ((1 - 2 * rng.integers(0, 2, 64)) + 1j * (1 - 2 * rng.integers(0, 2, 64))).astype(np.complex64)
    fs = c.FrameSyncNode(word, 0.5, 63)
    fs_timer = c.KernelTimer(REPS + 3).attach(fs)
    src = torch.empty(4 * n, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(4 * n, dtype=torch.uint8, device="cuda:0")
    row = rounds({
        "detect": lambda: with_timer(timer, lambda: node.run_dev(x.data_ptr(), n, stream=STREAM, raw=True)),
        "framesync": lambda: with_timer(fs_timer, lambda: fs.run_dev(x.data_ptr(), n, stream=STREAM, raw=True)),
        "copy": lambda: timed_events(lambda: dst.copy_(src)),
    })
    node.run_dev(x.data_ptr(), n, stream=STREAM, raw=True)
    name = "detect_n%d_L%d_W%d_G%d" % (n, L, W, G)
    print("%-30s detect %.1f us (kernel alone %.1f) [%s]   framesync P=64 G=63 %.1f us (kernel alone %.1f)   copy of %.1f MB %.1f us   "
          "%d detections   detect kernel / copy = %.2f   detect kernel / framesync kernel = %.2f"
          % (name, row["detect"][0], row["detect"][1], node.kernel(n), row["framesync"][0], row["framesync"][1], 8e-6 * n, row["copy"],
             node.found, row["detect"][1] / row["copy"], row["detect"][1] / row["framesync"][1]), flush=True)
    res[name] = {"detect_us": row["detect"][0], "detect_kernel_us": row["detect"][1], "framesync_us": row["framesync"][0],
                 "framesync_kernel_us": row["framesync"][1], "copy_us": float(row["copy"]), "detections": node.found}
    timer.close()
    fs_timer.close()


def correct_cell(res, n, F):
    n_frames = n // F
    rng = np.random.default_rng(F)
    x = torch.from_numpy((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)).to("cuda:0")
    out = torch.empty_like(x)
    cfo = rng.uniform(-0.01, 0.01, n_frames)
    node = c.OfdmSyncNode(80, 80, 0.5, 40, n_frame=F)
    timer = c.KernelTimer(REPS + 3).attach(node)
    mixer = c.MixerNode(0.01)
    src = torch.empty(8 * n, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(8 * n, dtype=torch.uint8, device="cuda:0")
    row = rounds({
        "correct": lambda: with_timer(timer, lambda: node.correct_dev(x.data_ptr(), n_frames, cfo, out.data_ptr(), STREAM)),
        "mixer": lambda: timed_events(lambda: mixer.run_dev(x.data_ptr(), n, out.data_ptr(), STREAM)),
        "copy": lambda: timed_events(lambda: dst.copy_(src)),
    })
    name = "correct_n%d_F%d" % (n, F)
    print("%-30s correct %.1f us (kernel alone %.1f), %d records   mixer %.1f us   copy of %.1f MB %.1f us   "
          "correct kernel / copy = %.2f   correct kernel / mixer = %.2f"
          % (name, row["correct"][0], row["correct"][1], n_frames, row["mixer"], 16e-6 * n, row["copy"], row["correct"][1] / row["copy"],
             row["correct"][1] / row["mixer"]), flush=True)
    res[name] = {"correct_us": row["correct"][0], "correct_kernel_us": row["correct"][1], "mixer_us": float(row["mixer"]),
                 "copy_us": float(row["copy"]), "records": n_frames}
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    res = {}
    for L, W, G in ((80, 80, 40), (320, 320, 160), (1280, 1280, 512)):
        detect_cell(res, 1 << 24, L, W, G)
        torch.cuda.empty_cache()
    for F in (1280, 20480):
        correct_cell(res, 1 << 24, F)
        torch.cuda.empty_cache()
    if "--json" in sys.argv:
        print(json.dumps(res))
