"""The rate-matching kernels on one MI355X: ratematch_tx_kernel and ratematch_rx_kernel at rate 3/4 (pattern 1,1,0,1,1,0) on
65536 frames of N = 140 coded bits and on 256 frames of N = 4108, with and without the 17-column interleaver, beside

  copy    a plain device copy of the bytes the launch moves (the records read plus the records written), as one copy of
          half that many bytes, timed in the same run

There is no earlier device route to compare with (the bits used to be picked on the host), so no ratio is promised.  Each
direction is timed twice: the project's KernelTimer (the launch alone) and an event pair around the whole run_dev call.
Median over ROUNDS rounds of the median of REPS calls, kernel and copy taking turns, one process, after a warm-up that lets
the clocks settle.  Prints one line per cell and writes them to profiles/ratematch_bench.txt (`--out PATH` for another
file); `--json` adds a JSON line.  No pass / fail figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS, ROUNDS = 20, 3
PATTERN = (1, 1, 0, 1, 1, 0)
COLS = 17


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


def cell(res, lines, direction, frames, N, cols, rng):
    E = int(np.count_nonzero(np.resize(np.array(PATTERN, np.uint8), N)))
    scramble = np.packbits(rng.integers(0, 2, E, dtype=np.uint8), bitorder="little")
    node = (c.RateMatchNode if direction == "tx" else c.RateDematchNode)(N, PATTERN, cols, scramble=scramble)
    if direction == "tx":
        data = rng.integers(0, 256, frames * node.in_frame_bytes, dtype=np.uint8)
    else:
        data = (8.0 * rng.standard_normal(frames * E)).astype(np.float32).view(np.uint8)
    d_in = torch.from_numpy(data).to("cuda:0")
    d_out = torch.empty(frames * node.out_frame_bytes, dtype=torch.uint8, device="cuda:0")
    timer = c.KernelTimer(REPS).attach(node)
    moved = frames * (node.in_frame_bytes + node.out_frame_bytes)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")

    def once():
        node.run_dev(d_in.data_ptr(), frames, d_out.data_ptr(), STREAM)

    # the records are those of the host-pointer form (the tests hold both to the numpy reference)
    once()
    torch.cuda.synchronize()
    few = min(frames, 64)
    host = node.run(data[: few * node.in_frame_bytes].view(np.uint8 if direction == "tx" else np.float32))
    same = bool(np.array_equal(d_out.cpu().numpy()[: few * node.out_frame_bytes], host.view(np.uint8).reshape(-1)))
    per = {"call": [], "kernel": [], "copy": []}
    for r in range(ROUNDS):
        for k in (("node", "copy") if r % 2 == 0 else ("copy", "node")):
            if k == "node":
                timer.reset()
                per["call"].append(timed_events(once))
                per["kernel"].append(float(np.median(timer.read_ms()) * 1e3))
            else:
                per["copy"].append(timed_events(lambda: dst.copy_(src)))
    row = {k: float(np.median(v)) for k, v in per.items()}
    row.update(frames=frames, n_coded=N, n_tx=E, cols=cols, bytes_moved=int(moved), records_equal_host_form=same,
               gbyte_per_s_kernel=moved / row["kernel"] * 1e-3, kernel_over_copy=row["kernel"] / row["copy"])
    name = "%s_frames%d_N%d_cols%d" % (direction, frames, N, cols)
    line = ("%-28s kernel alone %.1f us = %.1f GB/s moved   whole call %.1f us   copy of %.2f MB %.1f us   kernel / copy %.2f   "
            "records equal the host form: %s   [%s]" % (name, row["kernel"], row["gbyte_per_s_kernel"], row["call"], 1e-6 * moved, row["copy"],
                                                        row["kernel_over_copy"], same, node.kernel(frames)))
    print(line, flush=True)
    lines.append(line)
    res[name] = row
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ratematch_bench.txt")
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    res, lines = {}, ["scripts/bench_ratematch.py: rate 3/4 (1,1,0,1,1,0), scrambled, 0 or %d interleaver columns; median of %d rounds of %d calls"
                      % (COLS, ROUNDS, REPS)]
    for frames, N in ((65536, 140), (256, 4108)):
        for cols in (0, COLS):
            for direction in ("tx", "rx"):
                cell(res, lines, direction, frames, N, cols, rng)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
