"""The frame-check kernels on one MI355X: crc_attach_kernel and crc_check_kernel on 65536 frames of 64 + 16 bits (X-25's
parameters; two payload words, group 2) and on 256 frames of 2048 + 24 bits (CRC24A; 64 payload words, group 64), beside

  copy    a plain device copy of the bytes the launch moves (the records read plus everything written), as one copy of
          half that many bytes, timed in the same run

There is no earlier device route to compare with (a CRC used to be a host loop over frames), so no ratio is promised.  Each
direction is timed twice: the project's KernelTimer (the launch alone) and an event pair around the whole run_dev call.  The
check writes all four outputs.  Median over ROUNDS rounds of the median of REPS calls, kernel and copy taking turns, one
process, after a warm-up that lets the clocks settle.  Prints one line per cell and writes them to profiles/crc_bench.txt
(`--out PATH` for another file); `--json` adds a JSON line.  No pass / fail figure."""
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
CELLS = ((65536, 64, (16, 0x1021, 0xFFFF, 0xFFFF)), (256, 2048, (24, 0x864CFB, 0, 0)))


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


def cell(res, lines, direction, frames, T, params, rng):
    att = c.CrcAttachNode(*params, T)
    node = att if direction == "attach" else c.CrcCheckNode(*params, T)
    payload = rng.integers(0, 256, (frames, att.in_frame_bytes), dtype=np.uint8)
    data = payload if direction == "attach" else att.run(payload)        # the check reads good frames
    d_in = torch.from_numpy(data.reshape(-1)).to("cuda:0")
    d_out = torch.empty(frames * node.out_frame_bytes, dtype=torch.uint8, device="cuda:0")
    d_pass = torch.empty(frames, dtype=torch.int32, device="cuda:0")
    d_crc = torch.empty(frames, dtype=torch.int32, device="cuda:0")
    d_failed = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    timer = c.KernelTimer(REPS).attach(node)
    moved = frames * (node.in_frame_bytes + node.out_frame_bytes + (8 if direction == "check" else 0))
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")

    def once():
        if direction == "attach":
            node.run_dev(d_in.data_ptr(), frames, d_out.data_ptr(), STREAM)
        else:
            node.run_dev(d_in.data_ptr(), frames, d_out.data_ptr(), d_pass.data_ptr(), d_crc.data_ptr(), d_failed.data_ptr(), STREAM)

    # the records are those of the host-pointer form (the tests hold both to the bit-serial reference)
    once()
    torch.cuda.synchronize()
    few = min(frames, 64)
    host = node.run(data[:few])
    host = host if direction == "attach" else host[0]
    same = bool(np.array_equal(d_out.cpu().numpy()[: few * node.out_frame_bytes], host.reshape(-1)))
    if direction == "check":
        same = same and bool(d_pass.cpu().numpy().all()) and int(d_failed.cpu()[0]) == 0
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
    row.update(frames=frames, n_payload_bits=T, width=params[0], bytes_moved=int(moved), records_equal_host_form=same,
               gbyte_per_s_kernel=moved / row["kernel"] * 1e-3, kernel_over_copy=row["kernel"] / row["copy"])
    name = "%s_frames%d_T%d_W%d" % (direction, frames, T, params[0])
    line = ("%-30s kernel alone %.1f us = %.1f GB/s moved   whole call %.1f us   copy of %.2f MB %.1f us   kernel / copy %.2f   "
            "records equal the host form: %s   [%s]" % (name, row["kernel"], row["gbyte_per_s_kernel"], row["call"], 1e-6 * moved, row["copy"],
                                                        row["kernel_over_copy"], same, node.kernel(frames)))
    print(line, flush=True)
    lines.append(line)
    res[name] = row
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "crc_bench.txt")
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    res, lines = {}, ["scripts/bench_crc.py: attach and check (all four outputs), good frames; median of %d rounds of %d calls" % (ROUNDS, REPS)]
    for frames, T, params in CELLS:
        for direction in ("attach", "check"):
            cell(res, lines, direction, frames, T, params, rng)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
