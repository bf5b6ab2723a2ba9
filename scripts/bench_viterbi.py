"""The Viterbi decoder on one MI355X: viterbi_kernel at K = 7, n = 2 (171, 133), terminated, on 256 frames of 2048
information bits and on 65536 frames of 64, in decoded information bits per second, beside

  copy    a plain device copy of the bytes the launch moves (the LLR records read plus the bit records written), as one copy
          of half that many bytes

There is no earlier device route to compare with (the soft values used to be decoded on the host), so no ratio is promised.
The LLRs are those of a noisy channel (about 4 % raw errors), made on the host once.  The decoder is timed twice: the
project's KernelTimer (the launch alone) and an event pair around the whole run_dev call.  Median over ROUNDS rounds of the
median of REPS calls, decoder and copy taking turns, one process, after a warm-up that lets the clocks settle.  Prints one
line per cell and writes them to profiles/viterbi_bench.txt; `--json` adds a JSON line.  No pass / fail figure."""
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
K, GENS = 7, (0o171, 0o133)


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


def coded_llrs(frames, T, rng):
    """LLRs 2 y / sigma^2 of the coded bits of random frames at Es/N0 = 5 dB (unit components), f32 (frames, 2 * steps)."""
    u = rng.integers(0, 2, (frames, T), dtype=np.uint8)
    steps = T + K - 1
    pad = np.zeros((frames, K - 1 + steps), np.uint8)
    pad[:, K - 1: K - 1 + T] = u
    coded = np.zeros((frames, steps, 2), np.uint8)
    for j, g in enumerate(GENS):
        for e in range(K):
            if (g >> e) & 1:
                coded[:, :, j] ^= pad[:, e: e + steps]
    sigma = 10.0 ** (-5.0 / 20.0)
    y = (1.0 - 2.0 * coded.reshape(frames, -1)) + sigma * rng.standard_normal((frames, 2 * steps))
    return u, (2.0 * y / sigma ** 2).astype(np.float32)


def cell(res, lines, frames, T, rng):
    u, llr = coded_llrs(frames, T, rng)
    node = c.ViterbiNode(T, K, GENS, qscale=8.0)
    d_llr = torch.from_numpy(llr).to("cuda:0")
    d_bits = torch.empty(frames * node.out_frame_bytes, dtype=torch.uint8, device="cuda:0")
    timer = c.KernelTimer(REPS).attach(node)
    moved = frames * (node.in_frame_bytes + node.out_frame_bytes)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")

    def once():
        node.run_dev(d_llr.data_ptr(), frames, d_bits.data_ptr(), None, STREAM)

    once()
    torch.cuda.synchronize()
    got = np.unpackbits(d_bits.cpu().numpy().reshape(frames, -1), axis=1, bitorder="little")[:, :T]
    errors = int(np.count_nonzero(got != u))
    per = {"call": [], "kernel": [], "copy": []}
    for r in range(ROUNDS):
        for k in (("viterbi", "copy") if r % 2 == 0 else ("copy", "viterbi")):
            if k == "viterbi":
                timer.reset()
                per["call"].append(timed_events(once))
                per["kernel"].append(float(np.median(timer.read_ms()) * 1e3))
            else:
                per["copy"].append(timed_events(lambda: dst.copy_(src)))
    row = {k: float(np.median(v)) for k, v in per.items()}
    row.update(frames=frames, info_bits=T, bytes_moved=int(moved), bit_errors=errors,
               gbit_per_s_kernel=frames * T / row["kernel"] * 1e-3, gbit_per_s_call=frames * T / row["call"] * 1e-3)
    name = "frames%d_T%d" % (frames, T)
    line = ("%-18s kernel alone %.1f us = %.2f Gbit/s decoded   whole call %.1f us = %.2f Gbit/s   copy of %.2f MB %.1f us   "
            "%d bit errors of %d   [%s]" % (name, row["kernel"], row["gbit_per_s_kernel"], row["call"], row["gbit_per_s_call"], 1e-6 * moved,
                                            row["copy"], errors, frames * T, node.kernel(frames)))
    print(line, flush=True)
    lines.append(line)
    res[name] = row
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    res, lines = {}, ["scripts/bench_viterbi.py: K = 7, n = 2 (171, 133), terminated, qscale 8, Es/N0 = 5 dB; median of %d rounds of %d calls"
                      % (ROUNDS, REPS)]
    for frames, T in ((256, 2048), (65536, 64)):
        cell(res, lines, frames, T, rng)
    with open(os.path.join(ROOT, "profiles", "viterbi_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
