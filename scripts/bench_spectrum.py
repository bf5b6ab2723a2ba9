"""The spectrum estimator on one MI355X: SpectrumNode at N = 64, 256 and 1024 over 2^24 samples per call, Hann window, H = N / 2,
as a waterfall (K = 8: one launch, a row per eight segments) and as one power spectral density per call (K = the 2^24 / H
segments of a call: spectrum_kernel and spectrum_rows_kernel), each beside

  copy    a plain device copy of the bytes the call moves (input read plus rows written; with K > 32 the chunk sums written and
          read as well), as one copy of half that many bytes, event-pair timed in the same run
  fft     comms_fft_run_dev (FFTBatchNode) on as many contiguous N-point transforms as the call has segments: no window, no
          overlap, no power, and N complex values written per transform

`kernel` is spectrum_kernel alone, timed by the project's KernelTimer; `call` is the whole run_dev call between two events on the
stream (both launches where there are two).  Median over ROUNDS rounds of the median of REPS calls, the four taking turns, one
process, after a warm-up that lets the clocks settle.  The handle streams on from call to call: every timed call completes
2^24 / H segments.  Before the timing the rows of a 2^18-sample call are held to a float64 reference.  Prints one line per cell
and writes them to profiles/spectrum_bench.txt (`--out PATH` for another file); `--json` adds a JSON line.  No pass / fail figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS, ROUNDS = 10, 3
N_LOG2 = 24


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


def check(n, hop, x):
    """Rows of a short call against numpy, as the largest row error over the row's total."""
    node = c.SpectrumNode(n, "hann", hop, 8)
    got = node.run(x).astype(np.float64)
    w = c.window_taps("hann", n).astype(np.float64)
    idx = np.arange(got.shape[0] * 8)[:, None] * hop + np.arange(n)[None, :]
    p = np.abs(np.fft.fft(x[idx].astype(np.complex128) * w, axis=1)) ** 2
    want = float(np.float32(node.scale)) * p.reshape(-1, 8, n).sum(axis=1)
    return float(np.max(np.abs(got - want).sum(axis=1) / want.sum(axis=1)))


def cell(res, lines, n, total, d_x, x_head):
    hop = n // 2
    segs = total // hop
    err = check(n, hop, x_head)
    fft = c.FFTBatchNode(n, False)
    d_f = torch.empty(segs * n, dtype=torch.complex64, device="cuda:0")
    d_g = torch.empty(segs * n, dtype=torch.complex64, device="cuda:0")
    d_rows = torch.empty((segs // 8 + 2) * n, dtype=torch.float32, device="cuda:0")
    for what, avg in (("waterfall", 8), ("psd", segs)):
        node = c.SpectrumNode(n, "hann", hop, avg)
        call = lambda: node.run_dev(d_x.data_ptr(), total, d_rows.data_ptr(), STREAM)  # noqa: E731
        call()   # the first call is one segment short; the timed ones stream on
        torch.cuda.synchronize()
        name = node.kernel(total)
        rows = node.out_len(total)
        chunks = (segs + 31) // 32 if avg > 32 else 0
        moved = 8 * total + 4 * rows * n + 2 * 4 * chunks * n
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
        timers = {"kernel": c.KernelTimer(REPS + 3).attach(node), "fft": c.KernelTimer(REPS + 3).attach(fft)}
        calls = {"kernel": call, "fft": lambda: fft.run_dev(d_f.data_ptr(), segs * n, d_g.data_ptr(), STREAM)}
        per = {k: [] for k in ("kernel", "call", "fft", "copy")}
        order = ("kernel", "fft", "copy")
        for r in range(ROUNDS):
            for k in (order if r % 2 == 0 else order[::-1]):
                if k == "copy":
                    per[k].append(timed_events(lambda: dst.copy_(src)))
                else:
                    timers[k].reset()
                    t = timed_events(calls[k])
                    per[k].append(float(np.median(timers[k].read_ms()) * 1e3))
                    if k == "kernel":
                        per["call"].append(t)
        row = {k: float(np.median(v)) for k, v in per.items()}
        row.update(n_fft=n, hop=hop, avg=avg, segments=segs, rows=rows, bytes_moved=int(moved), check_row_err=err)
        row["kernel_over_copy"], row["call_over_copy"], row["call_over_fft"] = row["kernel"] / row["copy"], row["call"] / row["copy"], row["call"] / row["fft"]
        line = ("n%-5d %-9s K=%-7d spectrum_kernel alone %8.1f us   call %8.1f us = %6.1f GB/s moved, %6.2f Gsample/s   copy of %6.1f MB "
                "%7.1f us   call / copy %5.2f   fft of %d x %d %7.1f us   call / fft %5.2f   check: row error %.1e of the row   [%s]"
                % (n, what, avg, row["kernel"], row["call"], moved / row["call"] * 1e-3, total / row["call"] * 1e-3, 1e-6 * moved, row["copy"],
                   row["call_over_copy"], segs, n, row["fft"], row["call_over_fft"], err, name))
        print(line, flush=True)
        lines.append(line)
        res["n%d_%s" % (n, what)] = row
        for t in timers.values():
            t.close()
        del src, dst


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "spectrum_bench.txt")
    total = 1 << (int(sys.argv[sys.argv.index("--n-log2") + 1]) if "--n-log2" in sys.argv else N_LOG2)
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    del warm
    x = c.synth_iq(total, 0)
    d_x = torch.from_numpy(x).to("cuda:0")
    res, lines = {}, ["scripts/bench_spectrum.py: 2^%d samples per call, Hann window, H = N / 2; median of %d rounds of %d calls"
                      % (total.bit_length() - 1, ROUNDS, REPS)]
    for n in (64, 256, 1024):
        cell(res, lines, n, total, d_x, x[: 1 << 18])
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
