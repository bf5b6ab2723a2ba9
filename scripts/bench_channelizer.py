"""The polyphase channelizer on one MI355X (device pointers, events around each call; median over ROUNDS rounds of the
median of REPS calls, the forms taking turns round by round, one process):

  node    ChannelizerNode (one launch, channelizer_kernel), channel-major and frame-major
  series  the SAME handle forced to its series of M chain launches (the diagnostic build's COMMS_CHANNELIZER_SERIES; the
          chain kernels are the parent commit's).  The series reads the input M times: it is timed on the first
          n_s = min(n, 2^28 / M) samples of the cell's input, SERIES_REPS calls, and scaled by n / n_s.  At M = 1024
          n_s is 2^18 and the 1024 launches are launch-bound there, so the scaled figure overstates the series; its floor
          at the full n is M reads of the input, 8 M n bytes at the HBM rate (NOTES.md sets the node against that too)
  copy    a plain device copy of the node's footprint, 8 n + 8 M frames bytes read or written

for M in {8, 64, 1024}, D in {M, M / 2}, N in {4 M, 16 M}, at 2^24 and 2^26 input samples.  Runs on the diagnostic build
(comms_rs_amd/lib/libcomms_hip_diag.so, part of build()) unless COMMS_HIP_LIB names another library; `--no-series` skips
the series.  Prints one line per cell; `--json` adds a JSON summary line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("COMMS_HIP_LIB", os.path.join(ROOT, "comms_rs_amd", "lib", "libcomms_hip_diag.so"))
os.environ.pop("COMMS_CHANNELIZER_SERIES", None)
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS = 10
SERIES_REPS = 2
ROUNDS = 3
SERIES_READS = 1 << 28   # samples the series reads per call: M n_s
WITH_SERIES = "--no-series" not in sys.argv


def timed(fn, reps):
    fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)  # us


def lowpass(M, N):
    """Windowed sinc with its cutoff at half a channel spacing, unit gain at DC."""
    k = np.arange(N) - (N - 1) / 2
    return (np.sinc(k / M) / M * np.hamming(N)).astype(np.float32)


def rounds(runs):
    per = {k: [] for k in runs}
    keys = list(runs)
    for r in range(ROUNDS):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            per[k].append(timed(*runs[k]))
    return {k: float(np.median(v)) for k, v in per.items()}


def cell(res, M, D, N, sizes):
    taps = lowpass(M, N)
    nodes = {"node": c.ChannelizerNode(taps, M, D), "node_frame_major": c.ChannelizerNode(taps, M, D, layout="frame")}
    for n in sizes:
        x = torch.view_as_complex((torch.rand(2 * n, dtype=torch.float32, device="cuda:0") * 2 - 1).view(n, 2))
        frames = -(-n // D)
        outs = {k: torch.empty(M * frames, dtype=torch.complex64, device="cuda:0") for k in nodes}
        name = "M%d_D%d_N%d_n%d" % (M, D, N, n)
        runs = {}
        for k, node in nodes.items():
            runs[k] = (lambda node=node, out=outs[k]: node.run_dev(x.data_ptr(), n, out.data_ptr(), STREAM), REPS)
        half = (n + M * frames) // 2
        src, dst = torch.empty(half, dtype=torch.complex64, device="cuda:0"), torch.empty(half, dtype=torch.complex64, device="cuda:0")
        runs["copy"] = (lambda: dst.copy_(src), REPS)
        n_s = min(n, max(SERIES_READS // M // D * D, D))
        if WITH_SERIES:
            ser = nodes["node"]
            sout = torch.empty(M * (n_s // D), dtype=torch.complex64, device="cuda:0")

            def series():
                os.environ["COMMS_CHANNELIZER_SERIES"] = "1"
                try:
                    ser.run_dev(x.data_ptr(), n_s, sout.data_ptr(), STREAM)
                finally:
                    del os.environ["COMMS_CHANNELIZER_SERIES"]

            runs["series"] = (series, SERIES_REPS)
        kernel = nodes["node"].kernel(n)
        row = rounds(runs)
        line = "%-26s node %9.1f us (frame-major %9.1f)   copy of %7.1f MB %8.1f us, copy / node = %.2f" % (
            name, row["node"], row["node_frame_major"], 8e-6 * (n + M * frames), row["copy"], row["copy"] / row["node"])
        if WITH_SERIES:
            scaled = row["series"] * n / n_s
            row["series_n"] = n_s
            row["series_scaled"] = scaled
            line += "   series %10.1f us at n_s = %d -> %12.1f us scaled, series / node = %.0f" % (row["series"], n_s, scaled, scaled / row["node"])
        print(line + "   [" + kernel + "]", flush=True)
        res[name] = row
        del x, outs, src, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    res = {}
    for M in (8, 64, 1024):
        for D in (M, M // 2):
            for N in (4 * M, 16 * M):
                cell(res, M, D, N, (1 << 24, 1 << 26))
    if "--json" in sys.argv:
        print(json.dumps(res))
