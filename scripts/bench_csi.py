"""The channel-state kernels on one MI355X, each beside the kernel it derives from and beside

  copy    a plain device copy of the bytes the launch moves (everything read plus everything written), as one copy of half
          that many bytes, event-pair timed in the same run

  demod   ofdm_demod_kernel<N, true> (records and one channel-state record of D floats per frame) against ofdm_demod_kernel<N>
          on the same frames, N = 64 (802.11a's map) and N = 1024, two training symbols;
  demap   the weighted LLR form of demap_axis_kernel / demap_table_kernel against the plain LLR form on the same 2^24 symbols,
          for QPSK, 16-QAM, 64-QAM and 8-PSK, with weight periods 48 (a channel-state record), 1 (a scale per frame) and F (a
          weight per symbol).

Each cell is timed by the project's KernelTimer (the launch alone).  Median over ROUNDS rounds of the median of REPS calls, the
two kernels and the copy taking turns, one process, after a warm-up that lets the clocks settle.  Before it is timed the
channel-state form's records are compared with the plain form's, and the weighted form's with all weights 1.0 likewise.  Prints
one line per cell and writes them to profiles/csi_bench.txt (`--out PATH` for another file); `--json` adds a JSON line.  No pass /
fail figure."""
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
FRAME = 48 * 85     # symbols per demapper record: 85 OFDM symbols of 48 data carriers


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


def rounds(timers, calls, moved):
    """{name: us} of every call in `calls` ({name: (timer, fn)}) and of the copy of `moved` bytes, taking turns."""
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    per = {k: [] for k in list(calls) + ["copy"]}
    order = list(calls) + ["copy"]
    for r in range(ROUNDS):
        for k in (order if r % 2 == 0 else order[::-1]):
            if k == "copy":
                per[k].append(timed_events(lambda: dst.copy_(src)))
            else:
                timers[k].reset()
                timed_events(calls[k])
                per[k].append(float(np.median(timers[k].read_ms()) * 1e3))
    return {k: float(np.median(v)) for k, v in per.items()}


def carrier_map(n):
    kind = np.zeros(n, np.uint8)
    edge = 26 if n == 64 else n // 2 - n // 8
    for f in range(-edge, edge + 1):
        if f:
            kind[f % n] = 2 if (abs(f) in (7, 21) if n == 64 else f % 16 == 8) else 1
    return kind


def demod_cell(res, lines, n_fft, n_cp, n_syms, n_samples, rng):
    kind = carrier_map(n_fft)
    q = int(np.count_nonzero(kind == 2))
    unit = lambda k: np.exp(2j * np.pi * rng.random(k)).astype(np.complex64)  # noqa: E731
    node = c.OfdmDemodNode(n_fft, n_cp, kind, pilots=unit(q), train=unit(n_fft), n_train=2, n_syms=n_syms)
    frames = n_samples // node.frame_samples
    D = node.data_carriers
    x = (rng.standard_normal((frames, node.frame_samples)) + 1j * rng.standard_normal((frames, node.frame_samples))).astype(np.complex64)
    d_in = torch.from_numpy(x).to("cuda:0")
    d_out = torch.empty(frames * node.data_syms, dtype=torch.complex64, device="cuda:0")
    d_out2 = torch.empty_like(d_out)
    d_csi = torch.empty(frames * D, dtype=torch.float32, device="cuda:0")
    timer = c.KernelTimer(REPS + 3).attach(node)
    calls = {"plain": lambda: node.run_dev(d_in.data_ptr(), frames, d_out.data_ptr(), STREAM),
             "csi": lambda: node.run_dev(d_in.data_ptr(), frames, d_out2.data_ptr(), STREAM, csi_ptr=d_csi.data_ptr())}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(d_out.view(torch.float32), d_out2.view(torch.float32)))
    moved = 8 * frames * (node.frame_samples + node.data_syms)
    row = rounds({"plain": timer, "csi": timer}, calls, moved)
    row.update(frames=frames, bytes_moved=int(moved), csi_bytes=int(4 * frames * D), same_records=same, csi_over_plain=row["csi"] / row["plain"],
               plain_over_copy=row["plain"] / row["copy"])
    name = "demod_n%d" % n_fft
    line = ("%-22s plain %8.1f us   with csi %8.1f us (x %.3f, %5.1f MB of csi beside %6.1f MB)   copy %7.1f us   plain / copy %5.2f   "
            "same records: %s   [%s]" % (name, row["plain"], row["csi"], row["csi_over_plain"], 1e-6 * row["csi_bytes"], 1e-6 * moved, row["copy"],
                                         row["plain_over_copy"], same, node.kernel(frames)))
    print(line, flush=True)
    lines.append(line)
    res[name] = row
    timer.close()


def demap_cells(res, lines, name, m, table, n, rng):
    frames = n // FRAME
    n = frames * FRAME
    step = float(np.abs(table).max()) / np.sqrt(table.size)
    sym = table[rng.integers(0, table.size, n)] + (0.3 * step * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    d_sym = torch.from_numpy(np.ascontiguousarray(sym, np.complex64)).to("cuda:0")
    node = c.DemapNode(m, table, FRAME).set_llr_scale(0.5)
    d_out = torch.empty(frames * FRAME * m, dtype=torch.float32, device="cuda:0")
    d_out2 = torch.empty_like(d_out)
    timer = c.KernelTimer(REPS + 3).attach(node)
    for P in (48, 1, FRAME):
        d_w = torch.ones(frames * P, dtype=torch.float32, device="cuda:0")
        calls = {"plain": lambda: node.run_dev(d_sym.data_ptr(), frames, d_out.data_ptr(), STREAM),
                 "weighted": lambda: node.run_dev(d_sym.data_ptr(), frames, d_out2.data_ptr(), STREAM, weight_ptr=d_w.data_ptr(), weight_period=P)}
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        same = bool(torch.equal(d_out.view(torch.int32), d_out2.view(torch.int32)))
        d_w.copy_(torch.from_numpy(np.exp(rng.uniform(np.log(0.01), np.log(100.0), frames * P)).astype(np.float32)))
        moved = n * (8 + 4 * m)
        row = rounds({"plain": timer, "weighted": timer}, calls, moved)
        row.update(symbols=n, bits_per_sym=m, period=P, bytes_moved=int(moved), weight_bytes_read=int(4 * n), same_with_ones=same,
                   weighted_over_plain=row["weighted"] / row["plain"], plain_over_copy=row["plain"] / row["copy"])
        cell = "demap_%s_p%d" % (name, P)
        line = ("%-22s plain %8.1f us   weighted %8.1f us (x %.3f; 4 B more per symbol beside %2d B: x %.3f)   copy %7.1f us   plain / copy "
                "%5.2f   ones give the plain bytes: %s   [%s]" % (cell, row["plain"], row["weighted"], row["weighted_over_plain"], 8 + 4 * m,
                                                                  1 + 4.0 / (8 + 4 * m), row["copy"], row["plain_over_copy"], same, node.kernel(frames)))
        print(line, flush=True)
        lines.append(line)
        res[cell] = row
        del d_w
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "csi_bench.txt")
    n = 1 << (int(sys.argv[sys.argv.index("--n-log2") + 1]) if "--n-log2" in sys.argv else N_LOG2)
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    del warm
    rng = np.random.default_rng(3)
    res, lines = {}, ["scripts/bench_csi.py: 2^%d samples / symbols; median of %d rounds of %d calls" % (n.bit_length() - 1, ROUNDS, REPS)]
    demod_cell(res, lines, 64, 16, 85, n, rng)
    demod_cell(res, lines, 1024, 72, 14, n, rng)
    for name, m, table in (("qpsk", 2, c.qam_table(2)), ("16qam", 4, c.qam_table(4)), ("64qam", 6, c.qam_table(6)), ("8psk", 3, c.psk_table(3))):
        demap_cells(res, lines, name, m, table, n, rng)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
