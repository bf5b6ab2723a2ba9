"""The soft demapper's kernels on one MI355X: 2^24 symbols through demap_axis_kernel (the per-axis form a separable table gets)
and demap_table_kernel (the general form, forced with COMMS_DEMAP_TABLE) for QPSK, 16-, 64- and 256-QAM, and through the table
form alone for 8-PSK (not separable), LLR and BITS output, each beside

  copy    a plain device copy of the bytes the launch moves (the symbols read plus the records written), as one copy of half
          that many bytes, event-pair timed in the same run

Each cell is timed by the project's KernelTimer (the launch alone).  Median over ROUNDS rounds of the median of REPS calls,
kernel and copy taking turns, one process, after a warm-up that lets the clocks settle.  Before it is timed every cell's output
is compared with the other form's (the tests hold both to the brute-force reference).  Prints one line per cell and writes them
to profiles/demap_bench.txt (`--out PATH` for another file); `--json` adds a JSON line.  No pass / fail figure."""
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
FRAME = 1 << 12   # symbols per record
CELLS = (("qpsk", 2, lambda: c.qam_table(2)), ("16qam", 4, lambda: c.qam_table(4)), ("64qam", 6, lambda: c.qam_table(6)),
         ("256qam", 8, lambda: c.qam_table(8)), ("8psk", 3, lambda: c.psk_table(3)))


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


def cell(res, lines, name, m, table, fmt, d_sym, n, outputs):
    frames = n // FRAME
    forms = ("axis", "table") if "form=axis" in c.DemapNode(m, table, FRAME).kernel(1) else ("table",)
    for form in forms:
        node = c.DemapNode(m, table, FRAME, force_table=(form == "table")).set_output_format(fmt).set_llr_scale(0.5)
        assert ("form=%s" % form) in node.kernel(frames), node.kernel(frames)
        out_bytes = frames * node.out_frame_bytes
        d_out = torch.empty(out_bytes, dtype=torch.uint8, device="cuda:0")
        timer = c.KernelTimer(REPS + 3).attach(node)
        moved = 8 * n + out_bytes
        src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")

        def once():
            node.run_dev(d_sym.data_ptr(), frames, d_out.data_ptr(), STREAM)

        once()
        torch.cuda.synchronize()
        key = (name, fmt)
        same = True
        if key in outputs:
            same = bool(torch.equal(outputs[key], d_out))
        else:
            outputs[key] = d_out.clone()
        per = {"kernel": [], "copy": []}
        for r in range(ROUNDS):
            for k in (("node", "copy") if r % 2 == 0 else ("copy", "node")):
                if k == "node":
                    timer.reset()
                    timed_events(once)
                    per["kernel"].append(float(np.median(timer.read_ms()) * 1e3))
                else:
                    per["copy"].append(timed_events(lambda: dst.copy_(src)))
        row = {k: float(np.median(v)) for k, v in per.items()}
        row.update(symbols=n, bits_per_sym=m, bytes_moved=int(moved), equals_other_form=same, gbyte_per_s_kernel=moved / row["kernel"] * 1e-3,
                   gsym_per_s=n / row["kernel"] * 1e-3, kernel_over_copy=row["kernel"] / row["copy"])
        cell_name = "%s_%s_%s" % (name, fmt, form)
        line = ("%-18s kernel alone %8.1f us = %6.1f GB/s moved, %5.2f Gsym/s   copy of %6.1f MB %7.1f us   kernel / copy %5.2f   "
                "equal to the other form: %s   [%s]" % (cell_name, row["kernel"], row["gbyte_per_s_kernel"], row["gsym_per_s"], 1e-6 * moved,
                                                        row["copy"], row["kernel_over_copy"], same, node.kernel(frames)))
        print(line, flush=True)
        lines.append(line)
        res[cell_name] = row
        timer.close()
        del d_out, src, dst


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "demap_bench.txt")
    n = 1 << (int(sys.argv[sys.argv.index("--n-log2") + 1]) if "--n-log2" in sys.argv else N_LOG2)
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    del warm
    rng = np.random.default_rng(3)
    res, lines = {}, ["scripts/bench_demap.py: 2^%d symbols in records of %d, noisy table points; median of %d rounds of %d calls"
                      % (n.bit_length() - 1, FRAME, ROUNDS, REPS)]
    outputs = {}
    for name, m, make in CELLS:
        table = make()
        step = float(np.abs(table).max()) / np.sqrt(table.size)
        sym = table[rng.integers(0, table.size, n)] + (0.3 * step * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
        d_sym = torch.from_numpy(np.ascontiguousarray(sym, np.complex64)).to("cuda:0")
        for fmt in ("llr", "bits"):
            cell(res, lines, name, m, table, fmt, d_sym, n, outputs)
        outputs.clear()
        del d_sym
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
