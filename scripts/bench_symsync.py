"""The symbol synchroniser on one MI355X: symsync_kernel at L = 32, S = 4, 33 taps per phase (rrc_taps(1025 + 31, 128, 0.35)
cut to 32 * 33 taps) for 2^24 and 2^26 input samples, Complex<f32> and 2-bit output, beside

  copy    a plain device copy of the same footprint (8 n bytes read, 8 n / S or n / S / 4 written)
  chain   ChainNode with 33 complex taps at rate 4, mixer after the FIR: the nearest existing kernel

Kernel times by the project's KernelTimer (event pairs around the launch) for the two nodes, events around the copy;
median over ROUNDS rounds of the median of REPS calls, the forms taking turns round by round, one process, after a
warm-up that lets the clocks settle.  Prints one line per cell; `--json` adds a JSON summary line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS, ROUNDS = 30, 5
L, S, PER = 32, 4, 33


def timed_node(fn, timer):
    for _ in range(3):
        fn()
    timer.reset()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    return float(np.median(timer.read_ms()) * 1e3)  # us


def timed_events(fn):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)


def cell(res, n, bits):
    taps = c.rrc_taps(L * PER + 1, float(L * S), 0.35).real[: L * PER].astype(np.float32)
    x = torch.view_as_complex((torch.rand(2 * n, dtype=torch.float32, device="cuda:0") * 2 - 1).view(n, 2))
    m = n // S
    out_bytes = (m * bits + 7) // 8 if bits else 8 * m
    out = torch.empty(out_bytes + 8, dtype=torch.uint8, device="cuda:0")
    node = c.SymbolSyncNode(taps, L, S).set_output(bits or None)
    node.timing = 0.37
    node.set_rotation(2 * np.pi * 0.01, 0.0)
    plain = c.SymbolSyncNode(taps, L, S).set_output(bits or None)   # no rotation
    plain.timing = 0.37
    chain = c.ChainNode(2 * np.pi * 0.01, 0.0, c.rrc_taps(PER, float(S), 0.35), S, False, mixer_after_fir=True)
    if bits:
        chain.set_output_format("bits", bits)
    t_node, t_plain, t_chain = c.KernelTimer(REPS).attach(node), c.KernelTimer(REPS).attach(plain), c.KernelTimer(REPS).attach(chain)
    half = (8 * n + out_bytes) // 2
    src, dst = torch.empty(half, dtype=torch.uint8, device="cuda:0"), torch.empty(half, dtype=torch.uint8, device="cuda:0")
    runs = {
        "symsync": lambda: timed_node(lambda: node.run_dev(x.data_ptr(), n, out.data_ptr(), STREAM), t_node),
        "symsync_norot": lambda: timed_node(lambda: plain.run_dev(x.data_ptr(), n, out.data_ptr(), STREAM), t_plain),
        "chain": lambda: timed_node(lambda: chain.run_dev(x.data_ptr(), n, out.data_ptr(), stream=STREAM), t_chain),
        "copy": lambda: timed_events(lambda: dst.copy_(src)),
    }
    per = {k: [] for k in runs}
    keys = list(runs)
    for r in range(ROUNDS):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            per[k].append(runs[k]())
    row = {k: float(np.median(v)) for k, v in per.items()}
    name = "n%d_%s" % (n, "bits%d" % bits if bits else "c32")
    print("%-14s symsync %.1f us (no rotation %.1f) [%s]   chain %.1f us [%s]   copy of %.1f MB %.1f us   copy / symsync = %.2f   chain / symsync = %.2f"
          % (name, row["symsync"], row["symsync_norot"], node.kernel(n), row["chain"], chain.kernel, 1e-6 * (8 * n + out_bytes), row["copy"],
             row["copy"] / row["symsync"], row["chain"] / row["symsync"]), flush=True)
    res[name] = row
    for t in (t_node, t_plain, t_chain):
        t.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    res = {}
    for n in (1 << 24, 1 << 26):
        for bits in (0, 2):
            cell(res, n, bits)
            torch.cuda.empty_cache()
    if "--json" in sys.argv:
        print(json.dumps(res))
