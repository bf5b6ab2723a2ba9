"""The Complex<f32> synchronisation estimator on one MI355X: syncest_kernel at 2^24 samples, (n, d) = (4, 4) and (8, 8), beside

  f64     comms_timing_push_dev + comms_frequency_offset_estimate_dev on the PRE-WIDENED Complex<f64> copy of the same samples
          (the only route before this node; its host widening and the 16 B / sample upload are not counted)
  copy    a plain device copy of 8 bytes per sample (4 n read, 4 n written: the footprint of one read of the stream)

Every estimator call ends synchronised (the partials come back to the host), so all three are timed the same way: an event
pair around the call, i.e. launch, copy-back of the partials and the host's wait included; syncest additionally by the
project's KernelTimer (the launch alone).  Median over ROUNDS rounds of the median of REPS calls, the forms taking turns round
by round, one process, after a warm-up that lets the clocks settle.  Prints one line per cell; `--json` adds a JSON line."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS, ROUNDS = 30, 5


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


def cell(res, n_samples, n, d):
    x = torch.view_as_complex((torch.rand(2 * n_samples, dtype=torch.float32, device="cuda:0") * 2 - 1).view(n_samples, 2))
    x64 = x.to(torch.complex128)
    node = c.SyncEstimatorNode(n, d, 0.35)
    timer = c.KernelTimer(REPS).attach(node)
    old = c.TimingEstimatorNode(n, d, 0.35)
    lib, out = c.lib(), C.c_double()
    src = torch.empty(4 * n_samples, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(4 * n_samples, dtype=torch.uint8, device="cuda:0")

    def f64_route():
        old.run_dev(x64.data_ptr(), n_samples, STREAM)
        c._lib.check(lib.comms_frequency_offset_estimate_dev(x64.data_ptr(), n_samples, C.byref(out), 0, STREAM))

    def syncest_kernel_only():
        timer.reset()
        t = timed_events(lambda: node.run_dev(x.data_ptr(), n_samples, STREAM))
        return t, float(np.median(timer.read_ms()) * 1e3)

    per = {"syncest": [], "syncest_kernel": [], "f64": [], "copy": []}
    order = ["syncest", "f64", "copy"]
    for r in range(ROUNDS):
        for k in order[r % 3:] + order[:r % 3]:
            if k == "syncest":
                t, tk = syncest_kernel_only()
                per["syncest"].append(t)
                per["syncest_kernel"].append(tk)
            elif k == "f64":
                per["f64"].append(timed_events(f64_route))
            else:
                per["copy"].append(timed_events(lambda: dst.copy_(src)))
    row = {k: float(np.median(v)) for k, v in per.items()}
    a, b = node.run_dev(x.data_ptr(), n_samples, STREAM), old.run_dev(x64.data_ptr(), n_samples, STREAM)
    name = "n%d_sps%d_d%d" % (n_samples, n, d)
    print("%-18s syncest %.1f us (kernel alone %.1f) [%s]   f64 timing + frequency %.1f us   copy of %.1f MB %.1f us   "
          "f64 / syncest = %.2f   copy / syncest kernel = %.2f   |timing - f64 timing| = %.1e"
          % (name, row["syncest"], row["syncest_kernel"], node.kernel(n_samples), row["f64"], 8e-6 * n_samples, row["copy"],
             row["f64"] / row["syncest"], row["copy"] / row["syncest_kernel"], abs(a.timing - b)), flush=True)
    res[name] = row
    timer.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    res = {}
    for n, d in ((4, 4), (8, 8)):
        cell(res, 1 << 24, n, d)
        torch.cuda.empty_cache()
    if "--json" in sys.argv:
        print(json.dumps(res))
