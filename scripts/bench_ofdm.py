"""The OFDM kernels on one MI355X: ofdm_mod_kernel and ofdm_demod_kernel at N = 64, 256 and 1024 with CP = N / 4, T = 2 training
and S = 14 data symbols per frame, three quarters of the bins data, pilots every 16th bin, pilot phase correction on, and enough
frames for 2^24 samples, each beside

  copy    a plain device copy of the bytes the launch moves (input read plus output written), as one copy of half that many
          bytes, event-pair timed in the same run
  fft     comms_fft_run_dev (FFTBatchNode) on the same number of N-point transforms, contiguous: no prefix, no carrier map, no
          equaliser

Each kernel is timed by the project's KernelTimer (the launch alone).  Median over ROUNDS rounds of the median of REPS calls,
the three taking turns, one process, after a warm-up that lets the clocks settle.  Before it is timed the demodulator's output
of the modulator's frames is compared with the data that went in.  Prints one line per cell and writes them to
profiles/ofdm_bench.txt (`--out PATH` for another file); `--json` adds a JSON line.  No pass / fail figure."""
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
T, S = 2, 14


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


def carrier_map(n):
    kind = np.zeros(n, np.uint8)
    edge = n // 2 - n // 8
    for f in range(-edge, edge + 1):
        if f:
            kind[f % n] = 2 if f % 16 == 8 else 1
    return kind


def cell(res, lines, n, total):
    cp = n // 4
    kind = carrier_map(n)
    rng = np.random.default_rng(n)
    unit = lambda k: np.exp(2j * np.pi * rng.random(k)).astype(np.complex64)  # noqa: E731
    args = (n, cp, kind)
    kw = dict(pilots=unit(int((kind == 2).sum())), polarity=[1, -1, 1, 1], train=unit(n), n_train=T, n_syms=S, cpe=True)
    mod, dem = c.OfdmModNode(*args, **kw), c.OfdmDemodNode(*args, **kw)
    frames = max(1, total // mod.frame_samples)
    n_data, n_samp, n_xf = frames * mod.data_syms, frames * mod.frame_samples, frames * (T + S)
    z = ((rng.standard_normal(n_data) + 1j * rng.standard_normal(n_data)) / np.sqrt(2)).astype(np.complex64)
    d_z = torch.from_numpy(z).to("cuda:0")
    d_x = torch.empty(n_samp, dtype=torch.complex64, device="cuda:0")
    d_back = torch.empty(n_data, dtype=torch.complex64, device="cuda:0")
    fft = c.FFTBatchNode(n, False)
    d_f = torch.empty(n_xf * n, dtype=torch.complex64, device="cuda:0")
    d_g = torch.empty(n_xf * n, dtype=torch.complex64, device="cuda:0")
    calls = {"mod": lambda: mod.run_dev(d_z.data_ptr(), frames, d_x.data_ptr(), STREAM),
             "demod": lambda: dem.run_dev(d_x.data_ptr(), frames, d_back.data_ptr(), STREAM),
             "fft": lambda: fft.run_dev(d_f.data_ptr(), n_xf * n, d_g.data_ptr(), STREAM)}
    calls["mod"]()
    calls["demod"]()
    torch.cuda.synchronize()
    back = d_back.cpu().numpy()
    loop_err = float(np.abs(back - z).max())
    moved = 8 * (n_data + n_samp)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    timers = {"mod": c.KernelTimer(REPS + 3).attach(mod), "demod": c.KernelTimer(REPS + 3).attach(dem), "fft": c.KernelTimer(REPS + 3).attach(fft)}
    per = {k: [] for k in ("mod", "demod", "fft", "copy")}
    order = ("mod", "demod", "fft", "copy")
    for r in range(ROUNDS):
        for k in (order if r % 2 == 0 else order[::-1]):
            if k == "copy":
                per[k].append(timed_events(lambda: dst.copy_(src)))
            else:
                timers[k].reset()
                timed_events(calls[k])
                per[k].append(float(np.median(timers[k].read_ms()) * 1e3))
    row = {k: float(np.median(v)) for k, v in per.items()}
    row.update(n_fft=n, frames=frames, transforms=n_xf, bytes_moved=int(moved), loop_max_err=loop_err)
    for k in ("mod", "demod"):
        row[k + "_over_copy"] = row[k] / row["copy"]
        row[k + "_over_fft"] = row[k] / row["fft"]
        node = mod if k == "mod" else dem
        line = ("n%-5d %-5s kernel alone %8.1f us = %6.1f GB/s moved, %6.2f Gsample/s   copy of %6.1f MB %7.1f us   kernel / copy %5.2f   "
                "fft of %d x %d %7.1f us   kernel / fft %5.2f   mod->demod max |d| %.1e   [%s]"
                % (n, k, row[k], moved / row[k] * 1e-3, n_samp / row[k] * 1e-3, 1e-6 * moved, row["copy"], row[k + "_over_copy"], n_xf, n,
                   row["fft"], row[k + "_over_fft"], loop_err, node.kernel(frames)))
        print(line, flush=True)
        lines.append(line)
    res["n%d" % n] = row
    for t in timers.values():
        t.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ofdm_bench.txt")
    total = 1 << (int(sys.argv[sys.argv.index("--n-log2") + 1]) if "--n-log2" in sys.argv else N_LOG2)
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    del warm
    res, lines = {}, ["scripts/bench_ofdm.py: 2^%d samples, CP = N / 4, T = %d, S = %d, pilot phase correction on; median of %d rounds of %d calls"
                      % (total.bit_length() - 1, T, S, ROUNDS, REPS)]
    for n in (64, 256, 1024):
        cell(res, lines, n, total)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
