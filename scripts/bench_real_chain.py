"""The real-stream audio stage on one MI355X (device pointers, events around each call; median over ROUNDS rounds of
the median of REPS calls, the forms taking turns burst by burst):

  audio stage alone: RealFirDecimNode (one launch, rfir_decim_kernel) against the four launches the reference graph
      needs -- real_to_c32 -> complex FIR -> c32_re -> decimate, wired as bench.py's literal() wires them -- for
      (63 taps, /5), (127, /8), (255, /4), (63, /1) at n = 2^26 / 5, 2^24 and 2^26 real samples; beside each cell a plain
      device copy of the stage's footprint (4 n bytes in, 4 n / R out) and the kernel's fraction of it;
  the literal example end to end (examples/fm_radio.rs:144-152): u8 -> chain front end -> audio stage, five launches
      against two, 2^26 input samples, 200 steps behind a 200-launch warm-up.

`--series-only` times the four-launch leg alone (it needs nothing of the real-stream node: runs on any build).
Prints one line per case; `--json` adds a JSON summary line.  `rocprofv3 --kernel-trace --stats` of this script shows
which kernels each form launched."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS = 30
ROUNDS = 5
SERIES_ONLY = "--series-only" in sys.argv


def timed(fn, reps=REPS):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)  # us


def fm_radio_taps():
    g = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_kats.json")))
    return np.asarray(g["fm_radio_taps"]["taps_re"], np.float32)


def lowpass(n_taps, cutoff):
    k = np.arange(n_taps) - (n_taps - 1) / 2
    h = 2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(n_taps)
    return (h / h.sum()).astype(np.float32)


def series(taps, rate, n, x, out):
    """The four launches, device-resident, as bench.py's literal() wires them."""
    fir, dec = c.BatchFirNode(taps.astype(np.complex64)), c.DecimateNode(rate)
    lb, lc = torch.empty(n, dtype=torch.complex64, device="cuda:0"), torch.empty(n, dtype=torch.complex64, device="cuda:0")
    ld = torch.empty(n, dtype=torch.float32, device="cuda:0")

    def run():
        c.real_to_c32_dev(x.data_ptr(), n, lb.data_ptr(), 0, STREAM)
        fir.run_dev(lb.data_ptr(), n, lc.data_ptr(), STREAM)
        c.c32_re_dev(lc.data_ptr(), n, ld.data_ptr(), 0, STREAM)
        dec.run_dev(ld.data_ptr(), n, 4, out.data_ptr(), STREAM)

    run.keep = (fir, dec, lb, lc, ld)
    run.kernel = fir.kernel_for(n)
    return run


def stage(res, n_taps, rate, n, taps):
    x = torch.rand(n, dtype=torch.float32, device="cuda:0") * 2 - 1
    m = -(-n // rate)
    out_s, out_n = torch.empty(m, dtype=torch.float32, device="cuda:0"), torch.empty(m, dtype=torch.float32, device="cuda:0")
    runs = {"series": series(taps, rate, n, x, out_s)}
    name = "audio_%d_r%d_n%d" % (n_taps, rate, n)
    if not SERIES_ONLY:
        node = c.RealFirDecimNode(taps, rate)
        runs["node"] = lambda: node.run_dev(x.data_ptr(), n, out_n.data_ptr(), STREAM)
        # a plain copy of the stage's footprint: 4 n bytes read and written at once would count them twice, so: read 4 n, write 4 n / R
        # is approximated by copying (n + m) / 2 floats (that many bytes read AND written: 4 (n + m) in all)
        half = (n + m) // 2
        src, dst = torch.empty(half, dtype=torch.float32, device="cuda:0"), torch.empty(half, dtype=torch.float32, device="cuda:0")
        runs["copy"] = lambda: dst.copy_(src)
    per = {k: [] for k in runs}
    keys = list(runs)
    for r in range(ROUNDS):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            per[k].append(timed(runs[k]))
    row = {k: float(np.median(v)) for k, v in per.items()}
    line = "%-26s series %.1f us [%s]" % (name, row["series"], runs["series"].kernel)
    if not SERIES_ONLY:
        torch.cuda.synchronize()
        d = float((out_n - out_s).abs().max())
        line += "   node %.1f us [%s]   series / node = %.2f   copy of %.1f MB %.1f us, copy / node = %.2f   max|node - series| %.2e" % (
            row["node"], node.kernel(n), row["series"] / row["node"], 4e-6 * (n + m), row["copy"], row["copy"] / row["node"], d)
        row["max_abs_diff"] = d
    print(line, flush=True)
    res[name] = row


def literal(res, steps=200, warmup=200):
    t63 = fm_radio_taps()
    nl = (1 << 26) // 25 * 25
    n1, n2 = nl // 5, nl // 25
    u8 = torch.randint(0, 256, (2 * nl,), dtype=torch.uint8, device="cuda:0")
    la = torch.empty(n1, dtype=torch.float32, device="cuda:0")
    le5, le2 = torch.empty(n2, dtype=torch.float32, device="cuda:0"), torch.empty(n2, dtype=torch.float32, device="cuda:0")

    def front_node():
        f = c.ChainNode(0.0, 0.0, t63.astype(np.complex64), 5, True)
        f.set_input_format("u8")
        return f

    f5, f2 = front_node(), front_node()
    tail5 = series(t63, 5, n1, la, le5)

    def five():
        f5.run_dev(u8.data_ptr(), nl, la.data_ptr(), STREAM)
        tail5()

    forms = {"five_launches": five}
    if not SERIES_ONLY:
        audio = c.RealFirDecimNode(t63, 5)

        def two():
            f2.run_dev(u8.data_ptr(), nl, la.data_ptr(), STREAM)
            audio.run_dev(la.data_ptr(), n1, le2.data_ptr(), STREAM)

        forms["two_launches"] = two
    row = {}
    for name, fn in forms.items():
        for _ in range(warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / steps
        row[name] = ms
        print("literal example, 2^26 u8 input samples, %s: %.4f ms per step = %.1f Gsamples/s  [front: %s]" % (
            name, ms, nl / ms / 1e6, f5.kernel), flush=True)
    res["literal_example"] = row


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    res = {}
    cells = [(63, 5, fm_radio_taps()), (127, 8, lowpass(127, 1 / 16)), (255, 4, lowpass(255, 1 / 8)), (63, 1, fm_radio_taps())]
    for n in ((1 << 26) // 5, 1 << 24, 1 << 26):
        for n_taps, rate, taps in cells:
            stage(res, n_taps, rate, n, taps)
            torch.cuda.empty_cache()
    literal(res)
    if "--json" in sys.argv:
        print(json.dumps(res))
