"""Kernel time of the noise source and the AWGN node on one MI355X, read through comms_noise_set_timer (an event pair
around every launch), beside a plain device copy of the same footprint timed in the same run:

  awgn c32   8 B read + 8 B written per sample      normal f32   4 B written per value     bits packed  1/8 B per bit
  awgn i16   4 B read + 8 B written per sample      normal f64   8 B written per value     uniform      4 B written per value

at 2^24 and 2^28 samples (values, bits).  The copy moves (read + written) / 2 bytes, i.e. reads and writes as many bytes
in all as the kernel.  Method: the device is kept busy for a second first, every case is warmed up, then kernel and copy
take turns burst by burst (ROUNDS rounds of REPS launches, median of the per-round medians).

With the diagnostic build of the library (make -C comms_rs_amd/csrc diag; COMMS_HIP_LIB=.../libcomms_hip_diag.so) the
Box-Muller form is selectable per launch and `--forms` times both -- fast (v_log_f32 / v_sqrt_f32 / v_sin_f32 /
v_cos_f32: the product's) and accurate (logf / sqrtf / sincospif) -- and measures each one's largest error against
tests/noise_ref.py.
`--quick` runs 2^24 only.  Prints one line per case; `--json` adds a JSON summary line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import comms_rs_amd as c
import noise_ref as nr

REPS = 20
ROUNDS = 5
FORMS = "--forms" in sys.argv


def set_form(fast):
    os.environ["COMMS_NOISE_FAST"] = "1" if fast else "0"  # read per launch by the diagnostic build only


def kernel_us(node, fn, reps=REPS):
    t = c.KernelTimer(reps).attach(node)
    for _ in range(reps):
        fn()
    ms = t.read_ms()
    t.close()
    assert ms.size == reps
    return float(np.median(ms) * 1e3)


def copy_us(dst, src, reps=REPS):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        dst.copy_(src)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)


def cases(n):
    """name -> (bytes read + written, launch)"""
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(2 * n, dtype=torch.float32, device="cuda:0").normal_()
    i16 = torch.randint(-2000, 2000, (2 * n,), dtype=torch.int16, device="cuda:0")
    out = torch.empty(2 * n, dtype=torch.float32, device="cuda:0")
    src = c.NoiseSource(2024, 1)
    src16 = c.NoiseSource(2024, 1).set_input_format("i16", 1.0 / 2746.0)
    keep = (buf, i16, out)
    return keep, {
        "awgn_c32": (16 * n, src, lambda: src.awgn_dev(buf.data_ptr(), n, 0.5, out.data_ptr(), stream)),
        "awgn_c32_in_place": (16 * n, src, lambda: src.awgn_dev(buf.data_ptr(), n, 0.5, buf.data_ptr(), stream)),
        "awgn_i16": (12 * n, src16, lambda: src16.awgn_dev(i16.data_ptr(), n, 0.5, out.data_ptr(), stream)),
        "normal_f32": (4 * n, src, lambda: src.normal_dev(n, out.data_ptr(), stream=stream)),
        "normal_f64": (8 * n, src, lambda: src.normal_dev(n, out.data_ptr(), f64=True, stream=stream)),
        "uniform": (4 * n, src, lambda: src.uniform_dev(n, out.data_ptr(), stream=stream)),
        "bits_packed": (n // 8, src, lambda: src.bits_dev(n, out.data_ptr(), packed=True, stream=stream)),
    }


def settle():
    a = torch.empty(1 << 26, dtype=torch.float32, device="cuda:0")
    b = torch.empty_like(a)
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    while True:
        for _ in range(50):
            b.copy_(a)
        t1.record()
        torch.cuda.synchronize()
        if t0.elapsed_time(t1) > 1000.0:
            return


def accuracy(fast, n=1 << 22):
    set_form(fast)
    z_ref = nr.Source(12345, 7).normal(n)
    got = c.NoiseSource(12345, 7).normal(n).astype(np.float64)
    return float(np.max(np.abs(got - z_ref) / np.maximum(1.0, np.abs(z_ref))))


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    res = {"lib": os.path.basename(c.LIB_PATH)}
    forms = (("accurate", False), ("fast", True)) if FORMS else (("product", True),)
    if FORMS:
        assert "diag" in os.path.basename(c.LIB_PATH), "--forms needs the diagnostic build (COMMS_HIP_LIB)"
        for name, fast in forms:
            res["max_err_" + name] = accuracy(fast)
            print("Box-Muller %-8s max |z - z_ref| / max(1, |z_ref|) over 2^22 values: %.3e  (bound 2^-17 = %.3e)"
                  % (name, res["max_err_" + name], 2.0 ** -17), flush=True)
    settle()
    for lg in (24,) if "--quick" in sys.argv else (24, 28):
        n = 1 << lg
        keep, runs = cases(n)
        for name, (foot, node, fn) in runs.items():
            half = max(foot // 2, 16)
            a = torch.empty(half, dtype=torch.uint8, device="cuda:0")
            b = torch.empty(half, dtype=torch.uint8, device="cuda:0")
            uses_normal = name.startswith(("awgn", "normal"))
            legs = [(f, fast) for f, fast in forms] if uses_normal else [("kernel", True)]  # no Box-Muller stage: one form
            for f, fast in legs:  # warm-up
                set_form(fast)
                for _ in range(3):
                    fn()
            b.copy_(a)
            torch.cuda.synchronize()
            per = {f: [] for f, _ in legs}
            per["copy"] = []
            order = [f for f, _ in legs] + ["copy"]
            for r in range(ROUNDS):
                for k in order[r % len(order):] + order[:r % len(order)]:
                    if k == "copy":
                        per[k].append(copy_us(b, a))
                    else:
                        set_form(dict(legs)[k])
                        per[k].append(kernel_us(node, fn))
            row = {k: float(np.median(v)) for k, v in per.items()}
            row["footprint_bytes"] = foot
            line = "%-18s n=2^%d  %7.1f MB moved  copy %9.1f us (%.2f TB/s)" % (name, lg, foot / 1e6, row["copy"], foot / row["copy"] / 1e6)
            for f, _ in legs:
                line += "   %s %9.1f us = %.2f x copy, %.2f Gvalues/s" % (f, row[f], row[f] / row["copy"], n / row[f] / 1e3)
            print(line, flush=True)
            res["%s_2p%d" % (name, lg)] = row
            del a, b
        del keep, runs
        torch.cuda.empty_cache()
    if "--json" in sys.argv:
        print(json.dumps(res))
