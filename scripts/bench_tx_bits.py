"""The transmit front end on one MI355X (device pointers, events around each launch; pulse: median over
7 rounds of the median of 100, the variants interleaved):

  pulse: BASELINE config 1's chain (63-tap RRC x4 + fused mixer) at 2^20, 2^24 and 2^26 outputs, fed Complex<f32>
         symbols against packed bits (1 bit / symbol: BPSK; 2: QPSK), Complex<f32> and i16 output;
  prns:  2^30 bits, one byte per bit and packed, against a plain device write of the same number of bytes.

Prints one line per case; `--json` adds a JSON summary line at the end."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS = 100
ROUNDS = 7


def timed(fn, reps=REPS):
    for _ in range(5):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)  # us


def bench_pulse(res):
    taps = c.rrc_taps(63, 4.0, 0.25)
    dphase = 2 * np.pi * 0.1
    for lg in (20, 24, 26):
        n_out = 1 << lg
        n_sym = n_out // 4
        sym = torch.empty(n_sym, dtype=torch.complex64, device="cuda:0")
        c.synth_iq_dev(sym.data_ptr(), n_sym, 0)
        bits = torch.randint(0, 256, ((2 * n_sym + 7) // 8,), dtype=torch.uint8, device="cuda:0")
        out = torch.empty(n_out, dtype=torch.complex64, device="cuda:0")
        for fmt in ("c32", "i16"):
            runs = {}
            for inp in ("c32", "bits1", "bits2"):
                node = c.PulseNode(taps, 4).set_mixer(dphase)
                if fmt == "i16":
                    node.set_output_format("i16", 8192.0)
                src = sym
                if inp != "c32":
                    node.set_input_format("bits", int(inp[-1]))
                    src = bits
                runs[inp] = (lambda node=node, src=src: node.run_dev(src.data_ptr(), n_sym, out.data_ptr(), STREAM))
            # ROUNDS rounds, the three variants in a rotating order: clock drift and order effects cancel in the median
            per = {k: [] for k in runs}
            keys = list(runs)
            for r in range(ROUNDS):
                for k in keys[r % 3:] + keys[:r % 3]:
                    per[k].append(timed(runs[k]))
            row = {k: float(np.median(v)) for k, v in per.items()}
            in_b = {"c32": 8.0, "bits1": 1 / 8, "bits2": 2 / 8}
            ob = 8 if fmt == "c32" else 4
            line = "pulse 2^%d outputs, %s out: " % (lg, fmt) + "   ".join(
                "%s %.1f us (%.2f B/out, %.2f TB/s)" % (k, v, ob + in_b[k] / 4, n_out * (ob + in_b[k] / 4) / v / 1e6)
                for k, v in row.items())
            line += "   bits1 / c32 = %.3f, bits2 / c32 = %.3f" % (row["bits1"] / row["c32"], row["bits2"] / row["c32"])
            print(line, flush=True)
            res["pulse_2p%d_%s" % (lg, fmt)] = row


def bench_prns(res):
    n = 1 << 30
    buf = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    for w in (8, 64):
        node = c.PrnsNode(0xB8 if w == 8 else 0xD800000000000000, 1, w)
        row = {}
        for packed in (False, True):
            nbytes = n // 8 if packed else n
            t_gen = timed(lambda: node.run_dev(n, buf.data_ptr(), packed, STREAM), reps=20)
            t_fill = timed(lambda: buf[:nbytes].fill_(1), reps=20)
            key = "packed" if packed else "u8"
            row[key] = {"us": t_gen, "fill_us": t_fill, "fill_fraction": t_fill / t_gen}
            print("prns W=%d 2^30 bits %s: %.1f us (%.2f TB/s written); a plain device write of the same %d bytes: %.1f us "
                  "-> generation runs at %.2f of the write" % (w, key, t_gen, nbytes / t_gen / 1e6, nbytes, t_fill, t_fill / t_gen),
                  flush=True)
        res["prns_w%d" % w] = row


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    res = {}
    bench_pulse(res)
    bench_prns(res)
    if "--json" in sys.argv:
        print(json.dumps(res))
