"""The receive end's hard decisions on one MI355X (device pointers, events around each call; median over ROUNDS rounds
of the median of REPS calls, the forms interleaved):

  config 1's receive filter: mixer -> 63-tap RRC -> keep every 4th, i16 input, 2^24 and 2^26 input samples, BPSK and
      QPSK, in three forms: Complex<f32> output; bits out of fir_decim_kernel's store stage; Complex<f32> output followed
      by comms_sym_to_bits_dev;
  poly8: a 129-tap chain at rate 8 (i16 input, 2^24 samples), which runs on fir_polyphase: the decision pass behind it;
  wave:  a 63-tap chain at rate 8 with Complex<f32> input (2^24 samples), which runs on fir_decim_wave_kernel: the pass
         behind it.

Prints one line per case; `--json` adds a JSON summary line at the end.  `rocprofv3 --kernel-trace --stats` of this
script shows which kernels each form launched."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import comms_rs_amd as c

STREAM = torch.cuda.current_stream().cuda_stream
REPS = 50
ROUNDS = 5


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


def case(res, name, taps, rate, n, fmt, k, after=False):
    dphase = 2 * np.pi * 0.1
    if fmt == "i16":
        x = torch.randint(-8192, 8192, (2 * n,), dtype=torch.int16, device="cuda:0")
    else:
        x = torch.empty(n, dtype=torch.complex64, device="cuda:0")
        c.synth_iq_dev(x.data_ptr(), n, 0)
    n_dec = n // rate
    y = torch.empty(n_dec, dtype=torch.complex64, device="cuda:0")
    bits = torch.empty((n_dec * k + 7) // 8 + 16, dtype=torch.uint8, device="cuda:0")

    def node(out_bits):
        nd = c.ChainNode(dphase, 0.0, taps, rate, False, mixer_after_fir=after)
        if fmt == "i16":
            nd.set_input_format("i16", 1.0 / 8192)
        if out_bits:
            nd.set_output_format("bits", k)
        return nd

    a, b, p = node(False), node(True), node(False)
    runs = {
        "c32": lambda: a.run_dev(x.data_ptr(), n, y.data_ptr(), STREAM),
        "bits": lambda: b.run_dev(x.data_ptr(), n, bits.data_ptr(), STREAM),
        "c32+pass": lambda: (p.run_dev(x.data_ptr(), n, y.data_ptr(), STREAM),
                             c.sym_to_bits_dev(y.data_ptr(), n_dec, k, bits.data_ptr(), stream=STREAM)),
    }
    per = {key: [] for key in runs}
    keys = list(runs)
    for r in range(ROUNDS):
        for key in keys[r % 3:] + keys[:r % 3]:
            per[key].append(timed(runs[key]))
    row = {key: float(np.median(v)) for key, v in per.items()}
    in_b = 4.0 if fmt == "i16" else 8.0
    out_b = {"c32": 8.0 / rate, "bits": k / 8.0 / rate, "c32+pass": (8.0 + 8.0 + k / 8.0) / rate}
    line = "%s 2^%d samples k=%d: " % (name, int(np.log2(n)), k) + "   ".join(
        "%s %.1f us (%.3f B/sample)" % (key, v, in_b + out_b[key]) for key, v in row.items())
    line += "   bits / c32 = %.3f, bits / (c32+pass) = %.3f   [kernel: %s]" % (row["bits"] / row["c32"], row["bits"] / row["c32+pass"], b.kernel)
    print(line, flush=True)
    res["%s_2p%d_k%d" % (name, int(np.log2(n)), k)] = dict(row, kernel=b.kernel)


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    res = {}
    rrc63 = c.rrc_taps(63, 4.0, 0.25)
    for lg in (24, 26):
        for k in (1, 2):
            case(res, "config1_rx", rrc63, 4, 1 << lg, "i16", k)
    for k in (1, 2):
        case(res, "poly8_r8_129", c.rrc_taps(129, 8.0, 0.35), 8, 1 << 24, "i16", k)
    for k in (1, 2):
        case(res, "wave_r8_63", c.rrc_taps(63, 8.0, 0.35), 8, 1 << 24, "c32", k)
    if "--json" in sys.argv:
        print(json.dumps(res))
