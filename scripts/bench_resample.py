"""The rational resampler on one MI355X (device pointers, events around each call; median over ROUNDS rounds of the
median of REPS calls, the forms taking turns round by round, one process):

  node    ResampleNode (one launch, resample_kernel) at 2^22 and 2^26 input samples
  series  the launches it replaces -- upsample [-> real_to_c32] -> complex FIR [-> c32_re] -> decimate -- on the existing
          nodes.  Its scratch is n L samples of 8 bytes, twice: timed only where that fits comfortably (n L <= 2^27:
          2^18 inputs for L >= 147, 2^22 for L <= 3), beside the node at the same n
  copy    a plain device copy of the node's footprint, E n (1 + L / M) bytes read or written

for f32 (147, 152, 3528), (160, 147, 3840) and complex (3, 2, 96), (2, 3, 96), (147, 152, 3528).
`--series-only` times the series alone (it needs nothing of the resampler node: runs on any build).
Prints one line per cell; `--json` adds a JSON summary line.  `rocprofv3 --kernel-trace --stats` of this script shows
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
SERIES_MAX = 1 << 27   # upsampled samples the series is given


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


def lowpass(up, down, per):
    """Windowed sinc, `per` taps per phase, cutoff at the narrower Nyquist band, gain `up` at DC."""
    n, w = up * per, max(up, down)
    k = np.arange(n) - (n - 1) / 2
    return (up / w * np.sinc(k / w) * np.hamming(n)).astype(np.float32)


def rounds(runs):
    per = {k: [] for k in runs}
    keys = list(runs)
    for r in range(ROUNDS):
        for k in keys[r % len(keys):] + keys[:r % len(keys)]:
            per[k].append(timed(runs[k]))
    return {k: float(np.median(v)) for k, v in per.items()}


def series(taps, L, M, n, x, out, cplx):
    """The reference's nodes one by one, device-resident."""
    up, fir, dec = c.UpsampleNode(L), c.BatchFirNode(taps.astype(np.complex64)), c.DecimateNode(M)
    nu = n * L
    a, b = torch.empty(nu, dtype=torch.complex64, device="cuda:0"), torch.empty(nu, dtype=torch.complex64, device="cuda:0")

    def run():
        if cplx:
            up.run_dev(x.data_ptr(), n, 8, a.data_ptr(), STREAM)
            fir.run_dev(a.data_ptr(), nu, b.data_ptr(), STREAM)
            dec.run_dev(b.data_ptr(), nu, 8, out.data_ptr(), STREAM)
        else:
            up.run_dev(x.data_ptr(), n, 4, b.data_ptr(), STREAM)
            c.real_to_c32_dev(b.data_ptr(), nu, a.data_ptr(), 0, STREAM)
            fir.run_dev(a.data_ptr(), nu, b.data_ptr(), STREAM)
            c.c32_re_dev(b.data_ptr(), nu, a.data_ptr(), 0, STREAM)
            dec.run_dev(a.data_ptr(), nu, 4, out.data_ptr(), STREAM)

    run.keep = (up, fir, dec, a, b)
    run.kernel = fir.kernel_for(nu)
    return run


def cell(res, cplx, L, M, N, n, with_series):
    dt, E = (torch.complex64, 8) if cplx else (torch.float32, 4)
    taps = lowpass(L, M, N // L)
    assert taps.size == N
    x = (torch.rand(n * (2 if cplx else 1), dtype=torch.float32, device="cuda:0") * 2 - 1)
    x = torch.view_as_complex(x.view(n, 2)) if cplx else x
    m = -(-n * L // M)
    name = "%s_%d_%d_%d_n%d" % ("c32" if cplx else "f32", L, M, N, n)
    runs, outs = {}, {}
    if with_series:
        outs["series"] = torch.empty(m, dtype=dt, device="cuda:0")
        runs["series"] = series(taps, L, M, n, x, outs["series"], cplx)
    if not SERIES_ONLY:
        node = c.ResampleNode(taps, L, M, np.complex64 if cplx else np.float32)
        outs["node"] = torch.empty(m, dtype=dt, device="cuda:0")
        runs["node"] = lambda: node.run_dev(x.data_ptr(), n, outs["node"].data_ptr(), STREAM)
        # a copy of (n + m) / 2 samples reads and writes that many bytes each: E (n + m) in all, the node's footprint
        half = (n + m) // 2
        src, dst = torch.empty(half, dtype=dt, device="cuda:0"), torch.empty(half, dtype=dt, device="cuda:0")
        runs["copy"] = lambda: dst.copy_(src)
    if not runs:
        return
    row = rounds(runs)
    line = "%-28s" % name
    if with_series:
        line += " series %.1f us [%s]" % (row["series"], runs["series"].kernel)
    if not SERIES_ONLY:
        line += "   node %.1f us [%s]   copy of %.1f MB %.1f us, copy / node = %.2f" % (
            row["node"], node.kernel(n), 1e-6 * E * (n + m), row["copy"], row["copy"] / row["node"])
        if with_series:
            torch.cuda.synchronize()
            d = float((outs["node"] - outs["series"]).abs().max())
            line += "   series / node = %.1f   max|node - series| %.2e" % (row["series"] / row["node"], d)
            row["max_abs_diff"] = d
    print(line, flush=True)
    res[name] = row


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    res = {}
    cells = [(False, 147, 152, 3528), (False, 160, 147, 3840), (True, 3, 2, 96), (True, 2, 3, 96), (True, 147, 152, 3528)]
    for cplx, L, M, N in cells:
        for n in (1 << 18, 1 << 22, 1 << 26):
            fits = n * L <= SERIES_MAX
            if n == 1 << 18 and not (fits and (1 << 22) * L > SERIES_MAX):
                continue   # 2^18 only where it is the size at which the series runs
            if SERIES_ONLY and not fits:
                continue
            cell(res, cplx, L, M, N, n, fits)
            torch.cuda.empty_cache()
    if "--json" in sys.argv:
        print(json.dumps(res))
