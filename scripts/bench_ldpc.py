"""The LDPC decoder on one MI355X: ldpc_decode_kernel alone at two call shapes, 65536 frames of (12 x 24, Z = 27) and 256
frames of (32 x 64, Z = 128), at fixed iteration counts of 1 and 10, in decoded information bits per second and in us, beside

  copy     a plain device copy of the bytes the launch moves (the LLR records read plus the bit records written), as one copy
           of half that many bytes
  viterbi  viterbi_kernel (K = 7, n = 2, terminated) on the same number of frames of the same number of information bits

The LLRs are noise without a codeword behind it, so that no frame converges and every frame runs max_iters iterations (the
statuses are read back and counted).  Nothing here or in the reference did this job before, so there is no target figure.
Median over ROUNDS rounds of the median of REPS calls by the project's KernelTimer (the launch alone), the three taking turns,
one process, after a warm-up that lets the clocks settle.  Prints one line per cell and writes them to
profiles/ldpc_bench.txt; `--json` adds a JSON line.  No pass / fail figure."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import comms_rs_amd as c
import ldpc_ref as lr

STREAM = torch.cuda.current_stream().cuda_stream
REPS, ROUNDS = 10, 3


def timed_events(fn, reps=REPS, warm=2):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]) * 1e3)  # us


def kernel_us(timer, fn):
    timer.reset()
    timed_events(fn)
    return float(np.median(timer.read_ms()) * 1e3)


def cell(res, lines, frames, mb, nb, Z, iters, rng):
    B = lr.make_base(mb, nb, Z, 1)
    N, T = nb * Z, (nb - mb) * Z
    node = c.LdpcDecoderNode(B, Z, max_iters=iters)
    d_llr = torch.from_numpy((8.0 * rng.standard_normal((frames, N))).astype(np.float32)).to("cuda:0")
    d_bits = torch.empty(frames * node.out_frame_bytes, dtype=torch.uint8, device="cuda:0")
    d_st = torch.empty(frames, dtype=torch.int32, device="cuda:0")
    vit = c.ViterbiNode(T, qscale=1.0)
    v_llr = torch.from_numpy((8.0 * rng.standard_normal((frames, vit.in_frame_bytes // 4))).astype(np.float32)).to("cuda:0")
    v_bits = torch.empty(frames * vit.out_frame_bytes, dtype=torch.uint8, device="cuda:0")
    moved = frames * (node.in_frame_bytes + node.out_frame_bytes)
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(moved // 2, dtype=torch.uint8, device="cuda:0")
    t_dec, t_vit = c.KernelTimer(REPS + 2).attach(node), c.KernelTimer(REPS + 2).attach(vit)

    def decode():
        node.run_dev(d_llr.data_ptr(), frames, d_bits.data_ptr(), d_st.data_ptr(), STREAM)

    def viterbi():
        vit.run_dev(v_llr.data_ptr(), frames, v_bits.data_ptr(), None, STREAM)

    decode()
    torch.cuda.synchronize()
    converged = int((d_st.cpu().numpy() > 0).sum())
    per = {"ldpc": [], "viterbi": [], "copy": []}
    order = ("ldpc", "viterbi", "copy")
    for r in range(ROUNDS):
        for k in order[r % 3:] + order[: r % 3]:
            if k == "ldpc":
                per[k].append(kernel_us(t_dec, decode))
            elif k == "viterbi":
                per[k].append(kernel_us(t_vit, viterbi))
            else:
                per[k].append(timed_events(lambda: dst.copy_(src)))
    row = {k: float(np.median(v)) for k, v in per.items()}
    row.update(frames=frames, info_bits=T, iterations=iters, converged=converged, bytes_moved=int(moved),
               gbit_per_s=frames * T / row["ldpc"] * 1e-3, viterbi_gbit_per_s=frames * T / row["viterbi"] * 1e-3)
    name = "frames%d_%dx%d_Z%d_it%d" % (frames, mb, nb, Z, iters)
    line = ("%-30s kernel alone %.1f us = %.2f Gbit/s decoded (%.2f us per iteration of the call)   viterbi_kernel on %d x %d bits "
            "%.1f us = %.2f Gbit/s   copy of %.2f MB %.1f us   %d of %d frames converged   [%s]"
            % (name, row["ldpc"], row["gbit_per_s"], row["ldpc"] / iters, frames, T, row["viterbi"], row["viterbi_gbit_per_s"], 1e-6 * moved,
               row["copy"], converged, frames, node.kernel(frames)))
    print(line, flush=True)
    lines.append(line)
    res[name] = row
    t_dec.close()
    t_vit.close()


if __name__ == "__main__":
    assert c.device_count() >= 1, "needs an MI355X"
    warm = torch.empty(1 << 28, dtype=torch.uint8, device="cuda:0")
    for _ in range(200):   # settle the clocks
        warm.add_(1)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    res, lines = {}, ["scripts/bench_ldpc.py: norm16 = 12, qscale 1, noise-only LLRs (no frame converges); median of %d rounds of %d calls, "
                      "KernelTimer (the launch alone)" % (ROUNDS, REPS)]
    for frames, mb, nb, Z in ((65536, 12, 24, 27), (256, 32, 64, 128)):
        for iters in (1, 10):
            cell(res, lines, frames, mb, nb, Z, iters, rng)
    with open(os.path.join(ROOT, "profiles", "ldpc_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    if "--json" in sys.argv:
        print(json.dumps(res))
