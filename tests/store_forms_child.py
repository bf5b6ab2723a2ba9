"""The child process of tests/test_gpu_store_forms.py: `python store_forms_child.py` runs every case of CASES and prints one
line per case, "case <id> ok" or "case <id> FAIL <why>"; the last line is "done".

Two builds of the library are loaded into this one process through ctypes:
  WT     the diagnostic build with COMMS_WT_MIN_BYTES=0 in the environment (the parent sets both): every call that can take the
         16-byte write-through stores of csrc/common.hpp (store16<true>) takes them, whatever its size;
  PLAIN  the product build, whose threshold is the compile-time 32 MiB: no call here comes near it, so every call stores plainly.
Every comparison is bit for bit (torch.equal / np.array_equal): the mixer's arithmetic is the same in both forms and the
decimator copies bytes.  A launch error is an uncaught exception: nothing is launched behind it."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOB = "COMMS_WT_MIN_BYTES"
LIB_DIR = os.path.join(ROOT, "comms_rs_amd", "lib")
NUM_CU = 256                              # csrc/common.hpp: kNumCU
MIXER_SWEEP = 2 * 256 * 8 * NUM_CU        # samples one sweep of mixer_kernel<2> covers: 2 per lane, 256 lanes, 8 * kNumCU workgroups
DEC_SWEEP = 2 * 256 * 8 * NUM_CU          # outputs one sweep of decimate_kernel16 covers

MIXER_N = (2, 3, 511, 512, 513, MIXER_SWEEP - 1, MIXER_SWEEP + 3)
DEC_RATES = (2, 3, 8, 100)
DEC_NOUT = (1, 2, 3, 1023, 1024, 1025)
OTHER_ELEMS = (1, 2, 4, 16)

CASES = (["knob"] + ["mixer-n%d-%s-%s" % (n, w, p) for n in MIXER_N for w in ("inplace", "outofplace") for p in ("forms", "carry")]
         + ["decimate-r%d-m%d" % (r, m) for r in DEC_RATES for m in DEC_NOUT] + ["decimate-r2-m%d" % (DEC_SWEEP + 5)]
         + ["elem%d" % e for e in OTHER_ELEMS] + ["chain-twice"])

_vp, _sz = C.c_void_p, C.c_size_t


class Lib:
    """The few entries of include/comms_hip.h these cases need, of one build."""

    def __init__(self, path):
        self.l = l = C.CDLL(path)
        l.comms_mixer_create.argtypes = [C.c_double, C.c_double, C.c_int32, C.POINTER(_vp)]
        l.comms_mixer_run_dev.argtypes = [_vp, _vp, _sz, _vp, _vp]
        l.comms_mixer_destroy.argtypes = [_vp]
        l.comms_decimate_run_dev.argtypes = [_vp, _sz, _sz, _sz, _vp, C.POINTER(_sz), C.c_int32, _vp]
        l.comms_last_error.restype = C.c_char_p

    def ok(self, status):
        if status != 0:
            raise RuntimeError(self.l.comms_last_error().decode())

    def mixer(self, dphase, phase=0.0):
        h = _vp()
        self.ok(self.l.comms_mixer_create(dphase, phase, 0, C.byref(h)))
        return h

    def mix(self, h, src, n, dst, stream):
        self.ok(self.l.comms_mixer_run_dev(h, src, n, dst, stream))

    def free(self, *hs):
        for h in hs:
            self.ok(self.l.comms_mixer_destroy(h))

    def decimate(self, src, n, elem, rate, dst, stream):
        m = _sz()
        self.ok(self.l.comms_decimate_run_dev(src, n, elem, rate, dst, C.byref(m), 0, stream))
        return m.value


def main():
    import numpy as np
    import torch

    import oracle

    assert os.environ.get(KNOB) == "0", "the parent sets %s=0" % KNOB
    WT = Lib(os.path.join(LIB_DIR, "libcomms_hip_diag.so"))
    PLAIN = Lib(os.path.join(LIB_DIR, "libcomms_hip.so"))
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev)
    MIX_T = 2.0 * 3.14159265358979323846264338327950288  # csrc/common.hpp: kMixT

    def rand_c(n, seed):
        gen.manual_seed(seed)
        return torch.view_as_complex(torch.rand((n, 2), generator=gen, device=dev) * 2 - 1)

    def knob():
        # the diagnostic build alone reads the variable, once; the product build has neither the hook nor the knob
        WT.l.comms_debug_store_form.argtypes = [_sz]
        WT.l.comms_debug_store_form.restype = C.c_int32
        assert WT.l.comms_debug_store_form(16) == 1 and WT.l.comms_debug_store_form(0) == 0
        assert not hasattr(PLAIN.l, "comms_debug_store_form")

    def mixer_case(n, inplace, prop):
        # forms: any oscillator.  carry: dphase = T / 1024, an exact fraction of T whose advance over one grid sweep (2^20 samples)
        # is a whole number of turns.  The kernel evaluates a lane's first rotor in closed form from its 64-bit phase and steps it
        # by the sweep's rotor from sweep to sweep; a second call evaluates the same samples in closed form again.  Only where the
        # sweep's rotor is exactly (1, 0) are the two the same f64 numbers, so only there is "the second call equals the tail of
        # the one call, bit for bit" a property of the mixer at all; at other dphase the stepped rotor carries the rounding of its
        # steps (1 ulp of f32 at about one sample in a million: NOTES.md, "Store forms").  For odd n the second call also starts
        # on an odd sample of the one call, whose rotor is one step from its even neighbour's instead of a closed form of its own:
        # there the equality rests on the f32 rounding of the output absorbing the last bits of an f64 rotor.
        dphase, phase = (2 * np.pi * 0.1, 0.4) if prop == "forms" else (MIX_T / 1024, 0.4)
        x = rand_c(2 * n, n)
        xa, xb = x[:n].clone(), x[n:].clone()       # 16-byte aligned both: the second call takes the float4 kernel too
        out = {}
        for name, lib in (("wt", WT), ("plain", PLAIN)):
            two, one = lib.mixer(dphase, phase), lib.mixer(dphase, phase)
            if inplace:
                ya, yb, yf = xa.clone(), xb.clone(), x.clone()
                lib.mix(two, ya.data_ptr(), n, ya.data_ptr(), stream)
                lib.mix(two, yb.data_ptr(), n, yb.data_ptr(), stream)
                lib.mix(one, yf.data_ptr(), 2 * n, yf.data_ptr(), stream)
            else:
                ya, yb, yf = torch.full_like(xa, 7), torch.full_like(xb, 7), torch.full_like(x, 7)
                lib.mix(two, xa.data_ptr(), n, ya.data_ptr(), stream)
                lib.mix(two, xb.data_ptr(), n, yb.data_ptr(), stream)
                lib.mix(one, x.data_ptr(), 2 * n, yf.data_ptr(), stream)
            torch.cuda.synchronize()
            lib.free(two, one)
            out[name] = (ya, yb, yf)
        if prop == "forms":     # the two store forms, every output of every call
            for a, b in zip(out["wt"], out["plain"]):
                assert torch.equal(a.view(torch.int64), b.view(torch.int64)), "write-through and plain outputs differ"
            return
        for name in ("wt", "plain"):   # the phase carried from call to call
            ya, yb, yf = out[name]
            assert torch.equal(ya.view(torch.int64), yf[:n].view(torch.int64)), "%s: first call != head of the one call" % name
            bad = yb.view(torch.int64) != yf[n:].view(torch.int64)
            ulp = (torch.view_as_real(yb).view(torch.int32) - torch.view_as_real(yf[n:]).view(torch.int32)).abs().max()
            assert int(bad.sum()) == 0, ("%s: second call != tail of one call over the concatenation at %d of %d samples (at most %d ulp of f32)"
                                         % (name, int(bad.sum()), n, int(ulp)))

    def decimate_case(rate, n_out, elem=8):
        # n a multiple of the rate, and n = (n_out - 1) * rate + 1: the last kept sample is the last input sample
        for n in (n_out * rate, (n_out - 1) * rate + 1):
            gen.manual_seed(rate * 1000003 + n)
            raw = torch.randint(0, 256, (n * elem,), dtype=torch.uint8, generator=gen, device=dev)
            want = oracle.decimate(raw.cpu().numpy().reshape(n, elem), rate).reshape(-1)
            assert want.size == n_out * elem
            for off in ((0, 8) if elem == 8 else (0,)):   # 16-byte aligned output, and the same 8 bytes on (the 8-byte kernel)
                got = {}
                for name, lib in (("wt", WT), ("plain", PLAIN)):
                    buf = torch.full((n_out * elem + 32,), 0xA5, dtype=torch.uint8, device=dev)
                    m = lib.decimate(raw.data_ptr(), n, elem, rate, buf.data_ptr() + off, stream)
                    torch.cuda.synchronize()
                    assert m == n_out
                    got[name] = buf.cpu().numpy()
                    assert np.array_equal(got[name][off:off + n_out * elem], want), "%s != oracle (n=%d off=%d)" % (name, n, off)
                    assert np.all(got[name][:off] == 0xA5) and np.all(got[name][off + n_out * elem:] == 0xA5), "wrote outside the output"
                assert np.array_equal(got["wt"], got["plain"])

    def chain_twice():
        # mixer (in place) -> decimate / 8 -> mixer (in place) -> decimate / 8, twice on the same buffers on one stream with
        # no host synchronisation in between.  dphase = T k / n for powers of two k and n (an exact fraction of T): after n samples the oscillator is back
        # at exactly its start phase (turns are a 64-bit fraction of T), so round 2 on the same input must repeat round 1.
        n, r = 1 << 21, 8
        x = rand_c(n, 99)
        res = {}
        for name, lib in (("wt", WT), ("plain", PLAIN)):
            m1, m2 = lib.mixer(MIX_T * 4 / n), lib.mixer(MIX_T * 2 / (n // r))
            a, b, c = torch.empty_like(x), torch.empty(n // r, dtype=x.dtype, device=dev), torch.empty(n // r // r, dtype=x.dtype, device=dev)
            rounds = []
            for _ in range(2):
                a.copy_(x)  # (a device copy on the same stream)
                lib.mix(m1, a.data_ptr(), n, a.data_ptr(), stream)
                assert lib.decimate(a.data_ptr(), n, 8, r, b.data_ptr(), stream) == n // r
                lib.mix(m2, b.data_ptr(), n // r, b.data_ptr(), stream)
                assert lib.decimate(b.data_ptr(), n // r, 8, r, c.data_ptr(), stream) == n // r // r
                rounds.append((a.clone(), b.clone(), c.clone()))
                if name == "plain":
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            lib.free(m1, m2)
            res[name] = rounds
        for k in range(3):
            r1, r2 = res["wt"][0][k].view(torch.int64), res["wt"][1][k].view(torch.int64)
            assert torch.equal(r1, r2), "round 2 differs from round 1 in buffer %d" % k
            for j in range(2):
                assert torch.equal(res["wt"][j][k].view(torch.int64), res["plain"][j][k].view(torch.int64)), (j, k)
        # ... and the last stage against the oracle: c is every 8th sample of the twice-mixed b
        assert np.array_equal(oracle.decimate(res["wt"][1][1].cpu().numpy(), r), res["wt"][1][2].cpu().numpy())

    def run(case):
        p = case.split("-")
        if case == "knob":
            knob()
        elif p[0] == "mixer":
            mixer_case(int(p[1][1:]), p[2] == "inplace", p[3])
        elif p[0] == "decimate":
            decimate_case(int(p[1][1:]), int(p[2][1:]))
        elif p[0].startswith("elem"):
            decimate_case(8, 1025, elem=int(p[0][4:]))
        else:
            chain_twice()

    for case in CASES:
        try:
            run(case)
            print("case %s ok" % case, flush=True)
        except AssertionError as e:
            print("case %s FAIL %s" % (case, " ".join(str(e).split())[:300]), flush=True)
    print("done")


if __name__ == "__main__":
    main()
