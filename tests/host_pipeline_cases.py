"""Workloads of tests/test_gpu_host_pipeline.py (shared with the single-shot subprocess of that test): name ->
() -> (input, node factory, (input bytes, output bytes) per unit).  The node factory returns an object with .run; the input's
first axis is the sample axis."""
import numpy as np

def _lpf(n_taps, cutoff):
    k = np.arange(n_taps) - (n_taps - 1) / 2.0
    return (2 * cutoff * np.sinc(2 * cutoff * k) * np.hamming(n_taps)).astype(np.complex64)


def _case_fir_direct():
    import comms_rs_amd as c
    n = (5 << 20) + 12345
    return c.synth_iq(n, 0, 31), lambda: c.BatchFirNode(_lpf(31, 0.1)).set_algo(c.FIR_DIRECT), (8, 8)


def _case_fir_auto():
    import comms_rs_amd as c
    n = (6 << 20) + 777
    return c.synth_iq(n, 0, 32), lambda: c.BatchFirNode(c.rrc_taps(255, 8.0, 0.35)), (8, 8)


def _case_mixer():
    import comms_rs_amd as c
    n = (5 << 20) + 3
    return c.synth_iq(n, 0, 33), lambda: c.MixerNode(0.123, 0.4), (8, 8)


def _case_fmdemod():
    import comms_rs_amd as c
    n = (6 << 20) + 11
    return c.synth_iq(n, 0, 34), lambda: c.FMDemodNode(), (8, 4)


def _case_decimate():
    import comms_rs_amd as c
    n = (9 << 20) + 5  # not a multiple of the rate: the ragged tail is the last chunk's
    return c.synth_iq(n, 0, 35), lambda: c.DecimateNode(3), (24, 8)


def _case_upsample():
    import comms_rs_amd as c
    n = (2 << 20) + 9
    return c.synth_iq(n, 0, 36), lambda: c.UpsampleNode(4), (8, 32)


def _case_fft():
    import comms_rs_amd as c
    n = 4096 * 1300  # 1300 transforms of 4096 points
    return c.synth_iq(n, 0, 37), lambda: c.FFTBatchNode(4096, False), (4096 * 8, 4096 * 8)


def _case_chain_r2():
    import comms_rs_amd as c
    n = 2 * ((6 << 20) + 7)   # mixer -> 63 taps -> keep every 2nd: 16 B in, 8 B out per unit (a chain whose output is worth pipelining)
    return c.synth_iq(n, 0, 38), lambda: c.ChainNode(0.31, 0.2, _lpf(63, 1 / 5.0), 2, False), (16, 8)


# ---- the nodes that are not Complex<f32> in and out: Complex<f64> (16 B), Complex<i16> pairs (4 B), u8 pairs (2 B), bytes.
# The input's first axis is the sample axis: one sample is x.strides[0] bytes (in_elem below).
def in_elem(x):
    return x.strides[0]


def _c128(seed, n, scale=1.0):
    rng = np.random.default_rng(seed)
    return scale * (rng.standard_normal(n) + 1j * rng.standard_normal(n))


def _i16(seed, n):
    return np.random.default_rng(seed).integers(-32768, 32768, (n, 2), dtype=np.int16)   # full range: the sums wrap


class _Call:
    def __init__(self, fn):
        self.run = fn


def _case_fir_f64():
    import comms_rs_amd as c
    return _c128(60, (3 << 20) + 77), lambda: c.BatchFirNodeF64(_c128(61, 31, 0.3)), (16, 16)


def _case_fir_i16():
    import comms_rs_amd as c
    return _i16(62, (9 << 20) + 5), lambda: c.BatchFirNodeI16(_i16(63, 31)), (4, 4)


def _case_pulse_f64():
    import comms_rs_amd as c
    return _c128(64, (2 << 20) + 77), lambda: c.PulseNodeF64(_c128(65, 21, 0.2), 2), (16, 32)


def _case_pulse_i16():
    import comms_rs_amd as c
    return _i16(66, (4 << 20) + 5), lambda: c.PulseNodeI16(_i16(67, 30), 4), (4, 16)


def _case_fft_f64():
    import comms_rs_amd as c
    return _c128(68, 4096 * 700), lambda: c.FFTBatchNodeF64(4096, False), (4096 * 16, 4096 * 16)


def _case_fmdemod_f64():
    import comms_rs_amd as c
    return _c128(69, (3 << 20) + 11), lambda: c.FMDemodNodeF64(), (16, 8)


def _case_mixer_f64():
    import comms_rs_amd as c
    return _c128(70, (3 << 20) + 3), lambda: c.MixerNode(0.123, 0.4), (16, 16)   # complex128 in: MixerNode<f64>


def _case_i16_to_c32():
    import comms_rs_amd as c
    return _i16(71, (6 << 20) + 5), lambda: _Call(lambda x: c.iq_i16_to_c32(x, 1.0 / 8192)), (4, 8)


def _case_u8_to_c32():
    import comms_rs_amd as c
    x = np.random.default_rng(72).integers(0, 256, ((7 << 20) + 9, 2), dtype=np.uint8)
    return x, lambda: _Call(c.iq_u8_to_c32), (2, 8)


def _case_c32_to_i16():
    import comms_rs_amd as c
    n = (6 << 20) + 7
    return (6 * c.synth_iq(n, 0, 73)).astype(np.complex64), lambda: _Call(lambda x: c.iq_c32_to_i16(x, 8192.0)), (8, 4)


# ---- the remaining host entries that go through run_host_units with an output share worth pipelining
def _case_fir_direct_i16_in():
    import comms_rs_amd as c
    make = lambda: c.BatchFirNode(_lpf(31, 0.1)).set_algo(c.FIR_DIRECT).set_input_format("i16", 1.0 / 8192)  # noqa: E731
    return _i16(74, (6 << 20) + 5), make, (4, 8)


def _case_pulse():
    import comms_rs_amd as c
    return c.synth_iq((2 << 20) + 9, 0, 75), lambda: c.PulseNode(c.rrc_taps(63, 4.0, 0.35), 4), (8, 32)


def _case_awgn():
    import comms_rs_amd as c

    def make():
        src = c.NoiseSource(1234)
        return _Call(lambda x: src.awgn(x, 0.5))
    return c.synth_iq((5 << 20) + 3, 0, 76), make, (16, 16)   # the AWGN node's unit is a block of two samples


def _case_qpsk_bit_mod():
    import comms_rs_amd as c
    x = np.random.default_rng(77).integers(0, 4, (14 << 20) + 3, dtype=np.uint8)
    return x, lambda: _Call(c.qpsk_bit_mod), (1, 4)


def _case_rfir_r2():
    import comms_rs_amd as c
    n = 2 * ((6 << 20) + 7) + 1   # odd: the ragged tail is the last chunk's
    x = np.random.default_rng(78).standard_normal(n).astype(np.float32)
    return x, lambda: c.RealFirDecimNode(_lpf(63, 0.2).real.astype(np.float32), 2), (8, 4)


CASES = {"fir_direct": _case_fir_direct, "fir_auto": _case_fir_auto, "mixer": _case_mixer, "fmdemod": _case_fmdemod,
         "decimate": _case_decimate, "upsample": _case_upsample, "fft": _case_fft, "chain_r2": _case_chain_r2,
         "fir_f64": _case_fir_f64, "fir_i16": _case_fir_i16, "pulse_f64": _case_pulse_f64, "pulse_i16": _case_pulse_i16,
         "fft_f64": _case_fft_f64, "fmdemod_f64": _case_fmdemod_f64, "mixer_f64": _case_mixer_f64,
         "i16_to_c32": _case_i16_to_c32, "u8_to_c32": _case_u8_to_c32, "c32_to_i16": _case_c32_to_i16,
         "fir_direct_i16_in": _case_fir_direct_i16_in, "pulse": _case_pulse, "awgn": _case_awgn,
         "qpsk_bit_mod": _case_qpsk_bit_mod, "rfir_r2": _case_rfir_r2}
