"""Node classes over the C ABI, named and parameterised like the reference's.

Every class has
  run(x)                  host numpy in -> host numpy out (H2D + kernel + D2H)
  run_dev(in_ptr, n, out_ptr, stream=0)
                          raw device pointers (ints), asynchronous on `stream`
                          (a hipStream_t as int; 0 = HIP's legacy default stream,
                          _lib.STREAM_HANDLE = the handle's own stream).
torch tensors are not part of this API: callers pass tensor.data_ptr().
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib

_c64 = np.dtype(np.complex64)


def _as_c64(a):
    a = np.ascontiguousarray(a, dtype=np.complex64)
    return a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


_IQ = {"c32": (0, np.complex64, 1), "i16": (1, np.int16, 2), "u8": (2, np.uint8, 2)}


def _as_input(a, fmt):
    """Contiguous input array of a node whose input format is `fmt`, and its sample count."""
    code, dtype, per = _IQ[fmt]
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, a.size // per


def _get(ctype, fn, *args, tail=()):
    """The scalar that fn(*args, &value, *tail) writes: every getter, out_len and estimate of the C ABI.  `tail` is what
    follows the output in the handle-less entries: the device, and the stream of their device forms."""
    v = ctype()
    check(fn(*args, C.byref(v), *tail))
    return v.value


def device_count():
    try:
        return _get(C.c_int32, lib().comms_device_count)
    except _lib.CommsError:
        return 0


class _Handle:
    _prefix = None   # of the node's C functions: "comms_fir" for comms_fir_destroy, comms_fir_set_timer, comms_fir_get_kernel

    def __init__(self):
        self._h = C.c_void_p()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            getattr(lib(), self._prefix + "_destroy")(self._h)
            self._h = C.c_void_p()

    def set_timer(self, timer):
        """Attach a KernelTimer (None detaches): its pairs bracket the node's launch (a series: its FIR launch; the
        channelizer's series: channel 0's).  A node whose C side has no timer setter raises AttributeError."""
        check(getattr(lib(), self._prefix + "_set_timer")(self._h, timer._h if timer is not None else None))
        return self

    def _call(self, name, *args):
        """check(comms_<prefix>_<name>(*args)): the call of a body that several prefixes share."""
        check(getattr(lib(), self._prefix + "_" + name)(*args))

    def _kernel_name(self, *args, cap=240):
        """comms_*_get_kernel(handle, *args, name, cap), decoded."""
        buf = C.create_string_buffer(cap)
        check(getattr(lib(), self._prefix + "_get_kernel")(self._h, *args, buf, cap))
        return buf.value.decode()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _History:
    """The history accessors of a stream node (csrc/stream_call.hpp) over comms_<prefix>_{state_len, get_state, set_state}:
    `_state_dtype` and `_state_shape` are the numpy type and shape of ONE sample, `_state_args` names the attributes
    comms_<prefix>_state_len takes, `_state_get` / `_state_set` the C name stems where they differ (the chain's
    "_get_fir_state").  The length is fixed at create: the library is asked once per node.  A node without a state_len entry
    (the FIRs, the chain) passes its n_state."""
    _state_dtype = np.complex64
    _state_shape = ()
    _state_args = ()
    _state_len = None
    _state_get, _state_set = "_get_state", "_set_state"

    def state_len(self):
        if self._state_len is None:
            self._state_len = _get(C.c_size_t, getattr(lib(), self._prefix + "_state_len"), *[getattr(self, a) for a in self._state_args])
        return self._state_len

    def get_state(self, n_state=None):
        """The last n_state input samples (default: all state_len() of them), newest first."""
        n_state = self.state_len() if n_state is None else int(n_state)
        st = np.empty((n_state,) + self._state_shape, self._state_dtype)
        check(getattr(lib(), self._prefix + self._state_get)(self._h, _ptr(st), n_state))
        return st

    def set_state(self, state):
        state = np.ascontiguousarray(state, dtype=self._state_dtype)
        check(getattr(lib(), self._prefix + self._state_set)(self._h, _ptr(state), len(state.reshape((-1,) + self._state_shape))))
        return self


class _Position:
    """The stream index of a node that reports positions: comms_<prefix>_{get_position, set_position}."""

    def position(self):
        """Stream index of the next sample (symbol)."""
        return _get(C.c_uint64, getattr(lib(), self._prefix + "_get_position"), self._h)

    def set_position(self, position):
        check(getattr(lib(), self._prefix + "_set_position")(self._h, int(position)))
        return self


class _Detector(_Position):
    """What the two synchronisers share beside their history: the threshold, the default capacity of a call (detections are more
    than `guard` positions apart), the outputs of a call and the packing of its detections.  `_side` holds the dtypes of the
    per-detection outputs beside the detections: the OFDM synchroniser's cfo."""
    found = 0
    _side = ()

    def set_threshold(self, threshold):
        check(getattr(lib(), self._prefix + "_set_threshold")(self._h, float(threshold)))
        return self

    def _cap(self, n, cap):
        return (n + self.guard) // (self.guard + 1) if cap is None else int(cap)

    def _detect(self, fn, n, cap, raw, *args, tail=()):
        """fn(handle, *args, detections, *side outputs, cap, &found, *tail) with room for `cap` detections (None: as many as n
        positions can hold): the detections, or with side outputs the tuple (detections, *side), each cut to what was found."""
        cap = self._cap(n, cap)
        outs = [np.zeros(cap, dtype) for dtype in (FRAME_DETECTION_DTYPE,) + self._side]
        found = C.c_size_t()
        check(fn(self._h, *args, *[_ptr(o) if cap else None for o in outs], cap, C.byref(found), *tail))
        self.found = found.value
        dets = outs[0][: min(self.found, cap)]
        dets = dets if raw else [FrameDetection(d) for d in dets]
        return (dets, *[o[: len(dets)] for o in outs[1:]]) if self._side else dets


def _record(accessor, unit=1):
    """node -> the bytes of one record, from the handle's C accessor `accessor` (looked up at the first call), which counts
    units of `unit` bytes."""
    fn = []

    def nbytes(node):
        if not fn:
            fn.append(getattr(lib(), accessor))
        return fn[0](node._h) * unit
    return nbytes


class _FrameCall:
    """One per-frame entry of the C ABI (csrc/common.hpp: FrameCall): `run`(handle, records in, n_frames, records out, ...)
    and its device form `run`_dev(..., stream), looked up at the first call.  in_dtype / out_dtype are the numpy types of an
    input and an output element, in_bytes / out_bytes give node -> bytes of a record (_record, or host arithmetic).  A node
    holds one as data and calls it; a stream node with a per-frame entry beside its stream (OfdmSyncNode.correct) does the same."""

    def __init__(self, run, in_dtype, out_dtype, in_bytes, out_bytes):
        self._name, self._fns = run, None
        self.in_dtype, self.out_dtype, self.in_bytes, self.out_bytes = np.dtype(in_dtype), np.dtype(out_dtype), in_bytes, out_bytes

    def _c(self, dev):
        if self._fns is None:
            self._fns = getattr(lib(), self._name), getattr(lib(), self._name + "_dev")
        return self._fns[dev]

    def run(self, node, x, side=(), pre=(), tail=()):
        """Host form on any array of whole records: run(handle, x, n_frames, *pre, out, *side outputs, *tail) with a zero-filled
        output of shape (n_frames, elements per record) and one zero-filled side output of n_frames values per dtype of `side`;
        `pre` holds further per-frame input arrays, `tail` goes as it is.  Returns out, or with side outputs (out, *side
        outputs).  With no frames every array goes as NULL and nothing is launched."""
        x = np.ascontiguousarray(x, dtype=self.in_dtype)
        per = self.in_bytes(node) // self.in_dtype.itemsize
        if not per or x.size % per:
            raise ValueError("the input must hold whole records of %d values (%d bytes)" % (per, per * self.in_dtype.itemsize))
        n_frames = x.size // per
        out = np.zeros((n_frames, self.out_bytes(node) // self.out_dtype.itemsize), self.out_dtype)
        outs = [out] + [np.zeros(n_frames, dtype) for dtype in side]
        p_in, *ptrs = [_ptr(a) if n_frames else None for a in (x, *pre, *outs)]
        check(self._c(0)(node._h, p_in, n_frames, *ptrs, *tail))
        return tuple(outs) if side else out

    def run_dev(self, node, in_ptr, n_frames, *rest):
        """Device form: rest = the further pointers and the stream, as the C entry takes them."""
        check(self._c(1)(node._h, in_ptr, int(n_frames), *rest))


class _FrameNode:
    """A node whose run is one _FrameCall, `_frame`: frame-major records in, records out, all frames of a call in one launch."""
    _frame = None

    @property
    def in_frame_bytes(self):
        return self._frame.in_bytes(self)

    @property
    def out_frame_bytes(self):
        return self._frame.out_bytes(self)

    def run(self, frames):
        return self._frame.run(self, frames)

    def run_dev(self, in_ptr, n_frames, out_ptr, stream=0):
        self._frame.run_dev(self, in_ptr, n_frames, out_ptr, stream)


def _frame_call(prefix, in_dtype, out_dtype):
    """The _FrameCall of comms_<prefix>_run with the accessors comms_<prefix>_{in,out}_frame_bytes: what most nodes have."""
    return _FrameCall(prefix + "_run", in_dtype, out_dtype, _record(prefix + "_in_frame_bytes"), _record(prefix + "_out_frame_bytes"))


# ------------------------------------------------------------------ device buffers
class DeviceBuf:
    """Ref-counted device allocation (comms_buf_*): the device-resident message type."""

    def __init__(self, nbytes, device=0, _h=None):
        if _h is not None:
            self._h = _h
        else:
            self._h = C.c_void_p()
            check(lib().comms_buf_alloc(nbytes, device, C.byref(self._h)))

    @property
    def ptr(self):
        return lib().comms_buf_ptr(self._h) or 0

    @property
    def nbytes(self):
        return lib().comms_buf_size(self._h)

    def clone(self):
        """Rust `Clone`: bump the refcount, share the allocation."""
        check(lib().comms_buf_retain(self._h))
        return DeviceBuf(0, _h=self._h)

    def upload(self, arr, offset=0):
        arr = np.ascontiguousarray(arr)
        check(lib().comms_buf_upload(self._h, offset, _ptr(arr), arr.nbytes))
        return self

    def download(self, dtype, count, offset=0):
        out = np.empty(count, dtype)
        check(lib().comms_buf_download(self._h, offset, _ptr(out), out.nbytes))
        return out

    def release(self):
        if self._h:
            check(lib().comms_buf_release(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


# ------------------------------------------------------------------ FIR
class BatchFirNode(_History, _Handle):
    """BatchFirNode::new(taps, state) / run (fir_node.rs:193-220)."""
    _prefix = "comms_fir"

    def __init__(self, taps, state=None, device=0):
        super().__init__()
        taps = _as_c64(taps)
        if state is None:
            check(lib().comms_fir_create(_ptr(taps), taps.size, None, 0, device, C.byref(self._h)))
        else:
            state = _as_c64(state)
            check(lib().comms_fir_create(_ptr(taps), taps.size, _ptr(state), state.size, device, C.byref(self._h)))

    def set_algo(self, algo):
        check(lib().comms_fir_set_algo(self._h, algo))
        return self

    def algo_for(self, n):
        return _get(C.c_int32, lib().comms_fir_get_algo, self._h, n)

    def kernel_for(self, n):
        """Name of the kernel a batch of n samples is run by (diagnostics)."""
        return self._kernel_name(n, cap=64)

    _fmt = "c32"

    def set_input_format(self, fmt, scale=1.0):
        """Raw-IQ input: "c32" (default), "i16" (interleaved int16 re/im, times `scale`) or "u8"
        (RTL-SDR bytes, (x - 127.5) / 127.5).  run() then takes an integer array of 2 n values."""
        check(lib().comms_fir_set_input_format(self._h, _IQ[fmt][0], float(scale)))
        self._fmt = fmt
        return self

    def run(self, x):
        x, n = _as_input(x, self._fmt)
        out = np.empty(n, np.complex64)
        check(lib().comms_fir_run(self._h, _ptr(x), n, _ptr(out)))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_fir_run_dev(self._h, in_ptr, n, out_ptr, stream))

    def state(self, n_state):
        return self.get_state(n_state)

    def set_state(self, state):
        _History.set_state(self, state)


class FirNode(BatchFirNode):
    """FirNode::new(taps, state) / run(&Complex<T>) (fir_node.rs:89-113): one sample per call."""

    def run(self, x):
        return BatchFirNode.run(self, np.array([x], np.complex64))[0]


class PulseNode(_Handle):
    """PulseNode::new(taps, sam_per_sym) / run (pulse.rs:71-92)."""
    _prefix = "comms_pulse"

    def __init__(self, taps, sam_per_sym, device=0):
        super().__init__()
        taps = _as_c64(taps)
        self.sam_per_sym = int(sam_per_sym)
        check(lib().comms_pulse_create(_ptr(taps), taps.size, self.sam_per_sym, device, C.byref(self._h)))

    def set_mixer(self, dphase, phase=None):
        """Fuse the MixerNode::new(dphase, phase) that follows this node into its launch (transmit chain)."""
        check(lib().comms_pulse_set_mixer(self._h, float(dphase), 0.0 if phase is None else float(phase)))
        return self

    @property
    def phase(self):
        """Oscillator phase of the fused mixer for the next output sample."""
        return _get(C.c_double, lib().comms_pulse_get_phase, self._h)

    _out_i16 = False

    def set_output_format(self, fmt, scale=1.0):
        """"i16": run() returns int16 (n, 2) = `(scale * y) as i16`, the IQOutput wire format, written by the
        kernel's store stage; "c32" restores the default."""
        check(lib().comms_pulse_set_output_format(self._h, _IQ[fmt][0], float(scale)))
        self._out_i16 = fmt == "i16"
        return self

    _in_bits = 0

    def set_input_format(self, fmt, bits_per_sym=1, constellation=None):
        """"bits": run_bits() takes packed bits (LSB first, bits_per_sym = 1 or 2 per symbol) and the kernel maps
        value v to constellation[v] (2**bits_per_sym points; None = digital.rs's bpsk_bit_mod / qpsk_bit_mod tables);
        "c32" restores the default, run() on complex symbols.  The history carries across a switch."""
        if fmt not in ("c32", "bits"):
            raise ValueError("input format must be 'c32' or 'bits' (got %r)" % (fmt,))
        self._in_bits = _set_bits_format(lib().comms_pulse_set_input_format, self._h, bits_per_sym if fmt == "bits" else None, constellation)
        return self

    def _out_array(self, n_sym):
        if self._out_i16:
            return np.empty((n_sym * self.sam_per_sym, 2), np.int16)
        return np.empty(n_sym * self.sam_per_sym, np.complex64)

    def run_bits(self, packed, n_sym):
        """n_sym symbols from packed bits (uint8, LSB first; ceil(n_sym * bits_per_sym / 8) bytes) -> samples."""
        if not self._in_bits:
            raise ValueError("run_bits needs set_input_format('bits', ...)")
        n_sym = int(n_sym)
        b = np.ascontiguousarray(packed, dtype=np.uint8).ravel()
        if b.size < (n_sym * self._in_bits + 7) // 8:
            raise ValueError("packed holds fewer than n_sym * bits_per_sym bits")
        out = self._out_array(n_sym)
        check(lib().comms_pulse_run(self._h, _ptr(b), n_sym, _ptr(out)))
        return out

    def run(self, sym):
        """One symbol (scalar) -> sam_per_sym samples, or a batch of symbols."""
        if self._in_bits:
            raise ValueError("the node reads packed bits (set_input_format): use run_bits")
        s = _as_c64(np.atleast_1d(sym))
        out = self._out_array(s.size)
        check(lib().comms_pulse_run(self._h, _ptr(s), s.size, _ptr(out)))
        return out

    def run_dev(self, sym_ptr, n_sym, out_ptr, stream=0):
        check(lib().comms_pulse_run_dev(self._h, sym_ptr, n_sym, out_ptr, stream))


# ------------------------------------------------------------------ Complex<i16> and Complex<f64> instantiations
def _as_c16(a):
    a = np.ascontiguousarray(a, dtype=np.int16)
    return a.reshape(-1, 2)


def _as_c128(a):
    return np.ascontiguousarray(np.atleast_1d(a), dtype=np.complex128)


class _Exact(_Handle):
    """The nodes whose outputs are bit-identical to the reference's, over `comms_{fir,pulse}_{i16,f64}_*`.  A subclass names
    its ABI prefix `_abi`, the function `_arr` that makes a contiguous array of its sample type, and that type as the numpy
    `_dtype` and `_shape` of ONE sample: int16 (2,) for Complex<i16>, complex128 () for Complex<f64>."""
    _abi = _arr = _dtype = _shape = None

    def _n(self, a):
        """Samples in an array that _arr made."""
        return len(a.reshape((-1,) + self._shape))

    def _out(self, n):
        return np.empty((n,) + self._shape, self._dtype)

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        self._call("run_dev", self._h, in_ptr, n, out_ptr, stream)


class _ExactFir(_Exact):
    """BatchFirNode<T>::new(taps, state) / run (fir_node.rs:193-220).  A single sample in gives a single sample out: FirNode<T>."""

    def __init__(self, taps, state=None, device=0):
        super().__init__()
        taps = self._arr(taps)
        if state is None:
            self._call("create", _ptr(taps), self._n(taps), None, 0, device, C.byref(self._h))
        else:
            state = self._arr(state)
            self._call("create", _ptr(taps), self._n(taps), _ptr(state), self._n(state), device, C.byref(self._h))

    def run(self, x):
        single = np.shape(x) == self._shape
        x = self._arr(x)
        out = np.empty_like(x)
        self._call("run", self._h, _ptr(x), self._n(x), _ptr(out))
        return out[0] if single else out

    # _History's bodies on the sample type of the subclass; no mixin, because the ABI backs them in part: only Complex<f64>
    # has a set_state entry
    _state_get, _state_set = _History._state_get, _History._state_set
    _state_dtype, _state_shape = property(lambda self: self._dtype), property(lambda self: self._shape)

    def state(self, n_state):
        return _History.get_state(self, n_state)


class _ExactPulse(_Exact):
    """PulseNode<T>::new(taps, sam_per_sym) / run (pulse.rs:71-92)."""

    def __init__(self, taps, sam_per_sym, device=0):
        super().__init__()
        taps = self._arr(taps)
        self.sam_per_sym = int(sam_per_sym)
        self._call("create", _ptr(taps), self._n(taps), self.sam_per_sym, device, C.byref(self._h))

    def run(self, sym):
        s = self._arr(sym)
        out = self._out(self._n(s) * self.sam_per_sym)
        self._call("run", self._h, _ptr(s), self._n(s), _ptr(out))
        return out


class BatchFirNodeI16(_ExactFir):
    """BatchFirNode<i16> on Complex<i16> = int16 (n, 2) arrays, wrapping arithmetic.  A single sample has shape (2,)."""
    _abi, _arr, _dtype, _shape = "comms_fir_i16_", staticmethod(_as_c16), np.int16, (2,)
    _prefix = _abi[:-1]


class BatchFirNodeF64(_ExactFir):
    """BatchFirNode<f64> on Complex<f64> = numpy complex128: the reference's arithmetic operation for operation.  A single
    sample is a scalar."""
    _abi, _arr, _dtype, _shape = "comms_fir_f64_", staticmethod(_as_c128), np.complex128, ()
    _prefix = _abi[:-1]

    set_state = _History.set_state


FirNodeI16 = BatchFirNodeI16
FirNodeF64 = BatchFirNodeF64


class PulseNodeI16(_ExactPulse):
    """PulseNode<i16> on Complex<i16>."""
    _abi, _arr, _dtype, _shape = "comms_pulse_i16_", staticmethod(_as_c16), np.int16, (2,)
    _prefix = _abi[:-1]


class PulseNodeF64(_ExactPulse):
    """PulseNode<f64> on Complex<f64>, bit-identical to the reference."""
    _abi, _arr, _dtype, _shape = "comms_pulse_f64_", staticmethod(_as_c128), np.complex128, ()
    _prefix = _abi[:-1]


# ------------------------------------------------------------------ mixer
class MixerNode(_Handle):
    """MixerNode::new(dphase, phase) (mixer.rs:128-141); run() mixes a slice."""
    _prefix = "comms_mixer"

    def __init__(self, dphase, phase=None, device=0):
        super().__init__()
        check(lib().comms_mixer_create(float(dphase), 0.0 if phase is None else float(phase), device, C.byref(self._h)))

    def run(self, x):
        """Complex<f32> samples -> MixerNode<f32>; a numpy complex128 array (or scalar) -> MixerNode<f64>, Complex<f64>
        out: the sample type follows the input's dtype, as the reference's generic `MixerNode<T>` (mixer.rs:93) -- note that
        numpy's DEFAULT complex dtype is complex128.  Lists, Python scalars and every other dtype are converted to
        complex64 (tests/test_gpu_parity.py::test_mixer_run_dtype_follows_the_input_dtype pins this)."""
        scalar = np.ndim(x) == 0
        if isinstance(x, (np.ndarray, np.generic)) and x.dtype == np.complex128:
            a = np.ascontiguousarray(np.atleast_1d(x), dtype=np.complex128)
            out = np.empty_like(a)
            check(lib().comms_mixer_run_f64(self._h, _ptr(a), a.size, _ptr(out)))
            return out[0] if scalar else out
        a = _as_c64(np.atleast_1d(x))
        out = np.empty_like(a)
        check(lib().comms_mixer_run(self._h, _ptr(a), a.size, _ptr(out)))
        return out[0] if scalar else out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_mixer_run_dev(self._h, in_ptr, n, out_ptr, stream))

    def run_f64_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_mixer_run_f64_dev(self._h, in_ptr, n, out_ptr, stream))

    @property
    def phase(self):
        return _get(C.c_double, lib().comms_mixer_get_phase, self._h)

    @phase.setter
    def phase(self, value):
        """Phase of the next sample (checkpoint restore / start phase of a stream shard)."""
        check(lib().comms_mixer_set_phase(self._h, float(value)))


# ------------------------------------------------------------------ resampling
class _RateChange:
    """What DecimateNode and UpsampleNode share: comms_<_name>_{out_len, run, run_dev} on elements of any size, handle-less,
    the rate kept in the attribute that `_rate` names.  The C functions are looked up once per node."""
    _name = _rate = None

    def __init__(self, rate, device=0):
        setattr(self, self._rate, int(rate))
        self.device = device
        self._out_len, self._run, self._run_dev = (getattr(lib(), "comms_%s_%s" % (self._name, f)) for f in ("out_len", "run", "run_dev"))

    def out_len(self, n):
        return _get(C.c_size_t, self._out_len, n, getattr(self, self._rate))

    def run(self, x):
        x = np.ascontiguousarray(x)
        elem = x.dtype.itemsize * int(np.prod(x.shape[1:], dtype=np.int64))
        out = np.empty((self.out_len(x.shape[0]),) + x.shape[1:], x.dtype)
        m = _get(C.c_size_t, self._run, _ptr(x), x.shape[0], elem, getattr(self, self._rate), _ptr(out), tail=(self.device,))
        assert m == out.shape[0]
        return out

    def run_dev(self, in_ptr, n, elem, out_ptr, stream=0):
        return _get(C.c_size_t, self._run_dev, in_ptr, n, elem, getattr(self, self._rate), out_ptr, tail=(self.device, stream))


class DecimateNode(_RateChange):
    """DecimateNode::new(dec_rate) / decimate (resample_node.rs:23, :53-65)."""
    _name, _rate = "decimate", "dec_rate"

    def __init__(self, dec_rate, device=0):
        super().__init__(dec_rate, device)

    decimate = _RateChange.run


class UpsampleNode(_RateChange):
    """UpsampleNode::new(ups_rate) / upsample (resample_node.rs:87, :120-131)."""
    _name, _rate = "upsample", "ups_rate"

    def __init__(self, ups_rate, device=0):
        super().__init__(ups_rate, device)

    upsample = _RateChange.run


# ------------------------------------------------------------------ FM demod
def _flat_c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128).ravel()


class _FMDemod(_Handle):
    """FMDemodNode<T> over comms_<_prefix>_*: `_dtype` is the complex sample type, `_arr` makes a contiguous array of it; the
    output is its real type."""
    _dtype = _arr = None

    def __init__(self, device=0):
        super().__init__()
        self._call("create", device, C.byref(self._h))

    def run(self, x):
        x = self._arr(x)
        out = np.empty(x.size, x.real.dtype)
        self._call("run", self._h, _ptr(x), x.size, _ptr(out))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        self._call("run_dev", self._h, in_ptr, n, out_ptr, stream)

    @property
    def prev(self):
        """FM.prev (analog.rs:9,31): the last input sample of the previous batch."""
        p = np.zeros(1, self._dtype)
        self._call("get_prev", self._h, _ptr(p))
        return p[0]

    @prev.setter
    def prev(self, value):
        p = np.array([value], self._dtype)
        self._call("set_prev", self._h, _ptr(p))


class FMDemodNode(_FMDemod):
    """FMDemodNode::new() / run (analog_node.rs:43-51)."""
    _prefix, _dtype, _arr = "comms_fmdemod", np.complex64, staticmethod(_as_c64)


class FMDemodNodeF64(_FMDemod):
    """FMDemodNode<f64>::new() / run (analog_node.rs:20-52; FM::demod analog.rs:22-35) on Complex<f64>."""
    _prefix, _dtype, _arr = "comms_fmdemod_f64", np.complex128, staticmethod(_flat_c128)


# ------------------------------------------------------------------ FFT
class _FFTBatch(_Handle):
    """FFTBatchNode<T> over comms_<_prefix>_*: `_dtype` is the sample type, `_arr` makes a contiguous array of it."""
    _dtype = _arr = None

    def __init__(self, fft_size, ifft, device=0):
        super().__init__()
        self.fft_size = int(fft_size)
        self._call("create", self.fft_size, 1 if ifft else 0, device, C.byref(self._h))

    def run(self, x):
        x = self._arr(x)
        out = np.empty_like(x)
        self._call("run", self._h, _ptr(x), x.size, _ptr(out))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        self._call("run_dev", self._h, in_ptr, n, out_ptr, stream)


class _FFTSample:
    """The #[aggregate] form over an _FFTBatch: a sample per call, None until fft_size samples arrived, then their transform."""

    def __init__(self, fft_size, ifft, device=0):
        super().__init__(fft_size, ifft, device)
        self._samples = []

    def run(self, sample):
        self._samples.append(self._dtype(sample))
        if len(self._samples) == self.fft_size:
            res = _FFTBatch.run(self, np.array(self._samples, self._dtype))
            self._samples = []
            return res
        return None


class FFTBatchNode(_FFTBatch):
    """FFTBatchNode::new(fft_size, ifft) / run (fft_node.rs:65-83)."""
    _prefix, _dtype, _arr = "comms_fft", np.complex64, staticmethod(_as_c64)


class FFTBatchNodeF64(_FFTBatch):
    """FFTBatchNode<f64>::new(fft_size, ifft) / run (fft_node.rs:65-83) on Complex<f64> = numpy complex128 (comms_fft_f64_*):
    the instantiation of the reference's doc examples; correct to f64 rounding."""
    _prefix, _dtype, _arr = "comms_fft_f64", np.complex128, staticmethod(_flat_c128)


class FFTSampleNode(_FFTSample, FFTBatchNode):
    """FFTSampleNode::new(fft_size, ifft) / run (fft_node.rs:142-167), #[aggregate]:
    push one sample; returns None until fft_size samples arrived, then the FFT."""


class FFTSampleNodeF64(_FFTSample, FFTBatchNodeF64):
    """FFTSampleNode<f64> (fft_node.rs:142-167), #[aggregate]: a sample per call, the spectrum every fft_size samples."""


# ------------------------------------------------------------------ fused chain
class ChainNode(_History, _Handle):
    """mixer / FIR / decimate [/ FM demod] as one node (comms_chain_*), an additional node.
    mixer_after_fir=False: mixer -> FIR -> decimate [-> FM]; True: FIR -> mixer -> decimate."""
    _prefix = "comms_chain"
    _state_get, _state_set = "_get_fir_state", "_set_fir_state"

    def __init__(self, dphase, phase, taps, rate, fm_demod, device=0, mixer_after_fir=False, unfused=False,
                 kernel="auto"):
        """kernel: "auto", "freq" (always an overlap-save kernel: the 1024-point one up to 257 taps, the 4096- / 16384-point
        ones with mixer and decimator in their store stage up to 1537 / 4097), "time" (the decimating time-domain kernels wherever
        they apply) or "poly" (the polyphase frequency-domain kernel: rates 4, 8, 12 ... 64, <= 513 taps, 505 with FM demod)."""
        super().__init__()
        taps = _as_c64(taps)
        self.rate, self.fm_demod = int(rate), bool(fm_demod)
        flags = (1 if fm_demod else 0) | (2 if mixer_after_fir else 0) | (4 if unfused else 0)
        flags |= {"auto": 0, "freq": 8, "time": 16, "poly": 32}[kernel]
        check(lib().comms_chain_create_ex(float(dphase), float(phase), _ptr(taps), taps.size, self.rate,
                                          flags, device, C.byref(self._h)))

    def _is_fused(self):
        return _get(C.c_int32, lib().comms_chain_is_fused, self._h)

    @property
    def fused(self):
        return bool(self._is_fused())

    @property
    def kernel(self):
        """"unfused", "freq" (fir_os1024_kernel; fir_os4096_kernel / fir_os16k_kernel in their decimating form for 258 ... 4097
        taps), "time" (fir_decim_kernel / fir_decim_wave_kernel), "time_any" (fir_decim_any_kernel) or "poly" (fir_poly8_kernel:
        forced, picked at creation for 258 ... 513 taps, or what the chain's last call ran on)."""
        return ("unfused", "freq", "time", "time_any", "poly")[self._is_fused()]

    _fmt = "c32"

    def set_input_format(self, fmt, scale=1.0):
        """Raw-IQ input ("c32" / "i16" / "u8", see BatchFirNode.set_input_format): converted in the load
        stage of the time-domain chain kernel, by one extra pass in front of the other chain forms."""
        check(lib().comms_chain_set_input_format(self._h, _IQ[fmt][0], float(scale)))
        self._fmt = fmt
        return self

    _out_bits = 0

    def set_output_format(self, fmt, bits_per_sym=1, constellation=None):
        """"bits": run() returns hard decisions of the decimated samples as packed bits (np.uint8, LSB first,
        ceil(n / rate * bits_per_sym / 8) bytes; the inverse of PulseNode.set_input_format("bits", ...)), nearest of
        the 2**bits_per_sym points of `constellation` (None = digital.rs's tables; see comms_sym_to_bits for the rule);
        "c32" restores the default.  No FM chains.  History and phase carry across a switch."""
        if fmt not in ("c32", "bits"):
            raise ValueError("output format must be 'c32' or 'bits' (got %r)" % (fmt,))
        self._out_bits = _set_bits_format(lib().comms_chain_set_output_format, self._h, bits_per_sym if fmt == "bits" else None, constellation)
        return self

    def out_bytes(self, n):
        """Bytes of run's output for n input samples."""
        n_dec = int(n) // self.rate
        if self._out_bits:
            return (n_dec * self._out_bits + 7) // 8
        return n_dec * (4 if self.fm_demod else 8)

    def run(self, x):
        x, n = _as_input(x, self._fmt)
        if self._out_bits:
            out = np.empty(self.out_bytes(n), np.uint8)
        else:
            out = np.empty(n // self.rate, np.float32 if self.fm_demod else np.complex64)
        check(lib().comms_chain_run(self._h, _ptr(x), n, _ptr(out)))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_chain_run_dev(self._h, in_ptr, n, out_ptr, stream))

    def set_fir_state(self, state):
        """FIR history, reference layout (newest first) -- e.g. the halo of a sharded stream."""
        return self.set_state(state)

    def fir_state(self, n_state):
        return self.get_state(n_state)

    @property
    def phase(self):
        """Oscillator phase of the next input sample."""
        return _get(C.c_double, lib().comms_chain_get_phase, self._h)

    @phase.setter
    def phase(self, value):
        check(lib().comms_chain_set_phase(self._h, float(value)))

    @property
    def fm_prev(self):
        """FM.prev of the chain's demodulator: the last decimated filter output of the previous batch."""
        p = np.zeros(1, np.complex64)
        check(lib().comms_chain_get_fm_prev(self._h, _ptr(p)))
        return p[0]

    @fm_prev.setter
    def fm_prev(self, value):
        p = np.array([value], np.complex64)
        check(lib().comms_chain_set_fm_prev(self._h, _ptr(p)))


# ------------------------------------------------------------------ stream nodes with a device history
class RealFirDecimNode(_History, _Handle):
    """Real FIR with decimation (comms_rfir_*): the audio stage of examples/fm_radio.rs:98-164 -- Convert2Node ->
    BatchFirNode<f32> -> Convert3Node -> DecimateNode<f32>(rate) -- as one node over an f32 stream.  Any batch length:
    the decimator restarts at sample 0 of every call, the FIR history advances by all samples."""
    _prefix = "comms_rfir"
    _state_dtype = np.float32   # (no comms_rfir_state_len: get_state takes its n_state)

    def __init__(self, taps, rate, state=None, device=0):
        super().__init__()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.rate = int(rate)
        if state is None:
            check(lib().comms_rfir_create(_ptr(taps), taps.size, None, 0, self.rate, device, C.byref(self._h)))
        else:
            state = np.ascontiguousarray(state, dtype=np.float32)
            check(lib().comms_rfir_create(_ptr(taps), taps.size, _ptr(state), state.size, self.rate, device, C.byref(self._h)))

    def out_len(self, n):
        return _get(C.c_size_t, lib().comms_rfir_out_len, n, self.rate)

    def kernel(self, n):
        """What a batch of n samples is run by: "rfir_decim_kernel<..>", or "series: ..." (the four launches)."""
        return self._kernel_name(n, cap=160)

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(self.out_len(x.size), np.float32)
        check(lib().comms_rfir_run(self._h, _ptr(x), x.size, _ptr(out)))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_rfir_run_dev(self._h, in_ptr, n, out_ptr, stream))


class ResampleNode(_History, _Handle):
    """Rational resampler by up / down (comms_resample_*): UpsampleNode(up) -> BatchFirNode(Complex(taps, 0)) ->
    DecimateNode(down) as one node over an f32 or Complex<f32> stream, which forms only the products with input samples.
    Any batch length: ceil(n up / down) outputs per call, the decimator restarts at sample 0 of every call and the
    history -- (len(taps) - 1) // up INPUT samples -- advances by all samples."""
    _prefix = "comms_resample"
    _state_args = ("n_taps", "up")

    def __init__(self, taps, up, down, dtype=np.float32, device=0):
        super().__init__()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.dtype = self._state_dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.complex64)):
            raise TypeError("ResampleNode takes float32 or complex64 samples, not %s" % self.dtype)
        self.up, self.down, self.n_taps = int(up), int(down), taps.size
        check(lib().comms_resample_create(_ptr(taps), taps.size, self.up, self.down, self.dtype.itemsize, device, C.byref(self._h)))

    def out_len(self, n):
        return _get(C.c_size_t, lib().comms_resample_out_len, n, self.up, self.down)

    def kernel(self, n):
        """What a batch of n samples is run by: "resample_kernel<..> tile=.. lds=.. tiles=.. grid=.. max_grid=..", or "series: ..."
        (the launches)."""
        return self._kernel_name(n, cap=200)

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=self.dtype)
        out = np.empty(self.out_len(x.size), self.dtype)
        check(lib().comms_resample_run(self._h, _ptr(x), x.size, _ptr(out)))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_resample_run_dev(self._h, in_ptr, n, out_ptr, stream))


class ChannelizerNode(_History, _Handle):
    """Polyphase channelizer (comms_channelizer_*): M chains MixerNode(0, -2 pi k / M) -> BatchFirNode(Complex(taps, 0)) ->
    DecimateNode(down), k = 0 .. M-1, over one Complex<f32> stream as one node -- a polyphase filter bank that reads every
    sample once and spends len(taps) multiply-adds per frame (one output of each channel).  Any batch length: ceil(n / down)
    frames per call, returned as an array [channels][frames] (layout "channel", each row a contiguous stream) or
    [frames][channels] (layout "frame").  State: the last len(taps) - 1 input samples and the stream index mod M."""
    _prefix = "comms_channelizer"
    _state_args = ("n_taps",)
    LAYOUTS = {"channel": 0, "frame": 1, 0: 0, 1: 1}

    def __init__(self, taps, channels, down, layout="channel", device=0):
        super().__init__()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        if layout not in self.LAYOUTS:
            raise ValueError("layout is 'channel' or 'frame', not %r" % (layout,))
        self.layout = self.LAYOUTS[layout]
        self.channels, self.down, self.n_taps = int(channels), int(down), taps.size
        check(lib().comms_channelizer_create(_ptr(taps), taps.size, self.channels, self.down, self.layout, device, C.byref(self._h)))

    def out_len(self, n):
        """Frames of a call of n samples; the call writes out_len(n) * channels outputs."""
        return _get(C.c_size_t, lib().comms_channelizer_out_len, n, self.down)

    def kernel(self, n):
        """What a batch of n samples is run by: "channelizer_kernel<..> ...", or "series: ..." (the launches)."""
        return self._kernel_name(n)

    def shape(self, n):
        frames = self.out_len(n)
        return (frames, self.channels) if self.layout else (self.channels, frames)

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        out = np.empty(self.shape(x.size), np.complex64)
        check(lib().comms_channelizer_run(self._h, _ptr(x), x.size, _ptr(out)))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_channelizer_run_dev(self._h, in_ptr, n, out_ptr, stream))

    state = property(_History.get_state, _History.set_state)

    def get_phase(self):
        """The stream index of the next input sample, mod channels."""
        return _get(C.c_uint64, lib().comms_channelizer_get_phase, self._h)

    def set_phase(self, t):
        """Any stream index t >= 0 (reduced mod channels): where a shard starts."""
        check(lib().comms_channelizer_set_phase(self._h, int(t)))

    phase = property(get_phase, set_phase)


class SymbolSyncNode(_History, _Handle):
    """Symbol synchroniser (comms_symsync_*): matched filter with a fractional delay, symbol-rate sampler, rotation and
    (optionally) hard decision over a Complex<f32> stream as one node -- UpsampleNode(phases) -> BatchFirNode(Complex(taps,
    0)) -> skip mu -> DecimateNode(phases * sps) -> MixerNode -> decision, computing only the kept outputs.  taps are real,
    designed at `phases` times the input rate (rrc_taps(N, phases * sps, beta)); batches are multiples of sps samples and
    give n / sps outputs; the history -- (len(taps) - 1) // phases RAW input samples -- does not depend on the timing."""
    _prefix = "comms_symsync"
    _state_args = ("n_taps", "phases")
    _out_bits = 0

    def __init__(self, taps, phases, sps, device=0):
        super().__init__()
        taps = np.ascontiguousarray(taps, dtype=np.float32)
        self.phases, self.sps, self.n_taps = max(int(phases), 1), max(int(sps), 1), taps.size
        check(lib().comms_symsync_create(_ptr(taps), taps.size, int(phases), int(sps), device, C.byref(self._h)))

    def set_timing(self, tau):
        """The sampling instant in input samples (positive = later), rounded to 1 / phases and reduced mod sps."""
        check(lib().comms_symsync_set_timing(self._h, float(tau)))

    def get_timing(self):
        """mu, in steps of 1 / phases input samples: 0 <= mu < sps * phases."""
        return _get(C.c_uint32, lib().comms_symsync_get_timing, self._h)

    timing = property(get_timing, set_timing)

    def set_rotation(self, dphase, phase=0.0):
        """out[k] = y[k] * exp(i (phase + k dphase)), the mixer's convention; the phase carries across calls."""
        check(lib().comms_symsync_set_rotation(self._h, float(dphase), float(phase)))
        self._dphase = float(dphase)

    _dphase = 0.0

    def get_rotation(self):
        """(dphase as given, phase of the next output in [0, 2 pi))."""
        return self._dphase, _get(C.c_double, lib().comms_symsync_get_phase, self._h)

    rotation = property(get_rotation, lambda self, v: self.set_rotation(*v))

    def set_output(self, bits_per_sym=None, constellation=None):
        """bits_per_sym 1 or 2: run() returns hard decisions as packed bits (np.uint8, LSB first, ceil(n / sps *
        bits_per_sym / 8) bytes), nearest of the 2**bits_per_sym points of `constellation` (None = digital.rs's tables; see
        comms_sym_to_bits for the rule); None restores Complex<f32>.  State, phase and timing carry across a switch."""
        self._out_bits = _set_bits_format(lib().comms_symsync_set_output_format, self._h, bits_per_sym, constellation)
        return self

    def out_len(self, n):
        """Symbols of a call of n samples."""
        return _get(C.c_size_t, lib().comms_symsync_out_len, n, self.sps)

    def out_bytes(self, n):
        n_sym = self.out_len(n)
        return (n_sym * self._out_bits + 7) // 8 if self._out_bits else n_sym * 8

    def kernel(self, n):
        """What a batch of n samples is run by: "symsync_kernel<..> tile=.. wg=.. lds=.. tiles=.. grid=.. max_grid=.."."""
        return self._kernel_name(n)

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        out = np.empty(self.out_bytes(x.size), np.uint8) if self._out_bits else np.empty(self.out_len(x.size), np.complex64)
        check(lib().comms_symsync_run(self._h, _ptr(x), x.size, _ptr(out)))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_symsync_run_dev(self._h, in_ptr, n, out_ptr, stream))

    state = property(_History.get_state, _History.set_state)


class SpectrumNode(_History, _Position, _Handle):
    """Spectrum estimator (comms_spectrum_*): windowed, overlapping segments of a Complex<f32> stream -> forward n_fft-point
    transform -> |X|^2 -> the sum of `avg` segments per output row, times `scale`, in one launch (two when avg > 32).  `window`
    is a name ("rect", "hann", "hamming", "blackman": window_taps) or n_fft floats; hop defaults to n_fft / 2; scale defaults
    to 1 / (avg sum w^2), the Welch power spectral density estimate per bin; order "natural" (column k is bin k) or "centred"
    (fftshift).  Any batch length: a call returns the rows it completes, (rows, n_fft) float32, and the rows of a stream do
    not depend on how it is cut into calls.  State: the last n_fft - 1 samples (state), the stream index (position) and the
    sums of the incomplete row (acc)."""
    _prefix = "comms_spectrum"
    _state_args = ("n_fft",)
    ORDERS = {"natural": 0, "centred": 1, "centered": 1, 0: 0, 1: 1}

    def __init__(self, n_fft, window="hann", hop=None, avg=1, scale=None, order="natural", device=0):
        super().__init__()
        self.n_fft = int(n_fft)
        if order not in self.ORDERS:
            raise ValueError("order is 'natural' or 'centred', not %r" % (order,))
        window = window_taps(window, self.n_fft) if isinstance(window, str) else np.ascontiguousarray(window, dtype=np.float32)
        if window.size != self.n_fft:
            raise ValueError("the window has %d values, n_fft is %d" % (window.size, self.n_fft))
        self.window, self.order = window, self.ORDERS[order]
        self.hop, self.avg = (self.n_fft // 2 if hop is None else int(hop)), int(avg)
        self.scale = float(1.0 / (self.avg * np.sum(window.astype(np.float64) ** 2))) if scale is None else float(scale)
        check(lib().comms_spectrum_create(self.n_fft, _ptr(window), self.hop, self.avg, self.scale, self.order, device, C.byref(self._h)))

    def out_len(self, n):
        """Rows a call of n samples completes at the node's position."""
        return _get(C.c_size_t, lib().comms_spectrum_out_len, self._h, n)

    def kernel(self, n):
        """What a call of n samples is run by: "spectrum_kernel<..> ...", and " + spectrum_rows_kernel ..." when avg > 32."""
        return self._kernel_name(n)

    def run(self, x):
        x = np.ascontiguousarray(x, dtype=np.complex64)
        out = np.empty((self.out_len(x.size), self.n_fft), np.float32)
        check(lib().comms_spectrum_run(self._h, _ptr(x), x.size, _ptr(out) if out.size else None))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_spectrum_run_dev(self._h, in_ptr, n, out_ptr, stream))

    state = property(_History.get_state, _History.set_state)
    position = property(_Position.position, _Position.set_position)

    def get_acc(self):
        """The sums of the incomplete row: (2, n_fft) float32, R then the incomplete chunk's c, natural bin order."""
        acc = np.empty((2, self.n_fft), np.float32)
        check(lib().comms_spectrum_get_acc(self._h, _ptr(acc), acc.size))
        return acc

    def set_acc(self, acc):
        acc = np.ascontiguousarray(acc, dtype=np.float32)
        check(lib().comms_spectrum_set_acc(self._h, _ptr(acc), acc.size))

    acc = property(get_acc, set_acc)


_WINDOWS = {"rect": 0, "hann": 1, "hamming": 2, "blackman": 3}


def window_taps(kind, n):
    """The periodic (DFT-even) window `kind` ("rect", "hann", "hamming", "blackman", or its COMMS_WINDOW_* code) of n floats."""
    out = np.empty(int(n), np.float32)
    check(lib().comms_window_taps(_WINDOWS.get(kind, kind), int(n), _ptr(out)))
    return out


# ------------------------------------------------------------------ tap design
def _taps(fn, n_taps, *args):
    out = np.empty(int(n_taps), np.complex64)
    check(fn(int(n_taps), *args, _ptr(out)))
    return out


def rrc_taps(n_taps, sam_per_sym, beta):
    """util/math.rs:221-280; raises CommsError(code 1) for beta outside [0,1]."""
    return _taps(lib().comms_rrc_taps, n_taps, float(sam_per_sym), float(beta))


def rc_taps(n_taps, sam_per_sym, beta):
    return _taps(lib().comms_rc_taps, n_taps, float(sam_per_sym), float(beta))


def gaussian_taps(n_taps, sam_per_sym, alpha):
    return _taps(lib().comms_gaussian_taps, n_taps, float(sam_per_sym), float(alpha))


def rect_taps(n_taps):
    return _taps(lib().comms_rect_taps, n_taps)


# ------------------------------------------------------------------ raw IQ wire formats
def iq_i16_to_c32(x, scale=1.0, device=0):
    """int16 array of shape (n, 2) (re, im) -> complex64 (cast_complex, times scale)."""
    x = np.ascontiguousarray(x, dtype=np.int16).reshape(-1, 2)
    out = np.empty(x.shape[0], np.complex64)
    check(lib().comms_iq_i16_to_c32(_ptr(x), x.shape[0], float(scale), _ptr(out), device))
    return out


def iq_c32_to_i16(x, scale=1.0, device=0):
    """complex64 -> int16 (n, 2): `(scale * x) as i16` per component (Rust `as` semantics)."""
    x = _as_c64(x)
    out = np.empty((x.size, 2), np.int16)
    check(lib().comms_iq_c32_to_i16(_ptr(x), x.size, float(scale), _ptr(out), device))
    return out


def real_to_c32_dev(in_ptr, n, out_ptr, device=0, stream=0):
    """x -> Complex(x, 0) on the device (examples/fm_radio.rs Convert2Node)."""
    check(lib().comms_iq_real_to_c32_dev(in_ptr, n, out_ptr, device, stream))


def c32_re_dev(in_ptr, n, out_ptr, device=0, stream=0):
    """x -> x.re on the device (examples/fm_radio.rs Convert3Node)."""
    check(lib().comms_iq_c32_re_dev(in_ptr, n, out_ptr, device, stream))


def iq_u8_to_c32(x, device=0):
    """uint8 (n, 2) RTL-SDR bytes -> complex64: (x - 127.5) / 127.5."""
    x = np.ascontiguousarray(x, dtype=np.uint8).reshape(-1, 2)
    out = np.empty(x.shape[0], np.complex64)
    check(lib().comms_iq_u8_to_c32(_ptr(x), x.shape[0], _ptr(out), device))
    return out


# ------------------------------------------------------------------ digital modulation (digital.rs)
def _psk(fn, x, per, device):
    x = np.ascontiguousarray(x, dtype=np.uint8).ravel()
    out = np.empty((x.size * per, 2), np.int16)
    check(getattr(lib(), fn)(_ptr(x), x.size, _ptr(out), device))
    return out


def bpsk_byte_mod(x, device=0):
    """digital.rs:17-21 over a byte array: int16 (8n, 2) Complex<i16> symbols, bit i of a byte -> symbol i."""
    return _psk("comms_bpsk_byte_mod", x, 8, device)


def qpsk_byte_mod(x, device=0):
    """digital.rs:39-44 over a byte array: int16 (4n, 2), (byte >> 2i) & 3 -> symbol i."""
    return _psk("comms_qpsk_byte_mod", x, 4, device)


def bpsk_bit_mod(x, device=0):
    """digital.rs:6-14 over values 0 / 1 (anything else: CommsError, as the reference's None)."""
    return _psk("comms_bpsk_bit_mod", x, 1, device)


def qpsk_bit_mod(x, device=0):
    """digital.rs:24-36 over values 0..3 (anything else: CommsError, as the reference's None)."""
    return _psk("comms_qpsk_bit_mod", x, 1, device)


# ------------------------------------------------------------------ hard decisions, bit errors
def _constellation(constellation, bits_per_sym):
    if constellation is None:
        return None
    cons = _as_c64(constellation).ravel()
    if cons.size != 1 << int(bits_per_sym):
        raise ValueError("the constellation holds 2**bits_per_sym points")
    return cons


def _set_bits_format(fn, h, bits_per_sym, constellation):
    """The comms_*_set_{input,output}_format of a node that reads or writes packed bits beside Complex<f32>: bits_per_sym bits
    per symbol against `constellation` (None = digital.rs's tables), or Complex<f32> with bits_per_sym None.  Returns the bits
    per symbol now set (0: Complex<f32>)."""
    if bits_per_sym is None:
        check(fn(h, _lib.SYM_C32, 0, None))
        return 0
    cons = _constellation(constellation, bits_per_sym)
    check(fn(h, _lib.SYM_BITS, int(bits_per_sym), None if cons is None else _ptr(cons)))
    return int(bits_per_sym)


def sym_to_bits(sym, bits_per_sym, constellation=None, device=0):
    """Complex<f32> symbols -> packed hard-decision bits (np.uint8, LSB first, ceil(n * bits_per_sym / 8) bytes):
    nearest of the 2**bits_per_sym points of `constellation` (None = digital.rs's tables), by comms_sym_to_bits's rule."""
    s = _as_c64(sym).ravel()
    cons = _constellation(constellation, bits_per_sym)
    out = np.empty((s.size * int(bits_per_sym) + 7) // 8, np.uint8)
    check(lib().comms_sym_to_bits(_ptr(s), s.size, int(bits_per_sym), None if cons is None else _ptr(cons), _ptr(out), device))
    return out


def sym_to_bits_dev(sym_ptr, n_sym, bits_per_sym, out_ptr, constellation=None, device=0, stream=0):
    cons = _constellation(constellation, bits_per_sym)
    check(lib().comms_sym_to_bits_dev(sym_ptr, int(n_sym), int(bits_per_sym), None if cons is None else _ptr(cons), out_ptr,
                                      device, stream))


def bit_errors(a, b, n_bits, device=0):
    """popcount(a XOR b) over the first n_bits stream bits (LSB first) of two packed byte arrays, counted on the device."""
    a = np.ascontiguousarray(a, dtype=np.uint8).ravel()
    b = np.ascontiguousarray(b, dtype=np.uint8).ravel()
    n_bits = int(n_bits)
    if min(a.size, b.size) * 8 < n_bits:
        raise ValueError("the arrays hold fewer than n_bits bits")
    return _get(C.c_uint64, lib().comms_bit_errors, _ptr(a), _ptr(b), n_bits, tail=(device,))


def bit_errors_dev(a_ptr, b_ptr, n_bits, device=0, stream=0):
    return _get(C.c_uint64, lib().comms_bit_errors_dev, a_ptr, b_ptr, int(n_bits), tail=(device, stream))


# ------------------------------------------------------------------ PRNS source
def _bits_out(fn, h, n, packed):
    """The next n bits of a bit source's host entry: uint8 0 / 1 per bit, or packed LSB first."""
    n = int(n)
    out = np.empty((n + 7) // 8 if packed else n, np.uint8)
    check(fn(h, n, _lib.BITS_PACKED if packed else _lib.BITS_U8, _ptr(out)))
    return out


class PrnsNode(_Handle):
    """PrnsNode::new(poly_mask, state) (prns.rs:93-137) on an unsigned register of `width` = 8, 16, 32 or 64 bits:
    run() returns the next bit, as the reference; run_batch(n) the next n bits (uint8 0/1 per bit, or packed LSB
    first with packed=True), generated on the device.  `state` and skip(n) never wait for the device."""
    _prefix = "comms_prns"

    def __init__(self, poly_mask, state, width=8, device=0):
        super().__init__()
        self.width = int(width)
        check(lib().comms_prns_create(int(poly_mask), int(state), self.width, device, C.byref(self._h)))

    def run(self):
        return int(self.run_batch(1)[0])

    def run_batch(self, n, packed=False):
        return _bits_out(lib().comms_prns_run, self._h, n, packed)

    def run_dev(self, n, out_ptr, packed=False, stream=0):
        check(lib().comms_prns_run_dev(self._h, int(n), _lib.BITS_PACKED if packed else _lib.BITS_U8, out_ptr, stream))

    @property
    def state(self):
        return _get(C.c_uint64, lib().comms_prns_get_state, self._h)

    @state.setter
    def state(self, value):
        check(lib().comms_prns_set_state(self._h, int(value)))

    def skip(self, n):
        """Jump ahead n bits (any n < 2**64): shard r of a stream starts at skip(r * n)."""
        check(lib().comms_prns_skip(self._h, int(n)))
        return self


# ------------------------------------------------------------------ seeded noise source / AWGN channel
class NoiseSource(_Handle):
    """comms_noise_*: the counter-based source (Philox4x32-10 of (seed, stream); include/comms_hip.h has the contract)
    behind NormalNode / UniformNode / random_bit (util/rand_node.rs:26-152) and the AWGN channel node.  `pos` is the
    position in 32-bit stream words, kept on the host: reading, setting and skip(n) never wait for the device."""
    _prefix = "comms_noise"

    def __init__(self, seed, stream=0, device=0):
        super().__init__()
        self._fmt = "c32"
        check(lib().comms_noise_create(int(seed), int(stream), device, C.byref(self._h)))

    @property
    def pos(self):
        return _get(C.c_uint64, lib().comms_noise_get_pos, self._h)

    @pos.setter
    def pos(self, value):
        check(lib().comms_noise_set_pos(self._h, int(value)))

    def skip(self, n_words):
        check(lib().comms_noise_skip(self._h, int(n_words)))
        return self

    def bits(self, n, packed=False):
        """The next n bits: uint8 0 / 1 per bit, or packed LSB first (the PRNS layout)."""
        return _bits_out(lib().comms_noise_bits_run, self._h, n, packed)

    def bits_dev(self, n, out_ptr, packed=False, stream=0):
        check(lib().comms_noise_bits_run_dev(self._h, int(n), _lib.BITS_PACKED if packed else _lib.BITS_U8, out_ptr, stream))

    def uniform(self, n, lo=0.0, hi=1.0):
        out = np.empty(int(n), np.float32)
        check(lib().comms_noise_uniform_run(self._h, out.size, lo, hi, _ptr(out)))
        return out

    def uniform_dev(self, n, out_ptr, lo=0.0, hi=1.0, stream=0):
        check(lib().comms_noise_uniform_run_dev(self._h, int(n), lo, hi, out_ptr, stream))

    def normal(self, n, mu=0.0, sd=1.0, dtype=np.float32):
        """mu + sd * z as float32, or with dtype=np.float64 the f64 form (the f32 z widened)."""
        out = np.empty(int(n), dtype)
        fn = lib().comms_noise_normal_f64_run if out.dtype == np.float64 else lib().comms_noise_normal_run
        check(fn(self._h, out.size, float(mu), float(sd), _ptr(out)))
        return out

    def normal_dev(self, n, out_ptr, mu=0.0, sd=1.0, f64=False, stream=0):
        fn = lib().comms_noise_normal_f64_run_dev if f64 else lib().comms_noise_normal_run_dev
        check(fn(self._h, int(n), float(mu), float(sd), out_ptr, stream))

    def set_input_format(self, fmt, scale=1.0):
        """Input of awgn(): "c32" (default) or "i16" pairs times `scale`, converted in the kernel's load stage."""
        if fmt not in ("c32", "i16"):
            raise ValueError("the AWGN node reads 'c32' or 'i16'")
        check(lib().comms_awgn_set_input_format(self._h, _IQ[fmt][0], scale))
        self._fmt = fmt
        return self

    def awgn(self, x, sigma):
        """x + sigma * (z + i z'), one complex standard pair per sample."""
        a, n = _as_input(x, self._fmt)
        out = np.empty(n, np.complex64)
        check(lib().comms_awgn_run(self._h, _ptr(a), n, sigma, _ptr(out)))
        return out

    def awgn_dev(self, in_ptr, n, sigma, out_ptr, stream=0):
        """Device pointers; in_ptr == out_ptr (in place) is allowed with c32 input."""
        check(lib().comms_awgn_run_dev(self._h, in_ptr, int(n), sigma, out_ptr, stream))


# ------------------------------------------------------------------ block estimators
def frequency_offset_estimate(samples, device=0):
    """frequency_estimator.rs:27-42 on Complex<f64> samples."""
    x = np.ascontiguousarray(samples, dtype=np.complex128)
    return _get(C.c_double, lib().comms_frequency_offset_estimate, _ptr(x), x.size, tail=(device,))


def psk_phase_estimate(symbols, m, device=0):
    """phase_estimator.rs:26-33."""
    x = np.ascontiguousarray(symbols, dtype=np.complex128)
    return _get(C.c_double, lib().comms_psk_phase_estimate, _ptr(x), x.size, int(m), tail=(device,))


def qam_phase_estimate(symbols, device=0):
    """phase_estimator.rs:58-65."""
    x = np.ascontiguousarray(symbols, dtype=np.complex128)
    return _get(C.c_double, lib().comms_qam_phase_estimate, _ptr(x), x.size, tail=(device,))


class TimingEstimatorNode(_Handle):
    """TimingEstimatorNode::new(n, d, alpha) / run (timing_estimator.rs:116-136): Complex<f64>
    block in, timing offset in samples out."""
    _prefix = "comms_timing"

    def __init__(self, n, d, alpha, device=0):
        super().__init__()
        check(lib().comms_timing_create(int(n), int(d), float(alpha), device, C.byref(self._h)))

    def run(self, samples):
        x = np.ascontiguousarray(samples, dtype=np.complex128)
        return _get(C.c_double, lib().comms_timing_push, self._h, _ptr(x), x.size)

    def run_dev(self, in_ptr, n, stream=0):
        return _get(C.c_double, lib().comms_timing_push_dev, self._h, in_ptr, n, tail=(stream,))

    def kernel(self, n):
        """What a block of n samples is run by: "timing_kernel tile=.. wg=.. taps=.. filter_passes=.. tiles=.. grid=.. max_grid=.."."""
        return self._kernel_name(n)


class _SyncEstimateStruct(C.Structure):
    _fields_ = [("timing", C.c_double), ("freq", C.c_double), ("timing_sum", C.c_double * 2), ("freq_sum", C.c_double * 2)]


class SyncEstimate:
    """comms_sync_estimate_t: timing (samples) and freq (rad / sample) of one block, and the complex sums they are the
    angles of (to add over blocks or shards before taking the angle)."""
    __slots__ = ("timing", "freq", "timing_sum", "freq_sum")

    def __init__(self, s):
        self.timing, self.freq = s.timing, s.freq
        self.timing_sum = complex(s.timing_sum[0], s.timing_sum[1])
        self.freq_sum = complex(s.freq_sum[0], s.freq_sum[1])

    def __repr__(self):
        return "SyncEstimate(timing=%r, freq=%r, timing_sum=%r, freq_sum=%r)" % (self.timing, self.freq, self.timing_sum, self.freq_sum)


class SyncEstimatorNode(_Handle):
    """Timing and frequency estimates of a Complex<f32> block from one read of it (comms_syncest_*): TimingEstimator::push
    at (n, d, alpha) and frequency_offset_estimate of the widened samples, the timing filter in f32.  What to feed
    SymbolSyncNode (estimator at n = sps): timing = est.timing + (N - 1) / (2 phases), set_rotation(-est.freq * sps,
    -phase estimate)."""
    _prefix = "comms_syncest"

    def __init__(self, n, d, alpha, device=0):
        super().__init__()
        check(lib().comms_syncest_create(int(n), int(d), float(alpha), device, C.byref(self._h)))

    def run(self, samples):
        x = np.ascontiguousarray(samples, dtype=np.complex64)
        out = _SyncEstimateStruct()
        check(lib().comms_syncest_run(self._h, _ptr(x), x.size, C.byref(out)))
        return SyncEstimate(out)

    def run_dev(self, in_ptr, n, stream=0):
        out = _SyncEstimateStruct()
        check(lib().comms_syncest_run_dev(self._h, in_ptr, n, C.byref(out), stream))
        return SyncEstimate(out)

    def kernel(self, n):
        """What a block of n samples is run by: "syncest_kernel tile=.. wg=.. taps=.. lds=.. tiles=.. grid=.. max_grid=.."."""
        return self._kernel_name(n)


def psk_phase_estimate_c32(symbols, m, device=0):
    """phase_estimator.rs:26-33 on Complex<f32> symbols (widened in the kernel's load)."""
    x = np.ascontiguousarray(symbols, dtype=np.complex64)
    return _get(C.c_double, lib().comms_psk_phase_estimate_c32, _ptr(x), x.size, int(m), tail=(device,))


def qam_phase_estimate_c32(symbols, device=0):
    """phase_estimator.rs:58-65 on Complex<f32> symbols."""
    x = np.ascontiguousarray(symbols, dtype=np.complex64)
    return _get(C.c_double, lib().comms_qam_phase_estimate_c32, _ptr(x), x.size, tail=(device,))


def psk_phase_estimate_c32_dev(in_ptr, n, m, device=0, stream=0):
    return _get(C.c_double, lib().comms_psk_phase_estimate_c32_dev, in_ptr, n, int(m), tail=(device, stream))


def qam_phase_estimate_c32_dev(in_ptr, n, device=0, stream=0):
    return _get(C.c_double, lib().comms_qam_phase_estimate_c32_dev, in_ptr, n, tail=(device, stream))


class _FrameDetectionStruct(C.Structure):
    _fields_ = [("index", C.c_uint64), ("corr_re", C.c_float), ("corr_im", C.c_float), ("metric", C.c_float), ("energy", C.c_float)]


FRAME_DETECTION_DTYPE = np.dtype([("index", np.uint64), ("corr_re", np.float32), ("corr_im", np.float32), ("metric", np.float32),
                                  ("energy", np.float32)])


class FrameDetection:
    """comms_frame_detection_t: `index` of the word's first symbol in the stream, the correlation `corr` = c[index] (its angle
    is the rotation of the received word), the normalised `metric` in [0, 1] and the window's `energy`."""
    __slots__ = ("index", "corr", "metric", "energy")

    def __init__(self, s):
        self.index = int(s["index"])
        self.corr = complex(float(s["corr_re"]), float(s["corr_im"]))
        self.metric, self.energy = float(s["metric"]), float(s["energy"])

    @property
    def phase(self):
        """arg(corr): MixerNode(0, -phase) or SymbolSyncNode.set_rotation(dphase, phase_now - phase) takes it out."""
        return float(np.arctan2(self.corr.imag, self.corr.real))

    def __eq__(self, other):
        return isinstance(other, FrameDetection) and (self.index, self.corr, self.metric, self.energy) == (
            other.index, other.corr, other.metric, other.energy)

    def __repr__(self):
        return "FrameDetection(index=%d, corr=%r, metric=%r, energy=%r)" % (self.index, self.corr, self.metric, self.energy)


class FrameSyncNode(_History, _Detector, _Handle):
    """Frame synchroniser (comms_framesync_*): normalised correlation of a Complex<f32> symbol stream (SymbolSyncNode's
    output) with a known `word`, peak search over +-`guard` positions and the `threshold` in one launch that returns only the
    detections.  A call on n symbols decides n positions (a word is reported `guard` symbols after its end); flush() ends a
    stream.  Detections are bit-identical however the stream is cut into calls.  `cap` limits the detections returned (the
    lowest indices); `found` is the true count of the last call.  With raw=True a call returns the structured array
    (FRAME_DETECTION_DTYPE) instead of FrameDetection values."""
    _prefix = "comms_framesync"
    _state_args = ("n_word", "guard")

    def __init__(self, word, threshold, guard, device=0):
        super().__init__()
        word = np.ascontiguousarray(word, dtype=np.complex64)
        self.n_word, self.guard = word.size, int(guard)
        check(lib().comms_framesync_create(_ptr(word), word.size, float(threshold), int(guard), device, C.byref(self._h)))

    def run(self, symbols, cap=None, raw=False):
        x = np.ascontiguousarray(symbols, dtype=np.complex64)
        return self._detect(lib().comms_framesync_run, x.size, cap, raw, _ptr(x), x.size)

    def run_dev(self, in_ptr, n, cap=None, stream=0, raw=False):
        return self._detect(lib().comms_framesync_run_dev, n, cap, raw, in_ptr, n, tail=(stream,))

    def flush(self, cap=None, raw=False):
        """The positions still undecided, as if n_word + guard zero symbols followed; history zero afterwards, position kept."""
        return self._detect(lib().comms_framesync_flush, self.n_word + self.guard, cap, raw)

    state = _History.get_state   # the last n_state symbols (default: all n_word + 2 guard - 1), newest first

    def kernel(self, n):
        """What a call on n symbols is run by: "framesync_kernel tile=.. wg=.. word=.. guard=.. lds=.. tiles=.. grid=.. max_grid=.."."""
        return self._kernel_name(n)


class _FrameHeaderStruct(C.Structure):
    _fields_ = [("index", C.c_uint64), ("start", C.c_uint64), ("rot_re", C.c_float), ("rot_im", C.c_float), ("gain", C.c_float),
                ("metric", C.c_float)]


FRAME_HEADER_DTYPE = np.dtype([("index", np.uint64), ("start", np.uint64), ("rot_re", np.float32), ("rot_im", np.float32),
                               ("gain", np.float32), ("metric", np.float32)])
_SYM_FORMATS = {"c32": _lib.SYM_C32, "bits": _lib.SYM_BITS, "llr": _lib.SYM_LLR}


def _as_detections(detections):
    """FrameSyncNode's raw=True array, or its FrameDetection list, as a contiguous FRAME_DETECTION_DTYPE array."""
    if isinstance(detections, np.ndarray) and detections.dtype == FRAME_DETECTION_DTYPE:
        return np.ascontiguousarray(detections)
    detections = [] if detections is None else list(detections)
    out = np.zeros(len(detections), FRAME_DETECTION_DTYPE)
    for i, d in enumerate(detections):
        out[i] = (d.index, d.corr.real, d.corr.imag, d.metric, d.energy)
    return out


class DeframeNode(_History, _Position, _Handle):
    """Deframer (comms_deframe_*): takes the symbol stream FrameSyncNode takes, in the same calls, and the detections those
    calls return, and writes every frame that becomes complete in a call -- `n_payload` symbols from index + `offset`,
    derotated by the detection's correlation and, with normalise=True, scaled by word_energy / |corr| -- in one launch:
    packed bits ("bits"), max-log LLRs ("llr", positive = bit 0, scaled by llr_scale) or Complex<f32> symbols ("c32", the
    default), one record per frame.  A frame that ends in a later call stays pending and comes out of that call; the frames do
    not depend on how the stream is cut into calls.  `lookback` >= the frame synchroniser's guard - 1.  run() returns an array
    of shape (n_frames, n_payload) complex64, (n_frames, frame_bytes) uint8 or (n_frames, n_payload * bits_per_sym) float32;
    `headers` holds the FRAME_HEADER_DTYPE records of the last call."""
    _prefix = "comms_deframe"
    _state_args = ("n_payload", "lookback")

    def __init__(self, n_payload, offset, lookback, bits_per_sym=2, constellation=None, normalise=False, word_energy=None, device=0):
        super().__init__()
        self.n_payload, self.offset, self.lookback, self.bits_per_sym = int(n_payload), int(offset), int(lookback), int(bits_per_sym)
        self.format = "c32"
        self.headers = np.zeros(0, FRAME_HEADER_DTYPE)
        table = None if constellation is None else np.ascontiguousarray(constellation, dtype=np.complex64)
        if table is not None and table.size != 1 << self.bits_per_sym:
            raise ValueError("constellation must hold 2**bits_per_sym points")
        check(lib().comms_deframe_create(self.n_payload, self.offset, self.lookback, self.bits_per_sym,
                                         None if table is None else _ptr(table), _lib.DEFRAME_NORMALISE if normalise else 0, device,
                                         C.byref(self._h)))
        if word_energy is not None:
            self.set_word_energy(word_energy)

    def set_word_energy(self, word_energy):
        """sum |p|^2 of the word: what normalise=True divides |corr| into."""
        check(lib().comms_deframe_set_word_energy(self._h, float(word_energy)))
        return self

    def set_output_format(self, fmt):
        """ "c32" (default), "bits" or "llr"; may change between calls."""
        if fmt not in _SYM_FORMATS:
            raise ValueError("the deframer writes 'c32', 'bits' or 'llr'")
        check(lib().comms_deframe_set_output_format(self._h, _SYM_FORMATS[fmt]))
        self.format = fmt
        return self

    def set_llr_scale(self, scale):
        """s of L = s (D1 - D0): 1 / (2 sigma^2) for noise of sigma per component."""
        check(lib().comms_deframe_set_llr_scale(self._h, float(scale)))
        return self

    frame_bytes = _record("comms_deframe_frame_bytes")      # frame_bytes(): bytes of one output record in the format set

    def frames_ready(self, n, detections=None):
        """How many frames a call on n symbols with these detections would emit (host arithmetic)."""
        det = _as_detections(detections)
        return _get(C.c_size_t, lib().comms_deframe_frames_ready, self._h, int(n), _ptr(det) if det.size else None, det.size)

    def _shape(self, raw, n_frames):
        dtype = {"c32": np.complex64, "bits": np.uint8, "llr": np.float32}[self.format]
        fb = self.frame_bytes()
        return raw[: n_frames * fb].view(dtype).reshape(n_frames, fb // np.dtype(dtype).itemsize)

    def run(self, symbols, detections=None, cap=None):
        x = np.ascontiguousarray(symbols, dtype=np.complex64)
        det = _as_detections(detections)
        cap = self.frames_ready(x.size, det) if cap is None else int(cap)
        raw = np.zeros(cap * self.frame_bytes(), np.uint8)
        hdr, found = np.zeros(cap, FRAME_HEADER_DTYPE), C.c_size_t()
        check(lib().comms_deframe_run(self._h, _ptr(x), x.size, _ptr(det) if det.size else None, det.size, _ptr(raw) if cap else None,
                                      cap, _ptr(hdr) if cap else None, C.byref(found)))
        self.headers = hdr[: found.value]
        return self._shape(raw, found.value)

    def run_dev(self, in_ptr, n, detections, out_ptr, cap_frames, stream=0):
        """Device pointers; returns the number of frames written at out_ptr (frame f at f * frame_bytes())."""
        det = _as_detections(detections)
        cap = int(cap_frames)
        hdr, found = np.zeros(cap, FRAME_HEADER_DTYPE), C.c_size_t()
        check(lib().comms_deframe_run_dev(self._h, in_ptr, int(n), _ptr(det) if det.size else None, det.size, out_ptr, cap,
                                          _ptr(hdr) if cap else None, C.byref(found), stream))
        self.headers = hdr[: found.value]
        return found.value

    def flush(self):
        """Drops the pending (incomplete) frames and returns how many; history zero afterwards, position kept."""
        return _get(C.c_size_t, lib().comms_deframe_flush, self._h)

    state = _History.get_state   # the last n_state symbols (default: all max(lookback, n_payload - 1)), newest first

    # (set_position also forgets the pending frames: restore a checkpoint as set_state, set_position, set_pending)

    def pending(self):
        """The frames admitted and not yet complete (FRAME_HEADER_DTYPE), ascending."""
        n = _get(C.c_size_t, lib().comms_deframe_get_pending, self._h, None, 0)
        out = np.zeros(n, FRAME_HEADER_DTYPE)
        _get(C.c_size_t, lib().comms_deframe_get_pending, self._h, _ptr(out) if n else None, n)
        return out

    def set_pending(self, pending):
        pending = np.ascontiguousarray(pending, dtype=FRAME_HEADER_DTYPE)
        check(lib().comms_deframe_set_pending(self._h, _ptr(pending) if pending.size else None, pending.size))
        return self

    def kernel(self, n_frames):
        """What a call that emits n_frames frames is run by: "deframe_kernel wg=.. items=.. lanes=.. grid=.. max_grid=.. lds=.."."""
        return self._kernel_name(int(n_frames))


# ------------------------------------------------------------------ convolutional FEC
def _conv_args(K, n, gens, terminated):
    """(K, n, gens array or None, flags) of a code: gens=None is K = 7, g = (0o171, 0o133)."""
    g = None if gens is None else np.ascontiguousarray(gens, dtype=np.uint32)
    n = (2 if g is None else g.size) if n is None else int(n)
    if g is not None and g.size != n:
        raise ValueError("gens must hold n generators")
    return int(K), n, g, _lib.CONV_TERMINATED if terminated else _lib.CONV_TRUNCATED


class ConvEncoderNode(_FrameNode, _Handle):
    """Rate-1/n convolutional encoder (comms_convenc_*): frame-major records of `n_info_bits` packed bits (LSB first, each
    record ceil(bits / 8) bytes rounded up to 4) -> records of n * steps coded bits, coded bit j of step t at t * n + j, all
    frames of a call in one launch.  terminated=True appends K - 1 zero bits (steps = n_info_bits + K - 1).  Stateless:
    every frame starts in state 0.  run() takes and returns uint8 arrays of shape (n_frames, frame bytes)."""
    _prefix = "comms_convenc"
    _frame = _frame_call(_prefix, np.uint8, np.uint8)

    def __init__(self, n_info_bits, K=7, gens=None, n=None, terminated=True, device=0):
        super().__init__()
        K, n, g, flags = _conv_args(K, n, gens, terminated)
        self.n_info_bits, self.K, self.n = int(n_info_bits), K, n
        check(lib().comms_convenc_create(K, n, None if g is None else _ptr(g), flags, self.n_info_bits, device, C.byref(self._h)))

    def kernel(self, n_frames):
        """ "conv_encode_kernel wg=.. K=.. n=.. steps=.. words=.. grid=.. max_grid=.. lds=0" for a call on n_frames frames."""
        return self._kernel_name(int(n_frames))


class ViterbiNode(_FrameNode, _Handle):
    """Viterbi decoder of ConvEncoderNode's code (comms_viterbi_*): frame-major records of `record_llrs` f32 LLRs (positive =
    bit 0; the first n * steps are used; None = exactly that many) -> records of `n_info_bits` decoded bits, all frames of a
    call in one launch, one wave per frame.  The decisions are integer arithmetic on q = clamp(rint(L * qscale), -127, 127)
    (NaN: 0), so they are the bits of the definition exactly.  A DeframeNode "llr" record of at least n * steps values is a
    valid input as it stands.  run() returns uint8 (n_frames, out_frame_bytes); with metrics=True also the final int32
    path metric of every frame."""
    _prefix = "comms_viterbi"
    _frame = _frame_call(_prefix, np.float32, np.uint8)

    def __init__(self, n_info_bits, K=7, gens=None, n=None, terminated=True, record_llrs=None, qscale=None, device=0):
        super().__init__()
        K, n, g, flags = _conv_args(K, n, gens, terminated)
        self.n_info_bits, self.K, self.n = int(n_info_bits), K, n
        check(lib().comms_viterbi_create(K, n, None if g is None else _ptr(g), flags, self.n_info_bits,
                                         0 if record_llrs is None else int(record_llrs), device, C.byref(self._h)))
        if qscale is not None:
            self.set_quant_scale(qscale)

    def set_quant_scale(self, qscale):
        """q = clamp(rint(L * qscale), -127, 127): for LLRs 2 y / sigma^2 of unit symbols, about 127 / (6 + 4 / sigma^2)
        keeps all but the rarest values off the clamp."""
        check(lib().comms_viterbi_set_quant_scale(self._h, float(qscale)))
        return self

    def run(self, llr, metrics=False):
        return self._frame.run(self, llr, side=(np.int32,)) if metrics else self._frame.run(self, llr, tail=(None,))

    def run_dev(self, llr_ptr, n_frames, bits_ptr, metrics_ptr=None, stream=0):
        self._frame.run_dev(self, llr_ptr, n_frames, bits_ptr, metrics_ptr, stream)

    def kernel(self, n_frames):
        """ "viterbi_kernel<n,lds|workspace> wg=.. waves=.. K=.. steps=.. seam=.. grid=.. max_grid=.. lds=.. workspace=.."."""
        return self._kernel_name(int(n_frames))


# ------------------------------------------------------------------ LDPC coding
def _ldpc_base(base, Z):
    """The base matrix as a contiguous (mb, nb) int16 array: -1 is a zero block, b >= 0 the identity shifted by b."""
    B = np.ascontiguousarray(base, dtype=np.int16)
    if B.ndim != 2:
        raise ValueError("base must be a matrix of mb x nb entries")
    return B, int(Z)


class LdpcEncoderNode(_FrameNode, _Handle):
    """Encoder of a quasi-cyclic LDPC code with a dual-diagonal parity part (comms_ldpcenc_*): `base` is the mb x nb base
    matrix (-1: zero block; b >= 0: check z of block row i touches variable j Z + (z + b) mod Z), Z the lifting size.
    Frame-major records of T = (nb - mb) Z packed bits (LSB first, each record ceil(bits / 8) bytes rounded up to 4) ->
    records of N = nb Z coded bits [u | p_0 | ... | p_{mb-1}], all frames of a call in one launch, one wave per frame.
    run() takes and returns uint8 arrays of shape (n_frames, frame bytes)."""
    _prefix = "comms_ldpcenc"
    _frame = _frame_call(_prefix, np.uint8, np.uint8)

    def __init__(self, base, Z, device=0):
        super().__init__()
        B, self.Z = _ldpc_base(base, Z)
        self.mb, self.nb = B.shape
        self.n_info_bits, self.n_coded_bits = (self.nb - self.mb) * self.Z, self.nb * self.Z
        check(lib().comms_ldpcenc_create(self.mb, self.nb, self.Z, _ptr(B), device, C.byref(self._h)))

    def kernel(self, n_frames):
        """ "ldpc_encode_kernel wg=.. frames_per_wg=.. Z=.. grid=.. lds=.." for a call on n_frames frames."""
        return self._kernel_name(int(n_frames))


class LdpcDecoderNode(_FrameNode, _Handle):
    """Layered normalised min-sum decoder of LdpcEncoderNode's code family (comms_ldpcdec_*; any base matrix within the
    limits): frame-major records of `record_llrs` f32 LLRs (positive = bit 0; the first N are used; 0 = exactly N) ->
    records of T decoded bits, all frames of a call in one launch, one wave per frame, a frame's state in LDS.  Integer
    arithmetic on q = clamp(rint(L * qscale), -127, 127) (NaN: 0) with a fixed schedule, messages scaled by norm16 / 16, at
    most max_iters iterations with a stop at the first one whose hard decisions satisfy every check: the bits are those of
    the definition exactly.  run() returns uint8 (n_frames, out_frame_bytes); with status=True also one int32 per frame:
    the iterations run if the frame converged, -max_iters if it did not."""
    _prefix = "comms_ldpcdec"
    _frame = _frame_call(_prefix, np.float32, np.uint8)

    def __init__(self, base, Z, max_iters=20, norm16=12, record_llrs=0, qscale=1.0, device=0):
        super().__init__()
        B, self.Z = _ldpc_base(base, Z)
        self.mb, self.nb = B.shape
        self.n_info_bits, self.n_coded_bits, self.max_iters = (self.nb - self.mb) * self.Z, self.nb * self.Z, int(max_iters)
        check(lib().comms_ldpcdec_create(self.mb, self.nb, self.Z, _ptr(B), self.max_iters, int(norm16), int(record_llrs), device,
                                         C.byref(self._h)))
        if qscale != 1.0:
            self.set_quant_scale(qscale)

    def set_quant_scale(self, qscale):
        """q = clamp(rint(L * qscale), -127, 127), as ViterbiNode.set_quant_scale."""
        check(lib().comms_ldpcdec_set_quant_scale(self._h, float(qscale)))
        return self

    def run(self, llr, status=False):
        return self._frame.run(self, llr, side=(np.int32,)) if status else self._frame.run(self, llr, tail=(None,))

    def run_dev(self, llr_ptr, n_frames, bits_ptr, status_ptr=None, stream=0):
        self._frame.run_dev(self, llr_ptr, n_frames, bits_ptr, status_ptr, stream)

    def kernel(self, n_frames):
        """ "ldpc_decode_kernel wg=.. waves=.. frames_per_wg=.. mb=.. nb=.. Z=.. edges=.. max_iters=.. grid=.. lds=.."."""
        return self._kernel_name(int(n_frames))


# ------------------------------------------------------------------ rate matching
class _RateMatch(_FrameNode, _Handle):
    """One frame format of comms_ratematch_*: n_coded coded bits, a puncturing `pattern` (0 / 1 per coded position, repeated;
    None keeps everything), an interleaver over the n_tx_bits kept bits (`cols` columns of the pruned block interleaver, or an
    explicit `perm` with perm[k] the kept-bit index transmitted k-th) and `scramble`, n_tx_bits bits packed LSB first (uint8)
    that are XORed onto the transmitted bits, or None."""
    _prefix = "comms_ratematch"
    _direction = None

    def __init__(self, n_coded, pattern=None, cols=0, perm=None, scramble=None, record_llrs=0, device=0):
        super().__init__()
        self.n_coded = int(n_coded)
        pat = None if pattern is None else np.ascontiguousarray(pattern, dtype=np.uint8)
        pm = None if perm is None else np.ascontiguousarray(perm, dtype=np.uint32)
        sc = None if scramble is None else np.ascontiguousarray(scramble, dtype=np.uint8)
        kept = self.n_coded if pat is None or pat.size == 0 else int(np.count_nonzero(np.resize(pat, max(self.n_coded, 0))))
        if pm is not None and pm.size != kept:
            raise ValueError("perm must hold one entry per transmitted bit (%d)" % kept)
        if sc is not None and sc.size < (kept + 7) // 8:
            raise ValueError("scramble must hold %d packed bits" % kept)
        check(lib().comms_ratematch_create(self.n_coded, None if pat is None else _ptr(pat), 0 if pat is None else pat.size, int(cols),
                                           None if pm is None else _ptr(pm), None if sc is None else _ptr(sc), int(record_llrs), device,
                                           C.byref(self._h)))

    @property
    def n_tx_bits(self):
        return lib().comms_ratematch_n_tx_bits(self._h)

    def map(self):
        """src: the coded position that feeds transmitted bit k (uint32, n_tx_bits entries)."""
        src = np.zeros(self.n_tx_bits, np.uint32)
        check(lib().comms_ratematch_get_map(self._h, _ptr(src), src.size))
        return src

    def kernel(self, n_frames):
        """ "ratematch_tx_kernel | ratematch_rx_kernel wg=.. table=lds|global seam=.. n_coded=.. n_tx=.. words= | values=..
        grid=.. max_grid=.. lds=.." for a call on n_frames frames."""
        return self._kernel_name(self._direction, int(n_frames))


class RateMatchNode(_RateMatch):
    """Transmit rate matching between ConvEncoderNode and the bit-input modulators: frame-major records of n_coded packed
    bits (the encoder's records) -> records of n_tx_bits bits, tx_bit[k] = in_bit[map()[k]] ^ scramble_bit[k], all frames of a
    call in one launch.  Stateless.  run() takes and returns uint8 arrays of shape (n_frames, frame bytes)."""
    _direction = _lib.RATEMATCH_TX
    _frame = _frame_call("comms_ratematch_tx", np.uint8, np.uint8)

    def __init__(self, n_coded, pattern=None, cols=0, perm=None, scramble=None, device=0):
        super().__init__(n_coded, pattern, cols, perm, scramble, 0, device)


class RateDematchNode(_RateMatch):
    """Receive rate matching between DeframeNode ("llr") and ViterbiNode, of the same frame format as RateMatchNode: records
    of `record_llrs` f32 (0 = exactly n_tx_bits; the first n_tx_bits are used) -> records of n_coded f32, +0.0 at the punctured
    positions and elsewhere the input value with its sign bit toggled where the scramble bit is 1: a ViterbiNode input as it
    stands.  Stateless.  run() takes float32 and returns float32 (n_frames, n_coded)."""
    _direction = _lib.RATEMATCH_RX
    _frame = _frame_call("comms_ratematch_rx", np.float32, np.float32)

    def run(self, llr):
        return self._frame.run(self, llr)

    def run_dev(self, llr_ptr, n_frames, out_ptr, stream=0):
        self._frame.run_dev(self, llr_ptr, n_frames, out_ptr, stream)


# ------------------------------------------------------------------ frame check (CRC)
class _Crc(_FrameNode, _Handle):
    """One frame check of comms_crc_*: a `width`-bit CRC (1 ... 32) with polynomial `poly` (normal form, no x^width term),
    register `init` and final `xorout`, no reflection, over frames of `n_payload_bits` bits; the CRC follows the payload with
    its x^(width-1) coefficient first.  Records are packed LSB first, so (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF) is the
    Ethernet FCS."""
    _prefix = "comms_crc"
    _direction = None

    def __init__(self, width, poly, init, xorout, n_payload_bits, device=0):
        super().__init__()
        self.width, self.n_payload_bits = int(width), int(n_payload_bits)
        for v in (poly, init, xorout):
            if not 0 <= int(v) < (1 << 32):
                raise ValueError("poly, init and xorout are unsigned 32-bit values")
        check(lib().comms_crc_create(self.width, int(poly), int(init), int(xorout), self.n_payload_bits, device, C.byref(self._h)))

    _payload_bytes, _coded_bytes = _record("comms_crc_payload_frame_bytes"), _record("comms_crc_coded_frame_bytes")
    payload_frame_bytes, coded_frame_bytes = property(_payload_bytes), property(_coded_bytes)

    def kernel(self, n_frames):
        """ "crc_attach_kernel | crc_check_kernel wg=.. group=.. rounds=.. width=.. words=.. frames=.. grid=.. max_grid=.. lds=0"
        for a call on n_frames frames."""
        return self._kernel_name(self._direction, int(n_frames))


class CrcAttachNode(_Crc):
    """Appends the CRC in front of ConvEncoderNode: frame-major records of n_payload_bits packed bits -> records of
    n_payload_bits + width bits, all frames of a call in one launch.  Stateless.  run() takes and returns uint8 arrays of shape
    (n_frames, frame bytes)."""
    _direction = _lib.CRC_ATTACH
    _frame = _FrameCall("comms_crc_attach_run", np.uint8, np.uint8, _Crc._payload_bytes, _Crc._coded_bytes)


class CrcCheckNode(_Crc):
    """Checks the CRC behind ViterbiNode, of the same format as CrcAttachNode: records of n_payload_bits + width bits (the
    decoder's records with n_info_bits = n_payload_bits + width) -> the payload records, one pass flag per frame (int32, 1 =
    the recomputed CRC equals the received bits) and the recomputed CRC (uint32), all frames of a call in one launch.
    Stateless.  run() returns (payload, passed, crc); n_failed holds the failed frames of the last run().  run_dev takes a
    pointer per output, each may be None; the launch ADDS the call's failed frames to the uint32 at n_failed_ptr."""
    _direction = _lib.CRC_CHECK
    n_failed = 0
    _frame = _FrameCall("comms_crc_check_run", np.uint8, np.uint8, _Crc._coded_bytes, _Crc._payload_bytes)

    def run(self, frames):
        failed = C.c_size_t(0)
        payload, passed, crc = self._frame.run(self, frames, side=(np.int32, np.uint32), tail=(C.byref(failed),))
        self.n_failed = failed.value
        return payload, passed, crc

    def run_dev(self, in_ptr, n_frames, payload_ptr=None, pass_ptr=None, crc_ptr=None, n_failed_ptr=None, stream=0):
        self._frame.run_dev(self, in_ptr, n_frames, payload_ptr, pass_ptr, crc_ptr, n_failed_ptr, stream)


# ------------------------------------------------------------------ symbol mapper and soft demapper
def _table(fn, bits_per_sym, scale):
    out = np.zeros(256, np.complex64)                     # the largest table; a refused bits_per_sym writes nothing
    check(getattr(lib(), fn)(int(bits_per_sym), float(scale), _ptr(out)))
    return out[: 1 << int(bits_per_sym)].copy()


def qam_table(bits_per_sym, scale=1.0):
    """The Gray-coded square QAM table of comms_constellation_qam (bits_per_sym 2, 4, 6, 8; 1 is BPSK on the real axis): the
    low half of a value's bits chooses the real level, the high half the imaginary one, levels (2^k - 1 - 2 rank) * scale.
    Host arithmetic, no device.  np.complex64, 2**bits_per_sym points."""
    return _table("comms_constellation_qam", bits_per_sym, scale)


def psk_table(bits_per_sym, scale=1.0):
    """The Gray-coded PSK table of comms_constellation_psk (bits_per_sym 1 ... 4): point v at angle 2 pi rank(v) / 2^m, plus
    pi/4 at bits_per_sym = 2 (scale sqrt(2) gives digital.rs's QPSK table).  Host arithmetic, no device."""
    return _table("comms_constellation_psk", bits_per_sym, scale)


class SymbolMapNode(_FrameNode, _Handle):
    """Packed bit records -> frames of Complex<f32> symbols (comms_symmap_*), behind RateMatchNode and in front of PulseNode in
    "c32" input format: every record of n_bits bits (RateMatchNode's output record) becomes `word` (the known word a
    FrameSyncNode looks for, or None), ceil(n_bits / bits_per_sym) payload symbols table[v] -- v the record's next
    bits_per_sym bits, the first as the LSB, bits beyond n_bits reading as 0 -- and `gap` symbols (0, 0); all frames of a call
    in one launch.  constellation: 2**bits_per_sym points (qam_table, psk_table, or any), None = digital.rs's tables at 1 or 2
    bits.  Stateless.  run() takes uint8 (n_frames, in_frame_bytes) and returns complex64 (n_frames, out_frame_syms)."""
    _prefix = "comms_symmap"
    _frame = _FrameCall("comms_symmap_run", np.uint8, np.complex64, _record("comms_symmap_in_frame_bytes"), _record("comms_symmap_out_frame_syms", 8))

    def __init__(self, bits_per_sym, constellation, n_bits, word=None, gap=0, device=0):
        super().__init__()
        self.bits_per_sym, self.n_bits = int(bits_per_sym), int(n_bits)
        cons = None if constellation is None else _as_c64(constellation).ravel()
        if cons is not None and 1 <= self.bits_per_sym <= 8 and cons.size != 1 << self.bits_per_sym:
            raise ValueError("the constellation holds 2**bits_per_sym points")
        w = None if word is None else _as_c64(word).ravel()
        check(lib().comms_symmap_create(self.bits_per_sym, None if cons is None else _ptr(cons), self.n_bits,
                                        None if w is None or not w.size else _ptr(w), 0 if w is None else w.size, int(gap), device,
                                        C.byref(self._h)))

    @property
    def out_frame_syms(self):
        return self.out_frame_bytes // 8

    def kernel(self, n_frames):
        """ "symmap_kernel wg=.. bits=.. n_bits=.. word=.. payload=.. gap=.. syms=.. frames=.. grid=.. max_grid=.. lds=.."."""
        return self._kernel_name(int(n_frames))


class DemapNode(_FrameNode, _Handle):
    """Records of n_payload Complex<f32> symbols -> max-log LLRs ("llr", the default: bits_per_sym float32 per symbol, positive
    = bit 0, scaled by llr_scale = 1 / (2 sigma^2)) or packed hard bits ("bits") against a table of 2**bits_per_sym points
    (comms_demap_*), all frames of a call in one launch: behind DeframeNode in "c32" format with normalise=True, in front of
    RateDematchNode(record_llrs = n_payload * bits_per_sym).  The rule is sym_to_bits's and DeframeNode's over the whole table.
    A separable table (any square or rectangular QAM) runs per axis, the same bits from far fewer distances; force_table=True
    keeps the general form.  Stateless.  run() takes complex64 and returns float32 (n_frames, n_payload * bits_per_sym) or
    uint8 (n_frames, out_frame_bytes).  With weights= (float32 (n_frames, P), 1 <= P <= n_payload, "llr" only) symbol j of a
    frame is scaled by llr_scale * weights[frame, j mod P] and erased (+0.0) where that weight is not finite and positive:
    OfdmDemodNode.run(..., csi=True)'s channel state with P = its data carriers, or one 1 / (2 sigma^2) per frame with P = 1."""
    _prefix = "comms_demap"
    _formats = {"llr": _frame_call(_prefix, np.complex64, np.float32), "bits": _frame_call(_prefix, np.complex64, np.uint8)}
    _frame = property(lambda self: self._formats[self.format])

    def __init__(self, bits_per_sym, constellation, n_payload, force_table=False, device=0):
        super().__init__()
        self.bits_per_sym, self.n_payload = int(bits_per_sym), int(n_payload)
        self.format = "llr"
        cons = None if constellation is None else _as_c64(constellation).ravel()
        if cons is not None and 1 <= self.bits_per_sym <= 8 and cons.size != 1 << self.bits_per_sym:
            raise ValueError("the constellation holds 2**bits_per_sym points")
        check(lib().comms_demap_create(self.bits_per_sym, None if cons is None else _ptr(cons), self.n_payload,
                                       _lib.DEMAP_TABLE if force_table else 0, device, C.byref(self._h)))

    def set_output_format(self, fmt):
        """ "llr" (default) or "bits"; may change between calls."""
        if fmt not in ("llr", "bits"):
            raise ValueError("the output format is 'llr' or 'bits'")
        check(lib().comms_demap_set_output_format(self._h, _SYM_FORMATS[fmt]))
        self.format = fmt
        return self

    def set_llr_scale(self, scale):
        check(lib().comms_demap_set_llr_scale(self._h, float(scale)))
        return self

    def run(self, symbols, weights=None):
        if weights is None:
            return self._frame.run(self, symbols)
        # (comms_demap_run_weighted takes its weights in front of n_frames: not the shell's order of arguments)
        x = _as_c64(symbols)
        if x.size % self.n_payload:
            raise ValueError("the input must hold whole records of %d symbols" % self.n_payload)
        n_frames = x.size // self.n_payload
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.ndim != 2 or w.shape[0] != n_frames:
            raise ValueError("weights holds one record per frame: shape (n_frames, P)")
        out = np.zeros((n_frames, self.n_payload * self.bits_per_sym), np.float32)
        p_x, p_w, p_out = [_ptr(a) if n_frames else None for a in (x, w, out)]
        check(lib().comms_demap_run_weighted(self._h, p_x, p_w, w.shape[1], n_frames, p_out))
        return out

    def run_dev(self, sym_ptr, n_frames, out_ptr, stream=0, weight_ptr=None, weight_period=0):
        if weight_ptr is None:
            self._frame.run_dev(self, sym_ptr, n_frames, out_ptr, stream)
        else:
            check(lib().comms_demap_run_weighted_dev(self._h, sym_ptr, weight_ptr, int(weight_period), int(n_frames), out_ptr, stream))

    def kernel(self, n_frames):
        """ "demap_table_kernel<m,fmt> form=table ..." or "demap_axis_kernel<mI,mQ,fmt> form=axis ...", then "wg=.. bits=..
        payload=.. items=.. lanes=.. frames=.. grid=.. max_grid=.. lds=0"."""
        return self._kernel_name(int(n_frames))


# ------------------------------------------------------------------ OFDM modulator and demodulator
class _Ofdm(_FrameNode, _Handle):
    """One OFDM frame format of comms_ofdm_*: n_fft (64 ... 1024) bins, a cyclic prefix of n_cp samples, carrier_kind[n_fft]
    (0 null, 1 data, 2 pilot; bin 0 is DC), the base `pilots` in increasing bin order, `polarity` (floats that multiply the
    pilots of data symbol s by polarity[s mod len]; None = 1), n_train identical training symbols of frequency values
    train[n_fft] in front of the n_syms data symbols of every frame, cpe=True for the demodulator's pilot phase correction,
    tx_scale (None = 1 / sqrt(n_fft))."""
    _prefix = "comms_ofdm"
    _direction = None

    def __init__(self, n_fft, n_cp, carrier_kind, pilots=None, polarity=None, train=None, n_train=0, n_syms=1, cpe=False, tx_scale=None,
                 device=0):
        super().__init__()
        self.n_fft, self.n_cp, self.n_train, self.n_syms = int(n_fft), int(n_cp), int(n_train), int(n_syms)
        kind = np.ascontiguousarray(carrier_kind, dtype=np.uint8).ravel()
        if kind.size != max(self.n_fft, 0):
            raise ValueError("carrier_kind holds one entry per bin")
        pil = None if pilots is None else _as_c64(pilots).ravel()
        if (0 if pil is None else pil.size) != int(np.count_nonzero(kind == _lib.OFDM_PILOT)):
            raise ValueError("pilots holds one value per pilot carrier")
        pol = None if polarity is None else np.ascontiguousarray(polarity, dtype=np.float32).ravel()
        tr = None if train is None else _as_c64(train).ravel()
        if tr is not None and tr.size != kind.size:
            raise ValueError("train holds one value per bin")
        check(lib().comms_ofdm_create(self.n_fft, self.n_cp, _ptr(kind), None if pil is None or not pil.size else _ptr(pil),
                                      None if pol is None else _ptr(pol), 0 if pol is None else pol.size, None if tr is None else _ptr(tr),
                                      self.n_train, self.n_syms, _lib.OFDM_CPE if cpe else 0, device, C.byref(self._h)))
        if tx_scale is not None:
            self.set_scale(tx_scale)

    def set_scale(self, tx_scale):
        check(lib().comms_ofdm_set_scale(self._h, float(tx_scale)))
        return self

    _data_bytes, _sample_bytes = _record("comms_ofdm_data_syms", 8), _record("comms_ofdm_frame_samples", 8)

    @property
    def data_syms(self):
        """Data-carrier values per record: n_syms * (data carriers)."""
        return self._data_bytes() // 8

    @property
    def frame_samples(self):
        """(n_train + n_syms) * (n_fft + n_cp)."""
        return self._sample_bytes() // 8

    def kernel(self, n_frames):
        """ "ofdm_mod_kernel<N> | ofdm_demod_kernel<N> form=wave16 wg=.. n_fft=.. cp=.. data=.. pilots=.. train=.. syms=.. cpe=..
        lanes_per_sym=.. syms_per_wave=.. block=.. blocks=.. frames=.. items=.. grid=.. max_grid=.. lds=.." for a call on n_frames."""
        return self._kernel_name(self._direction, int(n_frames), cap=320)


class OfdmModNode(_Ofdm):
    """Records of data-carrier values -> frames of time samples, behind SymbolMapNode (no word, no gap): carrier map, pilots,
    training symbols, inverse transform scaled by tx_scale, cyclic prefix; all frames of a call in one launch.  Stateless.  run()
    takes complex64 (n_frames, data_syms), symbol-major, and returns complex64 (n_frames, frame_samples)."""
    _direction = _lib.OFDM_MOD
    _frame = _FrameCall("comms_ofdm_mod_run", np.complex64, np.complex64, _Ofdm._data_bytes, _Ofdm._sample_bytes)

    def run(self, symbols):
        return self._frame.run(self, symbols)


class OfdmDemodNode(_Ofdm):
    """Frames of received samples -> records of equalised data-carrier values, in front of DemapNode(n_payload = data_syms):
    prefix removal, transform, least-squares channel estimate from the n_train training symbols (without them: division by
    n_fft * tx_scale), one multiply per carrier, with cpe=True the pilots' common phase removed per symbol; all frames of a call
    in one launch.  Stateless.  run() takes complex64 (n_frames, frame_samples) and returns complex64 (n_frames, data_syms); with
    csi=True (n_train >= 1) it returns (records, csi), csi float32 (n_frames, data carriers): |H_k|^2 of every data carrier in bin
    order, the same launch with one store more -- DemapNode.run(records, weights=csi) weighs every carrier's LLRs by it."""
    _direction = _lib.OFDM_DEMOD
    _frame = _FrameCall("comms_ofdm_demod_run", np.complex64, np.complex64, _Ofdm._sample_bytes, _Ofdm._data_bytes)
    _frame_csi = _FrameCall("comms_ofdm_demod_csi_run", np.complex64, np.complex64, _Ofdm._sample_bytes, _Ofdm._data_bytes)

    @property
    def data_carriers(self):
        return self.data_syms // self.n_syms

    def run(self, samples, csi=False):
        if not csi:
            return self._frame.run(self, samples)
        # the side output is one record of data_carriers floats per frame: a sub-array dtype gives it that shape
        return self._frame_csi.run(self, samples, side=(np.dtype((np.float32, (self.data_carriers,))),))

    def run_dev(self, in_ptr, n_frames, out_ptr, stream=0, csi_ptr=None):
        if csi_ptr is None:
            self._frame.run_dev(self, in_ptr, n_frames, out_ptr, stream)
        else:
            self._frame_csi.run_dev(self, in_ptr, n_frames, out_ptr, csi_ptr, stream)


class OfdmSyncNode(_History, _Detector, _Handle):
    """OFDM stream synchroniser (comms_ofdmsync_*).  run() correlates the received sample stream with itself at `lag` over
    `window` samples, searches peaks of the normalised metric over +-`guard` positions above `threshold`, in one launch, and
    returns (detections, cfo): FrameDetection values whose `index` lies `advance` samples ahead of the peak, and the
    carrier-frequency offsets arg(corr) / lag in rad / sample (float64).  A call on n samples decides n positions; flush() ends a
    stream; the detections do not depend on how the stream is cut into calls.  The detections feed
    DeframeNode(n_frame, 0, lookback >= window + lag + guard + advance - 1) in "c32"; correct() then multiplies record f by
    exp(-i cfo[f] n), all records in one launch, in front of OfdmDemodNode.  `found` is the true count of the last call."""
    _prefix = "comms_ofdmsync"
    _state_args = ("lag", "window", "guard")
    _side = (np.float64,)

    def _record_bytes(self):
        return 8 * self.n_frame

    _correct = _FrameCall("comms_ofdmsync_correct_run", np.complex64, np.complex64, _record_bytes, _record_bytes)   # correct()

    def __init__(self, lag, window, threshold, guard, advance=0, n_frame=0, device=0):
        super().__init__()
        self.lag, self.window, self.guard, self.advance, self.n_frame = int(lag), int(window), int(guard), int(advance), int(n_frame)
        check(lib().comms_ofdmsync_create(self.lag, self.window, float(threshold), self.guard, self.advance, self.n_frame, device,
                                          C.byref(self._h)))

    @classmethod
    def for_format(cls, ofdm_node, threshold, guard, advance=0, device=0):
        """The node for OfdmModNode / OfdmDemodNode `ofdm_node`'s frames (n_train >= 2): lag = window = n_fft + n_cp and
        n_frame = frame_samples."""
        sym = ofdm_node.n_fft + ofdm_node.n_cp
        return cls(sym, sym, threshold, guard, advance=advance, n_frame=ofdm_node.frame_samples, device=device)

    @property
    def lookback(self):
        """The least `lookback` of the DeframeNode behind this node."""
        return self.window + self.lag + self.guard + self.advance - 1

    def run(self, samples, cap=None, raw=False):
        x = np.ascontiguousarray(samples, dtype=np.complex64)
        return self._detect(lib().comms_ofdmsync_run, x.size, cap, raw, _ptr(x), x.size)

    def run_dev(self, in_ptr, n, cap=None, stream=0, raw=False):
        return self._detect(lib().comms_ofdmsync_run_dev, n, cap, raw, in_ptr, n, tail=(stream,))

    def flush(self, cap=None, raw=False):
        """The positions still undecided, as if window + lag + guard zero samples followed; history zero afterwards, position kept."""
        return self._detect(lib().comms_ofdmsync_flush, self.window + self.lag + self.guard, cap, raw)

    def correct(self, records, cfo):
        """complex64 (n_frames, n_frame) records and one cfo per record -> the records times exp(-i cfo n)."""
        x = _as_c64(records)
        w = np.ascontiguousarray(cfo, dtype=np.float64).ravel()
        if w.size * self.n_frame != x.size:
            raise ValueError("records holds n_frame = %d samples, and cfo one value, per record" % self.n_frame)
        return self._correct.run(self, x, pre=(w,))

    def correct_dev(self, in_ptr, n_frames, cfo, out_ptr, stream=0):
        w = np.ascontiguousarray(cfo, dtype=np.float64).ravel()
        if w.size != int(n_frames):
            raise ValueError("cfo holds one value per record")
        self._correct.run_dev(self, in_ptr, n_frames, _ptr(w) if w.size else None, out_ptr, stream)

    state = _History.get_state   # the last n_state samples (default: all window + lag + 2 guard - 1), newest first

    def kernel(self, n):
        """What a call on n samples is run by: "ofdmsync_detect_kernel tile=.. wg=.. lag=.. window=.. guard=.. lds=.. tiles=.. grid=..".
        """
        return self._kernel_name(n)


def qfilt_taps(n_taps, alpha, sam_per_sym):
    """util/math.rs:307-342 (f64, real); even n_taps is incremented."""
    out = np.empty(lib().comms_qfilt_len(int(n_taps)), np.float64)
    check(lib().comms_qfilt_taps(int(n_taps), float(alpha), int(sam_per_sym), _ptr(out)))
    return out


class NcoNode(_Handle):
    """NcoNode::new(dphase, phase) (nco.rs:118-133) in block form: run() takes a vector of
    phase errors and returns exp(i*phase) per sample (Complex<f64>)."""
    _prefix = "comms_nco"

    def __init__(self, dphase, phase=None, device=0):
        super().__init__()
        check(lib().comms_nco_create(float(dphase), 0.0 if phase is None else float(phase), device,
                                     C.byref(self._h)))

    def run(self, perr):
        e = np.ascontiguousarray(perr, dtype=np.float64)
        out = np.empty(e.size, np.complex128)
        check(lib().comms_nco_run(self._h, _ptr(e), e.size, _ptr(out)))
        return out

    def run_dev(self, in_ptr, n, out_ptr, stream=0):
        check(lib().comms_nco_run_dev(self._h, in_ptr, n, out_ptr, stream))

    def kernel(self, n):
        """What a block of n phase errors is run by: "nco_sum_kernel+nco_scan_kernel+nco_apply_kernel tile=.. wg=.. tiles=..
        scan_sweeps=.. grid=.. max_grid=.."."""
        return self._kernel_name(n)

    @property
    def phase(self):
        return _get(C.c_double, lib().comms_nco_get_phase, self._h)


# ------------------------------------------------------------------ synthetic IQ
def synth_iq(n, first_index=0, seed=0xC0FFEE):
    out = np.empty(int(n), np.complex64)
    lib().comms_synth_iq_host(_ptr(out), out.size, first_index, seed)
    return out


def synth_iq_dev(out_ptr, n, first_index=0, seed=0xC0FFEE, device=0, stream=0):
    check(lib().comms_synth_iq_dev(out_ptr, n, first_index, seed, device, stream))


# ------------------------------------------------------------------ kernel timer
class KernelTimer:
    """comms_timer_*: hipEvent pairs recorded around a node's dominant kernel."""

    def __init__(self, n_pairs, device=0, stamps=False, stride=1):
        """stamps=False: hipEvent pairs (every `stride`-th launch of the attached node is bracketed);
        stamps=True: comms_timer_create_stamps -- the kernels stamp their own begin / end, no events, every launch an
        ordinary one (the kernel's duration in the stream); stamps="both": events every stride-th launch AND stamps
        on every launch (read_ms / read_stamps_ms)."""
        self._h = C.c_void_p()
        self.n = int(n_pairs)
        if stamps is True:
            check(lib().comms_timer_create_stamps(self.n, device, C.byref(self._h)))
        else:
            check(lib().comms_timer_create(self.n, device, C.byref(self._h)))
            if stamps == "both":
                check(lib().comms_timer_add_stamps(self._h, self.n))
            if stride != 1:
                check(lib().comms_timer_set_stride(self._h, int(stride)))

    def attach(self, node):
        name = node._prefix + "_set_timer"   # (a node without one: AttributeError)
        check(getattr(lib(), name)(node._h, self._h))
        self._node, self._setter = node, name
        return self

    def enable(self, on):
        """Detach from / re-attach to the node without touching what was recorded (to bracket only some launches)."""
        on = bool(on)
        if on != getattr(self, "_on", True):
            check(getattr(lib(), self._setter)(self._node._h, self._h if on else None))
            self._on = on

    def reset(self):
        check(lib().comms_timer_reset(self._h))

    def read_ms(self):
        out = np.zeros(self.n, np.float32)
        return out[: _get(C.c_size_t, lib().comms_timer_read, self._h, _ptr(out), self.n)].copy()

    def read_stamps_ms(self):
        """In-stream kernel durations of the stamped launches (0.0 where the launched kernel does not stamp)."""
        out = np.zeros(self.n, np.float32)
        return out[: _get(C.c_size_t, lib().comms_timer_read_stamps, self._h, _ptr(out), self.n)].copy()

    def close(self):
        if self._h:
            node = getattr(self, "_node", None)
            if node is not None and node._h:
                getattr(lib(), self._setter)(node._h, None)
            lib().comms_timer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
