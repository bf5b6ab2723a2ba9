//! comms-rs nodes whose `run()` executes on an MI355X through libcomms_hip.so.
//!
//! UNTESTED SOURCE (no Rust toolchain where this was written).  Each struct keeps the reference
//! node's name, TYPE PARAMETER, constructor signature and public `input` / `output` fields, and
//! derives `Node` with the reference's own `node_derive` macro, so `connect_nodes!` /
//! `start_nodes!` / `Graph` work unchanged and a graph switches by its `use` lines alone:
//!
//! ```ignore
//! use comms_rs::prelude::*;
//! // instead of comms_rs::filter::fir_node::BatchFirNode, comms_rs::util::resample_node::DecimateNode, ...
//! use comms_rs_hip::{BatchFirNode, DecimateNode, FMDemodNode};
//! // examples/fm_radio.rs:146-152, unchanged:
//! let mut dec1: DecimateNode<Complex<f32>> = DecimateNode::new(5);
//! let mut filt1: BatchFirNode<f32> = BatchFirNode::new(taps.clone(), None);
//! let mut fm = FMDemodNode::new();
//! let mut dec2: DecimateNode<f32> = DecimateNode::new(5);
//! connect_nodes!(filt1, output, dec1, input);
//! ```
//!
//! The reference's nodes are generic over any `T: Num + Copy + Send`; the kernels exist for the
//! sample types below (sealed traits -- another `T` is a compile error here, not a run-time one):
//!
//! | node | reference | `T` here |
//! |---|---|---|
//! | `FirNode<T>`, `BatchFirNode<T>`, `PulseNode<T>` | fir_node.rs:45,148; pulse.rs:38 | `f32`, `f64`, `i16` (`FirSample`) |
//! | `MixerNode<T>` | mixer.rs:93 | `f32`, `f64` (`MixerSample`) |
//! | `FFTBatchNode<T>`, `FFTSampleNode<T>`, `FMDemodNode<T>` | fft_node.rs:28,104; analog_node.rs:20 | `f32`, `f64` (`FloatSample`) |
//! | `DecimateNode<T>`, `UpsampleNode<T>` | resample_node.rs:10,74 | any `Copy + Send` type of 1, 2, 4, 8 or 16 bytes |
//! | `UniformNode<T>`, `random_bit()`, `NormalNode` | rand_node.rs:26,98,150 | `f32`, and `u8` over `[0, 2)` (`UniformSample`); plus `with_seed` |
pub mod ffi;

use comms_rs::prelude::*;
use ffi::*;
use num::{Complex, Num, Zero};
use std::marker::PhantomData;
use std::mem::size_of;
use std::os::raw::c_void;
use std::ptr;

fn to_err(st: comms_status_t) -> NodeError {
    // COMMS_ERR_ARG -> DataError, COMMS_ERR_DEVICE -> PermanentError (include/comms_hip.h)
    if st == COMMS_ERR_ARG { NodeError::DataError } else { NodeError::PermanentError }
}

mod sealed {
    pub trait Sealed {}
    impl Sealed for f32 {}
    impl Sealed for f64 {}
    impl Sealed for i16 {}
}

/// Sample types the FIR and pulse-shaping kernels are built for: `f32` (every BASELINE config), `f64` (the type of the
/// reference's batch_fir doc example and timing estimator; bit-identical outputs) and `i16` (the type of the reference's own
/// FIR / pulse goldens; wrapping arithmetic as in a release build).
pub trait FirSample: sealed::Sealed + Num + Copy + Send + 'static {
    #[doc(hidden)] type Fir;
    #[doc(hidden)] type Pulse;
    #[doc(hidden)] unsafe fn fir_create(taps: *const Complex<Self>, n_taps: usize, state: *const Complex<Self>, n_state: usize,
                                        out: *mut *mut Self::Fir) -> comms_status_t;
    #[doc(hidden)] unsafe fn fir_run(h: *mut Self::Fir, x: *const Complex<Self>, n: usize, y: *mut Complex<Self>) -> comms_status_t;
    #[doc(hidden)] unsafe fn fir_destroy(h: *mut Self::Fir);
    #[doc(hidden)] unsafe fn pulse_create(taps: *const Complex<Self>, n_taps: usize, sps: usize, out: *mut *mut Self::Pulse) -> comms_status_t;
    #[doc(hidden)] unsafe fn pulse_run(h: *mut Self::Pulse, sym: *const Complex<Self>, n: usize, y: *mut Complex<Self>) -> comms_status_t;
    #[doc(hidden)] unsafe fn pulse_destroy(h: *mut Self::Pulse);
}
impl FirSample for f32 {
    type Fir = comms_fir_t;
    type Pulse = comms_pulse_t;
    unsafe fn fir_create(t: *const Complex<f32>, n: usize, s: *const Complex<f32>, ns: usize, out: *mut *mut comms_fir_t) -> comms_status_t {
        comms_fir_create(t, n, s, ns, 0, out)
    }
    unsafe fn fir_run(h: *mut comms_fir_t, x: *const Complex<f32>, n: usize, y: *mut Complex<f32>) -> comms_status_t { comms_fir_run(h, x, n, y) }
    unsafe fn fir_destroy(h: *mut comms_fir_t) { comms_fir_destroy(h); }
    unsafe fn pulse_create(t: *const Complex<f32>, n: usize, sps: usize, out: *mut *mut comms_pulse_t) -> comms_status_t {
        comms_pulse_create(t, n, sps, 0, out)
    }
    unsafe fn pulse_run(h: *mut comms_pulse_t, s: *const Complex<f32>, n: usize, y: *mut Complex<f32>) -> comms_status_t { comms_pulse_run(h, s, n, y) }
    unsafe fn pulse_destroy(h: *mut comms_pulse_t) { comms_pulse_destroy(h); }
}
impl FirSample for i16 {
    type Fir = comms_fir_i16_t;
    type Pulse = comms_pulse_i16_t;
    unsafe fn fir_create(t: *const Complex<i16>, n: usize, s: *const Complex<i16>, ns: usize, out: *mut *mut comms_fir_i16_t) -> comms_status_t {
        comms_fir_i16_create(t, n, s, ns, 0, out)
    }
    unsafe fn fir_run(h: *mut comms_fir_i16_t, x: *const Complex<i16>, n: usize, y: *mut Complex<i16>) -> comms_status_t { comms_fir_i16_run(h, x, n, y) }
    unsafe fn fir_destroy(h: *mut comms_fir_i16_t) { comms_fir_i16_destroy(h); }
    unsafe fn pulse_create(t: *const Complex<i16>, n: usize, sps: usize, out: *mut *mut comms_pulse_i16_t) -> comms_status_t {
        comms_pulse_i16_create(t, n, sps, 0, out)
    }
    unsafe fn pulse_run(h: *mut comms_pulse_i16_t, s: *const Complex<i16>, n: usize, y: *mut Complex<i16>) -> comms_status_t { comms_pulse_i16_run(h, s, n, y) }
    unsafe fn pulse_destroy(h: *mut comms_pulse_i16_t) { comms_pulse_i16_destroy(h); }
}

impl FirSample for f64 {  // round 5: the reference's arithmetic operation for operation, bit-identical outputs (comms_fir_f64_*)
    type Fir = comms_fir_f64_t;
    type Pulse = comms_pulse_f64_t;
    unsafe fn fir_create(t: *const Complex<f64>, n: usize, s: *const Complex<f64>, ns: usize, out: *mut *mut comms_fir_f64_t) -> comms_status_t {
        comms_fir_f64_create(t, n, s, ns, 0, out)
    }
    unsafe fn fir_run(h: *mut comms_fir_f64_t, x: *const Complex<f64>, n: usize, y: *mut Complex<f64>) -> comms_status_t { comms_fir_f64_run(h, x, n, y) }
    unsafe fn fir_destroy(h: *mut comms_fir_f64_t) { comms_fir_f64_destroy(h); }
    unsafe fn pulse_create(t: *const Complex<f64>, n: usize, sps: usize, out: *mut *mut comms_pulse_f64_t) -> comms_status_t {
        comms_pulse_f64_create(t, n, sps, 0, out)
    }
    unsafe fn pulse_run(h: *mut comms_pulse_f64_t, s: *const Complex<f64>, n: usize, y: *mut Complex<f64>) -> comms_status_t { comms_pulse_f64_run(h, s, n, y) }
    unsafe fn pulse_destroy(h: *mut comms_pulse_f64_t) { comms_pulse_f64_destroy(h); }
}

/// Sample types of `MixerNode<T>`: `f32`, and `f64` -- the instantiation the reference's own mixer tests use
/// (mixer.rs:160-336), met at their 1e-6.
pub trait MixerSample: sealed::Sealed + Num + Copy + Send + 'static {
    #[doc(hidden)] unsafe fn mix(h: *mut comms_mixer_t, x: *const Complex<Self>, n: usize, y: *mut Complex<Self>) -> comms_status_t;
}
impl MixerSample for f32 {
    unsafe fn mix(h: *mut comms_mixer_t, x: *const Complex<f32>, n: usize, y: *mut Complex<f32>) -> comms_status_t { comms_mixer_run(h, x, n, y) }
}
impl MixerSample for f64 {
    unsafe fn mix(h: *mut comms_mixer_t, x: *const Complex<f64>, n: usize, y: *mut Complex<f64>) -> comms_status_t { comms_mixer_run_f64(h, x, n, y) }
}

/// Sample types of the FFT and FM-demodulation nodes: `f32` (the reference casts to f64 inside and back, fft/mod.rs:78-94; the
/// kernels compute in f32 within the north star's 1e-5) and `f64` (the instantiation of the reference's doc examples,
/// fft_node.rs:24,99: plain FP64 kernels, comms_fft_f64_* / comms_fmdemod_f64_*).
pub trait FloatSample: sealed::Sealed + Num + Copy + Send + Default + 'static {
    #[doc(hidden)] type Fft;
    #[doc(hidden)] type Fm;
    #[doc(hidden)] unsafe fn fft_create(fft_size: usize, ifft: i32, out: *mut *mut Self::Fft) -> comms_status_t;
    #[doc(hidden)] unsafe fn fft(h: *mut Self::Fft, x: *const Complex<Self>, n: usize, y: *mut Complex<Self>) -> comms_status_t;
    #[doc(hidden)] unsafe fn fft_destroy(h: *mut Self::Fft);
    #[doc(hidden)] unsafe fn fm_create(out: *mut *mut Self::Fm) -> comms_status_t;
    #[doc(hidden)] unsafe fn fm(h: *mut Self::Fm, x: *const Complex<Self>, n: usize, y: *mut Self) -> comms_status_t;
    #[doc(hidden)] unsafe fn fm_destroy(h: *mut Self::Fm);
}
impl FloatSample for f32 {
    type Fft = comms_fft_t;
    type Fm = comms_fmdemod_t;
    unsafe fn fft_create(fft_size: usize, ifft: i32, out: *mut *mut comms_fft_t) -> comms_status_t { comms_fft_create(fft_size, ifft, 0, out) }
    unsafe fn fft(h: *mut comms_fft_t, x: *const Complex<f32>, n: usize, y: *mut Complex<f32>) -> comms_status_t { comms_fft_run(h, x, n, y) }
    unsafe fn fft_destroy(h: *mut comms_fft_t) { comms_fft_destroy(h); }
    unsafe fn fm_create(out: *mut *mut comms_fmdemod_t) -> comms_status_t { comms_fmdemod_create(0, out) }
    unsafe fn fm(h: *mut comms_fmdemod_t, x: *const Complex<f32>, n: usize, y: *mut f32) -> comms_status_t { comms_fmdemod_run(h, x, n, y) }
    unsafe fn fm_destroy(h: *mut comms_fmdemod_t) { comms_fmdemod_destroy(h); }
}
impl FloatSample for f64 {
    type Fft = comms_fft_f64_t;
    type Fm = comms_fmdemod_f64_t;
    unsafe fn fft_create(fft_size: usize, ifft: i32, out: *mut *mut comms_fft_f64_t) -> comms_status_t { comms_fft_f64_create(fft_size, ifft, 0, out) }
    unsafe fn fft(h: *mut comms_fft_f64_t, x: *const Complex<f64>, n: usize, y: *mut Complex<f64>) -> comms_status_t { comms_fft_f64_run(h, x, n, y) }
    unsafe fn fft_destroy(h: *mut comms_fft_f64_t) { comms_fft_f64_destroy(h); }
    unsafe fn fm_create(out: *mut *mut comms_fmdemod_f64_t) -> comms_status_t { comms_fmdemod_f64_create(0, out) }
    unsafe fn fm(h: *mut comms_fmdemod_f64_t, x: *const Complex<f64>, n: usize, y: *mut f64) -> comms_status_t { comms_fmdemod_f64_run(h, x, n, y) }
    unsafe fn fm_destroy(h: *mut comms_fmdemod_f64_t) { comms_fmdemod_f64_destroy(h); }
}

fn czeros<T: Num + Copy>(n: usize) -> Vec<Complex<T>> { vec![Complex::new(T::zero(), T::zero()); n] }

/// `impl Node` for a per-sample node whose `run` costs a device launch: instead of the derive macro's
/// one-message `call` (node_derive/src/lib.rs:200-211) the node drains what is ALREADY queued behind
/// the first message (`recv`, then `try_recv` -- it never waits for more), runs the block in one launch
/// (`run_block`) and sends the outputs one by one in order.  Every receiver sees exactly the message
/// sequence the derived loop would produce; the C++ host runtime does the same (`DeriveNode::call`,
/// comms_rs_amd/host/comms/node.hpp) and is where this behaviour is tested: 16.5 Msamples/s through
/// MixerNode -> FirNode against ~40 ksamples/s with a launch per sample.
macro_rules! drained_node {
    ($name:ident, $bound:ident) => {
        impl<T: $bound> Node for $name<T> {
            fn start(&mut self) {
                for (send, val) in &self.output {
                    if let Some(v) = val { send.send(v.clone()).unwrap(); }
                }
                loop { if self.call().is_err() { break; } }
            }
            fn call(&mut self) -> Result<(), NodeError> {
                let block: Vec<Complex<T>> = match self.input {
                    Some(ref r) => {
                        let mut b = vec![r.recv().or(Err(NodeError::DataEnd))?];
                        while b.len() < (1 << 16) {
                            match r.try_recv() { Ok(v) => b.push(v), Err(_) => break }
                        }
                        b
                    }
                    None => return Err(NodeError::PermanentError),
                };
                let outs: Vec<Complex<T>> = self.run_block(&block)?;
                for res in outs {
                    for (send, _) in &self.output {
                        if send.send(res.clone()).is_err() { return Err(NodeError::CommError); }
                    }
                }
                Ok(())
            }
            fn is_connected(&self) -> bool { self.input.is_some() && !self.output.is_empty() }
        }
    };
}

/// fir_node.rs:148-221
#[derive(Node)]
#[pass_by_ref]
pub struct BatchFirNode<T>
where
    T: FirSample,
{
    pub input: NodeReceiver<Vec<Complex<T>>>,
    h: *mut T::Fir,
    pub output: NodeSender<Vec<Complex<T>>>,
}
// a handle is used by one thread at a time but not its creator: Send, never Sync
unsafe impl<T: FirSample> Send for BatchFirNode<T> {}
impl<T: FirSample> Drop for BatchFirNode<T> {
    fn drop(&mut self) { unsafe { T::fir_destroy(self.h) } }
}
impl<T> BatchFirNode<T>
where
    T: FirSample,
{
    pub fn new(taps: Vec<Complex<T>>, state: Option<Vec<Complex<T>>>) -> Self {
        let mut h = ptr::null_mut();
        let (sp, sn) = match &state { Some(s) => (s.as_ptr(), s.len()), None => (ptr::null(), 0) };
        let st = unsafe { T::fir_create(taps.as_ptr(), taps.len(), sp, sn, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_fir_create failed");   // the reference panics on a bad state too
        BatchFirNode { input: Default::default(), h, output: Default::default() }
    }
    pub fn run(&mut self, input: &[Complex<T>]) -> Result<Vec<Complex<T>>, NodeError> {
        let mut out = czeros::<T>(input.len());
        let st = unsafe { T::fir_run(self.h, input.as_ptr(), input.len(), out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// fir_node.rs:45-114 (one sample per message; queued samples run as one launch, see `drained_node!`)
pub struct FirNode<T>
where
    T: FirSample,
{
    pub input: NodeReceiver<Complex<T>>,
    h: *mut T::Fir,
    pub output: NodeSender<Complex<T>>,
}
unsafe impl<T: FirSample> Send for FirNode<T> {}
impl<T: FirSample> Drop for FirNode<T> {
    fn drop(&mut self) { unsafe { T::fir_destroy(self.h) } }
}
impl<T> FirNode<T>
where
    T: FirSample,
{
    pub fn new(taps: Vec<Complex<T>>, state: Option<Vec<Complex<T>>>) -> Self {
        let mut h = ptr::null_mut();
        let (sp, sn) = match &state { Some(s) => (s.as_ptr(), s.len()), None => (ptr::null(), 0) };
        let st = unsafe { T::fir_create(taps.as_ptr(), taps.len(), sp, sn, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_fir_create failed");
        FirNode { input: Default::default(), h, output: Default::default() }
    }
    pub fn run(&mut self, input: &Complex<T>) -> Result<Complex<T>, NodeError> {
        let mut out = Complex::new(T::zero(), T::zero());
        let st = unsafe { T::fir_run(self.h, input, 1, &mut out) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    pub fn run_block(&mut self, input: &[Complex<T>]) -> Result<Vec<Complex<T>>, NodeError> {
        let mut out = czeros::<T>(input.len());
        let st = unsafe { T::fir_run(self.h, input.as_ptr(), input.len(), out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}
drained_node!(FirNode, FirSample);

/// mixer.rs:93-148 -- argument order (dphase, phase) as in MixerNode::new (drained, see `drained_node!`)
pub struct MixerNode<T>
where
    T: MixerSample,
{
    pub input: NodeReceiver<Complex<T>>,
    h: *mut comms_mixer_t,
    pub output: NodeSender<Complex<T>>,
}
unsafe impl<T: MixerSample> Send for MixerNode<T> {}
impl<T: MixerSample> Drop for MixerNode<T> {
    fn drop(&mut self) { unsafe { comms_mixer_destroy(self.h); } }
}
impl<T> MixerNode<T>
where
    T: MixerSample,
{
    pub fn new(dphase: f64, phase: Option<f64>) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_mixer_create(dphase, phase.unwrap_or(0.0), 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_mixer_create failed");
        MixerNode { input: Default::default(), h, output: Default::default() }
    }
    pub fn run(&mut self, input: &Complex<T>) -> Result<Complex<T>, NodeError> {
        let mut out = Complex::new(T::zero(), T::zero());
        let st = unsafe { T::mix(self.h, input, 1, &mut out) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    pub fn run_block(&mut self, input: &[Complex<T>]) -> Result<Vec<Complex<T>>, NodeError> {
        let mut out = czeros::<T>(input.len());
        let st = unsafe { T::mix(self.h, input.as_ptr(), input.len(), out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// oscillator phase of the next sample: checkpoint hook / start phase of a stream shard
    pub fn phase(&self) -> f64 {
        let mut p = 0.0;
        let st = unsafe { comms_mixer_get_phase(self.h, &mut p) };
        assert_eq!(st, COMMS_OK, "comms_mixer_get_phase failed");
        p
    }
    pub fn set_phase(&mut self, phase: f64) {
        let st = unsafe { comms_mixer_set_phase(self.h, phase) };
        assert_eq!(st, COMMS_OK, "comms_mixer_set_phase failed");
    }
}
drained_node!(MixerNode, MixerSample);

/// pulse.rs:38-93
#[derive(Node)]
#[pass_by_ref]
pub struct PulseNode<T>
where
    T: FirSample,
{
    pub input: NodeReceiver<Complex<T>>,
    h: *mut T::Pulse,
    sam_per_sym: usize,
    pub output: NodeSender<Vec<Complex<T>>>,
}
unsafe impl<T: FirSample> Send for PulseNode<T> {}
impl<T: FirSample> Drop for PulseNode<T> {
    fn drop(&mut self) { unsafe { T::pulse_destroy(self.h) } }
}
impl<T> PulseNode<T>
where
    T: FirSample,
{
    pub fn new(taps: Vec<Complex<T>>, sam_per_sym: usize) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { T::pulse_create(taps.as_ptr(), taps.len(), sam_per_sym, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_pulse_create failed");
        PulseNode { input: Default::default(), h, sam_per_sym, output: Default::default() }
    }
    pub fn run(&mut self, input: &Complex<T>) -> Result<Vec<Complex<T>>, NodeError> {
        let mut out = czeros::<T>(self.sam_per_sym);
        let st = unsafe { T::pulse_run(self.h, input, 1, out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}
impl PulseNode<f32> {
    /// Transmit chain in one launch: fuses the `MixerNode::new(dphase, phase)` that follows (an addition; f32 only).
    pub fn with_mixer(self, dphase: f64, phase: Option<f64>) -> Self {
        let st = unsafe { comms_pulse_set_mixer(self.h, dphase, phase.unwrap_or(0.0)) };
        assert_eq!(st, COMMS_OK, "comms_pulse_set_mixer failed");
        self
    }
}

/// decimate / upsample of any element type by its size (include/comms_hip.h: elem = 1, 2, 4, 8 or 16 bytes)
fn resample<T: Copy>(up: bool, signal: &[T], rate: usize) -> Result<Vec<T>, NodeError> {
    let mut n_out = 0usize;
    let st = unsafe {
        if up { comms_upsample_out_len(signal.len(), rate, &mut n_out) } else { comms_decimate_out_len(signal.len(), rate, &mut n_out) }
    };
    if st != COMMS_OK { return Err(to_err(st)); }
    let mut out: Vec<T> = Vec::with_capacity(n_out);
    let (src, dst) = (signal.as_ptr() as *const c_void, out.as_mut_ptr() as *mut c_void);
    let st = unsafe {
        if up { comms_upsample_run(src, signal.len(), size_of::<T>(), rate, dst, &mut n_out, 0) }
        else { comms_decimate_run(src, signal.len(), size_of::<T>(), rate, dst, &mut n_out, 0) }
    };
    if st != COMMS_OK { return Err(to_err(st)); }
    unsafe { out.set_len(n_out) };   // every element was written by the library
    Ok(out)
}

/// resample_node.rs:10-66.  Any `T: Copy + Send` of 1, 2, 4, 8 or 16 bytes (`f32`, `Complex<f32>`, `Complex<f64>`,
/// `i16`, `u8` ...: the kernel copies elements by size, bit for bit); another size is `NodeError::DataError`.
#[derive(Node)]
#[pass_by_ref]
pub struct DecimateNode<T>
where
    T: Copy + Send,
{
    pub input: NodeReceiver<Vec<T>>,
    dec_rate: usize,
    pub output: NodeSender<Vec<T>>,
}
impl<T> DecimateNode<T>
where
    T: Copy + Send,
{
    pub fn new(dec_rate: usize) -> Self {
        DecimateNode { dec_rate, input: Default::default(), output: Default::default() }
    }
    pub fn run(&mut self, signal: &[T]) -> Result<Vec<T>, NodeError> {
        resample(false, signal, self.dec_rate)
    }
    /// resample_node.rs:53-65 (the reference exposes the function itself too, on `&self`)
    pub fn decimate(&self, data: &[T]) -> Vec<T> {
        resample(false, data, self.dec_rate).expect("comms_decimate_run failed")
    }
}

/// resample_node.rs:74-132.  `T::zero()` must be the all-zero bit pattern (true of every primitive number and of
/// `Complex` of them): the kernel fills the gaps with zero bytes.
#[derive(Node)]
#[pass_by_ref]
pub struct UpsampleNode<T>
where
    T: Copy + Send + Zero,
{
    pub input: NodeReceiver<Vec<T>>,
    ups_rate: usize,
    pub output: NodeSender<Vec<T>>,
}
impl<T> UpsampleNode<T>
where
    T: Copy + Send + Zero,
{
    pub fn new(ups_rate: usize) -> Self {
        UpsampleNode { input: Default::default(), ups_rate, output: Default::default() }
    }
    pub fn run(&mut self, signal: &[T]) -> Result<Vec<T>, NodeError> {
        resample(true, signal, self.ups_rate)
    }
    /// resample_node.rs:120-131
    pub fn upsample(&self, data: &[T]) -> Vec<T> {
        resample(true, data, self.ups_rate).expect("comms_upsample_run failed")
    }
}

/// analog_node.rs:20-52
#[derive(Node)]
#[pass_by_ref]
pub struct FMDemodNode<T>
where
    T: FloatSample,
{
    pub input: NodeReceiver<Vec<Complex<T>>>,
    h: *mut T::Fm,
    pub output: NodeSender<Vec<T>>,
}
unsafe impl<T: FloatSample> Send for FMDemodNode<T> {}
impl<T: FloatSample> Drop for FMDemodNode<T> {
    fn drop(&mut self) { unsafe { T::fm_destroy(self.h); } }
}
impl<T> FMDemodNode<T>
where
    T: FloatSample,
{
    pub fn new() -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { T::fm_create(&mut h) };
        assert_eq!(st, COMMS_OK, "comms_fmdemod_create failed");
        FMDemodNode { input: Default::default(), h, output: Default::default() }
    }
    pub fn run(&mut self, samples: &[Complex<T>]) -> Result<Vec<T>, NodeError> {
        let mut out = vec![T::zero(); samples.len()];
        let st = unsafe { T::fm(self.h, samples.as_ptr(), samples.len(), out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}
impl<T: FloatSample> Default for FMDemodNode<T> {
    fn default() -> Self { Self::new() }   // the reference derives Default (analog_node.rs:18)
}

/// Real FIR with decimation over an `f32` stream (an additional node): what examples/fm_radio.rs:98-164 wires as
/// `Convert2Node -> BatchFirNode<f32> -> Convert3Node -> DecimateNode<f32>`, for real taps, as one node.  `state`
/// as `BatchFirNode::new` takes it (newest first; `zip` truncation); any batch length, `ceil(n / rate)` outputs.
#[derive(Node)]
#[pass_by_ref]
pub struct RealFirDecimNode {
    pub input: NodeReceiver<Vec<f32>>,
    h: *mut comms_rfir_t,
    rate: usize,
    pub output: NodeSender<Vec<f32>>,
}
unsafe impl Send for RealFirDecimNode {}
impl Drop for RealFirDecimNode {
    fn drop(&mut self) { unsafe { comms_rfir_destroy(self.h); } }
}
impl RealFirDecimNode {
    pub fn new(taps: Vec<f32>, rate: usize, state: Option<Vec<f32>>) -> Self {
        let mut h = ptr::null_mut();
        let (sp, sn) = match &state {
            Some(s) => (s.as_ptr(), s.len()),
            None => (ptr::null(), 0),
        };
        let st = unsafe { comms_rfir_create(taps.as_ptr(), taps.len(), sp, sn, rate, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_rfir_create failed");
        RealFirDecimNode { input: Default::default(), h, rate, output: Default::default() }
    }
    pub fn run(&mut self, samples: &[f32]) -> Result<Vec<f32>, NodeError> {
        let mut m = 0usize;
        unsafe { comms_rfir_out_len(samples.len(), self.rate, &mut m); }
        let mut out = vec![0f32; m];
        let st = unsafe { comms_rfir_run(self.h, samples.as_ptr(), samples.len(), out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// The checkpoint hook: the last `n` input samples, newest first
    pub fn state(&mut self, n: usize) -> Result<Vec<f32>, NodeError> {
        let mut out = vec![0f32; n];
        let st = unsafe { comms_rfir_get_state(self.h, out.as_mut_ptr(), n) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// Sample types of the rational resampler: `f32` and `Complex<f32>`.
pub trait ResampleSample: Copy + Send + Zero + 'static {
    #[doc(hidden)] const ELEM: i32;
}
impl ResampleSample for f32 { const ELEM: i32 = COMMS_RESAMPLE_F32; }
impl ResampleSample for Complex<f32> { const ELEM: i32 = COMMS_RESAMPLE_C32; }

/// Rational resampler by `up / down` (an additional node): what the reference wires as
/// `UpsampleNode(up) -> BatchFirNode(Complex(taps, 0)) -> DecimateNode(down)`, for real taps, as one node that forms
/// only the products with input samples.  Any batch length, `ceil(n * up / down)` outputs per call; the state is
/// `(taps.len() - 1) / up` input samples.
#[derive(Node)]
#[pass_by_ref]
pub struct ResampleNode<T>
where
    T: ResampleSample,
{
    pub input: NodeReceiver<Vec<T>>,
    h: *mut comms_resample_t,
    up: usize,
    down: usize,
    pub output: NodeSender<Vec<T>>,
}
unsafe impl<T: ResampleSample> Send for ResampleNode<T> {}
impl<T: ResampleSample> Drop for ResampleNode<T> {
    fn drop(&mut self) { unsafe { comms_resample_destroy(self.h); } }
}
impl<T> ResampleNode<T>
where
    T: ResampleSample,
{
    pub fn new(taps: Vec<f32>, up: usize, down: usize) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_resample_create(taps.as_ptr(), taps.len(), up, down, T::ELEM, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_resample_create failed");
        ResampleNode { input: Default::default(), h, up, down, output: Default::default() }
    }
    pub fn run(&mut self, samples: &[T]) -> Result<Vec<T>, NodeError> {
        let mut m = 0usize;
        let st = unsafe { comms_resample_out_len(samples.len(), self.up, self.down, &mut m) };
        if st != COMMS_OK { return Err(to_err(st)); }
        let mut out = vec![T::zero(); m];
        let st = unsafe { comms_resample_run(self.h, samples.as_ptr() as *const c_void, samples.len(), out.as_mut_ptr() as *mut c_void) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// The checkpoint hook: the last `n` input samples, newest first
    pub fn state(&mut self, n: usize) -> Result<Vec<T>, NodeError> {
        let mut out = vec![T::zero(); n];
        let st = unsafe { comms_resample_get_state(self.h, out.as_mut_ptr() as *mut c_void, n) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// Checkpoint restore / the halo in front of a stream shard: exactly `(taps.len() - 1) / up` samples, newest first
    pub fn set_state(&mut self, state: &[T]) -> Result<(), NodeError> {
        let st = unsafe { comms_resample_set_state(self.h, state.as_ptr() as *const c_void, state.len()) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
}

/// Polyphase channelizer (an additional node): what the reference wires as `channels` chains
/// `MixerNode::new(0, -2 pi k / M) -> BatchFirNode(Complex(taps, 0)) -> DecimateNode(down)` on one source, as one node
/// that reads every sample once.  Any batch length, `ceil(n / down)` frames per call; the output carries a call's
/// `frames * channels` samples channel-major (`out[k * frames + j]`) unless built with `new_frame_major`.
#[derive(Node)]
#[pass_by_ref]
pub struct ChannelizerNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_channelizer_t,
    channels: usize,
    down: usize,
    pub output: NodeSender<Vec<Complex<f32>>>,
}
unsafe impl Send for ChannelizerNode {}
impl Drop for ChannelizerNode {
    fn drop(&mut self) { unsafe { comms_channelizer_destroy(self.h); } }
}
impl ChannelizerNode {
    fn with_layout(taps: Vec<f32>, channels: usize, down: usize, layout: i32) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_channelizer_create(taps.as_ptr(), taps.len(), channels, down, layout, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_channelizer_create failed");
        ChannelizerNode { input: Default::default(), h, channels, down, output: Default::default() }
    }
    pub fn new(taps: Vec<f32>, channels: usize, down: usize) -> Self {
        Self::with_layout(taps, channels, down, COMMS_CHANNELIZER_CHANNEL_MAJOR)
    }
    pub fn new_frame_major(taps: Vec<f32>, channels: usize, down: usize) -> Self {
        Self::with_layout(taps, channels, down, COMMS_CHANNELIZER_FRAME_MAJOR)
    }
    pub fn run(&mut self, samples: &[Complex<f32>]) -> Result<Vec<Complex<f32>>, NodeError> {
        let mut frames = 0usize;
        let st = unsafe { comms_channelizer_out_len(samples.len(), self.down, &mut frames) };
        if st != COMMS_OK { return Err(to_err(st)); }
        let mut out = vec![Complex::<f32>::zero(); frames * self.channels];
        let st = unsafe { comms_channelizer_run(self.h, samples.as_ptr(), samples.len(), out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// The checkpoint hooks: the last `n` input samples, newest first, and the stream index mod `channels`
    pub fn state(&mut self, n: usize) -> Result<Vec<Complex<f32>>, NodeError> {
        let mut out = vec![Complex::<f32>::zero(); n];
        let st = unsafe { comms_channelizer_get_state(self.h, out.as_mut_ptr(), n) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// Exactly `taps.len() - 1` samples, newest first
    pub fn set_state(&mut self, state: &[Complex<f32>]) -> Result<(), NodeError> {
        let st = unsafe { comms_channelizer_set_state(self.h, state.as_ptr(), state.len()) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    pub fn phase(&mut self) -> Result<u64, NodeError> {
        let mut t = 0u64;
        let st = unsafe { comms_channelizer_get_phase(self.h, &mut t) };
        if st == COMMS_OK { Ok(t) } else { Err(to_err(st)) }
    }
    /// Any stream index `t`; the node reduces it mod `channels`
    pub fn set_phase(&mut self, t: u64) -> Result<(), NodeError> {
        let st = unsafe { comms_channelizer_set_phase(self.h, t) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
}

/// Symbol synchroniser (an additional node): what the reference could only wire as `UpsampleNode(phases) ->
/// BatchFirNode(Complex(taps, 0)) -> [skip mu] -> DecimateNode(phases * sps) -> MixerNode`, as one node that computes only
/// the kept outputs.  Batches are multiples of `sps` samples and give `n / sps` symbols; the state is
/// `(taps.len() - 1) / phases` raw input samples, whatever the timing.  `set_timing` / `set_rotation` are the block-rate
/// loop's inputs (TimingEstimatorNode, a phase estimator); see include/comms_hip.h for what to feed them.  Packed bits out:
/// `SymbolSyncBitsNode`.  As the shim's other nodes it exposes no kernel name or timer hook (diagnostics stay in C / Python).
#[derive(Node)]
#[pass_by_ref]
pub struct SymbolSyncNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_symsync_t,
    sps: usize,
    pub output: NodeSender<Vec<Complex<f32>>>,
}
unsafe impl Send for SymbolSyncNode {}
impl Drop for SymbolSyncNode {
    fn drop(&mut self) { unsafe { comms_symsync_destroy(self.h); } }
}
impl SymbolSyncNode {
    pub fn new(taps: Vec<f32>, phases: usize, sps: usize) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_symsync_create(taps.as_ptr(), taps.len(), phases, sps, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_symsync_create failed");
        SymbolSyncNode { input: Default::default(), h, sps, output: Default::default() }
    }
    pub fn run(&mut self, samples: &[Complex<f32>]) -> Result<Vec<Complex<f32>>, NodeError> {
        let mut m = 0usize;
        let st = unsafe { comms_symsync_out_len(samples.len(), self.sps, &mut m) };
        if st != COMMS_OK { return Err(to_err(st)); }
        let mut out = vec![Complex::<f32>::zero(); m];
        let st = unsafe { comms_symsync_run(self.h, samples.as_ptr(), samples.len(), out.as_mut_ptr() as *mut c_void) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// The sampling instant in input samples (positive = later); holds until changed
    pub fn set_timing(&mut self, tau: f64) -> Result<(), NodeError> {
        let st = unsafe { comms_symsync_set_timing(self.h, tau) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    /// mu: the timing in steps of `1 / phases` input samples
    pub fn timing(&self) -> Result<u32, NodeError> {
        let mut mu = 0u32;
        let st = unsafe { comms_symsync_get_timing(self.h, &mut mu) };
        if st == COMMS_OK { Ok(mu) } else { Err(to_err(st)) }
    }
    /// `Mixer::new(phase, dphase)` at symbol rate (NOTE the argument order of the C entry, kept here)
    pub fn set_rotation(&mut self, dphase: f64, phase: f64) -> Result<(), NodeError> {
        let st = unsafe { comms_symsync_set_rotation(self.h, dphase, phase) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    /// Rotor phase of the next output, in [0, 2 pi)
    pub fn phase(&self) -> Result<f64, NodeError> {
        let mut p = 0f64;
        let st = unsafe { comms_symsync_get_phase(self.h, &mut p) };
        if st == COMMS_OK { Ok(p) } else { Err(to_err(st)) }
    }
    /// The checkpoint hook: the last `n` input samples, newest first
    pub fn state(&mut self, n: usize) -> Result<Vec<Complex<f32>>, NodeError> {
        let mut out = vec![Complex::<f32>::zero(); n];
        let st = unsafe { comms_symsync_get_state(self.h, out.as_mut_ptr(), n) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// Exactly `(taps.len() - 1) / phases` samples, newest first
    pub fn set_state(&mut self, state: &[Complex<f32>]) -> Result<(), NodeError> {
        let st = unsafe { comms_symsync_set_state(self.h, state.as_ptr(), state.len()) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
}

/// The symbol synchroniser with hard decisions out (`COMMS_SYM_BITS`): `ceil(n / sps * bits_per_sym / 8)` bytes of packed
/// bits per batch, LSB first, decided against digital.rs's tables (`bits_per_sym` 1: BPSK, 2: QPSK) in the kernel's store
/// stage.  Timing, rotation and state as `SymbolSyncNode`.
#[derive(Node)]
#[pass_by_ref]
pub struct SymbolSyncBitsNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_symsync_t,
    sps: usize,
    bits_per_sym: usize,
    pub output: NodeSender<Vec<u8>>,
}
unsafe impl Send for SymbolSyncBitsNode {}
impl Drop for SymbolSyncBitsNode {
    fn drop(&mut self) { unsafe { comms_symsync_destroy(self.h); } }
}
impl SymbolSyncBitsNode {
    pub fn new(taps: Vec<f32>, phases: usize, sps: usize, bits_per_sym: usize) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_symsync_create(taps.as_ptr(), taps.len(), phases, sps, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_symsync_create failed");
        let st = unsafe { comms_symsync_set_output_format(h, COMMS_SYM_BITS, bits_per_sym as i32, ptr::null()) };
        assert_eq!(st, COMMS_OK, "comms_symsync_set_output_format failed (bits_per_sym is 1 or 2)");
        SymbolSyncBitsNode { input: Default::default(), h, sps, bits_per_sym, output: Default::default() }
    }
    pub fn run(&mut self, samples: &[Complex<f32>]) -> Result<Vec<u8>, NodeError> {
        let mut m = 0usize;
        let st = unsafe { comms_symsync_out_len(samples.len(), self.sps, &mut m) };
        if st != COMMS_OK { return Err(to_err(st)); }
        let mut out = vec![0u8; (m * self.bits_per_sym + 7) / 8];
        let st = unsafe { comms_symsync_run(self.h, samples.as_ptr(), samples.len(), out.as_mut_ptr() as *mut c_void) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    pub fn set_timing(&mut self, tau: f64) -> Result<(), NodeError> {
        let st = unsafe { comms_symsync_set_timing(self.h, tau) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    pub fn set_rotation(&mut self, dphase: f64, phase: f64) -> Result<(), NodeError> {
        let st = unsafe { comms_symsync_set_rotation(self.h, dphase, phase) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    pub fn phase(&self) -> Result<f64, NodeError> {
        let mut p = 0f64;
        let st = unsafe { comms_symsync_get_phase(self.h, &mut p) };
        if st == COMMS_OK { Ok(p) } else { Err(to_err(st)) }
    }
    pub fn state(&mut self, n: usize) -> Result<Vec<Complex<f32>>, NodeError> {
        let mut out = vec![Complex::<f32>::zero(); n];
        let st = unsafe { comms_symsync_get_state(self.h, out.as_mut_ptr(), n) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    pub fn set_state(&mut self, state: &[Complex<f32>]) -> Result<(), NodeError> {
        let st = unsafe { comms_symsync_set_state(self.h, state.as_ptr(), state.len()) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
}

/// Sample types `UniformNode<T>` is built for: `f32` (values in `[start, end)`) and `u8` over `[0, 2)`, which is what
/// `random_bit()` returns (rand_node.rs:150-152).
pub trait UniformSample: Copy + Send + 'static {
    #[doc(hidden)] unsafe fn draw(h: *mut comms_noise_t, n: usize, lo: Self, hi: Self, out: *mut Self) -> comms_status_t;
    #[doc(hidden)] fn range_ok(lo: Self, hi: Self) -> bool;
    #[doc(hidden)] const GRAIN: usize;
}
impl UniformSample for f32 {
    unsafe fn draw(h: *mut comms_noise_t, n: usize, lo: f32, hi: f32, out: *mut f32) -> comms_status_t { comms_noise_uniform_run(h, n, lo, hi, out) }
    fn range_ok(lo: f32, hi: f32) -> bool { lo < hi && lo.is_finite() && hi.is_finite() }
    const GRAIN: usize = 1;
}
impl UniformSample for u8 {
    unsafe fn draw(h: *mut comms_noise_t, n: usize, _lo: u8, _hi: u8, out: *mut u8) -> comms_status_t { comms_noise_bits_run(h, n, COMMS_BITS_U8, out) }
    fn range_ok(lo: u8, hi: u8) -> bool { lo == 0 && hi == 2 }
    const GRAIN: usize = 32; // a bit draw consumes whole 32-bit words
}

/// Seed of a node built without one: the reference seeds from entropy (`StdRng::from_entropy`, rand_node.rs:61,125).
fn entropy_seed() -> u64 {
    use std::collections::hash_map::RandomState;
    use std::hash::{BuildHasher, Hasher};
    let mut h = RandomState::new().build_hasher(); // keyed from the operating system's entropy, per instance
    h.write_u64(std::time::SystemTime::now().duration_since(std::time::UNIX_EPOCH).map(|d| d.as_nanos() as u64).unwrap_or(0));
    h.finish()
}

const NOISE_BLOCK: usize = 4096; // values drawn per launch behind the per-call `run()`

/// rand_node.rs:26-75.  `new(start, end)` as the reference (seeded from entropy) plus `with_seed`: the values are those
/// of the library's counter-based source (include/comms_hip.h, "seeded noise source"), stream 0 of the seed.  `run()`
/// hands out one value per call from a block drawn in one launch; `run_block(n)` returns the next `n` values.
#[derive(Node)]
pub struct UniformNode<T>
where
    T: UniformSample,
{
    h: *mut comms_noise_t,
    lo: T,
    hi: T,
    buf: Vec<T>,
    pos: usize,
    pub output: NodeSender<T>,
}
unsafe impl<T: UniformSample> Send for UniformNode<T> {}
impl<T: UniformSample> Drop for UniformNode<T> {
    fn drop(&mut self) { unsafe { comms_noise_destroy(self.h); } }
}
impl<T> UniformNode<T>
where
    T: UniformSample,
{
    pub fn new(start: T, end: T) -> Self { Self::with_seed(start, end, entropy_seed()) }
    pub fn with_seed(start: T, end: T, seed: u64) -> Self {
        assert!(T::range_ok(start, end), "Uniform::new called with `low >= high`"); // rand's own panic
        let mut h = ptr::null_mut();
        let st = unsafe { comms_noise_create(seed, 0, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_noise_create failed");
        UniformNode { h, lo: start, hi: end, buf: Vec::new(), pos: 0, output: Default::default() }
    }
    fn refill(&mut self, n: usize, fill: T) -> Result<(), NodeError> {
        self.buf.clear();
        self.buf.resize(n, fill);
        self.pos = 0;
        let st = unsafe { T::draw(self.h, n, self.lo, self.hi, self.buf.as_mut_ptr()) };
        if st == COMMS_OK { Ok(()) } else { self.buf.clear(); Err(to_err(st)) }
    }
    pub fn run(&mut self) -> Result<T, NodeError> {
        if self.pos == self.buf.len() { let lo = self.lo; self.refill(NOISE_BLOCK, lo)?; }
        self.pos += 1;
        Ok(self.buf[self.pos - 1])
    }
    pub fn run_block(&mut self, n: usize) -> Result<Vec<T>, NodeError> {
        let mut out: Vec<T> = self.buf[self.pos..].to_vec();
        if out.len() >= n { out.truncate(n); self.pos += n; return Ok(out); }
        let need = n - out.len();
        let lo = self.lo;
        self.refill((need + T::GRAIN - 1) / T::GRAIN * T::GRAIN, lo)?;
        out.extend_from_slice(&self.buf[..need]);
        self.pos = need;
        Ok(out)
    }
}

/// rand_node.rs:150-152
pub fn random_bit() -> UniformNode<u8> { UniformNode::new(0u8, 2u8) }
pub fn random_bit_with_seed(seed: u64) -> UniformNode<u8> { UniformNode::with_seed(0u8, 2u8, seed) }

/// rand_node.rs:97-139: `f64` messages, `mu + std_dev * z` with the f32 `z` of the source widened.
#[derive(Node)]
pub struct NormalNode {
    h: *mut comms_noise_t,
    mu: f64,
    sd: f64,
    buf: Vec<f64>,
    pos: usize,
    pub output: NodeSender<f64>,
}
unsafe impl Send for NormalNode {}
impl Drop for NormalNode {
    fn drop(&mut self) { unsafe { comms_noise_destroy(self.h); } }
}
impl NormalNode {
    pub fn new(mu: f64, std_dev: f64) -> NormalNode { Self::with_seed(mu, std_dev, entropy_seed()) }
    pub fn with_seed(mu: f64, std_dev: f64, seed: u64) -> NormalNode {
        assert!(std_dev >= 0.0 && std_dev.is_finite() && mu.is_finite(), "Normal::new called with `std_dev` < 0"); // rand's own panic
        let mut h = ptr::null_mut();
        let st = unsafe { comms_noise_create(seed, 0, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_noise_create failed");
        NormalNode { h, mu, sd: std_dev, buf: Vec::new(), pos: 0, output: Default::default() }
    }
    fn refill(&mut self, n: usize) -> Result<(), NodeError> {
        self.buf.clear();
        self.buf.resize(n, 0.0);
        self.pos = 0;
        let st = unsafe { comms_noise_normal_f64_run(self.h, n, self.mu, self.sd, self.buf.as_mut_ptr()) };
        if st == COMMS_OK { Ok(()) } else { self.buf.clear(); Err(to_err(st)) }
    }
    pub fn run(&mut self) -> Result<f64, NodeError> {
        if self.pos == self.buf.len() { self.refill(NOISE_BLOCK)?; }
        self.pos += 1;
        Ok(self.buf[self.pos - 1])
    }
    pub fn run_block(&mut self, n: usize) -> Result<Vec<f64>, NodeError> {
        let mut out: Vec<f64> = self.buf[self.pos..].to_vec();
        if out.len() >= n { out.truncate(n); self.pos += n; return Ok(out); }
        let need = n - out.len();
        self.refill(need)?;
        out.extend_from_slice(&self.buf[..need]);
        self.pos = need;
        Ok(out)
    }
}

/// AWGN channel (an additional node): `out = in + sigma * (z + i z')`, one complex standard pair per sample, consecutive
/// across messages (comms_awgn_run).
#[derive(Node)]
#[pass_by_ref]
pub struct AwgnNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_noise_t,
    sigma: f32,
    pub output: NodeSender<Vec<Complex<f32>>>,
}
unsafe impl Send for AwgnNode {}
impl Drop for AwgnNode {
    fn drop(&mut self) { unsafe { comms_noise_destroy(self.h); } }
}
impl AwgnNode {
    pub fn new(sigma: f32) -> Self { Self::with_seed(sigma, entropy_seed(), 0) }
    pub fn with_seed(sigma: f32, seed: u64, stream: u64) -> Self {
        assert!(sigma >= 0.0 && sigma.is_finite(), "sigma must be finite and >= 0");
        let mut h = ptr::null_mut();
        let st = unsafe { comms_noise_create(seed, stream, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_noise_create failed");
        AwgnNode { input: Default::default(), h, sigma, output: Default::default() }
    }
    pub fn run(&mut self, samples: &[Complex<f32>]) -> Result<Vec<Complex<f32>>, NodeError> {
        let mut out = czeros::<f32>(samples.len());
        let st = unsafe { comms_awgn_run(self.h, samples.as_ptr() as *const c_void, samples.len(), self.sigma, out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// fft_node.rs:28-84
#[derive(Node)]
#[pass_by_ref]
pub struct FFTBatchNode<T>
where
    T: FloatSample,
{
    pub input: NodeReceiver<Vec<Complex<T>>>,
    h: *mut T::Fft,
    pub output: NodeSender<Vec<Complex<T>>>,
}
unsafe impl<T: FloatSample> Send for FFTBatchNode<T> {}
impl<T: FloatSample> Drop for FFTBatchNode<T> {
    fn drop(&mut self) { unsafe { T::fft_destroy(self.h); } }
}
impl<T> FFTBatchNode<T>
where
    T: FloatSample,
{
    pub fn new(fft_size: usize, ifft: bool) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { T::fft_create(fft_size, ifft as i32, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_fft_create failed");
        FFTBatchNode { input: Default::default(), h, output: Default::default() }
    }
    pub fn run(&mut self, data: &[Complex<T>]) -> Result<Vec<Complex<T>>, NodeError> {
        let mut out = czeros::<T>(data.len());
        let st = unsafe { T::fft(self.h, data.as_ptr(), data.len(), out.as_mut_ptr()) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }   // rustfft would panic on a wrong length
    }
}

/// fft_node.rs:104-168: `#[aggregate]` -- a sample per message in, a spectrum out every `fft_size` samples
/// (`run` returns `Ok(None)` in between and the derived `call` sends nothing, node_derive/src/lib.rs:139-151).
#[derive(Node)]
#[aggregate]
#[pass_by_ref]
pub struct FFTSampleNode<T>
where
    T: FloatSample,
{
    pub input: NodeReceiver<Complex<T>>,
    h: *mut T::Fft,
    fft_size: usize,
    samples: Vec<Complex<T>>,
    pub output: NodeSender<Vec<Complex<T>>>,
}
unsafe impl<T: FloatSample> Send for FFTSampleNode<T> {}
impl<T: FloatSample> Drop for FFTSampleNode<T> {
    fn drop(&mut self) { unsafe { T::fft_destroy(self.h); } }
}
impl<T> FFTSampleNode<T>
where
    T: FloatSample,
{
    pub fn new(fft_size: usize, ifft: bool) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { T::fft_create(fft_size, ifft as i32, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_fft_create failed");
        FFTSampleNode { input: Default::default(), h, fft_size, samples: Vec::with_capacity(fft_size), output: Default::default() }
    }
    pub fn run(&mut self, sample: &Complex<T>) -> Result<Option<Vec<Complex<T>>>, NodeError> {
        self.samples.push(*sample);
        if self.samples.len() != self.fft_size { return Ok(None); }
        let mut out = czeros::<T>(self.fft_size);
        let st = unsafe { T::fft(self.h, self.samples.as_ptr(), self.fft_size, out.as_mut_ptr()) };
        self.samples.clear();
        if st == COMMS_OK { Ok(Some(out)) } else { Err(to_err(st)) }
    }
}

// ------------------------------------------------------------------ additions (no counterpart in the reference)

macro_rules! handle_node {
    ($name:ident, $destroy:ident) => {
        unsafe impl Send for $name {}
        impl Drop for $name {
            fn drop(&mut self) { unsafe { $destroy(self.h); } }
        }
    };
}

/// An additional node: MixerNode -> BatchFirNode -> DecimateNode [-> FMDemodNode] (or
/// BatchFirNode -> MixerNode -> DecimateNode with `mixer_after_fir`) as one launch
/// (comms_chain_*).  `ChainNode` emits Complex<f32>, `FmChainNode` the demodulated f32.
#[derive(Node)]
#[pass_by_ref]
pub struct ChainNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_chain_t,
    rate: usize,
    pub output: NodeSender<Vec<Complex<f32>>>,
}
handle_node!(ChainNode, comms_chain_destroy);
impl ChainNode {
    pub fn new(dphase: f64, phase: Option<f64>, taps: Vec<Complex<f32>>, rate: usize, mixer_after_fir: bool) -> Self {
        let mut h = ptr::null_mut();
        let flags = if mixer_after_fir { COMMS_CHAIN_MIXER_AFTER_FIR } else { 0 };
        let st = unsafe { comms_chain_create_ex(dphase, phase.unwrap_or(0.0), taps.as_ptr(), taps.len(), rate, flags, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_chain_create_ex failed");
        ChainNode { input: Default::default(), h, rate, output: Default::default() }
    }
    pub fn run(&mut self, input: &[Complex<f32>]) -> Result<Vec<Complex<f32>>, NodeError> {
        if self.rate == 0 || input.len() % self.rate != 0 { return Err(NodeError::DataError); }
        let mut out = vec![Complex::new(0.0f32, 0.0); input.len() / self.rate];
        let st = unsafe { comms_chain_run(self.h, input.as_ptr(), input.len(), out.as_mut_ptr() as *mut _) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

#[derive(Node)]
#[pass_by_ref]
pub struct FmChainNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_chain_t,
    rate: usize,
    pub output: NodeSender<Vec<f32>>,
}
handle_node!(FmChainNode, comms_chain_destroy);
impl FmChainNode {
    pub fn new(dphase: f64, phase: Option<f64>, taps: Vec<Complex<f32>>, rate: usize) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe {
            comms_chain_create_ex(dphase, phase.unwrap_or(0.0), taps.as_ptr(), taps.len(), rate, COMMS_CHAIN_FM_DEMOD, 0, &mut h)
        };
        assert_eq!(st, COMMS_OK, "comms_chain_create_ex failed");
        FmChainNode { input: Default::default(), h, rate, output: Default::default() }
    }
    pub fn run(&mut self, input: &[Complex<f32>]) -> Result<Vec<f32>, NodeError> {
        if self.rate == 0 || input.len() % self.rate != 0 { return Err(NodeError::DataError); }
        let mut out = vec![0.0f32; input.len() / self.rate];
        let st = unsafe { comms_chain_run(self.h, input.as_ptr(), input.len(), out.as_mut_ptr() as *mut _) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    /// The chain's whole cross-call state (FIR history newest first, oscillator phase, FM.prev): what a
    /// checkpoint stores and what the node of the next stream shard starts from (analog.rs:9,31; fir_node.rs:193-211).
    pub fn state(&mut self, n_taps: usize) -> Result<(Vec<Complex<f32>>, f64, Complex<f32>), NodeError> {
        let mut hist = vec![Complex::new(0.0f32, 0.0); n_taps];
        let (mut phase, mut prev) = (0.0f64, Complex::new(0.0f32, 0.0));
        for st in [unsafe { comms_chain_get_fir_state(self.h, hist.as_mut_ptr(), n_taps) },
                   unsafe { comms_chain_get_phase(self.h, &mut phase) },
                   unsafe { comms_chain_get_fm_prev(self.h, &mut prev) }].iter() {
            if *st != COMMS_OK { return Err(to_err(*st)); }
        }
        Ok((hist, phase, prev))
    }
    pub fn set_state(&mut self, hist: &[Complex<f32>], phase: f64, prev: Complex<f32>) -> Result<(), NodeError> {
        for st in [unsafe { comms_chain_set_fir_state(self.h, hist.as_ptr(), hist.len()) },
                   unsafe { comms_chain_set_phase(self.h, phase) },
                   unsafe { comms_chain_set_fm_prev(self.h, &prev) }].iter() {
            if *st != COMMS_OK { return Err(to_err(*st)); }
        }
        Ok(())
    }
}

/// The literal front end of examples/fm_radio.rs:82-90,144-152: RTL-SDR bytes in, demodulated audio-rate
/// f32 out, one launch per block -- the u8 -> f32 conversion happens in the kernel's load stage (2 B/sample
/// from HBM).  `input` carries the raw interleaved (re, im) bytes exactly as the radio delivers them.
#[derive(Node)]
#[pass_by_ref]
pub struct RtlFmChainNode {
    pub input: NodeReceiver<Vec<u8>>,
    h: *mut comms_chain_t,
    rate: usize,
    pub output: NodeSender<Vec<f32>>,
}
handle_node!(RtlFmChainNode, comms_chain_destroy);
impl RtlFmChainNode {
    pub fn new(taps: Vec<Complex<f32>>, rate: usize) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_chain_create_ex(0.0, 0.0, taps.as_ptr(), taps.len(), rate, COMMS_CHAIN_FM_DEMOD, 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_chain_create_ex failed");
        assert_eq!(unsafe { comms_chain_set_input_format(h, COMMS_IQ_U8, 1.0) }, COMMS_OK);
        RtlFmChainNode { input: Default::default(), h, rate, output: Default::default() }
    }
    pub fn run(&mut self, bytes: &[u8]) -> Result<Vec<f32>, NodeError> {
        let n = bytes.len() / 2;
        if self.rate == 0 || n % self.rate != 0 { return Err(NodeError::DataError); }
        let mut out = vec![0.0f32; n / self.rate];
        let st = unsafe { comms_chain_run(self.h, bytes.as_ptr() as *const _, n, out.as_mut_ptr() as *mut _) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// demodulation/timing_estimator.rs:116-136
#[derive(Node)]
#[pass_by_ref]
pub struct TimingEstimatorNode {
    pub input: NodeReceiver<Vec<Complex<f64>>>,
    h: *mut comms_timing_t,
    pub output: NodeSender<f64>,
}
handle_node!(TimingEstimatorNode, comms_timing_destroy);
impl TimingEstimatorNode {
    /// `Err(())` stands for the reference's `MathError::InvalidRolloffError`.
    pub fn new(n: u32, d: u32, alpha: f64) -> Result<Self, ()> {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_timing_create(n, d, alpha, 0, &mut h) };
        if st != COMMS_OK { return Err(()); }
        Ok(TimingEstimatorNode { input: Default::default(), h, output: Default::default() })
    }
    pub fn run(&mut self, input: &[Complex<f64>]) -> Result<f64, NodeError> {
        let mut est = 0.0f64;
        let st = unsafe { comms_timing_push(self.h, input.as_ptr() as *const f64, input.len(), &mut est) };
        if st == COMMS_OK { Ok(est) } else { Err(to_err(st)) }
    }
}

/// Timing and frequency estimates of a `Complex<f32>` block from one read of it (an additional node, comms_syncest_*):
/// `TimingEstimator::push` at `(n, d, alpha)` and `frequency_offset_estimate` of the widened samples.  The message is the
/// whole `comms_sync_estimate_t`; `tau()` turns its timing into what `SymbolSyncNode::set_timing` takes, and
/// `psk_phase_estimate_c32` / `qam_phase_estimate_c32` cover the symbols (`set_rotation(-freq * sps, -phase)`).
#[derive(Node)]
#[pass_by_ref]
pub struct SyncEstimatorNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_syncest_t,
    n: u32,
    pub output: NodeSender<comms_sync_estimate_t>,
}
handle_node!(SyncEstimatorNode, comms_syncest_destroy);
impl SyncEstimatorNode {
    /// `Err(())`: a bad rolloff (the reference's `MathError::InvalidRolloffError`) or a filter beyond the kernel's limits
    /// (`n <= 256`, `2 n d + 1 <= 1024`).
    pub fn new(n: u32, d: u32, alpha: f64) -> Result<Self, ()> {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_syncest_create(n, d, alpha, 0, &mut h) };
        if st != COMMS_OK { return Err(()); }
        Ok(SyncEstimatorNode { input: Default::default(), h, n, output: Default::default() })
    }
    pub fn run(&mut self, input: &[Complex<f32>]) -> Result<comms_sync_estimate_t, NodeError> {
        let mut est = comms_sync_estimate_t::default();
        let st = unsafe { comms_syncest_run(self.h, input.as_ptr(), input.len(), &mut est) };
        if st == COMMS_OK { Ok(est) } else { Err(to_err(st)) }
    }
    /// The `tau` of a `SymbolSyncNode` whose prototype has `n_taps` taps over `phases` phases (its sps = this node's n):
    /// `timing + (n_taps - 1) / (2 phases)` modulo n.
    pub fn tau(&self, est: &comms_sync_estimate_t, n_taps: usize, phases: usize) -> f64 {
        let delay = (n_taps.max(1) - 1) as f64 / (2.0 * phases.max(1) as f64);
        (est.timing + delay).rem_euclid(self.n as f64)
    }
}

/// phase_estimator.rs:26-33 on `Complex<f32>` symbols (widened in the kernel's load).
pub fn psk_phase_estimate_c32(symbols: &[Complex<f32>], m: u32) -> Result<f64, NodeError> {
    let mut out = 0.0f64;
    let st = unsafe { comms_psk_phase_estimate_c32(symbols.as_ptr(), symbols.len(), m, &mut out, 0) };
    if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
}

/// phase_estimator.rs:58-65 on `Complex<f32>` symbols.
pub fn qam_phase_estimate_c32(symbols: &[Complex<f32>]) -> Result<f64, NodeError> {
    let mut out = 0.0f64;
    let st = unsafe { comms_qam_phase_estimate_c32(symbols.as_ptr(), symbols.len(), &mut out, 0) };
    if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
}

/// Frame synchroniser (an additional node, comms_framesync_*): finds a known `word` in the `Complex<f32>` symbol stream that
/// `SymbolSyncNode` sends and returns, per block, the detections the block decides (possibly none), ordered by stream index.
/// `index + word.len()` is the first payload symbol and `corr_im.atan2(corr_re)` the rotation to take out
/// (`MixerNode::new(0.0, Some(-angle))`).  A block of n symbols decides n positions: a word is reported `guard` symbols after
/// its end; `flush` ends a stream.  The detections do not depend on how the stream is cut into blocks.
#[derive(Node)]
#[pass_by_ref]
pub struct FrameSyncNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_framesync_t,
    n_word: usize,
    guard: usize,
    pub output: NodeSender<Vec<comms_frame_detection_t>>,
}
handle_node!(FrameSyncNode, comms_framesync_destroy);
impl FrameSyncNode {
    /// `Err(())`: a word of fewer than 2 or more than 512 symbols, not finite or without energy, a guard beyond 512 or a
    /// threshold outside (0, 1].
    pub fn new(word: &[Complex<f32>], threshold: f64, guard: usize) -> Result<Self, ()> {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_framesync_create(word.as_ptr(), word.len(), threshold, guard, 0, &mut h) };
        if st != COMMS_OK { return Err(()); }
        Ok(FrameSyncNode { input: Default::default(), h, n_word: word.len(), guard, output: Default::default() })
    }
    pub fn run(&mut self, input: &[Complex<f32>]) -> Result<Vec<comms_frame_detection_t>, NodeError> {
        // detections are more than `guard` apart: no call on n symbols has more than ceil(n / (guard + 1))
        let cap = (input.len() + self.guard) / (self.guard + 1);
        let mut out = vec![comms_frame_detection_t::default(); cap];
        let mut found = 0usize;
        let st = unsafe { comms_framesync_run(self.h, input.as_ptr(), input.len(), out.as_mut_ptr(), cap, &mut found) };
        if st != COMMS_OK { return Err(to_err(st)); }
        out.truncate(found);
        Ok(out)
    }
    /// The positions still undecided, as if `word.len() + guard` zero symbols followed; the history is zero afterwards.
    pub fn flush(&mut self) -> Result<Vec<comms_frame_detection_t>, NodeError> {
        let cap = (self.n_word + 2 * self.guard) / (self.guard + 1);
        let mut out = vec![comms_frame_detection_t::default(); cap];
        let mut found = 0usize;
        let st = unsafe { comms_framesync_flush(self.h, out.as_mut_ptr(), cap, &mut found) };
        if st != COMMS_OK { return Err(to_err(st)); }
        out.truncate(found);
        Ok(out)
    }
    /// Stream index of the next symbol (checkpoints; the first index of a stream shard).
    pub fn position(&self) -> u64 {
        let mut t = 0u64;
        unsafe { comms_framesync_get_position(self.h, &mut t) };
        t
    }
    pub fn set_position(&mut self, position: u64) -> Result<(), NodeError> {
        let st = unsafe { comms_framesync_set_position(self.h, position) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    pub fn set_threshold(&mut self, threshold: f64) -> Result<(), NodeError> {
        let st = unsafe { comms_framesync_set_threshold(self.h, threshold) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
}

/// What `DeframeNode` sends per block: the records of the frames that became complete in it, back to back (frame f at
/// `data[f * frame_bytes..]`), and one header per frame.
#[derive(Clone, Debug, Default, PartialEq)]
pub struct Frames {
    pub data: Vec<u8>,
    pub headers: Vec<comms_deframe_header_t>,
    pub frame_bytes: usize,
}

/// Deframer (an additional node, comms_deframe_*): takes the symbol blocks `FrameSyncNode` takes and, on `detections`, what
/// `FrameSyncNode` sent for the same block; sends the payloads of the frames that became complete in the block -- `n_payload`
/// symbols from `index + offset`, derotated by the detection's correlation -- as packed bits (`COMMS_SYM_BITS`), max-log LLRs
/// (`COMMS_SYM_LLR`, f32, positive = bit 0) or symbols (`COMMS_SYM_C32`), all by one launch.  A payload that ends in a later
/// block comes out of that block.  `lookback` >= the frame synchroniser's guard - 1.
#[derive(Node)]
#[pass_by_ref]
pub struct DeframeNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    pub detections: NodeReceiver<Vec<comms_frame_detection_t>>,
    h: *mut comms_deframe_t,
    pub output: NodeSender<Frames>,
}
handle_node!(DeframeNode, comms_deframe_destroy);
impl DeframeNode {
    /// `word_energy`: `Some(sum |p|^2)` scales every payload by it over |corr| (COMMS_DEFRAME_NORMALISE).
    /// `Err(())`: n_payload outside 1 ..= 2^20, offset or lookback beyond 2^20, bits_per_sym not 1 or 2, an unknown format.
    pub fn new(n_payload: usize, offset: usize, lookback: usize, bits_per_sym: i32, format: i32, word_energy: Option<f64>) -> Result<Self, ()> {
        let mut h = ptr::null_mut();
        let flags = if word_energy.is_some() { COMMS_DEFRAME_NORMALISE } else { 0 };
        let st = unsafe { comms_deframe_create(n_payload, offset, lookback, bits_per_sym, ptr::null(), flags, 0, &mut h) };
        if st != COMMS_OK { return Err(()); }
        let node = DeframeNode { input: Default::default(), detections: Default::default(), h, output: Default::default() };
        if let Some(ep) = word_energy {
            if unsafe { comms_deframe_set_word_energy(node.h, ep) } != COMMS_OK { return Err(()); }
        }
        if unsafe { comms_deframe_set_output_format(node.h, format) } != COMMS_OK { return Err(()); }
        Ok(node)
    }
    /// s of L = s (D1 - D0): 1 / (2 sigma^2).
    pub fn set_llr_scale(&mut self, scale: f32) -> Result<(), NodeError> {
        let st = unsafe { comms_deframe_set_llr_scale(self.h, scale) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    pub fn run(&mut self, input: &[Complex<f32>], detections: &[comms_frame_detection_t]) -> Result<Frames, NodeError> {
        let mut cap = 0usize;
        let st = unsafe { comms_deframe_frames_ready(self.h, input.len(), detections.as_ptr(), detections.len(), &mut cap) };
        if st != COMMS_OK { return Err(to_err(st)); }
        let frame_bytes = unsafe { comms_deframe_frame_bytes(self.h) };
        let mut out = Frames { data: vec![0u8; cap * frame_bytes], headers: vec![comms_deframe_header_t::default(); cap], frame_bytes };
        let mut found = 0usize;
        let st = unsafe {
            comms_deframe_run(self.h, input.as_ptr(), input.len(), detections.as_ptr(), detections.len(),
                              out.data.as_mut_ptr() as *mut c_void, cap, out.headers.as_mut_ptr(), &mut found)
        };
        if st != COMMS_OK { return Err(to_err(st)); }
        Ok(out)
    }
    /// Drops the incomplete frames and returns how many; the history is zero afterwards, the position kept.
    pub fn flush(&mut self) -> Result<usize, NodeError> {
        let mut dropped = 0usize;
        let st = unsafe { comms_deframe_flush(self.h, &mut dropped) };
        if st == COMMS_OK { Ok(dropped) } else { Err(to_err(st)) }
    }
    pub fn position(&self) -> u64 {
        let mut t = 0u64;
        unsafe { comms_deframe_get_position(self.h, &mut t) };
        t
    }
}

/// Convolutional encoder (an additional node, comms_convenc_*): a message is whole records of packed information bits (LSB
/// first, `in_frame_bytes()` each), the output the records of n * steps coded bits (`out_frame_bytes()` each), coded bit j of
/// step t at t * n + j.  `gens`: `None` = K = 7, (0o171, 0o133).  Stateless: every frame starts in state 0.
#[derive(Node)]
#[pass_by_ref]
pub struct ConvEncoderNode {
    pub input: NodeReceiver<Vec<u8>>,
    h: *mut comms_convenc_t,
    pub output: NodeSender<Vec<u8>>,
}
handle_node!(ConvEncoderNode, comms_convenc_destroy);
impl ConvEncoderNode {
    /// `Err(())`: K outside 3 ..= 7, other than 2 or 3 generators, a generator outside 1 .. 2^K, more than 2^16 steps.
    pub fn new(n_info_bits: usize, k: i32, gens: Option<&[u32]>, terminated: bool) -> Result<Self, ()> {
        let mut h = ptr::null_mut();
        let flags = if terminated { COMMS_CONV_TERMINATED } else { COMMS_CONV_TRUNCATED };
        let (n, g) = match gens { Some(g) => (g.len() as i32, g.as_ptr()), None => (2, ptr::null()) };
        let st = unsafe { comms_convenc_create(k, n, g, flags, n_info_bits, 0, &mut h) };
        if st != COMMS_OK { return Err(()); }
        Ok(ConvEncoderNode { input: Default::default(), h, output: Default::default() })
    }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_convenc_in_frame_bytes(self.h) } }
    pub fn out_frame_bytes(&self) -> usize { unsafe { comms_convenc_out_frame_bytes(self.h) } }
    pub fn run(&mut self, records: &[u8]) -> Result<Vec<u8>, NodeError> {
        let fin = self.in_frame_bytes();
        if fin == 0 || records.len() % fin != 0 { return Err(NodeError::DataError); }
        let n_frames = records.len() / fin;
        let mut out = vec![0u8; n_frames * self.out_frame_bytes()];
        let st = unsafe { comms_convenc_run(self.h, records.as_ptr() as *const c_void, n_frames, out.as_mut_ptr() as *mut c_void) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// Viterbi decoder of `ConvEncoderNode`'s code (an additional node, comms_viterbi_*): takes `DeframeNode`'s `COMMS_SYM_LLR`
/// message (records of at least n * steps f32 values, positive = bit 0) and sends the decoded records under the same headers,
/// all frames by one launch.  Integer decisions on q = clamp(rint(L * qscale), -127, 127).
#[derive(Node)]
#[pass_by_ref]
pub struct ViterbiNode {
    pub input: NodeReceiver<Frames>,
    h: *mut comms_viterbi_t,
    pub output: NodeSender<Frames>,
}
handle_node!(ViterbiNode, comms_viterbi_destroy);
impl ViterbiNode {
    /// `record_llrs`: values per input record, 0 = exactly n * steps.  `Err(())` as `ConvEncoderNode::new`, or fewer values.
    pub fn new(n_info_bits: usize, k: i32, gens: Option<&[u32]>, terminated: bool, record_llrs: usize) -> Result<Self, ()> {
        let mut h = ptr::null_mut();
        let flags = if terminated { COMMS_CONV_TERMINATED } else { COMMS_CONV_TRUNCATED };
        let (n, g) = match gens { Some(g) => (g.len() as i32, g.as_ptr()), None => (2, ptr::null()) };
        let st = unsafe { comms_viterbi_create(k, n, g, flags, n_info_bits, record_llrs, 0, &mut h) };
        if st != COMMS_OK { return Err(()); }
        Ok(ViterbiNode { input: Default::default(), h, output: Default::default() })
    }
    pub fn set_quant_scale(&mut self, qscale: f32) -> Result<(), NodeError> {
        let st = unsafe { comms_viterbi_set_quant_scale(self.h, qscale) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_viterbi_in_frame_bytes(self.h) } }
    pub fn out_frame_bytes(&self) -> usize { unsafe { comms_viterbi_out_frame_bytes(self.h) } }
    pub fn run(&mut self, frames: &Frames) -> Result<Frames, NodeError> {
        let n_frames = frames.headers.len();
        if frames.frame_bytes != self.in_frame_bytes() || frames.data.len() < n_frames * frames.frame_bytes { return Err(NodeError::DataError); }
        let frame_bytes = self.out_frame_bytes();
        let mut out = Frames { data: vec![0u8; n_frames * frame_bytes], headers: frames.headers.clone(), frame_bytes };
        let st = unsafe {
            comms_viterbi_run(self.h, frames.data.as_ptr() as *const f32, n_frames, out.data.as_mut_ptr() as *mut c_void, ptr::null_mut())
        };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// One frame format of the rate matching (comms_ratematch_*), the same on both sides of the link: `pattern` holds 0 / 1 per
/// coded position and repeats (empty keeps everything), `cols` is the width of the pruned block interleaver over the kept bits
/// (0, 1: none) or `perm` an explicit permutation of them (`cols` = 0 then), `scramble` one bit per transmitted bit packed LSB
/// first (empty: none).
#[derive(Clone, Default)]
pub struct RateMatchFormat {
    pub n_coded: usize,
    pub pattern: Vec<u8>,
    pub cols: usize,
    pub perm: Vec<u32>,
    pub scramble: Vec<u8>,
}
impl RateMatchFormat {
    /// `Err(())`: what comms_ratematch_create refuses, or a `perm` / `scramble` that does not cover the transmitted bits.
    fn create(&self, record_llrs: usize) -> Result<*mut comms_ratematch_t, ()> {
        let kept = (0..self.n_coded).filter(|i| self.pattern.is_empty() || self.pattern[i % self.pattern.len()] != 0).count();
        if (!self.perm.is_empty() && self.perm.len() != kept) || (!self.scramble.is_empty() && self.scramble.len() < (kept + 7) / 8) { return Err(()); }
        let opt = |p: *const u8, empty: bool| if empty { ptr::null() } else { p };
        let perm = if self.perm.is_empty() { ptr::null() } else { self.perm.as_ptr() };
        let mut h = ptr::null_mut();
        let st = unsafe {
            comms_ratematch_create(self.n_coded, opt(self.pattern.as_ptr(), self.pattern.is_empty()), self.pattern.len(), self.cols, perm,
                                   opt(self.scramble.as_ptr(), self.scramble.is_empty()) as *const c_void, record_llrs, 0, &mut h)
        };
        if st == COMMS_OK { Ok(h) } else { Err(()) }
    }
}

/// Transmit rate matching (an additional node): takes `ConvEncoderNode`'s records of `n_coded` packed bits and sends records of
/// `n_tx_bits()` bits -- selected, permuted and whitened -- that the bit-input modulators take as they stand.  Stateless.
#[derive(Node)]
#[pass_by_ref]
pub struct RateMatchNode {
    pub input: NodeReceiver<Vec<u8>>,
    h: *mut comms_ratematch_t,
    pub output: NodeSender<Vec<u8>>,
}
handle_node!(RateMatchNode, comms_ratematch_destroy);
impl RateMatchNode {
    pub fn new(format: &RateMatchFormat) -> Result<Self, ()> {
        Ok(RateMatchNode { input: Default::default(), h: format.create(0)?, output: Default::default() })
    }
    pub fn n_tx_bits(&self) -> usize { unsafe { comms_ratematch_n_tx_bits(self.h) } }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_ratematch_tx_in_frame_bytes(self.h) } }
    pub fn out_frame_bytes(&self) -> usize { unsafe { comms_ratematch_tx_out_frame_bytes(self.h) } }
    pub fn run(&mut self, records: &[u8]) -> Result<Vec<u8>, NodeError> {
        let fin = self.in_frame_bytes();
        if fin == 0 || records.len() % fin != 0 { return Err(NodeError::DataError); }
        let n_frames = records.len() / fin;
        let mut out = vec![0u8; n_frames * self.out_frame_bytes()];
        let st = unsafe { comms_ratematch_tx_run(self.h, records.as_ptr() as *const c_void, n_frames, out.as_mut_ptr() as *mut c_void) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// Receive rate matching (an additional node): takes `DeframeNode`'s `COMMS_SYM_LLR` message (records of at least
/// `n_tx_bits()` f32 values) and sends records of `n_coded` values under the same headers, +0.0 at the punctured positions:
/// `ViterbiNode`'s input with `record_llrs` = 0.
#[derive(Node)]
#[pass_by_ref]
pub struct RateDematchNode {
    pub input: NodeReceiver<Frames>,
    h: *mut comms_ratematch_t,
    pub output: NodeSender<Frames>,
}
handle_node!(RateDematchNode, comms_ratematch_destroy);
impl RateDematchNode {
    /// `record_llrs`: values per input record, 0 = exactly the transmitted bits.
    pub fn new(format: &RateMatchFormat, record_llrs: usize) -> Result<Self, ()> {
        Ok(RateDematchNode { input: Default::default(), h: format.create(record_llrs)?, output: Default::default() })
    }
    pub fn n_tx_bits(&self) -> usize { unsafe { comms_ratematch_n_tx_bits(self.h) } }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_ratematch_rx_in_frame_bytes(self.h) } }
    pub fn out_frame_bytes(&self) -> usize { unsafe { comms_ratematch_rx_out_frame_bytes(self.h) } }
    pub fn run(&mut self, frames: &Frames) -> Result<Frames, NodeError> {
        let n_frames = frames.headers.len();
        if frames.frame_bytes != self.in_frame_bytes() || frames.data.len() < n_frames * frames.frame_bytes { return Err(NodeError::DataError); }
        let frame_bytes = self.out_frame_bytes();
        let mut out = Frames { data: vec![0u8; n_frames * frame_bytes], headers: frames.headers.clone(), frame_bytes };
        let st = unsafe { comms_ratematch_rx_run(self.h, frames.data.as_ptr() as *const f32, n_frames, out.data.as_mut_ptr() as *mut f32) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// One frame check (comms_crc_*), the same on both sides of the link: a `width`-bit CRC (1 ..= 32) with polynomial `poly` in
/// normal form without the x^width term, register `init` and final `xorout`, no reflection, over frames of `n_payload_bits`
/// bits.  Records are packed LSB first: (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF) is the Ethernet FCS.
#[derive(Clone, Copy, Default)]
pub struct CrcSpec {
    pub width: i32,
    pub poly: u32,
    pub init: u32,
    pub xorout: u32,
    pub n_payload_bits: usize,
}
impl CrcSpec {
    /// `Err(())`: what comms_crc_create refuses.
    fn create(&self) -> Result<*mut comms_crc_t, ()> {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_crc_create(self.width, self.poly, self.init, self.xorout, self.n_payload_bits, 0, &mut h) };
        if st == COMMS_OK { Ok(h) } else { Err(()) }
    }
}

/// Appends the CRC (an additional node), in front of `ConvEncoderNode`: takes records of `n_payload_bits` packed bits and sends
/// records of `n_payload_bits + width` bits.  Stateless.
#[derive(Node)]
#[pass_by_ref]
pub struct CrcAttachNode {
    pub input: NodeReceiver<Vec<u8>>,
    h: *mut comms_crc_t,
    pub output: NodeSender<Vec<u8>>,
}
handle_node!(CrcAttachNode, comms_crc_destroy);
impl CrcAttachNode {
    pub fn new(spec: &CrcSpec) -> Result<Self, ()> {
        Ok(CrcAttachNode { input: Default::default(), h: spec.create()?, output: Default::default() })
    }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_crc_payload_frame_bytes(self.h) } }
    pub fn out_frame_bytes(&self) -> usize { unsafe { comms_crc_coded_frame_bytes(self.h) } }
    pub fn run(&mut self, records: &[u8]) -> Result<Vec<u8>, NodeError> {
        let fin = self.in_frame_bytes();
        if fin == 0 || records.len() % fin != 0 { return Err(NodeError::DataError); }
        let n_frames = records.len() / fin;
        let mut out = vec![0u8; n_frames * self.out_frame_bytes()];
        let st = unsafe { comms_crc_attach_run(self.h, records.as_ptr() as *const c_void, n_frames, out.as_mut_ptr() as *mut c_void) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// What `CrcCheckNode` sends: the payload records and, per frame, whether the recomputed CRC equals the received bits.
#[derive(Clone, Default)]
pub struct CheckedFrames {
    pub payload: Vec<u8>,
    pub passed: Vec<i32>,
    pub n_failed: usize,
}

/// Checks the CRC (an additional node), behind `ViterbiNode` with `n_info_bits = n_payload_bits + width`: takes the decoder's
/// records and sends the payload records with one pass flag per frame.  Stateless.
#[derive(Node)]
#[pass_by_ref]
pub struct CrcCheckNode {
    pub input: NodeReceiver<Vec<u8>>,
    h: *mut comms_crc_t,
    pub output: NodeSender<CheckedFrames>,
}
handle_node!(CrcCheckNode, comms_crc_destroy);
impl CrcCheckNode {
    pub fn new(spec: &CrcSpec) -> Result<Self, ()> {
        Ok(CrcCheckNode { input: Default::default(), h: spec.create()?, output: Default::default() })
    }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_crc_coded_frame_bytes(self.h) } }
    pub fn out_frame_bytes(&self) -> usize { unsafe { comms_crc_payload_frame_bytes(self.h) } }
    pub fn run(&mut self, records: &[u8]) -> Result<CheckedFrames, NodeError> {
        let fin = self.in_frame_bytes();
        if fin == 0 || records.len() % fin != 0 { return Err(NodeError::DataError); }
        let n_frames = records.len() / fin;
        let mut out = CheckedFrames { payload: vec![0u8; n_frames * self.out_frame_bytes()], passed: vec![0i32; n_frames], n_failed: 0 };
        let st = unsafe {
            comms_crc_check_run(self.h, records.as_ptr() as *const c_void, n_frames, out.payload.as_mut_ptr() as *mut c_void,
                                out.passed.as_mut_ptr(), ptr::null_mut(), &mut out.n_failed)
        };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// The Gray-coded square QAM table of comms_constellation_qam (`bits_per_sym` 2, 4, 6, 8; 1 is BPSK): host arithmetic, no device.
pub fn qam_table(bits_per_sym: i32, scale: f64) -> Result<Vec<Complex<f32>>, ()> {
    if !(1..=8).contains(&bits_per_sym) { return Err(()); }
    let mut t = vec![Complex::new(0.0f32, 0.0f32); 1usize << bits_per_sym];
    let st = unsafe { comms_constellation_qam(bits_per_sym, scale, t.as_mut_ptr() as *mut comms_c32) };
    if st == COMMS_OK { Ok(t) } else { Err(()) }
}
/// The Gray-coded PSK table of comms_constellation_psk (`bits_per_sym` 1 ..= 4; pi/4 offset at 2): host arithmetic, no device.
pub fn psk_table(bits_per_sym: i32, scale: f64) -> Result<Vec<Complex<f32>>, ()> {
    if !(1..=8).contains(&bits_per_sym) { return Err(()); }
    let mut t = vec![Complex::new(0.0f32, 0.0f32); 1usize << bits_per_sym];
    let st = unsafe { comms_constellation_psk(bits_per_sym, scale, t.as_mut_ptr() as *mut comms_c32) };
    if st == COMMS_OK { Ok(t) } else { Err(()) }
}

fn c32_or_null(v: &[Complex<f32>]) -> *const comms_c32 {
    if v.is_empty() { ptr::null() } else { v.as_ptr() as *const comms_c32 }
}

/// Symbol mapper (comms_symmap_*; an additional node), behind `RateMatchNode`: takes records of `n_bits` packed bits and sends,
/// per record, `word`, ceil(n_bits / bits_per_sym) points of `constellation` (empty = digital.rs's tables at 1 or 2 bits) and
/// `gap` zero symbols -- the stream `PulseNode` shapes and `FrameSyncNode` / `DeframeNode` take apart again.  Stateless.
#[derive(Node)]
#[pass_by_ref]
pub struct SymbolMapNode {
    pub input: NodeReceiver<Vec<u8>>,
    h: *mut comms_symmap_t,
    pub output: NodeSender<Vec<Complex<f32>>>,
}
handle_node!(SymbolMapNode, comms_symmap_destroy);
impl SymbolMapNode {
    /// `Err(())`: what comms_symmap_create refuses.
    pub fn new(bits_per_sym: i32, constellation: &[Complex<f32>], n_bits: usize, word: &[Complex<f32>], gap: usize) -> Result<Self, ()> {
        if !constellation.is_empty() && (1..=8).contains(&bits_per_sym) && constellation.len() != 1usize << bits_per_sym { return Err(()); }
        let mut h = ptr::null_mut();
        let st = unsafe {
            comms_symmap_create(bits_per_sym, c32_or_null(constellation), n_bits,
                                c32_or_null(word), word.len(), gap, 0, &mut h)
        };
        if st == COMMS_OK { Ok(SymbolMapNode { input: Default::default(), h, output: Default::default() }) } else { Err(()) }
    }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_symmap_in_frame_bytes(self.h) } }
    pub fn out_frame_syms(&self) -> usize { unsafe { comms_symmap_out_frame_syms(self.h) } }
    pub fn run(&mut self, records: &[u8]) -> Result<Vec<Complex<f32>>, NodeError> {
        let fin = self.in_frame_bytes();
        if fin == 0 || records.len() % fin != 0 { return Err(NodeError::DataError); }
        let n_frames = records.len() / fin;
        let mut out = vec![Complex::new(0.0f32, 0.0f32); n_frames * self.out_frame_syms()];
        let st = unsafe { comms_symmap_run(self.h, records.as_ptr() as *const c_void, n_frames, out.as_mut_ptr() as *mut comms_c32) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// Soft demapper (comms_demap_*; an additional node), behind `DeframeNode` in the `COMMS_SYM_C32` format (normalising): takes
/// records of `n_payload` symbols and sends, under the same headers, max-log LLRs (`COMMS_SYM_LLR`: `n_payload * bits_per_sym`
/// f32 per record, `RateDematchNode`'s input with that `record_llrs`) or packed hard bits (`COMMS_SYM_BITS`).  Stateless.
#[derive(Node)]
#[pass_by_ref]
pub struct DemapNode {
    pub input: NodeReceiver<Frames>,
    h: *mut comms_demap_t,
    pub output: NodeSender<Frames>,
}
handle_node!(DemapNode, comms_demap_destroy);
impl DemapNode {
    /// `format`: COMMS_SYM_LLR or COMMS_SYM_BITS; `llr_scale`: 1 / (2 sigma^2) at the table's scale; `force_table`: the general
    /// kernel form for a separable table too.  `Err(())`: what the library refuses.
    pub fn new(bits_per_sym: i32, constellation: &[Complex<f32>], n_payload: usize, format: i32, llr_scale: f32, force_table: bool) -> Result<Self, ()> {
        if !constellation.is_empty() && (1..=8).contains(&bits_per_sym) && constellation.len() != 1usize << bits_per_sym { return Err(()); }
        let mut h = ptr::null_mut();
        let st = unsafe {
            comms_demap_create(bits_per_sym, c32_or_null(constellation), n_payload,
                               if force_table { COMMS_DEMAP_TABLE } else { 0 }, 0, &mut h)
        };
        if st != COMMS_OK { return Err(()); }
        let node = DemapNode { input: Default::default(), h, output: Default::default() };   // (dropped, and so destroyed, on an error below)
        let ok = unsafe { comms_demap_set_output_format(node.h, format) == COMMS_OK && comms_demap_set_llr_scale(node.h, llr_scale) == COMMS_OK };
        if ok { Ok(node) } else { Err(()) }
    }
    pub fn in_frame_bytes(&self) -> usize { unsafe { comms_demap_in_frame_bytes(self.h) } }
    pub fn out_frame_bytes(&self) -> usize { unsafe { comms_demap_out_frame_bytes(self.h) } }
    pub fn run(&mut self, frames: &Frames) -> Result<Frames, NodeError> {
        let n_frames = frames.headers.len();
        if frames.frame_bytes != self.in_frame_bytes() || frames.data.len() < n_frames * frames.frame_bytes { return Err(NodeError::DataError); }
        let frame_bytes = self.out_frame_bytes();
        let mut out = Frames { data: vec![0u8; n_frames * frame_bytes], headers: frames.headers.clone(), frame_bytes };
        let st = unsafe { comms_demap_run(self.h, frames.data.as_ptr() as *const comms_c32, n_frames, out.data.as_mut_ptr() as *mut c_void) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// One OFDM frame format (comms_ofdm_create's arguments): `carrier_kind` holds `n_fft` entries (COMMS_OFDM_NULL / _DATA /
/// _PILOT, bin 0 = DC), `pilots` one value per pilot carrier, `polarity` the per-symbol pilot signs (empty = 1), `train` the
/// `n_fft` frequency values of the `n_train` training symbols in front of the `n_syms` data symbols of every frame.
pub struct OfdmFormat<'a> {
    pub n_fft: i32,
    pub n_cp: i32,
    pub carrier_kind: &'a [u8],
    pub pilots: &'a [Complex<f32>],
    pub polarity: &'a [f32],
    pub train: &'a [Complex<f32>],
    pub n_train: usize,
    pub n_syms: usize,
    pub cpe: bool,
}

fn ofdm_create(f: &OfdmFormat) -> Result<*mut comms_ofdm_t, ()> {
    if f.n_fft < 0 || f.carrier_kind.len() != f.n_fft as usize { return Err(()); }
    if f.pilots.len() != f.carrier_kind.iter().filter(|&&k| k as i32 == COMMS_OFDM_PILOT).count() { return Err(()); }
    if (f.n_train > 0 || !f.train.is_empty()) && f.train.len() != f.carrier_kind.len() { return Err(()); }
    let mut h = ptr::null_mut();
    let st = unsafe {
        comms_ofdm_create(f.n_fft, f.n_cp, f.carrier_kind.as_ptr(), c32_or_null(f.pilots),
                          if f.polarity.is_empty() { ptr::null() } else { f.polarity.as_ptr() }, f.polarity.len(),
                          c32_or_null(f.train), f.n_train, f.n_syms, if f.cpe { COMMS_OFDM_CPE } else { 0 }, 0, &mut h)
    };
    if st == COMMS_OK { Ok(h) } else { Err(()) }
}

/// OFDM modulator (comms_ofdm_mod_*; an additional node), behind `SymbolMapNode` without word and gap: takes records of
/// `data_syms()` data-carrier values and sends `frame_samples()` time samples per record -- training symbols, then the data
/// symbols with pilots, each behind its cyclic prefix.  Stateless.
#[derive(Node)]
#[pass_by_ref]
pub struct OfdmModNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_ofdm_t,
    pub output: NodeSender<Vec<Complex<f32>>>,
}
handle_node!(OfdmModNode, comms_ofdm_destroy);
impl OfdmModNode {
    /// `Err(())`: what comms_ofdm_create refuses.
    pub fn new(format: &OfdmFormat) -> Result<Self, ()> {
        Ok(OfdmModNode { input: Default::default(), h: ofdm_create(format)?, output: Default::default() })
    }
    pub fn data_syms(&self) -> usize { unsafe { comms_ofdm_data_syms(self.h) } }
    pub fn frame_samples(&self) -> usize { unsafe { comms_ofdm_frame_samples(self.h) } }
    pub fn run(&mut self, records: &[Complex<f32>]) -> Result<Vec<Complex<f32>>, NodeError> {
        let fin = self.data_syms();
        if fin == 0 || records.len() % fin != 0 { return Err(NodeError::DataError); }
        let n_frames = records.len() / fin;
        let mut out = vec![Complex::new(0.0f32, 0.0f32); n_frames * self.frame_samples()];
        let st = unsafe { comms_ofdm_mod_run(self.h, records.as_ptr() as *const comms_c32, n_frames, out.as_mut_ptr() as *mut comms_c32) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// OFDM demodulator (comms_ofdm_demod_*; an additional node), in front of `DemapNode` with `n_payload = data_syms()`: takes
/// frames of `frame_samples()` received samples and sends the equalised data-carrier values -- channel estimate from the
/// training symbols, one multiply per carrier, with `cpe` the pilots' common phase removed per symbol.  Stateless.
#[derive(Node)]
#[pass_by_ref]
pub struct OfdmDemodNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_ofdm_t,
    pub output: NodeSender<Vec<Complex<f32>>>,
}
handle_node!(OfdmDemodNode, comms_ofdm_destroy);
impl OfdmDemodNode {
    /// `Err(())`: what comms_ofdm_create refuses.
    pub fn new(format: &OfdmFormat) -> Result<Self, ()> {
        Ok(OfdmDemodNode { input: Default::default(), h: ofdm_create(format)?, output: Default::default() })
    }
    pub fn data_syms(&self) -> usize { unsafe { comms_ofdm_data_syms(self.h) } }
    pub fn frame_samples(&self) -> usize { unsafe { comms_ofdm_frame_samples(self.h) } }
    pub fn run(&mut self, samples: &[Complex<f32>]) -> Result<Vec<Complex<f32>>, NodeError> {
        let fin = self.frame_samples();
        if fin == 0 || samples.len() % fin != 0 { return Err(NodeError::DataError); }
        let n_frames = samples.len() / fin;
        let mut out = vec![Complex::new(0.0f32, 0.0f32); n_frames * self.data_syms()];
        let st = unsafe { comms_ofdm_demod_run(self.h, samples.as_ptr() as *const comms_c32, n_frames, out.as_mut_ptr() as *mut comms_c32) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// What `OfdmSyncNode` sends per block: the detections the block decides (possibly none), ordered by stream index, and next to
/// each its carrier-frequency offset `corr_im.atan2(corr_re) / lag` in rad / sample.
#[derive(Clone, Debug, Default, PartialEq)]
pub struct OfdmDetections {
    pub detections: Vec<comms_frame_detection_t>,
    pub cfo: Vec<f64>,
}

/// OFDM stream synchroniser (comms_ofdmsync_*; an additional node), in front of `DeframeNode`: correlates the received
/// `Complex<f32>` sample stream with itself at `lag` over `window` samples (the repeated training symbol: `lag = window =
/// n_fft + n_cp`), searches peaks of the normalised metric over +-`guard` positions above `threshold` and sends, per block, the
/// frame starts (`index` lies `advance` samples ahead of the peak) with their offsets.  A block of n samples decides n
/// positions; `flush` ends a stream; the detections do not depend on how the stream is cut into blocks.  The deframer behind it:
/// `DeframeNode::new(n_frame, 0, lookback(), .., COMMS_SYM_C32, None)`, then `OfdmCfoCorrectNode`.
#[derive(Node)]
#[pass_by_ref]
pub struct OfdmSyncNode {
    pub input: NodeReceiver<Vec<Complex<f32>>>,
    h: *mut comms_ofdmsync_t,
    lag: usize,
    window: usize,
    guard: usize,
    advance: usize,
    pub output: NodeSender<OfdmDetections>,
}
handle_node!(OfdmSyncNode, comms_ofdmsync_destroy);
impl OfdmSyncNode {
    /// `Err(())`: lag outside 1 ..= 2048, window outside 2 ..= 2048, a threshold outside (0, 1], a guard beyond 512 or an advance
    /// beyond 2048.
    pub fn new(lag: usize, window: usize, threshold: f64, guard: usize, advance: usize) -> Result<Self, ()> {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_ofdmsync_create(lag, window, threshold, guard, advance, 0, 0, &mut h) };
        if st != COMMS_OK { return Err(()); }
        Ok(OfdmSyncNode { input: Default::default(), h, lag, window, guard, advance, output: Default::default() })
    }
    /// The node for the frames of `format` (n_train >= 2): `lag = window = n_fft + n_cp`.
    pub fn for_format(format: &OfdmFormat, threshold: f64, guard: usize, advance: usize) -> Result<Self, ()> {
        if format.n_fft < 0 || format.n_cp < 0 { return Err(()); }
        let sym = (format.n_fft + format.n_cp) as usize;
        Self::new(sym, sym, threshold, guard, advance)
    }
    /// The least `lookback` of the `DeframeNode` behind this node.
    pub fn lookback(&self) -> usize { self.window + self.lag + self.guard + self.advance - 1 }
    fn collect<F>(&mut self, n: usize, call: F) -> Result<OfdmDetections, NodeError>
    where
        F: FnOnce(*mut comms_ofdmsync_t, *mut comms_frame_detection_t, *mut f64, usize, *mut usize) -> comms_status_t,
    {
        // detections are more than `guard` apart: no call that decides n positions has more than ceil(n / (guard + 1))
        let cap = (n + self.guard) / (self.guard + 1);
        let mut out = OfdmDetections { detections: vec![comms_frame_detection_t::default(); cap], cfo: vec![0.0f64; cap] };
        let mut found = 0usize;
        let st = call(self.h, out.detections.as_mut_ptr(), out.cfo.as_mut_ptr(), cap, &mut found);
        if st != COMMS_OK { return Err(to_err(st)); }
        out.detections.truncate(found);
        out.cfo.truncate(found);
        Ok(out)
    }
    pub fn run(&mut self, input: &[Complex<f32>]) -> Result<OfdmDetections, NodeError> {
        self.collect(input.len(), |h, out, cfo, cap, found| unsafe {
            comms_ofdmsync_run(h, input.as_ptr() as *const comms_c32, input.len(), out, cfo, cap, found)
        })
    }
    /// The positions still undecided, as if `window + lag + guard` zero samples followed; the history is zero afterwards.
    pub fn flush(&mut self) -> Result<OfdmDetections, NodeError> {
        self.collect(self.window + self.lag + self.guard, |h, out, cfo, cap, found| unsafe { comms_ofdmsync_flush(h, out, cfo, cap, found) })
    }
    /// The last `window + lag + 2 guard - 1` raw samples, newest first (checkpoints; the halo in front of a stream shard).
    pub fn state(&self) -> Result<Vec<Complex<f32>>, NodeError> {
        let mut n = 0usize;
        let st = unsafe { comms_ofdmsync_state_len(self.lag, self.window, self.guard, &mut n) };
        if st != COMMS_OK { return Err(to_err(st)); }
        let mut state = vec![Complex::new(0.0f32, 0.0f32); n];
        let st = unsafe { comms_ofdmsync_get_state(self.h, state.as_mut_ptr() as *mut comms_c32, n) };
        if st == COMMS_OK { Ok(state) } else { Err(to_err(st)) }
    }
    pub fn set_state(&mut self, state: &[Complex<f32>]) -> Result<(), NodeError> {
        let st = unsafe { comms_ofdmsync_set_state(self.h, state.as_ptr() as *const comms_c32, state.len()) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    /// Stream index of the next sample (checkpoints; the first index of a stream shard).
    pub fn position(&self) -> u64 {
        let mut t = 0u64;
        unsafe { comms_ofdmsync_get_position(self.h, &mut t) };
        t
    }
    pub fn set_position(&mut self, position: u64) -> Result<(), NodeError> {
        let st = unsafe { comms_ofdmsync_set_position(self.h, position) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
    pub fn set_threshold(&mut self, threshold: f64) -> Result<(), NodeError> {
        let st = unsafe { comms_ofdmsync_set_threshold(self.h, threshold) };
        if st == COMMS_OK { Ok(()) } else { Err(to_err(st)) }
    }
}

/// The correct stage of the OFDM synchroniser (comms_ofdmsync_correct_*; an additional node), between `DeframeNode`
/// (`COMMS_SYM_C32`, records of `n_frame` samples) and `OfdmDemodNode`: takes the deframer's message and, on `found`, what
/// `OfdmSyncNode` sent for the same block; sends record f times exp(-i cfo n), all records by one launch, under the same
/// headers.  A frame's offset arrives with its detection and is kept until its record does; a record whose detection was never
/// seen is `NodeError::DataError`.
#[derive(Node)]
#[pass_by_ref]
pub struct OfdmCfoCorrectNode {
    pub input: NodeReceiver<Frames>,
    pub found: NodeReceiver<OfdmDetections>,
    h: *mut comms_ofdmsync_t,
    n_frame: usize,
    pending: Vec<(u64, f64)>,   // (index, cfo) of the detections whose records are still to come, ascending
    pub output: NodeSender<Frames>,
}
handle_node!(OfdmCfoCorrectNode, comms_ofdmsync_destroy);
impl OfdmCfoCorrectNode {
    /// `Err(())`: n_frame outside 1 ..= 2^20.
    pub fn new(n_frame: usize) -> Result<Self, ()> {
        if n_frame == 0 { return Err(()); }
        let mut h = ptr::null_mut();
        let st = unsafe { comms_ofdmsync_create(1, 2, 1.0, 0, 0, n_frame, 0, &mut h) };   // the detect stage of this handle is not used
        if st != COMMS_OK { return Err(()); }
        Ok(OfdmCfoCorrectNode { input: Default::default(), found: Default::default(), h, n_frame, pending: Vec::new(), output: Default::default() })
    }
    /// `records` holds `cfo.len()` records of `n_frame` samples.
    pub fn correct(&mut self, records: &[Complex<f32>], cfo: &[f64]) -> Result<Vec<Complex<f32>>, NodeError> {
        if records.len() != cfo.len() * self.n_frame { return Err(NodeError::DataError); }
        let mut out = vec![Complex::new(0.0f32, 0.0f32); records.len()];
        let st = unsafe {
            comms_ofdmsync_correct_run(self.h, records.as_ptr() as *const comms_c32, cfo.len(), cfo.as_ptr(), out.as_mut_ptr() as *mut comms_c32)
        };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
    pub fn run(&mut self, frames: &Frames, found: &OfdmDetections) -> Result<Frames, NodeError> {
        let n_frames = frames.headers.len();
        let frame_bytes = self.n_frame * size_of::<Complex<f32>>();
        if found.cfo.len() != found.detections.len() || frames.frame_bytes != frame_bytes || frames.data.len() < n_frames * frame_bytes {
            return Err(NodeError::DataError);
        }
        self.pending.extend(found.detections.iter().zip(&found.cfo).map(|(d, &w)| (d.index, w)));
        let mut cfo = Vec::with_capacity(n_frames);
        for hd in &frames.headers {
            match self.pending.iter().position(|&(index, _)| index == hd.index) {
                Some(at) => {
                    cfo.push(self.pending[at].1);
                    self.pending.drain(..=at);   // records come in ascending index: what lies before was dropped by the deframer
                }
                None => return Err(NodeError::DataError),
            }
        }
        let mut out = Frames { data: vec![0u8; n_frames * frame_bytes], headers: frames.headers.clone(), frame_bytes };
        let st = unsafe {
            comms_ofdmsync_correct_run(self.h, frames.data.as_ptr() as *const comms_c32, n_frames, cfo.as_ptr(), out.data.as_mut_ptr() as *mut comms_c32)
        };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// demodulation/nco.rs:118-133 in block form: a vector of phase errors per message.
#[derive(Node)]
#[pass_by_ref]
pub struct BatchNcoNode {
    pub input: NodeReceiver<Vec<f64>>,
    h: *mut comms_nco_t,
    pub output: NodeSender<Vec<Complex<f64>>>,
}
handle_node!(BatchNcoNode, comms_nco_destroy);
impl BatchNcoNode {
    pub fn new(dphase: f64, phase: Option<f64>) -> Self {
        let mut h = ptr::null_mut();
        let st = unsafe { comms_nco_create(dphase, phase.unwrap_or(0.0), 0, &mut h) };
        assert_eq!(st, COMMS_OK, "comms_nco_create failed");
        BatchNcoNode { input: Default::default(), h, output: Default::default() }
    }
    pub fn run(&mut self, perr: &[f64]) -> Result<Vec<Complex<f64>>, NodeError> {
        let mut out = vec![Complex::new(0.0f64, 0.0); perr.len()];
        let st = unsafe { comms_nco_run(self.h, perr.as_ptr(), perr.len(), out.as_mut_ptr() as *mut f64) };
        if st == COMMS_OK { Ok(out) } else { Err(to_err(st)) }
    }
}

/// demodulation/frequency_estimator.rs:27-42, phase_estimator.rs:26-33, :58-65 (free functions there too;
/// they cannot fail there, so a device failure panics here)
pub fn frequency_offset_estimate(samples: &[Complex<f64>]) -> f64 {
    let mut out = 0.0f64;
    let st = unsafe { comms_frequency_offset_estimate(samples.as_ptr() as *const f64, samples.len(), &mut out, 0) };
    assert_eq!(st, COMMS_OK, "comms_frequency_offset_estimate failed");
    out
}
pub fn psk_phase_estimate(symbols: &[Complex<f64>], m: u32) -> f64 {
    let mut out = 0.0f64;
    let st = unsafe { comms_psk_phase_estimate(symbols.as_ptr() as *const f64, symbols.len(), m, &mut out, 0) };
    assert_eq!(st, COMMS_OK, "comms_psk_phase_estimate failed");
    out
}
pub fn qam_phase_estimate(symbols: &[Complex<f64>]) -> f64 {
    let mut out = 0.0f64;
    let st = unsafe { comms_qam_phase_estimate(symbols.as_ptr() as *const f64, symbols.len(), &mut out, 0) };
    assert_eq!(st, COMMS_OK, "comms_qam_phase_estimate failed");
    out
}

/// Device-resident message: `Clone` bumps the library's refcount (the derive macro clones once per sender,
/// node_derive/src/lib.rs:156).  `T` is the element type the bytes are read as.
pub struct DeviceBuf<T> { b: *mut comms_buf_t, pub len: usize, _t: PhantomData<T> }
unsafe impl<T: Send> Send for DeviceBuf<T> {}
impl<T> Clone for DeviceBuf<T> {
    fn clone(&self) -> Self { unsafe { comms_buf_retain(self.b) }; DeviceBuf { b: self.b, len: self.len, _t: PhantomData } }
}
impl<T> Drop for DeviceBuf<T> {
    fn drop(&mut self) { unsafe { comms_buf_release(self.b) }; }
}

/// One stream over several GPUs (host arithmetic of `include/comms_hip.h`, "stream shards"):
/// contiguous shards, and per neighbour pair one hand-over of the raw samples in front of the shard.  The
/// library moves no samples between GPUs itself: the host passes the halo with its own transport (RCCL
/// send / recv, MPI, a channel between node threads) and calls these three around it.
pub mod shard {
    use super::*;
    /// `[start, stop)` of `rank`'s share of `total` units (samples, or FFT transforms)
    pub fn range(total: usize, world: u32, rank: u32) -> (usize, usize) {
        let (mut a, mut b) = (0usize, 0usize);
        let st = unsafe { comms_shard_range(total, world, rank, &mut a, &mut b) };
        assert_eq!(st, COMMS_OK, "comms_shard_range failed");
        (a, b)
    }
    /// the samples before a shard (time order, as many as taps) -> `BatchFirNode::new(taps, Some(state))`
    pub fn state_from_halo(halo: &[Complex<f32>]) -> Vec<Complex<f32>> {
        let mut state = vec![Complex::new(0.0f32, 0.0); halo.len()];
        let st = unsafe { comms_state_from_halo(halo.as_ptr(), halo.len(), state.as_mut_ptr()) };
        assert_eq!(st, COMMS_OK, "comms_state_from_halo failed");
        state
    }
    /// oscillator phase of stream sample `first_index` -> `MixerNode::new(dphase, Some(phase))` of the shard's node
    pub fn mixer_phase(phase0: f64, dphase: f64, first_index: i64) -> f64 {
        let mut ph = 0.0f64;
        let st = unsafe { comms_shard_mixer_phase(phase0, dphase, first_index, &mut ph) };
        assert_eq!(st, COMMS_OK, "comms_shard_mixer_phase failed");
        ph
    }
    /// raw samples a fused chain shard runs through first (outputs dropped): FIR history + the sample FM.prev comes from
    pub fn chain_prefix_len(n_taps: usize, rate: usize, fm_demod: bool) -> usize {
        let mut n = 0usize;
        let st = unsafe { comms_chain_prefix_len(n_taps, rate, fm_demod as i32, &mut n) };
        assert_eq!(st, COMMS_OK, "comms_chain_prefix_len failed");
        n
    }
}
