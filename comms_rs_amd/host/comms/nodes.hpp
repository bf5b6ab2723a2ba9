// nodes.hpp -- the hot-path DSP nodes of comms-rs, backed by libcomms_hip (MI355X).
//
// Same struct names, constructor arguments and public `input` / `output` fields as
// the reference, so a graph written against comms-rs
// reads the same here:
//   FirNode / BatchFirNode::new(taps, state)      src/filter/fir_node.rs:89, :193
//   FFTBatchNode / FFTSampleNode::new(size, ifft) src/fft/fft_node.rs:65, :142
//   MixerNode::new(dphase, phase)                 src/mixer.rs:128
//   PulseNode::new(taps, sam_per_sym)             src/pulse.rs:71
//   DecimateNode / UpsampleNode::new(rate)        src/util/resample_node.rs:23, :87
//   FMDemodNode::new()                            src/modulation/analog_node.rs:43
//   TimingEstimatorNode::new(n, d, alpha)         src/demodulation/timing_estimator.rs:123
//   NcoNode::new(dphase, phase) (block form)      src/demodulation/nco.rs:118
//   PrnsNode::new(poly_mask, state)               src/prns.rs:93-137
//   NormalNode::new(mu, std_dev), UniformNode<T>::new(start, end), random_bit()   src/util/rand_node.rs:60, :124, :150
//
// How the header is built:
//   Owned<H, Destroy>   the one owner of an opaque comms_*_t*; create<>() runs a *_create entry into it.  No class here
//                       writes a move constructor or a destructor for a handle: moves are implicit or `= default`.
//   a description       (FirOp, ChainOp, RealFirDecimOp, SymbolSyncOp ...) states once what is particular to an operation:
//                       its handle and parameters, prepare(n, m) -- what precedes a launch, m = the output length --, the
//                       host-pointer entry launch(), the *_run_dev entry launch_dev(), and its extras as public members
//                       (kernel(n), channels(), fused_kind(), flush(), the `update` channel).
//   Ports<In, Out>      the `input` / `output` fields with receivers() / senders(), and the teardown order: handle, stream, channels.
//   HostNode<D, Op>     turns a description into the node on std::vector messages: every run() goes H2D -> kernel -> D2H
//                       through the C ABI, messages moved through the channels by value as in the reference.
//   DevNode<D, Op>      turns it into the node on device-resident messages (DeviceBuf<T>, clone = refcount bump) on a stream
//                       of its own -- what the roofline numbers use.
// The public node types are thin: a constructor with the reference's parameter list, and the name its errors carry.
// Sources, per-sample nodes (run_block) and the nodes whose output is a host value have run() bodies of their own over the
// same descriptions and the same owner.
//
// Error convention: comms_status_t 1 -> NodeError::DataError, 2 -> PermanentError.
// Constructors throw std::runtime_error when a handle cannot be created (the
// reference panics in the same places); there is no CPU fallback.
#pragma once

#include <cmath>
#include <limits>
#include <complex>
#include <cstring>
#include <memory>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../../include/comms_hip.h"
#include "node.hpp"

namespace comms {

using Complex32 = std::complex<float>;
static_assert(sizeof(Complex32) == sizeof(comms_c32), "Complex<f32> must be interleaved {re, im}");

inline const comms_c32* c32(const Complex32* p) { return reinterpret_cast<const comms_c32*>(p); }
inline comms_c32* c32(Complex32* p) { return reinterpret_cast<comms_c32*>(p); }
using Complex64 = std::complex<double>;  // num::Complex<f64>
static_assert(sizeof(Complex64) == sizeof(comms_c64), "Complex<f64> must be interleaved {re, im}");
inline const comms_c64* c64(const Complex64* p) { return reinterpret_cast<const comms_c64*>(p); }
inline comms_c64* c64(Complex64* p) { return reinterpret_cast<comms_c64*>(p); }

inline void throw_on(comms_status_t st, const char* what) {
    if (st != COMMS_OK) throw std::runtime_error(std::string(what) + ": " + comms_last_error());
}
inline NodeError to_node_error(comms_status_t st) {
    return st == COMMS_ERR_ARG ? NodeError::DataError : NodeError::PermanentError;
}
// what a run() returns: `out` (moved from) when the C call succeeded, its NodeError otherwise
template <class T>
Result<T> ok_or(comms_status_t st, T& out) {
    if (st != COMMS_OK) return to_node_error(st);
    return std::move(out);
}

// ---------------------------------------------------------------- handle ownership
// The owner of an opaque C handle: move-only, released through the handle's comms_*_destroy entry.
template <auto Destroy>
struct Destroyer {
    template <class H>
    void operator()(H* h) const { Destroy(h); }
};
template <class H, auto Destroy>
using Owned = std::unique_ptr<H, Destroyer<Destroy>>;

// runs a *_create entry (its last argument receives the handle) into the owner O; a failure throws "<who>: <last error>".
// A constructor that throws after this still releases the handle: the owner is a member by then.
template <class O, class F, class... A>
O create(const char* who, F make, A... args) {
    typename O::pointer h = nullptr;
    throw_on(make(args..., &h), who);
    return O(h);
}

// the *_get_kernel entries: what a handle launches for n samples, as text ("<kernel><..> ...", or "series: ..." for the launches
// of a fallback)
template <class F, class H>
std::string kernel_name(F get_kernel, const H* h, size_t n) {
    char name[240] = {0};
    get_kernel(h, n, name, sizeof name);
    return name;
}

// ---------------------------------------------------------------- device-resident message
template <class T>
class DeviceBuf {
public:
    DeviceBuf() = default;
    explicit DeviceBuf(size_t count, int device = 0) : count_(count) {
        throw_on(comms_buf_alloc(count * sizeof(T), device, &b_), "comms_buf_alloc");
    }
    DeviceBuf(const DeviceBuf& o) : b_(o.b_), count_(o.count_) {  // Clone = retain
        if (b_) comms_buf_retain(b_);
    }
    DeviceBuf(DeviceBuf&& o) noexcept : b_(o.b_), count_(o.count_) { o.b_ = nullptr; }
    DeviceBuf& operator=(DeviceBuf o) noexcept {
        std::swap(b_, o.b_);
        std::swap(count_, o.count_);
        return *this;
    }
    ~DeviceBuf() {
        if (b_) comms_buf_release(b_);
    }
    static DeviceBuf from_host(const std::vector<T>& v, int device = 0) {
        DeviceBuf d(v.size(), device);
        throw_on(comms_buf_upload(d.b_, 0, v.data(), v.size() * sizeof(T)), "comms_buf_upload");
        return d;
    }
    std::vector<T> to_host() const {
        std::vector<T> v(count_);
        throw_on(comms_buf_download(b_, 0, v.data(), count_ * sizeof(T)), "comms_buf_download");
        return v;
    }
    T* ptr() const { return static_cast<T*>(comms_buf_ptr(b_)); }
    comms_buf_t* raw() const { return b_; }  // for comms_buf_{wait_ready,record_use,record_ready}
    size_t size() const { return count_; }
    int device() const { return comms_buf_device(b_); }

private:
    comms_buf_t* b_ = nullptr;
    size_t count_ = 0;
};

// ---------------------------------------------------------------- the two shells
// A description Op has
//     using In, Out;                                      element types of a message
//     Op(const char* who, <its parameters>);              creates the handle; `who` names the node in the error
//     comms_status_t prepare(size_t n, size_t& m);        what precedes the launch of an n-element message; m = its output length
//     comms_status_t launch(const In*, size_t n, Out*);               the host-pointer entry (synchronous)
//     comms_status_t launch_dev(const In*, size_t n, Out*, void* s);  the *_run_dev entry on stream s
// (the three protected), and whatever else is public on the node.  A shell derives from it, so the extras need no forwarding.

// The channel fields of a one-in / one-out node, and how DeriveNode finds them.  First among a node's bases, so it goes last:
// a node releases its handle before its senders disconnect, and a consumer that sees its channel end finds the producer's
// device work over.
template <class In, class Out>
struct Ports {
    NodeReceiver<In> input;
    NodeSender<Out> output;
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }
};

struct SameLength {  // prepare() of the operations that give one output element per input element
    comms_status_t prepare(size_t n, size_t& m) const {
        m = n;
        return COMMS_OK;
    }
};

// The node on host vectors.  D is the public node type (what DeriveNode wants).
template <class D, class Op>
class HostNode : public DeriveNode<D>, public Ports<std::vector<typename Op::In>, std::vector<typename Op::Out>>, public Op {
public:
    template <class... A>
    explicit HostNode(const char* who, A&&... a) : Op(who, std::forward<A>(a)...) {}
    HostNode(HostNode&&) = default;  // a node is moved into its thread, never copied

    Result<std::vector<typename Op::Out>> run(const std::vector<typename Op::In>& in) {
        size_t m = 0;
        comms_status_t st = Op::prepare(in.size(), m);
        if (st != COMMS_OK) return to_node_error(st);
        std::vector<typename Op::Out> out(m);
        return ok_or(Op::launch(in.data(), in.size(), out.data()), out);
    }
};

// Device-resident messages are DeviceBuf<T>: nothing crosses PCIe between nodes and nothing ever synchronises
// the device.  Every node owns a stream (DevStream); run() is
//     wait_ready(in)  ->  one asynchronous launch on the node's stream  ->  record_use(in),
//     record_ready(out)  ->  send(out)
// so the consumer's stream starts its own launch only after the producer's has finished, while the
// node threads themselves run ahead of the device.  An edge stays on ONE GPU: the buffer's events
// belong to its device and the kernels read it directly, so a message whose device is not the node's is a
// DataError (COMMS_ERR_ARG) -- between GPUs the host copies or sends the samples itself (sharding, below).  Output
// buffers come from the library's cache (no hipMalloc / hipFree in steady state); a buffer's
// memory is recycled only after the launches that read it.  to_host() waits for the producer.
class DevStream {
public:
    explicit DevStream(int device) : s_(nullptr, Retire{device}) {
        void* s = nullptr;
        throw_on(comms_stream_create(device, &s), "comms_stream_create");
        s_.reset(s);
    }
    // the producer of `in` has finished before anything later on this stream starts (no host wait); no cross-device edges
    template <class T>
    comms_status_t wait(const DeviceBuf<T>& in) const {
        return in.device() != device() ? COMMS_ERR_ARG : comms_buf_wait_ready(in.raw(), get());
    }
    // `launch(stream)` is the node's *_run_dev call
    template <class TI, class TO, class F>
    comms_status_t submit(const DeviceBuf<TI>& in, DeviceBuf<TO>& out, F&& launch) const {
        comms_status_t st = out.device() != device() ? COMMS_ERR_ARG : wait(in);
        if (st == COMMS_OK) st = launch(get());
        if (st == COMMS_OK) st = comms_buf_record_use(in.raw(), get());
        if (st == COMMS_OK) st = comms_buf_record_ready(out.raw(), get());
        return st;
    }
    void* get() const { return s_.get(); }
    int device() const { return s_.get_deleter().device; }

private:
    struct Retire {
        int device;
        void operator()(void* s) const {
            comms_stream_synchronize(device, s);
            comms_stream_destroy(device, s);
        }
    };
    std::unique_ptr<void, Retire> s_;
};

// A description on a stream of its own: the one place where a device node is put together.
template <class Op>
struct OnStream : protected DevStream, public Op {  // bases go in reverse order: the handle, whose destroy quiesces this stream, before the stream
    template <class... A>
    explicit OnStream(int device, const char* who, A&&... a) : DevStream(device), Op(who, std::forward<A>(a)...) {}
};

// The node on device-resident messages.
template <class D, class Op>
class DevNode : public DeriveNode<D>, public Ports<DeviceBuf<typename Op::In>, DeviceBuf<typename Op::Out>>, public OnStream<Op> {
public:
    using OnStream<Op>::OnStream;
    DevNode(DevNode&&) = default;

    Result<DeviceBuf<typename Op::Out>> run(const DeviceBuf<typename Op::In>& in) {
        size_t m = 0;
        comms_status_t st = Op::prepare(in.size(), m);
        if (st != COMMS_OK) return to_node_error(st);
        DeviceBuf<typename Op::Out> out(m, this->device());
        return ok_or(this->submit(in, out, [&](void* s) { return Op::launch_dev(in.ptr(), in.size(), out.ptr(), s); }), out);
    }
};

// ---------------------------------------------------------------- sample types
// What the C ABI offers per sample type, as the Rust shim's FirSample / MixSample / SpectralSample traits have it: the
// interleaved {re, im} struct, the handle types and the entry points.  Complex<i16> (wrapping arithmetic) has the FIR and
// the pulse shaper only; the *_run_dev entries are bound where a device-resident node uses them (Complex<f32>).
using Complex16 = std::complex<int16_t>;
static_assert(sizeof(Complex16) == sizeof(comms_c16), "Complex<i16> must be interleaved {re, im}");
inline const comms_c16* c16(const Complex16* p) { return reinterpret_cast<const comms_c16*>(p); }
inline comms_c16* c16(Complex16* p) { return reinterpret_cast<comms_c16*>(p); }

template <class T>
struct Sample;
template <>
struct Sample<Complex32> {
    using Abi = comms_c32;
    using Real = float;
    using Fir = comms_fir_t;
    using Pulse = comms_pulse_t;
    using Fft = comms_fft_t;
    using Fm = comms_fmdemod_t;
    static constexpr auto fir_create = comms_fir_create;
    static constexpr auto fir_run = comms_fir_run;
    static constexpr auto fir_run_dev = comms_fir_run_dev;
    static constexpr auto fir_destroy = comms_fir_destroy;
    static constexpr auto pulse_create = comms_pulse_create;
    static constexpr auto pulse_run = comms_pulse_run;
    static constexpr auto pulse_run_dev = comms_pulse_run_dev;
    static constexpr auto pulse_destroy = comms_pulse_destroy;
    static constexpr auto mixer_run = comms_mixer_run;
    static constexpr auto mixer_run_dev = comms_mixer_run_dev;
    static constexpr auto fft_create = comms_fft_create;
    static constexpr auto fft_run = comms_fft_run;
    static constexpr auto fft_run_dev = comms_fft_run_dev;
    static constexpr auto fft_destroy = comms_fft_destroy;
    static constexpr auto fm_create = comms_fmdemod_create;
    static constexpr auto fm_run = comms_fmdemod_run;
    static constexpr auto fm_run_dev = comms_fmdemod_run_dev;
    static constexpr auto fm_destroy = comms_fmdemod_destroy;
};
template <>
struct Sample<Complex16> {
    using Abi = comms_c16;
    using Fir = comms_fir_i16_t;
    using Pulse = comms_pulse_i16_t;
    static constexpr auto fir_create = comms_fir_i16_create;
    static constexpr auto fir_run = comms_fir_i16_run;
    static constexpr auto fir_destroy = comms_fir_i16_destroy;
    static constexpr auto pulse_create = comms_pulse_i16_create;
    static constexpr auto pulse_run = comms_pulse_i16_run;
    static constexpr auto pulse_destroy = comms_pulse_i16_destroy;
};
template <>
struct Sample<Complex64> {
    using Abi = comms_c64;
    using Real = double;
    using Fir = comms_fir_f64_t;
    using Pulse = comms_pulse_f64_t;
    using Fft = comms_fft_f64_t;
    using Fm = comms_fmdemod_f64_t;
    static constexpr auto fir_create = comms_fir_f64_create;
    static constexpr auto fir_run = comms_fir_f64_run;
    static constexpr auto fir_destroy = comms_fir_f64_destroy;
    static constexpr auto pulse_create = comms_pulse_f64_create;
    static constexpr auto pulse_run = comms_pulse_f64_run;
    static constexpr auto pulse_destroy = comms_pulse_f64_destroy;
    static constexpr auto mixer_run = comms_mixer_run_f64;
    static constexpr auto fft_create = comms_fft_f64_create;
    static constexpr auto fft_run = comms_fft_f64_run;
    static constexpr auto fft_destroy = comms_fft_f64_destroy;
    static constexpr auto fm_create = comms_fmdemod_f64_create;
    static constexpr auto fm_run = comms_fmdemod_f64_run;
    static constexpr auto fm_destroy = comms_fmdemod_f64_destroy;
};
template <class T>
const typename Sample<T>::Abi* abi(const T* p) { return reinterpret_cast<const typename Sample<T>::Abi*>(p); }
template <class T>
typename Sample<T>::Abi* abi(T* p) { return reinterpret_cast<typename Sample<T>::Abi*>(p); }

// ---------------------------------------------------------------- FIR
// The node templates below take the public node type D (what DeriveNode wants, and D::kNew names the node when its
// constructor throws) and the sample type T.  The public names follow each group.
template <class T>
struct FirOp : protected SameLength {
    using In = T;
    using Out = T;
    FirOp(const char* who, const std::vector<T>& taps, const std::optional<std::vector<T>>& state, int device)
        : h_(create<decltype(h_)>(who, Sample<T>::fir_create, abi(taps.data()), taps.size(), state ? abi(state->data()) : nullptr,
                                  state ? state->size() : 0, device)) {}

protected:
    comms_status_t launch(const T* in, size_t n, T* out) { return Sample<T>::fir_run(h_.get(), abi(in), n, abi(out)); }
    comms_status_t launch_dev(const T* in, size_t n, T* out, void* s) { return Sample<T>::fir_run_dev(h_.get(), abi(in), n, abi(out), s); }
    Owned<typename Sample<T>::Fir, Sample<T>::fir_destroy> h_;
};

template <class D, class T>
class BatchFirNodeOf : public HostNode<D, FirOp<T>> {
public:
    BatchFirNodeOf(const std::vector<T>& taps, const std::optional<std::vector<T>>& state = std::nullopt, int device = 0)
        : BatchFirNodeOf::HostNode(D::kNew, taps, state, device) {}
    typename Sample<T>::Fir* handle() const { return this->h_.get(); }
};

template <class D, class T>
class FirNodeOf : public DeriveNode<D>, public Ports<T, T>, public FirOp<T> {
public:
    FirNodeOf(const std::vector<T>& taps, const std::optional<std::vector<T>>& state = std::nullopt, int device = 0)
        : FirOp<T>(D::kNew, taps, state, device) {}

    Result<T> run(const T& in) {
        T out;
        return ok_or(this->launch(&in, 1, &out), out);
    }
    // the samples already queued behind the first one, in one launch (DeriveNode::call): the
    // filter's state runs through the block exactly as through the same samples one by one
    Result<std::vector<T>> run_block(const std::vector<T>& ins) {
        std::vector<T> out(ins.size());
        return ok_or(this->launch(ins.data(), ins.size(), out.data()), out);
    }
};

// ---------------------------------------------------------------- pulse shaping
// T is the sample type of the taps (and of the handle).  A message holds symbols of type T, or -- bits_per_sym 1 or 2 -- packed
// bits, LSB first, whole bytes; sam_per_sym outputs per symbol.
template <class T, class I = T, class O = T>
struct PulseOp {
    using In = I;
    using Out = O;
    PulseOp(const char* who, const std::vector<T>& taps, size_t sam_per_sym, int device, int bits_per_sym = 0)
        : h_(create<decltype(h_)>(who, Sample<T>::pulse_create, abi(taps.data()), taps.size(), sam_per_sym, device)),
          sps_(sam_per_sym),
          k_(bits_per_sym) {}

protected:
    size_t symbols(size_t n) const { return k_ ? n * 8 / static_cast<size_t>(k_) : n; }
    comms_status_t prepare(size_t n, size_t& m) const {
        m = symbols(n) * sps_;
        return COMMS_OK;
    }
    comms_status_t launch(const In* in, size_t n, Out* out) {
        return Sample<T>::pulse_run(h_.get(), reinterpret_cast<const typename Sample<T>::Abi*>(in), symbols(n),
                                    reinterpret_cast<typename Sample<T>::Abi*>(out));
    }
    comms_status_t launch_dev(const In* in, size_t n, Out* out, void* s) {
        return Sample<T>::pulse_run_dev(h_.get(), reinterpret_cast<const typename Sample<T>::Abi*>(in), symbols(n),
                                        reinterpret_cast<typename Sample<T>::Abi*>(out), s);
    }
    Owned<typename Sample<T>::Pulse, Sample<T>::pulse_destroy> h_;
    size_t sps_;
    int k_;
};

template <class D, class T>
class PulseNodeOf : public DeriveNode<D>, public Ports<T, std::vector<T>>, public PulseOp<T> {
public:
    PulseNodeOf(const std::vector<T>& taps, size_t sam_per_sym, int device = 0) : PulseOp<T>(D::kNew, taps, sam_per_sym, device) {}

    Result<std::vector<T>> run(const T& sym) {
        std::vector<T> out(this->sps_);
        return ok_or(this->launch(&sym, 1, out.data()), out);
    }
    // queued symbols in one launch; still one Vec of sam_per_sym samples per symbol downstream
    Result<std::vector<std::vector<T>>> run_block(const std::vector<T>& syms) {
        const size_t sps = this->sps_;
        std::vector<T> flat(syms.size() * sps);
        comms_status_t st = this->launch(syms.data(), syms.size(), flat.data());
        if (st != COMMS_OK) return to_node_error(st);
        std::vector<std::vector<T>> out(syms.size());
        for (size_t i = 0; i < syms.size(); ++i) out[i].assign(flat.begin() + i * sps, flat.begin() + (i + 1) * sps);
        return out;
    }
};

// f32: every BASELINE config, the tuned kernels (comms_fir_*, comms_pulse_*)
struct BatchFirNode : BatchFirNodeOf<BatchFirNode, Complex32> {
    using BatchFirNodeOf::BatchFirNodeOf;
    static constexpr const char* kNew = "BatchFirNode::new";
};
struct FirNode : FirNodeOf<FirNode, Complex32> {
    using FirNodeOf::FirNodeOf;
    static constexpr const char* kNew = "FirNode::new";
};
struct PulseNode : PulseNodeOf<PulseNode, Complex32> {
    using PulseNodeOf::PulseNodeOf;
    static constexpr const char* kNew = "PulseNode::new";
    // transmit chain in one launch: the MixerNode::new(dphase, phase) that follows is fused in
    // (the i16 store stage, comms_pulse_set_output_format, is offered on the device-resident node below)
    PulseNode& with_mixer(double dphase, std::optional<double> phase = std::nullopt) {
        throw_on(comms_pulse_set_mixer(h_.get(), dphase, phase.value_or(0.0)), "PulseNode::with_mixer");
        return *this;
    }
};
class BatchFirNodeDev : public DevNode<BatchFirNodeDev, FirOp<Complex32>> {
public:
    BatchFirNodeDev(const std::vector<Complex32>& taps, const std::optional<std::vector<Complex32>>& state = std::nullopt, int device = 0)
        : DevNode(device, "BatchFirNodeDev::new", taps, state, device) {}
};
// PulseNode over whole symbol blocks: n symbols in, n * sam_per_sym samples out
class BatchPulseNodeDev : public DevNode<BatchPulseNodeDev, PulseOp<Complex32>> {
public:
    BatchPulseNodeDev(const std::vector<Complex32>& taps, size_t sam_per_sym, int device = 0)
        : DevNode(device, "BatchPulseNodeDev::new", taps, sam_per_sym, device) {}
    BatchPulseNodeDev& with_mixer(double dphase, std::optional<double> phase = std::nullopt) {
        throw_on(comms_pulse_set_mixer(h_.get(), dphase, phase.value_or(0.0)), "BatchPulseNodeDev::with_mixer");
        return *this;
    }
};

// Complex<i16>: the reference's nodes are generic over the sample type and its own tests run on Complex<i16>
// (fir_node.rs:259-313, pulse.rs:129-183); wrapping arithmetic (comms_fir_i16_*, comms_pulse_i16_*)
struct BatchFirNodeI16 : BatchFirNodeOf<BatchFirNodeI16, Complex16> {
    using BatchFirNodeOf::BatchFirNodeOf;
    static constexpr const char* kNew = "BatchFirNode<i16>::new";
};
struct FirNodeI16 : FirNodeOf<FirNodeI16, Complex16> {
    using FirNodeOf::FirNodeOf;
    static constexpr const char* kNew = "FirNode<i16>::new";
};
struct PulseNodeI16 : PulseNodeOf<PulseNodeI16, Complex16> {
    using PulseNodeOf::PulseNodeOf;
    static constexpr const char* kNew = "PulseNode<i16>::new";
};

// Complex<f64>: the reference's own doc example of batch_fir (fir.rs:68-86) and its timing estimator
// (timing_estimator.rs:102-103) run on Complex<f64>; the reference's arithmetic operation for operation, outputs
// bit-identical to it (comms_fir_f64_*, comms_pulse_f64_*)
struct BatchFirNodeF64 : BatchFirNodeOf<BatchFirNodeF64, Complex64> {
    using BatchFirNodeOf::BatchFirNodeOf;
    static constexpr const char* kNew = "BatchFirNode<f64>::new";
};
struct FirNodeF64 : FirNodeOf<FirNodeF64, Complex64> {
    using FirNodeOf::FirNodeOf;
    static constexpr const char* kNew = "FirNode<f64>::new";
};
struct PulseNodeF64 : PulseNodeOf<PulseNodeF64, Complex64> {
    using PulseNodeOf::PulseNodeOf;
    static constexpr const char* kNew = "PulseNode<f64>::new";
};

// ---------------------------------------------------------------- PRNS source
// A source node (no input): run() returns the next bit of the LFSR (prns.rs:131-133), as the reference.  The bits are
// generated on the device kBlock at a time and handed out one per run(); state() is the register before the NEXT bit
// run() returns (the handle itself has already advanced past the block -- comms_prns_skip makes that exact and
// host-only).  width = 8, 16, 32 or 64 (PrnsNode<u8/u16/u32/u64>).
class PrnsNode : public DeriveNode<PrnsNode> {
public:
    NodeSender<uint8_t> output;
    static constexpr size_t kBlock = 4096;

    PrnsNode(uint64_t poly_mask, uint64_t state, int width = 8, int device = 0)
        : h_(create<decltype(h_)>("PrnsNode::new", comms_prns_create, poly_mask, state, width, device)), start_(state) {}

    Result<uint8_t> run() {
        if (pos_ == buf_.size()) {
            uint64_t s = 0;
            comms_status_t st = comms_prns_get_state(h_.get(), &s);
            buf_.resize(kBlock);
            if (st == COMMS_OK) st = comms_prns_run(h_.get(), kBlock, COMMS_BITS_U8, buf_.data());
            if (st != COMMS_OK) {
                buf_.clear();
                pos_ = 0;
                return to_node_error(st);
            }
            start_ = s;
            pos_ = 0;
        }
        return buf_[pos_++];
    }
    // the register before the next bit run() returns (PrnGen's `state`)
    uint64_t state() {
        uint64_t ahead = 0, s = 0;
        throw_on(comms_prns_get_state(h_.get(), &ahead), "PrnsNode::state");
        throw_on(comms_prns_set_state(h_.get(), start_), "PrnsNode::state");
        throw_on(comms_prns_skip(h_.get(), pos_), "PrnsNode::state");
        throw_on(comms_prns_get_state(h_.get(), &s), "PrnsNode::state");
        throw_on(comms_prns_set_state(h_.get(), ahead), "PrnsNode::state");
        return s;
    }
    auto receivers() { return std::tie(); }
    auto senders() { return std::tie(output); }

private:
    Owned<comms_prns_t, comms_prns_destroy> h_;
    std::vector<uint8_t> buf_;
    size_t pos_ = 0;
    uint64_t start_ = 0;  // register at buf_[0]
};

// ---------------------------------------------------------------- random sources (util/rand_node.rs) and the AWGN channel
// NormalNode::new(mu, std_dev), UniformNode<T>::new(start, end) and random_bit() with the reference's names and argument
// order.  The reference seeds a host generator from entropy (StdRng::from_entropy, rand_node.rs:61,125); here the values
// come from the library's counter-based source (comms_noise_*, stream 0 of `seed`), and without a seed one is drawn from
// std::random_device.  As source nodes they keep the reference's run(): one value per call, handed out of a block drawn
// in one launch; run_block(n) returns the next n values of the same sequence in (at most) one launch.
inline uint64_t entropy_seed() {
    std::random_device rd;
    return (static_cast<uint64_t>(rd()) << 32) | static_cast<uint64_t>(rd());
}
using NoiseHandle = Owned<comms_noise_t, comms_noise_destroy>;

// CRTP base: D::draw(n, out) draws n values (n a multiple of D::kGrain) from the stream position
template <class D, class T>
class NoiseSourceNode : public DeriveNode<D> {
public:
    NodeSender<T> output;
    static constexpr size_t kBlock = 4096;

    NoiseSourceNode(std::optional<uint64_t> seed, int device, const char* what)
        : seed_(seed ? *seed : entropy_seed()), h_(create<NoiseHandle>(what, comms_noise_create, seed_, uint64_t(0), device)) {}

    Result<T> run() {
        if (pos_ == buf_.size()) {
            comms_status_t st = refill(kBlock);
            if (st != COMMS_OK) return to_node_error(st);
        }
        return buf_[pos_++];
    }
    // the next n values of the sequence run() hands out, drawn in one launch (what is left of run()'s block goes first)
    Result<std::vector<T>> run_block(size_t n) {
        std::vector<T> out(buf_.begin() + static_cast<std::ptrdiff_t>(pos_), buf_.end());
        if (out.size() >= n) {
            out.resize(n);
            pos_ += n;
            return out;
        }
        const size_t need = n - out.size();
        comms_status_t st = refill((need + D::kGrain - 1) / D::kGrain * D::kGrain);
        if (st != COMMS_OK) return to_node_error(st);
        out.insert(out.end(), buf_.begin(), buf_.begin() + static_cast<std::ptrdiff_t>(need));
        pos_ = need;
        return out;
    }
    uint64_t seed() const { return seed_; }
    auto receivers() { return std::tie(); }
    auto senders() { return std::tie(output); }

private:
    uint64_t seed_;  // before h_: the create reads it

protected:
    NoiseHandle h_;

private:
    comms_status_t refill(size_t n) {
        buf_.resize(n);
        pos_ = 0;
        comms_status_t st = static_cast<D&>(*this).draw(n, buf_.data());
        if (st != COMMS_OK) buf_.clear();
        return st;
    }
    std::vector<T> buf_;
    size_t pos_ = 0;
};

class NormalNode : public NoiseSourceNode<NormalNode, double> {
public:
    static constexpr size_t kGrain = 1;
    NormalNode(double mu, double std_dev, std::optional<uint64_t> seed = std::nullopt, int device = 0)
        : NoiseSourceNode(seed, device, "NormalNode::new"), mu_(mu), sd_(std_dev) {
        if (!(std_dev >= 0.0) || !std::isfinite(std_dev) || !std::isfinite(mu)) throw std::runtime_error("NormalNode::new: std_dev < 0 or not finite");
    }
    comms_status_t draw(size_t n, double* out) { return comms_noise_normal_f64_run(h_.get(), n, mu_, sd_, out); }

private:
    double mu_, sd_;
};

template <class T>
class UniformNode;

// UniformNode<f32>: values in [start, end)
template <>
class UniformNode<float> : public NoiseSourceNode<UniformNode<float>, float> {
public:
    static constexpr size_t kGrain = 1;
    UniformNode(float start, float end, std::optional<uint64_t> seed = std::nullopt, int device = 0)
        : NoiseSourceNode(seed, device, "UniformNode::new"), lo_(start), hi_(end) {
        if (!(start < end) || !std::isfinite(start) || !std::isfinite(end)) throw std::runtime_error("UniformNode::new: start >= end");  // Uniform::new panics
    }
    comms_status_t draw(size_t n, float* out) { return comms_noise_uniform_run(h_.get(), n, lo_, hi_, out); }

private:
    float lo_, hi_;
};

// UniformNode<u8> over [0, 2): what random_bit() returns (rand_node.rs:150-152) -- the bit draw of the source
template <>
class UniformNode<uint8_t> : public NoiseSourceNode<UniformNode<uint8_t>, uint8_t> {
public:
    static constexpr size_t kGrain = 32;  // a bit draw consumes whole 32-bit words
    UniformNode(uint8_t start, uint8_t end, std::optional<uint64_t> seed = std::nullopt, int device = 0)
        : NoiseSourceNode(seed, device, "UniformNode::new") {
        if (start != 0 || end != 2) throw std::runtime_error("UniformNode<u8>::new: only the range [0, 2) of random_bit() is implemented");
    }
    comms_status_t draw(size_t n, uint8_t* out) { return comms_noise_bits_run(h_.get(), n, COMMS_BITS_U8, out); }
};

inline UniformNode<uint8_t> random_bit(std::optional<uint64_t> seed = std::nullopt, int device = 0) {
    return UniformNode<uint8_t>(0, 2, seed, device);
}

// AWGN channel (an additional node): out = in + sigma * (z + i z'), one complex standard pair per sample, the pairs of
// consecutive messages consecutive in the source's stream (comms_awgn_run)
struct AwgnOp : protected SameLength {
    using In = Complex32;
    using Out = Complex32;
    AwgnOp(const char* who, float sigma, std::optional<uint64_t> seed, uint64_t stream, int device)
        : h_(create<NoiseHandle>(who, comms_noise_create, seed ? *seed : entropy_seed(), stream, device)), sigma_(sigma) {}

protected:
    comms_status_t launch(const Complex32* in, size_t n, Complex32* out) { return comms_awgn_run(h_.get(), in, n, sigma_, c32(out)); }
    comms_status_t launch_dev(const Complex32* in, size_t n, Complex32* out, void* s) {
        return comms_awgn_run_dev(h_.get(), in, n, sigma_, c32(out), s);
    }
    NoiseHandle h_;
    float sigma_;
};
class AwgnNode : public HostNode<AwgnNode, AwgnOp> {
public:
    AwgnNode(float sigma, std::optional<uint64_t> seed = std::nullopt, uint64_t stream = 0, int device = 0)
        : HostNode("AwgnNode::new", sigma, seed, stream, device) {}
};
class AwgnNodeDev : public DevNode<AwgnNodeDev, AwgnOp> {
public:
    AwgnNodeDev(float sigma, std::optional<uint64_t> seed = std::nullopt, uint64_t stream = 0, int device = 0)
        : DevNode(device, "AwgnNodeDev::new", sigma, seed, stream, device) {}
};

// ---------------------------------------------------------------- a digital link from bits to bits (additional nodes)
// Transmit: packed bits (LSB first, bits_per_sym = 1 or 2 per symbol, whole bytes per message) -> constellation -> pulse
// shaping -> mixer -> (scale * y) as i16, one launch per message (comms_pulse_set_input_format / _set_output_format).
class PulseBitsNode : public HostNode<PulseBitsNode, PulseOp<Complex32, uint8_t, Complex16>> {
public:
    PulseBitsNode(const std::vector<Complex32>& taps, size_t sam_per_sym, int bits_per_sym, double dphase, float scale,
                  const std::vector<Complex32>& constellation = {}, int device = 0)
        : HostNode("PulseBitsNode::new", taps, sam_per_sym, device, bits_per_sym) {
        throw_on(comms_pulse_set_mixer(h_.get(), dphase, 0.0), "PulseBitsNode::new");
        throw_on(comms_pulse_set_input_format(h_.get(), COMMS_SYM_BITS, bits_per_sym, constellation.empty() ? nullptr : c32(constellation.data())),
                 "PulseBitsNode::new");
        throw_on(comms_pulse_set_output_format(h_.get(), COMMS_IQ_I16, scale), "PulseBitsNode::new");
    }
};

// mixer / FIR / decimate [/ FM demod] as ONE launch (comms_chain_*; additional nodes, the results of the reference nodes in
// series).  A message is a whole number of decimation periods.  In: Complex32, or what comms_chain_set_input_format names;
// Out: Complex32, float with FM demod, or -- bits_per_sym 1 or 2 -- the hard decisions as packed bits, LSB first, each message
// from bit 0 of its first byte.
template <class I, class O>
struct ChainOp {
    using In = I;
    using Out = O;
    ChainOp(const char* who, double dphase, double phase, const std::vector<Complex32>& taps, size_t rate, int32_t flags, int device,
            int bits_per_sym = 0)
        : h_(create<decltype(h_)>(who, comms_chain_create_ex, dphase, phase, c32(taps.data()), taps.size(), rate, flags, device)),
          rate_(rate),
          k_(bits_per_sym) {}
    int fused_kind() const {  // 0 four kernels, 1 overlap-save fusion, 2 time-domain decimating kernel, 3 its any-rate form, 4 the polyphase
                              // frequency-domain kernel (what the last call ran on: rates 4, 8, 12 ... 64)
        int32_t f = 0;
        comms_chain_is_fused(h_.get(), &f);
        return f;
    }

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        if (rate_ == 0 || n % rate_) return COMMS_ERR_ARG;
        m = k_ ? (n / rate_ * static_cast<size_t>(k_) + 7) / 8 : n / rate_;
        return COMMS_OK;
    }
    comms_status_t launch(const In* in, size_t n, Out* out) { return comms_chain_run(h_.get(), reinterpret_cast<const comms_c32*>(in), n, out); }
    comms_status_t launch_dev(const In* in, size_t n, Out* out, void* s) {
        return comms_chain_run_dev(h_.get(), reinterpret_cast<const comms_c32*>(in), n, out, s);
    }
    Owned<comms_chain_t, comms_chain_destroy> h_;
    size_t rate_;
    int k_;
};

// Receive: i16 samples -> mixer -> matched FIR -> keep every rate-th -> hard decisions -> packed bits (LSB first), one chain
// (comms_chain_set_input_format / _set_output_format): ceil(n / rate * bits_per_sym / 8) bytes per message, each message
// from bit 0 of its first byte -- whole bytes when n is a multiple of 8 * rate / bits_per_sym.
class ChainBitsNode : public HostNode<ChainBitsNode, ChainOp<Complex16, uint8_t>> {
public:
    ChainBitsNode(double dphase, double phase, const std::vector<Complex32>& taps, size_t rate, int bits_per_sym, float in_scale,
                  const std::vector<Complex32>& constellation = {}, bool mixer_after_fir = false, int device = 0)
        : HostNode("ChainBitsNode::new", dphase, phase, taps, rate, mixer_after_fir ? COMMS_CHAIN_MIXER_AFTER_FIR : 0, device, bits_per_sym) {
        throw_on(comms_chain_set_input_format(h_.get(), COMMS_IQ_I16, in_scale), "ChainBitsNode::new");
        throw_on(comms_chain_set_output_format(h_.get(), COMMS_SYM_BITS, bits_per_sym, constellation.empty() ? nullptr : c32(constellation.data())),
                 "ChainBitsNode::new");
    }
};

// Real FIR + decimator over an f32 stream as ONE node (comms_rfir_*; an additional node): the results of the audio stage of
// examples/fm_radio.rs:98-164 -- Convert2Node -> BatchFirNode<f32> -> Convert3Node -> DecimateNode<f32>(rate) -- for real
// taps.  Any message length: ceil(n / rate) outputs, the decimator restarting with every message as DecimateNode does.
struct RealFirDecimOp {
    using In = float;
    using Out = float;
    RealFirDecimOp(const char* who, const std::vector<float>& taps, size_t rate, const std::optional<std::vector<float>>& state, int device)
        : h_(create<decltype(h_)>(who, comms_rfir_create, taps.data(), taps.size(), state ? state->data() : nullptr,
                                  state ? state->size() : 0, rate, device)),
          rate_(rate) {}
    std::string kernel(size_t n) const { return kernel_name(comms_rfir_get_kernel, h_.get(), n); }  // "rfir_decim_kernel<..>", or the four launches

protected:
    comms_status_t prepare(size_t n, size_t& m) const { return comms_rfir_out_len(n, rate_, &m); }
    comms_status_t launch(const float* in, size_t n, float* out) { return comms_rfir_run(h_.get(), in, n, out); }
    comms_status_t launch_dev(const float* in, size_t n, float* out, void* s) { return comms_rfir_run_dev(h_.get(), in, n, out, s); }
    Owned<comms_rfir_t, comms_rfir_destroy> h_;
    size_t rate_;
};
class RealFirDecimNode : public HostNode<RealFirDecimNode, RealFirDecimOp> {
public:
    RealFirDecimNode(const std::vector<float>& taps, size_t rate, const std::optional<std::vector<float>>& state = std::nullopt, int device = 0)
        : HostNode("RealFirDecimNode::new", taps, rate, state, device) {}
};
// on device-resident messages: the angles a ChainNodeDev<float> sends never leave the device
class RealFirDecimNodeDev : public DevNode<RealFirDecimNodeDev, RealFirDecimOp> {
public:
    RealFirDecimNodeDev(const std::vector<float>& taps, size_t rate, const std::optional<std::vector<float>>& state = std::nullopt, int device = 0)
        : DevNode(device, "RealFirDecimNodeDev::new", taps, rate, state, device) {}
};

// Rational resampler by up / down as ONE node (comms_resample_*; an additional node): the results of
// UpsampleNode(up) -> BatchFirNode(Complex(taps, 0)) -> DecimateNode(down) for real taps, over float or Complex32
// messages.  Any message length: ceil(n up / down) outputs, the decimator restarting with every message.
template <class T>
struct ResampleElem;
template <>
struct ResampleElem<float> {
    static constexpr int32_t value = COMMS_RESAMPLE_F32;
};
template <>
struct ResampleElem<Complex32> {
    static constexpr int32_t value = COMMS_RESAMPLE_C32;
};

template <class T>
struct ResampleOp {
    using In = T;
    using Out = T;
    ResampleOp(const char* who, const std::vector<float>& taps, size_t up, size_t down, int device)
        : h_(create<decltype(h_)>(who, comms_resample_create, taps.data(), taps.size(), up, down, ResampleElem<T>::value, device)),
          up_(up),
          down_(down) {}
    std::string kernel(size_t n) const { return kernel_name(comms_resample_get_kernel, h_.get(), n); }  // "resample_kernel<..> ...", or the launches

protected:
    comms_status_t prepare(size_t n, size_t& m) const { return comms_resample_out_len(n, up_, down_, &m); }
    comms_status_t launch(const T* in, size_t n, T* out) { return comms_resample_run(h_.get(), in, n, out); }
    comms_status_t launch_dev(const T* in, size_t n, T* out, void* s) { return comms_resample_run_dev(h_.get(), in, n, out, s); }
    Owned<comms_resample_t, comms_resample_destroy> h_;
    size_t up_, down_;
};
template <class T>
class ResampleNode : public HostNode<ResampleNode<T>, ResampleOp<T>> {
public:
    ResampleNode(const std::vector<float>& taps, size_t up, size_t down, int device = 0)
        : ResampleNode::HostNode("ResampleNode::new", taps, up, down, device) {}
};
template <class T>
class ResampleNodeDev : public DevNode<ResampleNodeDev<T>, ResampleOp<T>> {
public:
    ResampleNodeDev(const std::vector<float>& taps, size_t up, size_t down, int device = 0)
        : ResampleNodeDev::DevNode(device, "ResampleNodeDev::new", taps, up, down, device) {}
};

// Polyphase channelizer as ONE node (comms_channelizer_*; an additional node): the results of M chains
// MixerNode(0, -2 pi k / M) -> BatchFirNode(Complex(taps, 0)) -> DecimateNode(down) over one Complex32 stream.  Any message
// length: ceil(n / down) frames.  One sender carries a message's frames x M outputs in the node's layout
// (COMMS_CHANNELIZER_CHANNEL_MAJOR: channel k is out[k frames .. (k + 1) frames)); connect it to as many receivers as there
// are consumers.
struct ChannelizerOp {
    using In = Complex32;
    using Out = Complex32;
    ChannelizerOp(const char* who, const std::vector<float>& taps, size_t channels, size_t down, int32_t layout, int device)
        : h_(create<decltype(h_)>(who, comms_channelizer_create, taps.data(), taps.size(), channels, down, layout, device)),
          channels_(channels),
          down_(down) {}
    size_t channels() const { return channels_; }
    std::string kernel(size_t n) const { return kernel_name(comms_channelizer_get_kernel, h_.get(), n); }  // "channelizer_kernel<..> ...", or the launches

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        comms_status_t st = comms_channelizer_out_len(n, down_, &m);  // frames
        m *= channels_;
        return st;
    }
    comms_status_t launch(const Complex32* in, size_t n, Complex32* out) { return comms_channelizer_run(h_.get(), c32(in), n, c32(out)); }
    comms_status_t launch_dev(const Complex32* in, size_t n, Complex32* out, void* s) {
        return comms_channelizer_run_dev(h_.get(), c32(in), n, c32(out), s);
    }
    Owned<comms_channelizer_t, comms_channelizer_destroy> h_;
    size_t channels_, down_;
};
class ChannelizerNode : public HostNode<ChannelizerNode, ChannelizerOp> {
public:
    ChannelizerNode(const std::vector<float>& taps, size_t channels, size_t down, int32_t layout = COMMS_CHANNELIZER_CHANNEL_MAJOR, int device = 0)
        : HostNode("ChannelizerNode::new", taps, channels, down, layout, device) {}
};
// on device-resident messages: channel k of a channel-major message is a contiguous device stream
class ChannelizerNodeDev : public DevNode<ChannelizerNodeDev, ChannelizerOp> {
public:
    ChannelizerNodeDev(const std::vector<float>& taps, size_t channels, size_t down, int32_t layout = COMMS_CHANNELIZER_CHANNEL_MAJOR, int device = 0)
        : DevNode(device, "ChannelizerNodeDev::new", taps, channels, down, layout, device) {}
};

// Spectrum estimator as ONE node (comms_spectrum_*; an additional node): windowed, overlapping segments of a Complex32 stream ->
// forward transform -> |X|^2 -> the sum of `avg` segments per row, times scale.  Any message length; a message carries the rows
// its samples complete, rows x n_fft floats, and a call that completes no row sends no message (the #[aggregate] form).
// scale <= 0 asks for the Welch scale 1 / (avg sum w^2).
struct SpectrumOp {
    using In = Complex32;
    using Out = float;
    SpectrumOp(const char* who, int32_t n_fft, const std::vector<float>& window, size_t hop, size_t avg, float scale, int32_t order, int device)
        : n_fft_(static_cast<size_t>(n_fft)) {
        if (window.size() != n_fft_) throw std::runtime_error(std::string(who) + ": the window must hold n_fft values");
        if (!(scale > 0.0f)) {
            double e = 0.0;
            for (float w : window) e += static_cast<double>(w) * w;
            scale = static_cast<float>(1.0 / (static_cast<double>(avg ? avg : 1) * e));
        }
        h_ = create<decltype(h_)>(who, comms_spectrum_create, n_fft, window.data(), hop, avg, scale, order, device);
    }
    size_t n_fft() const { return n_fft_; }
    std::string kernel(size_t n) const { return kernel_name(comms_spectrum_get_kernel, h_.get(), n); }  // "spectrum_kernel<..> ..."
    // comms_window_taps: "rect", "hann", "hamming", "blackman" as COMMS_WINDOW_*
    static std::vector<float> window(int32_t kind, size_t n) {
        std::vector<float> w(n);
        throw_on(comms_window_taps(kind, n, w.data()), "comms_window_taps");
        return w;
    }

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        comms_status_t st = comms_spectrum_out_len(h_.get(), n, &m);  // rows
        m *= n_fft_;
        return st;
    }
    comms_status_t launch(const Complex32* in, size_t n, float* out) { return comms_spectrum_run(h_.get(), c32(in), n, out); }
    comms_status_t launch_dev(const Complex32* in, size_t n, float* out, void* s) { return comms_spectrum_run_dev(h_.get(), c32(in), n, out, s); }
    Owned<comms_spectrum_t, comms_spectrum_destroy> h_;
    size_t n_fft_;
};
class SpectrumNode : public DeriveNode<SpectrumNode>, public Ports<std::vector<Complex32>, std::vector<float>>, public SpectrumOp {
public:
    SpectrumNode(int32_t n_fft, const std::vector<float>& window, size_t hop, size_t avg = 1, float scale = 0.0f,
                 int32_t order = COMMS_SPECTRUM_NATURAL, int device = 0)
        : SpectrumOp("SpectrumNode::new", n_fft, window, hop, avg, scale, order, device) {}
    SpectrumNode(SpectrumNode&&) = default;

    Result<std::optional<std::vector<float>>> run(const std::vector<Complex32>& in) {
        size_t m = 0;
        comms_status_t st = prepare(in.size(), m);
        if (st != COMMS_OK) return to_node_error(st);
        std::vector<float> rows(m);
        st = launch(in.data(), in.size(), rows.data());
        if (st != COMMS_OK) return to_node_error(st);
        if (!m) return std::optional<std::vector<float>>(std::nullopt);
        return std::optional<std::vector<float>>(std::move(rows));
    }
};
// on device-resident messages
class SpectrumNodeDev : public DeriveNode<SpectrumNodeDev>, public Ports<DeviceBuf<Complex32>, DeviceBuf<float>>, public OnStream<SpectrumOp> {
public:
    SpectrumNodeDev(int32_t n_fft, const std::vector<float>& window, size_t hop, size_t avg = 1, float scale = 0.0f,
                    int32_t order = COMMS_SPECTRUM_NATURAL, int device = 0)
        : OnStream<SpectrumOp>(device, "SpectrumNodeDev::new", n_fft, window, hop, avg, scale, order, device) {}
    SpectrumNodeDev(SpectrumNodeDev&&) = default;

    Result<std::optional<DeviceBuf<float>>> run(const DeviceBuf<Complex32>& in) {
        size_t m = 0;
        comms_status_t st = prepare(in.size(), m);
        if (st != COMMS_OK) return to_node_error(st);
        DeviceBuf<float> rows(m ? m : 1, this->device());   // (a call without a row still advances the state: it writes nothing here)
        st = this->submit(in, rows, [&](void* s) { return launch_dev(in.ptr(), in.size(), rows.ptr(), s); });
        if (st != COMMS_OK) return to_node_error(st);
        if (!m) return std::optional<DeviceBuf<float>>(std::nullopt);
        return std::optional<DeviceBuf<float>>(std::move(rows));
    }
};

// Symbol synchroniser as ONE node (comms_symsync_*; an additional node): matched filter with a fractional delay, symbol-rate
// sampler, rotation and -- with set_output_bits -- hard decision, the results of UpsampleNode(phases) -> BatchFirNode(Complex(
// taps, 0)) -> skip mu -> DecimateNode(phases sps) -> MixerNode.  Messages are multiples of sps samples and give n / sps
// symbols (Complex32), or their packed bits (uint8_t, SymbolSyncNode<uint8_t>).
// A second channel, `update`, carries what a block-rate loop (TimingEstimatorNode, a phase estimator) decides between
// blocks: every update queued when a block arrives is applied before it, in order, and the node never waits for one -- the
// channel may stay unconnected.  A NaN field leaves that setting as it is.  dphase is fixed at construction: an update
// carries no increment, and a phase update is applied with the constructor's.
struct SymbolSyncUpdate {
    double tau;    // comms_symsync_set_timing: the sampling instant in input samples
    double phase;  // comms_symsync_set_rotation(dphase, phase): rotor phase of the next output
};
template <class O>
struct SymbolSyncOp {
    static_assert(std::is_same_v<O, Complex32> || std::is_same_v<O, uint8_t>, "symbols (Complex32) or packed bits (uint8_t)");
    using In = Complex32;
    using Out = O;
    NodeReceiver<SymbolSyncUpdate> update;  // optional; host values, drained before each block

    SymbolSyncOp(const char* who, const std::vector<float>& taps, size_t phases, size_t sps, double dphase, int bits_per_sym, int device)
        : h_(create<decltype(h_)>(who, comms_symsync_create, taps.data(), taps.size(), phases, sps, device)),
          sps_(sps < 1 ? 1 : sps),
          dphase_(dphase),
          bits_(std::is_same_v<O, uint8_t> ? bits_per_sym : 0) {
        throw_on(comms_symsync_set_rotation(h_.get(), dphase, 0.0), who);
        if (bits_) throw_on(comms_symsync_set_output_format(h_.get(), COMMS_SYM_BITS, bits_, nullptr), who);
    }
    std::string kernel(size_t n) const { return kernel_name(comms_symsync_get_kernel, h_.get(), n); }  // "symsync_kernel<..> ..."

protected:
    // applies the queued updates; m = the elements of the message's output: symbols, or bytes of packed bits
    comms_status_t prepare(size_t n, size_t& m) {
        while (update) {
            const std::optional<SymbolSyncUpdate> u = update->try_recv();
            if (!u) break;
            comms_status_t st = COMMS_OK;
            if (!std::isnan(u->tau)) st = comms_symsync_set_timing(h_.get(), u->tau);
            if (st == COMMS_OK && !std::isnan(u->phase)) st = comms_symsync_set_rotation(h_.get(), dphase_, u->phase);
            if (st != COMMS_OK) return st;
        }
        const size_t n_sym = n / sps_;
        m = bits_ ? (n_sym * static_cast<size_t>(bits_) + 7) / 8 : n_sym;
        return COMMS_OK;
    }
    comms_status_t launch(const Complex32* in, size_t n, Out* out) { return comms_symsync_run(h_.get(), c32(in), n, out); }
    comms_status_t launch_dev(const Complex32* in, size_t n, Out* out, void* s) { return comms_symsync_run_dev(h_.get(), c32(in), n, out, s); }
    Owned<comms_symsync_t, comms_symsync_destroy> h_;
    size_t sps_;
    double dphase_;
    int bits_;
};
template <class Out = Complex32>
class SymbolSyncNode : public HostNode<SymbolSyncNode<Out>, SymbolSyncOp<Out>> {
public:
    SymbolSyncNode(const std::vector<float>& taps, size_t phases, size_t sps, double dphase = 0.0, int bits_per_sym = 2, int device = 0)
        : SymbolSyncNode::HostNode("SymbolSyncNode::new", taps, phases, sps, dphase, bits_per_sym, device) {}
};
template <class Out = Complex32>
class SymbolSyncNodeDev : public DevNode<SymbolSyncNodeDev<Out>, SymbolSyncOp<Out>> {
public:
    SymbolSyncNodeDev(const std::vector<float>& taps, size_t phases, size_t sps, double dphase = 0.0, int bits_per_sym = 2, int device = 0)
        : SymbolSyncNodeDev::DevNode(device, "SymbolSyncNodeDev::new", taps, phases, sps, dphase, bits_per_sym, device) {}
};

// ---------------------------------------------------------------- mixer
template <class T>
struct MixerOp : protected SameLength {
    using In = T;
    using Out = T;
    MixerOp(const char* who, double dphase, std::optional<double> phase, int device)
        : h_(create<decltype(h_)>(who, comms_mixer_create, dphase, phase.value_or(0.0), device)) {}

protected:
    comms_status_t launch(const T* in, size_t n, T* out) { return Sample<T>::mixer_run(h_.get(), abi(in), n, abi(out)); }
    comms_status_t launch_dev(const T* in, size_t n, T* out, void* s) { return Sample<T>::mixer_run_dev(h_.get(), abi(in), n, abi(out), s); }
    Owned<comms_mixer_t, comms_mixer_destroy> h_;
};

template <class D, class T>
class MixerNodeOf : public DeriveNode<D>, public Ports<T, T>, public MixerOp<T> {
public:
    // NB (dphase, phase): the node's order, not Mixer::new's (mixer.rs:128 vs :43)
    explicit MixerNodeOf(double dphase, std::optional<double> phase = std::nullopt, int device = 0) : MixerOp<T>(D::kNew, dphase, phase, device) {}

    Result<T> run(const T& in) {
        T out;
        return ok_or(this->launch(&in, 1, &out), out);
    }
    Result<std::vector<T>> run_block(const std::vector<T>& ins) {  // see FirNodeOf::run_block
        std::vector<T> out(ins.size());
        return ok_or(this->launch(ins.data(), ins.size(), out.data()), out);
    }
};

struct MixerNode : MixerNodeOf<MixerNode, Complex32> {
    using MixerNodeOf::MixerNodeOf;
    static constexpr const char* kNew = "MixerNode::new";
};
// MixerNode<f64> (src/mixer.rs:93-148 with T = f64, the type of the reference's own mixer tests :160-336)
struct MixerNode64 : MixerNodeOf<MixerNode64, Complex64> {
    using MixerNodeOf::MixerNodeOf;
    static constexpr const char* kNew = "MixerNode<f64>::new";
};

// The reference has no batch mixer node; this one mixes a whole Vec per message.
class BatchMixerNode : public HostNode<BatchMixerNode, MixerOp<Complex32>> {
public:
    explicit BatchMixerNode(double dphase, std::optional<double> phase = std::nullopt, int device = 0)
        : HostNode("BatchMixerNode::new", dphase, phase, device) {}
};
class BatchMixerNodeDev : public DevNode<BatchMixerNodeDev, MixerOp<Complex32>> {
public:
    explicit BatchMixerNodeDev(double dphase, std::optional<double> phase = std::nullopt, int device = 0)
        : DevNode(device, "BatchMixerNodeDev::new", dphase, phase, device) {}
};

// ---------------------------------------------------------------- decimate / upsample (T: Copy)
// No handle: the rate and the device are all there is.  OutLen / Run / RunDev are the comms_decimate_* or comms_upsample_* entries.
template <class T, auto OutLen, auto Run, auto RunDev>
struct RateOp {
    using In = T;
    using Out = T;
    RateOp(const char*, size_t rate, int device) : rate_(rate), device_(device) {}

protected:
    comms_status_t prepare(size_t n, size_t& m) const { return OutLen(n, rate_, &m); }
    comms_status_t launch(const T* in, size_t n, T* out) const { return Run(in, n, sizeof(T), rate_, out, nullptr, device_); }
    comms_status_t launch_dev(const T* in, size_t n, T* out, void* s) const { return RunDev(in, n, sizeof(T), rate_, out, nullptr, device_, s); }
    comms_status_t apply(const std::vector<T>& data, std::vector<T>& out) const {
        size_t m = 0;
        comms_status_t st = prepare(data.size(), m);
        if (st != COMMS_OK) return st;
        out.resize(m);
        return launch(data.data(), data.size(), out.data());
    }
    size_t rate_;
    int device_;
};
template <class T>
using DecimateOp = RateOp<T, comms_decimate_out_len, comms_decimate_run, comms_decimate_run_dev>;
template <class T>
using UpsampleOp = RateOp<T, comms_upsample_out_len, comms_upsample_run, comms_upsample_run_dev>;

template <class T>
class DecimateNode : public HostNode<DecimateNode<T>, DecimateOp<T>> {
public:
    explicit DecimateNode(size_t dec_rate, int device = 0) : DecimateNode::HostNode(nullptr, dec_rate, device) {}
    comms_status_t decimate(const std::vector<T>& data, std::vector<T>& out) const { return this->apply(data, out); }
};
template <class T>
class UpsampleNode : public HostNode<UpsampleNode<T>, UpsampleOp<T>> {
public:
    explicit UpsampleNode(size_t ups_rate, int device = 0) : UpsampleNode::HostNode(nullptr, ups_rate, device) {}
    comms_status_t upsample(const std::vector<T>& data, std::vector<T>& out) const { return this->apply(data, out); }
};
class DecimateNodeDev : public DevNode<DecimateNodeDev, DecimateOp<Complex32>> {
public:
    explicit DecimateNodeDev(size_t dec_rate, int device = 0) : DevNode(device, nullptr, dec_rate, device) {}
};
class UpsampleNodeDev : public DevNode<UpsampleNodeDev, UpsampleOp<Complex32>> {
public:
    explicit UpsampleNodeDev(size_t ups_rate, int device = 0) : DevNode(device, nullptr, ups_rate, device) {}
};

// ---------------------------------------------------------------- FM demod
template <class T>
struct FmOp : protected SameLength {
    using In = T;
    using Out = typename Sample<T>::Real;
    FmOp(const char* who, int device) : h_(create<decltype(h_)>(who, Sample<T>::fm_create, device)) {}

protected:
    comms_status_t launch(const T* in, size_t n, Out* out) { return Sample<T>::fm_run(h_.get(), abi(in), n, out); }
    comms_status_t launch_dev(const T* in, size_t n, Out* out, void* s) { return Sample<T>::fm_run_dev(h_.get(), abi(in), n, out, s); }
    Owned<typename Sample<T>::Fm, Sample<T>::fm_destroy> h_;
};
template <class D, class T>
class FMDemodNodeOf : public HostNode<D, FmOp<T>> {
public:
    explicit FMDemodNodeOf(int device = 0) : FMDemodNodeOf::HostNode(D::kNew, device) {}
};

// ---------------------------------------------------------------- FFT
// the message may hold any whole number of transforms (the reference: exactly one); a wrong length panics inside rustfft in
// the reference, here it is DataError
template <class T>
struct FftOp : protected SameLength {
    using In = T;
    using Out = T;
    FftOp(const char* who, size_t fft_size, bool ifft, int device) : h_(create<decltype(h_)>(who, Sample<T>::fft_create, fft_size, ifft ? 1 : 0, device)) {}

protected:
    comms_status_t launch(const T* in, size_t n, T* out) { return Sample<T>::fft_run(h_.get(), abi(in), n, abi(out)); }
    comms_status_t launch_dev(const T* in, size_t n, T* out, void* s) { return Sample<T>::fft_run_dev(h_.get(), abi(in), n, abi(out), s); }
    Owned<typename Sample<T>::Fft, Sample<T>::fft_destroy> h_;
};
template <class D, class T>
class FFTBatchNodeOf : public HostNode<D, FftOp<T>> {
public:
    FFTBatchNodeOf(size_t fft_size, bool ifft, int device = 0) : FFTBatchNodeOf::HostNode(D::kNew, fft_size, ifft, device) {}
};

struct FMDemodNode : FMDemodNodeOf<FMDemodNode, Complex32> {
    using FMDemodNodeOf::FMDemodNodeOf;
    static constexpr const char* kNew = "FMDemodNode::new";
};
struct FFTBatchNode : FFTBatchNodeOf<FFTBatchNode, Complex32> {
    using FFTBatchNodeOf::FFTBatchNodeOf;
    static constexpr const char* kNew = "FFTBatchNode::new";
};
// FFTBatchNode<f64> (the instantiation of the reference's doc examples, fft_node.rs:24) and FMDemodNode<f64>
// (analog_node.rs:20 with T = f64): plain FP64 kernels, correct to f64 rounding (comms_fft_f64_*, comms_fmdemod_f64_*)
struct FFTBatchNodeF64 : FFTBatchNodeOf<FFTBatchNodeF64, Complex64> {
    using FFTBatchNodeOf::FFTBatchNodeOf;
    static constexpr const char* kNew = "FFTBatchNode<f64>::new";
};
struct FMDemodNodeF64 : FMDemodNodeOf<FMDemodNodeF64, Complex64> {
    using FMDemodNodeOf::FMDemodNodeOf;
    static constexpr const char* kNew = "FMDemodNode<f64>::new";
};
class FFTBatchNodeDev : public DevNode<FFTBatchNodeDev, FftOp<Complex32>> {
public:
    FFTBatchNodeDev(size_t fft_size, bool ifft, int device = 0) : DevNode(device, "FFTBatchNodeDev::new", fft_size, ifft, device) {}
};
class FMDemodNodeDev : public DevNode<FMDemodNodeDev, FmOp<Complex32>> {
public:
    explicit FMDemodNodeDev(int device = 0) : DevNode(device, "FMDemodNodeDev::new", device) {}
};

// #[aggregate]: run returns Some(vec) every fft_size pushes, None otherwise
class FFTSampleNode : public DeriveNode<FFTSampleNode>, public Ports<Complex32, std::vector<Complex32>>, public FftOp<Complex32> {
public:
    FFTSampleNode(size_t fft_size, bool ifft, int device = 0) : FftOp("FFTSampleNode::new", fft_size, ifft, device), n_(fft_size) {}

    Result<std::optional<std::vector<Complex32>>> run(const Complex32& sample) {
        samples_.push_back(sample);
        if (samples_.size() != n_) return std::optional<std::vector<Complex32>>(std::nullopt);
        std::vector<Complex32> out(n_);
        comms_status_t st = launch(samples_.data(), n_, out.data());
        samples_.clear();
        if (st != COMMS_OK) return to_node_error(st);
        return std::optional<std::vector<Complex32>>(std::move(out));
    }
    // queued samples at once: every completed run of fft_size samples becomes one output message
    // (all of them transformed by one batched launch); the remainder waits in `samples_` as before
    Result<std::vector<std::vector<Complex32>>> run_block(const std::vector<Complex32>& ins) {
        samples_.insert(samples_.end(), ins.begin(), ins.end());
        const size_t k = n_ ? samples_.size() / n_ : 0;
        std::vector<std::vector<Complex32>> outs;
        if (!k) return outs;
        std::vector<Complex32> flat(k * n_);
        comms_status_t st = launch(samples_.data(), k * n_, flat.data());
        samples_.erase(samples_.begin(), samples_.begin() + k * n_);
        if (st != COMMS_OK) return to_node_error(st);
        outs.resize(k);
        for (size_t i = 0; i < k; ++i) outs[i].assign(flat.begin() + i * n_, flat.begin() + (i + 1) * n_);
        return outs;
    }

private:
    size_t n_;
    std::vector<Complex32> samples_;
};

// ---------------------------------------------------------------- tap design
inline std::vector<Complex32> rrc_taps(uint32_t n_taps, double sam_per_sym, double beta) {
    std::vector<Complex32> t(n_taps);
    throw_on(comms_rrc_taps(n_taps, sam_per_sym, beta, c32(t.data())), "rrc_taps");  // MathError::InvalidRolloffError
    return t;
}
inline std::vector<Complex32> rc_taps(uint32_t n_taps, double sam_per_sym, double beta) {
    std::vector<Complex32> t(n_taps);
    throw_on(comms_rc_taps(n_taps, sam_per_sym, beta, c32(t.data())), "rc_taps");
    return t;
}
inline std::vector<Complex32> gaussian_taps(uint32_t n_taps, double sam_per_sym, double alpha) {
    std::vector<Complex32> t(n_taps);
    throw_on(comms_gaussian_taps(n_taps, sam_per_sym, alpha, c32(t.data())), "gaussian_taps");
    return t;
}
inline std::vector<Complex32> rect_taps(size_t n_taps) {
    std::vector<Complex32> t(n_taps);
    throw_on(comms_rect_taps(n_taps, c32(t.data())), "rect_taps");
    return t;
}

// ---------------------------------------------------------------- demodulation
// TimingEstimatorNode::new(n, d, alpha) -> Result<Self, MathError>; run(&[Complex<f64>]) -> f64
// (src/demodulation/timing_estimator.rs:116-136).  A bad alpha throws (the reference returns Err).
class TimingEstimatorNode : public DeriveNode<TimingEstimatorNode> {
public:
    NodeReceiver<std::vector<Complex64>> input;
    NodeSender<double> output;

    TimingEstimatorNode(uint32_t n, uint32_t d, double alpha, int device = 0)
        : h_(create<decltype(h_)>("TimingEstimatorNode::new", comms_timing_create, n, d, alpha, device)) {}

    Result<double> run(const std::vector<Complex64>& samples) {
        double est = 0.0;
        return ok_or(comms_timing_push(h_.get(), reinterpret_cast<const double*>(samples.data()), samples.size(), &est), est);
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    Owned<comms_timing_t, comms_timing_destroy> h_;
};

// Timing and frequency estimates of a Complex<f32> block from one read of it (comms_syncest_*; an additional node):
// TimingEstimator::push at (n, d, alpha) and frequency_offset_estimate of the widened samples.  Two outputs per block:
// `output` carries the whole comms_sync_estimate_t, `update` the SymbolSyncUpdate{tau, NaN} that puts a SymbolSyncNode of
// (n_taps, phases) -- its sps = n -- on the symbol centres: tau = timing + (n_taps - 1) / (2 phases) (mod n); the NaN leaves
// the synchroniser's phase alone.  `update` plugs straight into SymbolSyncNode::update.
// The output is a host value on either message kind (the call synchronises its stream), so the two nodes have run() bodies
// of their own over the description.
struct SyncEstimate {
    comms_sync_estimate_t estimate;
    SymbolSyncUpdate update;
    operator comms_sync_estimate_t() const { return estimate; }
    operator SymbolSyncUpdate() const { return update; }
};
struct SyncEstimatorOp {
    SyncEstimatorOp(const char* who, uint32_t n, uint32_t d, double alpha, size_t n_taps, size_t phases, int device)
        : h_(create<decltype(h_)>(who, comms_syncest_create, n, d, alpha, device)),
          n_(n),
          delay_(n_taps ? static_cast<double>(n_taps - 1) / (2.0 * static_cast<double>(phases < 1 ? 1 : phases)) : 0.0) {}
    std::string kernel(size_t n) const { return kernel_name(comms_syncest_get_kernel, h_.get(), n); }  // "syncest_kernel ..."

protected:
    Result<SyncEstimate> estimate(const Complex32* in, size_t n) {
        comms_sync_estimate_t e{};
        return message(comms_syncest_run(h_.get(), c32(in), n, &e), e);
    }
    Result<SyncEstimate> estimate_dev(const Complex32* in, size_t n, void* s) {
        comms_sync_estimate_t e{};
        return message(comms_syncest_run_dev(h_.get(), c32(in), n, &e, s), e);
    }

private:
    Result<SyncEstimate> message(comms_status_t st, const comms_sync_estimate_t& e) const {
        if (st != COMMS_OK) return to_node_error(st);
        double tau = std::fmod(e.timing + delay_, static_cast<double>(n_));
        if (tau < 0) tau += static_cast<double>(n_);
        return SyncEstimate{e, SymbolSyncUpdate{tau, std::numeric_limits<double>::quiet_NaN()}};
    }
    Owned<comms_syncest_t, comms_syncest_destroy> h_;
    uint32_t n_;
    double delay_;
};

template <class In>
struct SyncEstimatorPorts {  // as Ports, with the second sender
    NodeReceiver<In> input;
    NodeSender<comms_sync_estimate_t> output;
    NodeSender<SymbolSyncUpdate> update;
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output, update); }
};
class SyncEstimatorNode : public DeriveNode<SyncEstimatorNode>, public SyncEstimatorPorts<std::vector<Complex32>>, public SyncEstimatorOp {
public:
    SyncEstimatorNode(uint32_t n, uint32_t d, double alpha, size_t n_taps, size_t phases, int device = 0)
        : SyncEstimatorOp("SyncEstimatorNode::new", n, d, alpha, n_taps, phases, device) {}
    Result<SyncEstimate> run(const std::vector<Complex32>& samples) { return estimate(samples.data(), samples.size()); }
};
class SyncEstimatorNodeDev : public DeriveNode<SyncEstimatorNodeDev>, public SyncEstimatorPorts<DeviceBuf<Complex32>>, public OnStream<SyncEstimatorOp> {
public:
    SyncEstimatorNodeDev(uint32_t n, uint32_t d, double alpha, size_t n_taps, size_t phases, int device = 0)
        : OnStream(device, "SyncEstimatorNodeDev::new", n, d, alpha, n_taps, phases, device) {}
    Result<SyncEstimate> run(const DeviceBuf<Complex32>& in) {
        comms_status_t st = wait(in);
        if (st != COMMS_OK) return to_node_error(st);
        return estimate_dev(in.ptr(), in.size(), get());
    }
};

// Frame synchroniser (comms_framesync_*; an additional node): takes SymbolSyncNode<Complex32>'s symbol output and sends, per
// block, the detections of a known word that the block decides -- possibly none -- as a vector ordered by stream index.
// index + word.size() is the first payload symbol, atan2(corr_im, corr_re) the rotation to take out.  A block of n symbols
// decides n positions, so a word is reported by the block that brings the last symbol of its guard window; flush() ends a
// stream.  The detections do not depend on how the stream is cut into blocks.  They are host values on either message kind
// (the call synchronises its stream): run() bodies of their own, as the estimator's.
struct FrameSyncOp {
    using Detections = std::vector<comms_frame_detection_t>;
    FrameSyncOp(const char* who, const std::vector<Complex32>& word, double threshold, size_t guard, int device)
        : h_(create<decltype(h_)>(who, comms_framesync_create, c32(word.data()), word.size(), threshold, guard, device)),
          n_word_(word.size()),
          guard_(guard) {}
    Result<Detections> flush() {  // a flush decides word + guard positions
        return collect(n_word_ + guard_, [&](auto* out, size_t cap, size_t* found) { return comms_framesync_flush(h_.get(), out, cap, found); });
    }
    std::string kernel(size_t n) const { return kernel_name(comms_framesync_get_kernel, h_.get(), n); }  // "framesync_kernel ..."

protected:
    Result<Detections> detect(const Complex32* in, size_t n) {
        return collect(n, [&](auto* out, size_t cap, size_t* found) { return comms_framesync_run(h_.get(), c32(in), n, out, cap, found); });
    }
    Result<Detections> detect_dev(const Complex32* in, size_t n, void* s) {
        return collect(n, [&](auto* out, size_t cap, size_t* found) { return comms_framesync_run_dev(h_.get(), c32(in), n, out, cap, found, s); });
    }

private:
    // no call that decides n positions has more than (n + guard) / (guard + 1) detections: they are more than `guard` apart
    template <class F>
    Result<Detections> collect(size_t n, F&& call) {
        Detections out((n + guard_) / (guard_ + 1));
        size_t found = 0;
        comms_status_t st = call(out.data(), out.size(), &found);
        if (st != COMMS_OK) return to_node_error(st);
        out.resize(found);
        return out;
    }
    Owned<comms_framesync_t, comms_framesync_destroy> h_;
    size_t n_word_, guard_;
};

class FrameSyncNode : public DeriveNode<FrameSyncNode>, public Ports<std::vector<Complex32>, FrameSyncOp::Detections>, public FrameSyncOp {
public:
    FrameSyncNode(const std::vector<Complex32>& word, double threshold, size_t guard, int device = 0)
        : FrameSyncOp("FrameSyncNode::new", word, threshold, guard, device) {}
    Result<Detections> run(const std::vector<Complex32>& symbols) { return detect(symbols.data(), symbols.size()); }
};
// on device-resident messages: SymbolSyncNodeDev<Complex32>'s output
class FrameSyncNodeDev : public DeriveNode<FrameSyncNodeDev>, public Ports<DeviceBuf<Complex32>, FrameSyncOp::Detections>, public OnStream<FrameSyncOp> {
public:
    FrameSyncNodeDev(const std::vector<Complex32>& word, double threshold, size_t guard, int device = 0)
        : OnStream(device, "FrameSyncNodeDev::new", word, threshold, guard, device) {}
    Result<Detections> run(const DeviceBuf<Complex32>& in) {
        comms_status_t st = wait(in);
        if (st != COMMS_OK) return to_node_error(st);
        return detect_dev(in.ptr(), in.size(), get());
    }
};

// Deframer (comms_deframe_*; an additional node): takes the symbol blocks FrameSyncNode takes and, on a second receiver, the
// detections FrameSyncNode sent for the same block, and sends per block the frames that became complete in it -- possibly
// none -- as one message: the records back to back (frame f at data[f * frame_bytes]; packed bits, LLRs or symbols, see
// `format`) and one header per frame.  A payload that ends in a later block comes out of that block; the frames do not
// depend on how the stream is cut into blocks.  Connect SymbolSyncNode's output to both nodes.  One description, two shells
// with run() bodies of their own (two receivers; the call synchronises its stream), as the frame synchroniser's.
template <class Store>
struct FramesOf {
    Store data;                                    // headers.size() * frame_bytes bytes hold the records (a buffer may be longer)
    std::vector<comms_deframe_header_t> headers;   // one per frame, ascending index
    size_t frame_bytes = 0;
    size_t size() const { return headers.size(); }
};
struct DeframeOp {
    using Detections = FrameSyncOp::Detections;
    using Frames = FramesOf<std::vector<uint8_t>>;
    using FramesDev = FramesOf<DeviceBuf<uint8_t>>;
    // format: COMMS_SYM_C32, COMMS_SYM_BITS or COMMS_SYM_LLR; word_energy > 0 turns COMMS_DEFRAME_NORMALISE on
    DeframeOp(const char* who, size_t n_payload, size_t offset, size_t lookback, int bits_per_sym, int32_t format, double word_energy,
              float llr_scale, int device)
        : h_(create<decltype(h_)>(who, comms_deframe_create, n_payload, offset, lookback, bits_per_sym, static_cast<const comms_c32*>(nullptr),
                                  word_energy > 0.0 ? COMMS_DEFRAME_NORMALISE : 0, device)) {
        if (word_energy > 0.0) throw_on(comms_deframe_set_word_energy(h_.get(), word_energy), who);
        throw_on(comms_deframe_set_output_format(h_.get(), format), who);
        throw_on(comms_deframe_set_llr_scale(h_.get(), llr_scale), who);
    }
    size_t frame_bytes() const { return comms_deframe_frame_bytes(h_.get()); }
    size_t flush() {  // drops the incomplete frames; how many
        size_t dropped = 0;
        throw_on(comms_deframe_flush(h_.get(), &dropped), "DeframeNode::flush");
        return dropped;
    }
    std::string kernel(size_t n_frames) const { return kernel_name(comms_deframe_get_kernel, h_.get(), n_frames); }  // "deframe_kernel ..."

protected:
    Result<Frames> extract(const Complex32* in, size_t n, const Detections& dets) {
        Frames out;
        size_t cap = 0;
        comms_status_t st = ready(n, dets, out, cap);
        if (st != COMMS_OK) return to_node_error(st);
        out.data.resize(cap * out.frame_bytes);
        size_t found = 0;
        st = comms_deframe_run(h_.get(), c32(in), n, dets.data(), dets.size(), out.data.data(), cap, out.headers.data(), &found);
        return ok_or(st, out);
    }
    Result<FramesDev> extract_dev(const Complex32* in, size_t n, const Detections& dets, void* s, int device) {
        FramesDev out;
        size_t cap = 0;
        comms_status_t st = ready(n, dets, out, cap);
        if (st != COMMS_OK) return to_node_error(st);
        out.data = DeviceBuf<uint8_t>(cap ? cap * out.frame_bytes : 8, device);
        size_t found = 0;
        st = comms_deframe_run_dev(h_.get(), c32(in), n, dets.data(), dets.size(), out.data.ptr(), cap, out.headers.data(), &found, s);
        if (st == COMMS_OK) st = comms_buf_record_ready(out.data.raw(), s);
        return ok_or(st, out);
    }

private:
    template <class F>
    comms_status_t ready(size_t n, const Detections& dets, F& out, size_t& cap) const {
        const comms_status_t st = comms_deframe_frames_ready(h_.get(), n, dets.data(), dets.size(), &cap);
        out.headers.resize(cap);
        out.frame_bytes = frame_bytes();
        return st;
    }
    Owned<comms_deframe_t, comms_deframe_destroy> h_;
};

template <class Sym, class Out>
struct DeframePorts {  // as Ports, with the second receiver
    NodeReceiver<Sym> input;                               // the symbol blocks
    NodeReceiver<DeframeOp::Detections> detections;        // FrameSyncNode's message for the same block
    NodeSender<Out> output;
    auto receivers() { return std::tie(input, detections); }
    auto senders() { return std::tie(output); }
};
class DeframeNode : public DeriveNode<DeframeNode>, public DeframePorts<std::vector<Complex32>, DeframeOp::Frames>, public DeframeOp {
public:
    DeframeNode(size_t n_payload, size_t offset, size_t lookback, int bits_per_sym = 2, int32_t format = COMMS_SYM_BITS, double word_energy = 0.0,
                float llr_scale = 1.0f, int device = 0)
        : DeframeOp("DeframeNode::new", n_payload, offset, lookback, bits_per_sym, format, word_energy, llr_scale, device) {}
    Result<Frames> run(const std::vector<Complex32>& symbols, const Detections& dets) { return extract(symbols.data(), symbols.size(), dets); }
};
// on device-resident messages: SymbolSyncNodeDev<Complex32>'s output in, the records in a DeviceBuf out (headers on the host)
class DeframeNodeDev : public DeriveNode<DeframeNodeDev>, public DeframePorts<DeviceBuf<Complex32>, DeframeOp::FramesDev>, public OnStream<DeframeOp> {
public:
    DeframeNodeDev(size_t n_payload, size_t offset, size_t lookback, int bits_per_sym = 2, int32_t format = COMMS_SYM_BITS, double word_energy = 0.0,
                   float llr_scale = 1.0f, int device = 0)
        : OnStream(device, "DeframeNodeDev::new", n_payload, offset, lookback, bits_per_sym, format, word_energy, llr_scale, device) {}
    Result<FramesDev> run(const DeviceBuf<Complex32>& in, const Detections& dets) {
        comms_status_t st = wait(in);
        if (st != COMMS_OK) return to_node_error(st);
        auto out = extract_dev(in.ptr(), in.size(), dets, get(), device());
        if (out.is_ok()) st = comms_buf_record_use(in.raw(), get());
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
};

// Convolutional FEC (comms_convenc_*, comms_viterbi_*; additional nodes).  A code is (K, generators, terminated); no
// generators = the defaults of K = 7, (0171, 0133).  One description per operation, two shells each.
struct ConvCodeSpec {
    size_t n_info_bits;
    int K = 7;
    std::vector<uint32_t> gens = {};
    bool terminated = true;
    int n() const { return gens.empty() ? 2 : static_cast<int>(gens.size()); }
    const uint32_t* g() const { return gens.empty() ? nullptr : gens.data(); }
    int32_t flags() const { return terminated ? COMMS_CONV_TERMINATED : COMMS_CONV_TRUNCATED; }
};

// Encoder: a message is whole records of packed information bits (in_frame_bytes() each, LSB first), the output the records
// of coded bits (out_frame_bytes() each) -- the bytes PulseBitsNode and the byte modulators take as they stand.
struct ConvEncOp {
    using In = uint8_t;
    using Out = uint8_t;
    ConvEncOp(const char* who, const ConvCodeSpec& code, int device)
        : h_(create<decltype(h_)>(who, comms_convenc_create, code.K, code.n(), code.g(), code.flags(), code.n_info_bits, device)) {}
    size_t in_frame_bytes() const { return comms_convenc_in_frame_bytes(h_.get()); }
    size_t out_frame_bytes() const { return comms_convenc_out_frame_bytes(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_name(comms_convenc_get_kernel, h_.get(), n_frames); }  // "conv_encode_kernel ..."

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        if (n % in_frame_bytes()) return COMMS_ERR_ARG;
        m = n / in_frame_bytes() * out_frame_bytes();
        return COMMS_OK;
    }
    comms_status_t launch(const uint8_t* in, size_t n, uint8_t* out) { return comms_convenc_run(h_.get(), in, n / in_frame_bytes(), out); }
    comms_status_t launch_dev(const uint8_t* in, size_t n, uint8_t* out, void* s) {
        return comms_convenc_run_dev(h_.get(), in, n / in_frame_bytes(), out, s);
    }
    Owned<comms_convenc_t, comms_convenc_destroy> h_;
};
class ConvEncoderNode : public HostNode<ConvEncoderNode, ConvEncOp> {
public:
    explicit ConvEncoderNode(const ConvCodeSpec& code, int device = 0) : HostNode("ConvEncoderNode::new", code, device) {}
};
class ConvEncoderNodeDev : public DevNode<ConvEncoderNodeDev, ConvEncOp> {
public:
    explicit ConvEncoderNodeDev(const ConvCodeSpec& code, int device = 0) : DevNode(device, "ConvEncoderNodeDev::new", code, device) {}
};

// Decoder: takes DeframeNode's message in the COMMS_SYM_LLR format (records of frame_bytes / 4 >= n * steps values) and
// sends the decoded records under the same headers: frame f at data[f * frame_bytes], frame_bytes = out_frame_bytes().
// A message without frames passes through empty.
struct ViterbiOp {
    using Frames = DeframeOp::Frames;
    using FramesDev = DeframeOp::FramesDev;
    // record_llrs: values per input record (0: exactly n * steps); qscale: comms_viterbi_set_quant_scale
    ViterbiOp(const char* who, const ConvCodeSpec& code, size_t record_llrs, float qscale, int device)
        : h_(create<decltype(h_)>(who, comms_viterbi_create, code.K, code.n(), code.g(), code.flags(), code.n_info_bits, record_llrs, device)) {
        throw_on(comms_viterbi_set_quant_scale(h_.get(), qscale), who);
    }
    size_t in_frame_bytes() const { return comms_viterbi_in_frame_bytes(h_.get()); }
    size_t out_frame_bytes() const { return comms_viterbi_out_frame_bytes(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_name(comms_viterbi_get_kernel, h_.get(), n_frames); }  // "viterbi_kernel<..> ..."

protected:
    Result<Frames> decode(const Frames& in) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        Frames out{std::vector<uint8_t>(in.size() * out_frame_bytes()), in.headers, out_frame_bytes()};
        return ok_or(comms_viterbi_run(h_.get(), reinterpret_cast<const float*>(in.data.data()), in.size(), out.data.data(), nullptr), out);
    }
    Result<FramesDev> decode_dev(const FramesDev& in, const DevStream& on) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        FramesDev out{DeviceBuf<uint8_t>(in.size() ? in.size() * out_frame_bytes() : 8, on.device()), in.headers, out_frame_bytes()};
        return ok_or(on.submit(in.data, out.data, [&](void* s) {
            return comms_viterbi_run_dev(h_.get(), reinterpret_cast<const float*>(in.data.ptr()), in.size(), out.data.ptr(), nullptr, s);
        }), out);
    }
    Owned<comms_viterbi_t, comms_viterbi_destroy> h_;
};
class ViterbiNode : public DeriveNode<ViterbiNode>, public Ports<ViterbiOp::Frames, ViterbiOp::Frames>, public ViterbiOp {
public:
    explicit ViterbiNode(const ConvCodeSpec& code, size_t record_llrs = 0, float qscale = 1.0f, int device = 0)
        : ViterbiOp("ViterbiNode::new", code, record_llrs, qscale, device) {}
    Result<Frames> run(const Frames& in) { return decode(in); }
};
// on device-resident messages: DeframeNodeDev's records in, the decoded records in a DeviceBuf out (headers on the host)
class ViterbiNodeDev : public DeriveNode<ViterbiNodeDev>, public Ports<ViterbiOp::FramesDev, ViterbiOp::FramesDev>, public OnStream<ViterbiOp> {
public:
    explicit ViterbiNodeDev(const ConvCodeSpec& code, size_t record_llrs = 0, float qscale = 1.0f, int device = 0)
        : OnStream(device, "ViterbiNodeDev::new", code, record_llrs, qscale, device) {}
    Result<FramesDev> run(const FramesDev& in) { return decode_dev(in, *this); }
};

// LDPC coding (comms_ldpcenc_*, comms_ldpcdec_*; additional nodes).  A code is its base matrix (mb x nb entries, row-major; -1 a
// zero block, b >= 0 the identity shifted by b) and the lifting size Z.  One description per operation, two shells each.
struct LdpcCodeSpec {
    int mb, nb, Z;
    std::vector<int16_t> base;   // mb * nb entries
    const int16_t* b() const { return base.size() == static_cast<size_t>(mb) * static_cast<size_t>(nb) ? base.data() : nullptr; }
};

// Encoder: a message is whole records of (nb - mb) Z packed information bits (in_frame_bytes() each, LSB first), the output the
// records of nb Z coded bits (out_frame_bytes() each) -- the bytes PulseBitsNode and the byte modulators take as they stand.
struct LdpcEncOp {
    using In = uint8_t;
    using Out = uint8_t;
    LdpcEncOp(const char* who, const LdpcCodeSpec& code, int device)
        : h_(create<decltype(h_)>(who, comms_ldpcenc_create, code.mb, code.nb, code.Z, code.b(), device)) {}
    size_t in_frame_bytes() const { return comms_ldpcenc_in_frame_bytes(h_.get()); }
    size_t out_frame_bytes() const { return comms_ldpcenc_out_frame_bytes(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_name(comms_ldpcenc_get_kernel, h_.get(), n_frames); }  // "ldpc_encode_kernel ..."

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        if (n % in_frame_bytes()) return COMMS_ERR_ARG;
        m = n / in_frame_bytes() * out_frame_bytes();
        return COMMS_OK;
    }
    comms_status_t launch(const uint8_t* in, size_t n, uint8_t* out) { return comms_ldpcenc_run(h_.get(), in, n / in_frame_bytes(), out); }
    comms_status_t launch_dev(const uint8_t* in, size_t n, uint8_t* out, void* s) {
        return comms_ldpcenc_run_dev(h_.get(), in, n / in_frame_bytes(), out, s);
    }
    Owned<comms_ldpcenc_t, comms_ldpcenc_destroy> h_;
};
class LdpcEncoderNode : public HostNode<LdpcEncoderNode, LdpcEncOp> {
public:
    explicit LdpcEncoderNode(const LdpcCodeSpec& code, int device = 0) : HostNode("LdpcEncoderNode::new", code, device) {}
};
class LdpcEncoderNodeDev : public DevNode<LdpcEncoderNodeDev, LdpcEncOp> {
public:
    explicit LdpcEncoderNodeDev(const LdpcCodeSpec& code, int device = 0) : DevNode(device, "LdpcEncoderNodeDev::new", code, device) {}
};

// Decoder: takes DeframeNode's message in the COMMS_SYM_LLR format (records of frame_bytes / 4 >= nb Z values) and sends the
// decoded records under the same headers: frame f at data[f * frame_bytes], frame_bytes = out_frame_bytes().  A message without
// frames passes through empty.
struct LdpcDecSpec {
    int max_iters = 20, norm16 = 12;
    size_t record_llrs = 0;      // values per input record (0: exactly nb Z)
    float qscale = 1.0f;         // comms_ldpcdec_set_quant_scale
};
struct LdpcDecOp {
    using Frames = DeframeOp::Frames;
    using FramesDev = DeframeOp::FramesDev;
    LdpcDecOp(const char* who, const LdpcCodeSpec& code, const LdpcDecSpec& dec, int device)
        : h_(create<decltype(h_)>(who, comms_ldpcdec_create, code.mb, code.nb, code.Z, code.b(), dec.max_iters, dec.norm16, dec.record_llrs, device)) {
        throw_on(comms_ldpcdec_set_quant_scale(h_.get(), dec.qscale), who);
    }
    size_t in_frame_bytes() const { return comms_ldpcdec_in_frame_bytes(h_.get()); }
    size_t out_frame_bytes() const { return comms_ldpcdec_out_frame_bytes(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_name(comms_ldpcdec_get_kernel, h_.get(), n_frames); }  // "ldpc_decode_kernel ..."

protected:
    Result<Frames> decode(const Frames& in) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        Frames out{std::vector<uint8_t>(in.size() * out_frame_bytes()), in.headers, out_frame_bytes()};
        return ok_or(comms_ldpcdec_run(h_.get(), reinterpret_cast<const float*>(in.data.data()), in.size(), out.data.data(), nullptr), out);
    }
    Result<FramesDev> decode_dev(const FramesDev& in, const DevStream& on) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        FramesDev out{DeviceBuf<uint8_t>(in.size() ? in.size() * out_frame_bytes() : 8, on.device()), in.headers, out_frame_bytes()};
        return ok_or(on.submit(in.data, out.data, [&](void* s) {
            return comms_ldpcdec_run_dev(h_.get(), reinterpret_cast<const float*>(in.data.ptr()), in.size(), out.data.ptr(), nullptr, s);
        }), out);
    }
    Owned<comms_ldpcdec_t, comms_ldpcdec_destroy> h_;
};
class LdpcDecoderNode : public DeriveNode<LdpcDecoderNode>, public Ports<LdpcDecOp::Frames, LdpcDecOp::Frames>, public LdpcDecOp {
public:
    explicit LdpcDecoderNode(const LdpcCodeSpec& code, const LdpcDecSpec& dec = {}, int device = 0)
        : LdpcDecOp("LdpcDecoderNode::new", code, dec, device) {}
    Result<Frames> run(const Frames& in) { return decode(in); }
};
// on device-resident messages: DeframeNodeDev's records in, the decoded records in a DeviceBuf out (headers on the host)
class LdpcDecoderNodeDev : public DeriveNode<LdpcDecoderNodeDev>, public Ports<LdpcDecOp::FramesDev, LdpcDecOp::FramesDev>, public OnStream<LdpcDecOp> {
public:
    explicit LdpcDecoderNodeDev(const LdpcCodeSpec& code, const LdpcDecSpec& dec = {}, int device = 0)
        : OnStream(device, "LdpcDecoderNodeDev::new", code, dec, device) {}
    Result<FramesDev> run(const FramesDev& in) { return decode_dev(in, *this); }
};

// Rate matching (comms_ratematch_*; additional nodes): puncturer, interleaver and scrambler of one frame format, the same
// description on both sides of the link.  One description per direction, two shells each.
struct RateMatchSpec {
    size_t n_coded;                       // the encoder's n * steps
    std::vector<uint8_t> pattern = {};    // 0 / 1 per coded position, repeated; empty keeps everything
    size_t cols = 0;                      // columns of the pruned block interleaver (0, 1: none) ...
    std::vector<uint32_t> perm = {};      // ... or an explicit permutation of the kept bits (cols = 0 then)
    std::vector<uint8_t> scramble = {};   // one bit per transmitted bit, packed LSB first; empty: none
    const uint8_t* p() const { return pattern.empty() ? nullptr : pattern.data(); }
    const uint32_t* pi() const { return perm.empty() ? nullptr : perm.data(); }
    const uint8_t* s() const { return scramble.empty() ? nullptr : scramble.data(); }
};
struct RateMatchHandle {
    // perm and scramble are read for as many entries as the pattern keeps positions: checked here, where their lengths are known
    RateMatchHandle(const char* who, const RateMatchSpec& f, size_t record_llrs, int device) {
        size_t kept = 0;
        for (size_t i = 0; i < f.n_coded; ++i) kept += f.pattern.empty() || f.pattern[i % f.pattern.size()] != 0;
        if ((!f.perm.empty() && f.perm.size() != kept) || (!f.scramble.empty() && f.scramble.size() < (kept + 7) / 8))
            throw std::runtime_error(std::string(who) + ": perm and scramble must hold one entry per transmitted bit");
        h_ = create<decltype(h_)>(who, comms_ratematch_create, f.n_coded, f.p(), f.pattern.size(), f.cols, f.pi(), static_cast<const void*>(f.s()),
                                  record_llrs, device);
    }
    size_t n_tx_bits() const { return comms_ratematch_n_tx_bits(h_.get()); }
    std::vector<uint32_t> map() const {   // src: the coded position that feeds transmitted bit k
        std::vector<uint32_t> src(n_tx_bits());
        throw_on(comms_ratematch_get_map(h_.get(), src.data(), src.size()), "RateMatch::map");
        return src;
    }

protected:
    std::string kernel_of(int32_t direction, size_t n_frames) const {
        return kernel_name([direction](const comms_ratematch_t* h, size_t n, char* name, size_t len) { return comms_ratematch_get_kernel(h, direction, n, name, len); },
                           h_.get(), n_frames);
    }
    Owned<comms_ratematch_t, comms_ratematch_destroy> h_;
};

// Transmit: a message is whole records of coded bits (in_frame_bytes() each: ConvEncoderNode's output as it stands), the output
// the records of transmitted bits (out_frame_bytes() each) -- the bytes PulseBitsNode and the byte modulators take.
struct RateMatchOp : RateMatchHandle {
    using In = uint8_t;
    using Out = uint8_t;
    RateMatchOp(const char* who, const RateMatchSpec& format, int device) : RateMatchHandle(who, format, 0, device) {}
    size_t in_frame_bytes() const { return comms_ratematch_tx_in_frame_bytes(h_.get()); }
    size_t out_frame_bytes() const { return comms_ratematch_tx_out_frame_bytes(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_of(COMMS_RATEMATCH_TX, n_frames); }  // "ratematch_tx_kernel ..."

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        if (n % in_frame_bytes()) return COMMS_ERR_ARG;
        m = n / in_frame_bytes() * out_frame_bytes();
        return COMMS_OK;
    }
    comms_status_t launch(const uint8_t* in, size_t n, uint8_t* out) { return comms_ratematch_tx_run(h_.get(), in, n / in_frame_bytes(), out); }
    comms_status_t launch_dev(const uint8_t* in, size_t n, uint8_t* out, void* s) {
        return comms_ratematch_tx_run_dev(h_.get(), in, n / in_frame_bytes(), out, s);
    }
};
class RateMatchNode : public HostNode<RateMatchNode, RateMatchOp> {
public:
    explicit RateMatchNode(const RateMatchSpec& format, int device = 0) : HostNode("RateMatchNode::new", format, device) {}
};
class RateMatchNodeDev : public DevNode<RateMatchNodeDev, RateMatchOp> {
public:
    explicit RateMatchNodeDev(const RateMatchSpec& format, int device = 0) : DevNode(device, "RateMatchNodeDev::new", format, device) {}
};

// Receive: takes DeframeNode's message in the COMMS_SYM_LLR format (records of frame_bytes / 4 >= n_tx_bits() values) and sends
// records of n_coded values under the same headers, zeros at the punctured positions: ViterbiNode's input (record_llrs = 0).
// A message without frames passes through empty.
struct RateDematchOp : RateMatchHandle {
    using Frames = DeframeOp::Frames;
    using FramesDev = DeframeOp::FramesDev;
    // record_llrs: values per input record (0: exactly n_tx_bits())
    RateDematchOp(const char* who, const RateMatchSpec& format, size_t record_llrs, int device) : RateMatchHandle(who, format, record_llrs, device) {}
    size_t in_frame_bytes() const { return comms_ratematch_rx_in_frame_bytes(h_.get()); }
    size_t out_frame_bytes() const { return comms_ratematch_rx_out_frame_bytes(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_of(COMMS_RATEMATCH_RX, n_frames); }  // "ratematch_rx_kernel ..."

protected:
    Result<Frames> dematch(const Frames& in) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        Frames out{std::vector<uint8_t>(in.size() * out_frame_bytes()), in.headers, out_frame_bytes()};
        return ok_or(comms_ratematch_rx_run(h_.get(), reinterpret_cast<const float*>(in.data.data()), in.size(), reinterpret_cast<float*>(out.data.data())), out);
    }
    Result<FramesDev> dematch_dev(const FramesDev& in, const DevStream& on) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        FramesDev out{DeviceBuf<uint8_t>(in.size() ? in.size() * out_frame_bytes() : 8, on.device()), in.headers, out_frame_bytes()};
        return ok_or(on.submit(in.data, out.data, [&](void* s) {
            return comms_ratematch_rx_run_dev(h_.get(), reinterpret_cast<const float*>(in.data.ptr()), in.size(), reinterpret_cast<float*>(out.data.ptr()), s);
        }), out);
    }
};
class RateDematchNode : public DeriveNode<RateDematchNode>, public Ports<RateDematchOp::Frames, RateDematchOp::Frames>, public RateDematchOp {
public:
    explicit RateDematchNode(const RateMatchSpec& format, size_t record_llrs = 0, int device = 0)
        : RateDematchOp("RateDematchNode::new", format, record_llrs, device) {}
    Result<Frames> run(const Frames& in) { return dematch(in); }
};
// on device-resident messages: DeframeNodeDev's records in, the dematched records in a DeviceBuf out (headers on the host)
class RateDematchNodeDev : public DeriveNode<RateDematchNodeDev>, public Ports<RateDematchOp::FramesDev, RateDematchOp::FramesDev>, public OnStream<RateDematchOp> {
public:
    explicit RateDematchNodeDev(const RateMatchSpec& format, size_t record_llrs = 0, int device = 0)
        : OnStream(device, "RateDematchNodeDev::new", format, record_llrs, device) {}
    Result<FramesDev> run(const FramesDev& in) { return dematch_dev(in, *this); }
};

// Frame check (comms_crc_*; additional nodes): a CRC of 1 ... 32 bits over frames of fixed length, the same description on both
// sides of the link.  One description per direction, two shells each.
struct CrcSpec {
    int width;              // W, 1 ... 32
    uint32_t poly;          // normal form, without the x^W term
    uint32_t init = 0;
    uint32_t xorout = 0;
    size_t n_payload_bits;  // T, with T + W <= 2^16
};
struct CrcHandle {
    CrcHandle(const char* who, const CrcSpec& f, int device)
        : h_(create<decltype(h_)>(who, comms_crc_create, static_cast<int32_t>(f.width), f.poly, f.init, f.xorout, f.n_payload_bits, device)) {}
    size_t payload_frame_bytes() const { return comms_crc_payload_frame_bytes(h_.get()); }
    size_t coded_frame_bytes() const { return comms_crc_coded_frame_bytes(h_.get()); }

protected:
    std::string kernel_of(int32_t direction, size_t n_frames) const {
        return kernel_name([direction](const comms_crc_t* h, size_t n, char* name, size_t len) { return comms_crc_get_kernel(h, direction, n, name, len); },
                           h_.get(), n_frames);
    }
    Owned<comms_crc_t, comms_crc_destroy> h_;
};

// Attach: a message is whole records of payload bits (in_frame_bytes() each), the output the records of payload + CRC bits
// (out_frame_bytes() each) -- ConvEncoderNode's input with n_info_bits = T + W as they stand.
struct CrcAttachOp : CrcHandle {
    using In = uint8_t;
    using Out = uint8_t;
    CrcAttachOp(const char* who, const CrcSpec& format, int device) : CrcHandle(who, format, device) {}
    size_t in_frame_bytes() const { return payload_frame_bytes(); }
    size_t out_frame_bytes() const { return coded_frame_bytes(); }
    std::string kernel(size_t n_frames) const { return kernel_of(COMMS_CRC_ATTACH, n_frames); }  // "crc_attach_kernel ..."

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        if (n % in_frame_bytes()) return COMMS_ERR_ARG;
        m = n / in_frame_bytes() * out_frame_bytes();
        return COMMS_OK;
    }
    comms_status_t launch(const uint8_t* in, size_t n, uint8_t* out) { return comms_crc_attach_run(h_.get(), in, n / in_frame_bytes(), out); }
    comms_status_t launch_dev(const uint8_t* in, size_t n, uint8_t* out, void* s) {
        return comms_crc_attach_run_dev(h_.get(), in, n / in_frame_bytes(), out, s);
    }
};
class CrcAttachNode : public HostNode<CrcAttachNode, CrcAttachOp> {
public:
    explicit CrcAttachNode(const CrcSpec& format, int device = 0) : HostNode("CrcAttachNode::new", format, device) {}
};
class CrcAttachNodeDev : public DevNode<CrcAttachNodeDev, CrcAttachOp> {
public:
    explicit CrcAttachNodeDev(const CrcSpec& format, int device = 0) : DevNode(device, "CrcAttachNodeDev::new", format, device) {}
};

// Check: takes ViterbiNode's message (records of T + W decoded bits under the deframer's headers) and sends the payload records
// under the same headers with one pass flag per frame: 1 where the recomputed CRC equals the received bits.  A message without
// frames passes through empty.
template <class Store, class Flags>
struct CheckedOf {
    FramesOf<Store> frames;   // the payload records, frame_bytes = out_frame_bytes()
    Flags passed;             // int32 per frame
    size_t size() const { return frames.size(); }
};
struct CrcCheckOp : CrcHandle {
    using Frames = DeframeOp::Frames;
    using FramesDev = DeframeOp::FramesDev;
    using Checked = CheckedOf<std::vector<uint8_t>, std::vector<int32_t>>;
    using CheckedDev = CheckedOf<DeviceBuf<uint8_t>, DeviceBuf<int32_t>>;
    CrcCheckOp(const char* who, const CrcSpec& format, int device) : CrcHandle(who, format, device) {}
    size_t in_frame_bytes() const { return coded_frame_bytes(); }
    size_t out_frame_bytes() const { return payload_frame_bytes(); }
    std::string kernel(size_t n_frames) const { return kernel_of(COMMS_CRC_CHECK, n_frames); }  // "crc_check_kernel ..."

protected:
    Result<Checked> check(const Frames& in) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        Checked out{{std::vector<uint8_t>(in.size() * out_frame_bytes()), in.headers, out_frame_bytes()}, std::vector<int32_t>(in.size())};
        return ok_or(comms_crc_check_run(h_.get(), in.data.data(), in.size(), out.frames.data.data(), out.passed.data(), nullptr, nullptr), out);
    }
    Result<CheckedDev> check_dev(const FramesDev& in, const DevStream& on) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        const size_t n = in.size();
        CheckedDev out{{DeviceBuf<uint8_t>(n ? n * out_frame_bytes() : 8, on.device()), in.headers, out_frame_bytes()},
                       DeviceBuf<int32_t>(n ? n : 2, on.device())};
        comms_status_t st = on.submit(in.data, out.frames.data, [&](void* s) {
            return comms_crc_check_run_dev(h_.get(), in.data.ptr(), n, out.frames.data.ptr(), out.passed.ptr(), nullptr, nullptr, s);
        });
        if (st == COMMS_OK) st = comms_buf_record_ready(out.passed.raw(), on.get());   // the same launch wrote the flags
        return ok_or(st, out);
    }
};
class CrcCheckNode : public DeriveNode<CrcCheckNode>, public Ports<CrcCheckOp::Frames, CrcCheckOp::Checked>, public CrcCheckOp {
public:
    explicit CrcCheckNode(const CrcSpec& format, int device = 0) : CrcCheckOp("CrcCheckNode::new", format, device) {}
    Result<Checked> run(const Frames& in) { return check(in); }
};
// on device-resident messages: ViterbiNodeDev's records in, the payload records and the flags in DeviceBufs out (headers on the host)
class CrcCheckNodeDev : public DeriveNode<CrcCheckNodeDev>, public Ports<CrcCheckOp::FramesDev, CrcCheckOp::CheckedDev>, public OnStream<CrcCheckOp> {
public:
    explicit CrcCheckNodeDev(const CrcSpec& format, int device = 0) : OnStream(device, "CrcCheckNodeDev::new", format, device) {}
    Result<CheckedDev> run(const FramesDev& in) { return check_dev(in, *this); }
};

// Symbol mapper and soft demapper (comms_symmap_*, comms_demap_*; additional nodes): the constellation stages of a coded link with
// 1 ... 8 bits per symbol.  One description per operation, two shells each.
inline std::vector<Complex32> qam_table(int bits_per_sym, double scale = 1.0) {
    std::vector<Complex32> t(size_t(1) << (bits_per_sym >= 0 && bits_per_sym <= 8 ? bits_per_sym : 0));
    throw_on(comms_constellation_qam(bits_per_sym, scale, reinterpret_cast<comms_c32*>(t.data())), "qam_table");
    return t;
}
inline std::vector<Complex32> psk_table(int bits_per_sym, double scale = 1.0) {
    std::vector<Complex32> t(size_t(1) << (bits_per_sym >= 0 && bits_per_sym <= 8 ? bits_per_sym : 0));
    throw_on(comms_constellation_psk(bits_per_sym, scale, reinterpret_cast<comms_c32*>(t.data())), "psk_table");
    return t;
}
struct SymbolMapSpec {
    int bits_per_sym;                      // m, 1 ... 8
    std::vector<Complex32> constellation;  // 2^m points; empty = digital.rs's tables (m <= 2)
    size_t n_bits;                         // E bits per input record (RateMatchNode's n_tx_bits())
    std::vector<Complex32> word = {};      // sent in front of every frame's symbols
    size_t gap = 0;                        // zero symbols behind them
};
// Map: a message is whole records of n_bits packed bits (in_frame_bytes() each: RateMatchNode's output as it stands), the output
// out_frame_syms() symbols per record -- word, payload, gap -- which PulseNode takes.
struct SymbolMapOp {
    using In = uint8_t;
    using Out = Complex32;
    SymbolMapOp(const char* who, const SymbolMapSpec& f, int device) {
        if (!f.constellation.empty() && f.bits_per_sym >= 1 && f.bits_per_sym <= 8 && f.constellation.size() != size_t(1) << f.bits_per_sym)
            throw std::runtime_error(std::string(who) + ": the constellation holds 2^bits_per_sym points");
        h_ = create<decltype(h_)>(who, comms_symmap_create, static_cast<int32_t>(f.bits_per_sym),
                                  f.constellation.empty() ? nullptr : reinterpret_cast<const comms_c32*>(f.constellation.data()), f.n_bits,
                                  f.word.empty() ? nullptr : reinterpret_cast<const comms_c32*>(f.word.data()), f.word.size(), f.gap, device);
    }
    size_t in_frame_bytes() const { return comms_symmap_in_frame_bytes(h_.get()); }
    size_t out_frame_syms() const { return comms_symmap_out_frame_syms(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_name(comms_symmap_get_kernel, h_.get(), n_frames); }  // "symmap_kernel ..."

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        if (n % in_frame_bytes()) return COMMS_ERR_ARG;
        m = n / in_frame_bytes() * out_frame_syms();
        return COMMS_OK;
    }
    comms_status_t launch(const uint8_t* in, size_t n, Complex32* out) {
        return comms_symmap_run(h_.get(), in, n / in_frame_bytes(), reinterpret_cast<comms_c32*>(out));
    }
    comms_status_t launch_dev(const uint8_t* in, size_t n, Complex32* out, void* s) {
        return comms_symmap_run_dev(h_.get(), in, n / in_frame_bytes(), reinterpret_cast<comms_c32*>(out), s);
    }
    Owned<comms_symmap_t, comms_symmap_destroy> h_;
};
class SymbolMapNode : public HostNode<SymbolMapNode, SymbolMapOp> {
public:
    explicit SymbolMapNode(const SymbolMapSpec& format, int device = 0) : HostNode("SymbolMapNode::new", format, device) {}
};
class SymbolMapNodeDev : public DevNode<SymbolMapNodeDev, SymbolMapOp> {
public:
    explicit SymbolMapNodeDev(const SymbolMapSpec& format, int device = 0) : DevNode(device, "SymbolMapNodeDev::new", format, device) {}
};

// Demap: takes DeframeNode's message in the COMMS_SYM_C32 format (records of n_payload symbols, normalised to the table's scale)
// and sends records of max-log LLRs (COMMS_SYM_LLR: n_payload * bits_per_sym f32, RateDematchNode's input with that record_llrs)
// or packed hard bits (COMMS_SYM_BITS) under the same headers.  A message without frames passes through empty.
struct DemapSpec {
    int bits_per_sym;
    std::vector<Complex32> constellation;  // 2^m points; empty = digital.rs's tables (m <= 2)
    size_t n_payload;                      // F symbols per record
    int32_t format = COMMS_SYM_LLR;
    float llr_scale = 1.0f;                // 1 / (2 sigma^2) at the table's scale
    bool force_table = false;              // COMMS_DEMAP_TABLE: the general kernel form for a separable table too
};
struct DemapOp {
    using Frames = DeframeOp::Frames;
    using FramesDev = DeframeOp::FramesDev;
    DemapOp(const char* who, const DemapSpec& f, int device) {
        if (!f.constellation.empty() && f.bits_per_sym >= 1 && f.bits_per_sym <= 8 && f.constellation.size() != size_t(1) << f.bits_per_sym)
            throw std::runtime_error(std::string(who) + ": the constellation holds 2^bits_per_sym points");
        h_ = create<decltype(h_)>(who, comms_demap_create, static_cast<int32_t>(f.bits_per_sym),
                                  f.constellation.empty() ? nullptr : reinterpret_cast<const comms_c32*>(f.constellation.data()), f.n_payload,
                                  static_cast<int32_t>(f.force_table ? COMMS_DEMAP_TABLE : 0), device);
        throw_on(comms_demap_set_output_format(h_.get(), f.format), who);
        throw_on(comms_demap_set_llr_scale(h_.get(), f.llr_scale), who);
    }
    size_t in_frame_bytes() const { return comms_demap_in_frame_bytes(h_.get()); }
    size_t out_frame_bytes() const { return comms_demap_out_frame_bytes(h_.get()); }
    std::string kernel(size_t n_frames) const { return kernel_name(comms_demap_get_kernel, h_.get(), n_frames); }  // "demap_table_kernel ..." | "demap_axis_kernel ..."

protected:
    Result<Frames> demap(const Frames& in) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        Frames out{std::vector<uint8_t>(in.size() * out_frame_bytes()), in.headers, out_frame_bytes()};
        return ok_or(comms_demap_run(h_.get(), reinterpret_cast<const comms_c32*>(in.data.data()), in.size(), out.data.data()), out);
    }
    Result<FramesDev> demap_dev(const FramesDev& in, const DevStream& on) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        FramesDev out{DeviceBuf<uint8_t>(in.size() ? in.size() * out_frame_bytes() : 16, on.device()), in.headers, out_frame_bytes()};
        return ok_or(on.submit(in.data, out.data, [&](void* s) {
            return comms_demap_run_dev(h_.get(), reinterpret_cast<const comms_c32*>(in.data.ptr()), in.size(), out.data.ptr(), s);
        }), out);
    }
    Owned<comms_demap_t, comms_demap_destroy> h_;
};
class DemapNode : public DeriveNode<DemapNode>, public Ports<DemapOp::Frames, DemapOp::Frames>, public DemapOp {
public:
    explicit DemapNode(const DemapSpec& format, int device = 0) : DemapOp("DemapNode::new", format, device) {}
    Result<Frames> run(const Frames& in) { return demap(in); }
};
// on device-resident messages: DeframeNodeDev's records in, the demapped records in a DeviceBuf out (headers on the host)
class DemapNodeDev : public DeriveNode<DemapNodeDev>, public Ports<DemapOp::FramesDev, DemapOp::FramesDev>, public OnStream<DemapOp> {
public:
    explicit DemapNodeDev(const DemapSpec& format, int device = 0) : OnStream(device, "DemapNodeDev::new", format, device) {}
    Result<FramesDev> run(const FramesDev& in) { return demap_dev(in, *this); }
};

// OFDM modulator and demodulator (comms_ofdm_*; additional nodes): the step between SymbolMapNode and DemapNode.  One description
// of the frame format, one operation per direction, two shells each.
struct OfdmSpec {
    int n_fft;                             // 64, 128, 256, 512 or 1024
    int n_cp;                              // 0 ... n_fft
    std::vector<uint8_t> carrier_kind;     // n_fft entries, bin 0 = DC: COMMS_OFDM_NULL / _DATA / _PILOT
    std::vector<Complex32> pilots = {};    // one per pilot carrier, increasing bin order
    std::vector<float> polarity = {};      // pilots of data symbol s times polarity[s mod size]; empty = 1
    std::vector<Complex32> train = {};     // n_fft frequency values of the training symbols (n_train > 0)
    size_t n_train = 0;                    // identical training symbols in front of every frame
    size_t n_syms = 1;                     // data symbols per frame
    bool cpe = false;                      // COMMS_OFDM_CPE: the demodulator removes the pilots' common phase per symbol
    float tx_scale = 0.0f;                 // 0 = the default, 1 / sqrt(n_fft)
};
template <bool MOD>
struct OfdmOp {
    using In = Complex32;
    using Out = Complex32;
    OfdmOp(const char* who, const OfdmSpec& f, int device) {
        if (f.n_fft < 0 || f.carrier_kind.size() != static_cast<size_t>(f.n_fft))
            throw std::runtime_error(std::string(who) + ": carrier_kind holds one entry per bin");
        size_t q = 0;
        for (uint8_t k : f.carrier_kind) q += k == COMMS_OFDM_PILOT;
        if (f.pilots.size() != q) throw std::runtime_error(std::string(who) + ": pilots holds one value per pilot carrier");
        if ((f.n_train || !f.train.empty()) && f.train.size() != f.carrier_kind.size())
            throw std::runtime_error(std::string(who) + ": train holds one value per bin");
        h_ = create<decltype(h_)>(who, comms_ofdm_create, static_cast<int32_t>(f.n_fft), static_cast<int32_t>(f.n_cp), f.carrier_kind.data(),
                                  f.pilots.empty() ? nullptr : reinterpret_cast<const comms_c32*>(f.pilots.data()),
                                  f.polarity.empty() ? nullptr : f.polarity.data(), f.polarity.size(),
                                  f.train.empty() ? nullptr : reinterpret_cast<const comms_c32*>(f.train.data()), f.n_train, f.n_syms,
                                  static_cast<int32_t>(f.cpe ? COMMS_OFDM_CPE : 0), device);
        if (f.tx_scale != 0.0f) throw_on(comms_ofdm_set_scale(h_.get(), f.tx_scale), who);
    }
    size_t data_syms() const { return comms_ofdm_data_syms(h_.get()); }
    size_t frame_samples() const { return comms_ofdm_frame_samples(h_.get()); }
    size_t in_frame() const { return MOD ? data_syms() : frame_samples(); }
    size_t out_frame() const { return MOD ? frame_samples() : data_syms(); }
    std::string kernel(size_t n_frames) const {   // "ofdm_mod_kernel<N> ..." | "ofdm_demod_kernel<N> ..."
        constexpr int32_t direction = MOD ? COMMS_OFDM_MOD : COMMS_OFDM_DEMOD;
        return kernel_name([](const comms_ofdm_t* h, size_t n, char* name, size_t len) { return comms_ofdm_get_kernel(h, direction, n, name, len); },
                           h_.get(), n_frames);
    }

protected:
    comms_status_t prepare(size_t n, size_t& m) const {
        if (n % in_frame()) return COMMS_ERR_ARG;
        m = n / in_frame() * out_frame();
        return COMMS_OK;
    }
    comms_status_t launch(const Complex32* in, size_t n, Complex32* out) {
        const auto* i = reinterpret_cast<const comms_c32*>(in);
        auto* o = reinterpret_cast<comms_c32*>(out);
        return MOD ? comms_ofdm_mod_run(h_.get(), i, n / in_frame(), o) : comms_ofdm_demod_run(h_.get(), i, n / in_frame(), o);
    }
    comms_status_t launch_dev(const Complex32* in, size_t n, Complex32* out, void* s) {
        const auto* i = reinterpret_cast<const comms_c32*>(in);
        auto* o = reinterpret_cast<comms_c32*>(out);
        return MOD ? comms_ofdm_mod_run_dev(h_.get(), i, n / in_frame(), o, s) : comms_ofdm_demod_run_dev(h_.get(), i, n / in_frame(), o, s);
    }
    Owned<comms_ofdm_t, comms_ofdm_destroy> h_;
};
// OfdmMod: a message is whole records of data_syms() data-carrier values (SymbolMapNode's output with no word and no gap), the
// output frame_samples() time samples per record.  OfdmDemod: the reverse, equalised; its output is DemapNode's input.
class OfdmModNode : public HostNode<OfdmModNode, OfdmOp<true>> {
public:
    explicit OfdmModNode(const OfdmSpec& format, int device = 0) : HostNode("OfdmModNode::new", format, device) {}
};
class OfdmModNodeDev : public DevNode<OfdmModNodeDev, OfdmOp<true>> {
public:
    explicit OfdmModNodeDev(const OfdmSpec& format, int device = 0) : DevNode(device, "OfdmModNodeDev::new", format, device) {}
};
class OfdmDemodNode : public HostNode<OfdmDemodNode, OfdmOp<false>> {
public:
    explicit OfdmDemodNode(const OfdmSpec& format, int device = 0) : HostNode("OfdmDemodNode::new", format, device) {}
};
class OfdmDemodNodeDev : public DevNode<OfdmDemodNodeDev, OfdmOp<false>> {
public:
    explicit OfdmDemodNodeDev(const OfdmSpec& format, int device = 0) : DevNode(device, "OfdmDemodNodeDev::new", format, device) {}
};

// OfdmDemodCsi: the demodulator behind OfdmCfoCorrectNode with its channel state (comms_ofdm_demod_csi_run; n_train >= 1).  Takes
// the frame message (records of frame_samples() samples) and sends the equalised records under the same headers together with
// one record of data_carriers() floats per frame, |H_k|^2 of every data carrier -- WeightedDemapNode's input.  A message without
// frames passes through empty.
template <class Store, class Csi>
struct EqualisedOf {
    FramesOf<Store> frames;   // the equalised records, frame_bytes = data_syms() * sizeof(Complex32)
    Csi csi;                  // csi_period floats per frame
    size_t csi_period = 0;
    size_t size() const { return frames.size(); }
};
struct OfdmDemodCsiOp : OfdmOp<false> {
    using Frames = DeframeOp::Frames;
    using FramesDev = DeframeOp::FramesDev;
    using Equalised = EqualisedOf<std::vector<uint8_t>, std::vector<float>>;
    using EqualisedDev = EqualisedOf<DeviceBuf<uint8_t>, DeviceBuf<float>>;
    OfdmDemodCsiOp(const char* who, const OfdmSpec& f, int device) : OfdmOp<false>(who, f, device) {
        for (uint8_t k : f.carrier_kind) carriers_ += k == COMMS_OFDM_DATA;
        if (!f.n_train) throw std::runtime_error(std::string(who) + ": the channel state needs a training symbol");
    }
    size_t data_carriers() const { return carriers_; }
    size_t in_frame_bytes() const { return frame_samples() * sizeof(Complex32); }
    size_t out_frame_bytes() const { return data_syms() * sizeof(Complex32); }

protected:
    Result<Equalised> demod(const Frames& in) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        Equalised out{{std::vector<uint8_t>(in.size() * out_frame_bytes()), in.headers, out_frame_bytes()}, std::vector<float>(in.size() * carriers_), carriers_};
        return ok_or(comms_ofdm_demod_csi_run(h_.get(), reinterpret_cast<const comms_c32*>(in.data.data()), in.size(),
                                              reinterpret_cast<comms_c32*>(out.frames.data.data()), out.csi.data()), out);
    }
    Result<EqualisedDev> demod_dev(const FramesDev& in, const DevStream& on) {
        if (in.frame_bytes != in_frame_bytes() || in.data.size() < in.size() * in.frame_bytes) return NodeError::DataError;
        const size_t n = in.size();
        EqualisedDev out{{DeviceBuf<uint8_t>(n ? n * out_frame_bytes() : 8, on.device()), in.headers, out_frame_bytes()},
                         DeviceBuf<float>(n ? n * carriers_ : 2, on.device()), carriers_};
        comms_status_t st = on.submit(in.data, out.frames.data, [&](void* s) {
            return comms_ofdm_demod_csi_run_dev(h_.get(), reinterpret_cast<const comms_c32*>(in.data.ptr()), n,
                                                reinterpret_cast<comms_c32*>(out.frames.data.ptr()), out.csi.ptr(), s);
        });
        if (st == COMMS_OK) st = comms_buf_record_ready(out.csi.raw(), on.get());   // the same launch wrote the channel state
        return ok_or(st, out);
    }
    size_t carriers_ = 0;
};
class OfdmDemodCsiNode : public DeriveNode<OfdmDemodCsiNode>, public Ports<OfdmDemodCsiOp::Frames, OfdmDemodCsiOp::Equalised>, public OfdmDemodCsiOp {
public:
    explicit OfdmDemodCsiNode(const OfdmSpec& format, int device = 0) : OfdmDemodCsiOp("OfdmDemodCsiNode::new", format, device) {}
    Result<Equalised> run(const Frames& in) { return demod(in); }
};
class OfdmDemodCsiNodeDev : public DeriveNode<OfdmDemodCsiNodeDev>, public Ports<OfdmDemodCsiOp::FramesDev, OfdmDemodCsiOp::EqualisedDev>, public OnStream<OfdmDemodCsiOp> {
public:
    explicit OfdmDemodCsiNodeDev(const OfdmSpec& format, int device = 0) : OnStream(device, "OfdmDemodCsiNodeDev::new", format, device) {}
    Result<EqualisedDev> run(const FramesDev& in) { return demod_dev(in, *this); }
};

// WeightedDemap: takes OfdmDemodCsiNode's message -- symbol records and csi_period weights per frame -- and sends the LLR records
// of comms_demap_run_weighted under the same headers: symbol j of a frame is scaled by llr_scale * csi[j mod csi_period] and
// erased (+0.0) where that weight is not finite and positive.  The spec's format stays COMMS_SYM_LLR.
struct WeightedDemapOp : DemapOp {
    using Equalised = OfdmDemodCsiOp::Equalised;
    using EqualisedDev = OfdmDemodCsiOp::EqualisedDev;
    WeightedDemapOp(const char* who, const DemapSpec& f, int device) : DemapOp(who, f, device) {
        if (f.format != COMMS_SYM_LLR) throw std::runtime_error(std::string(who) + ": weighted demapping gives LLRs");
    }

protected:
    template <class E>
    bool fits(const E& in) const {
        return in.frames.frame_bytes == in_frame_bytes() && in.frames.data.size() >= in.size() * in.frames.frame_bytes && in.csi_period >= 1 &&
               in.csi.size() >= in.size() * in.csi_period;
    }
    Result<Frames> demap_weighted(const Equalised& in) {
        if (!fits(in)) return NodeError::DataError;
        Frames out{std::vector<uint8_t>(in.size() * out_frame_bytes()), in.frames.headers, out_frame_bytes()};
        return ok_or(comms_demap_run_weighted(h_.get(), reinterpret_cast<const comms_c32*>(in.frames.data.data()), in.csi.data(), in.csi_period,
                                              in.size(), out.data.data()), out);
    }
    Result<FramesDev> demap_weighted_dev(const EqualisedDev& in, const DevStream& on) {
        if (!fits(in)) return NodeError::DataError;
        FramesDev out{DeviceBuf<uint8_t>(in.size() ? in.size() * out_frame_bytes() : 16, on.device()), in.frames.headers, out_frame_bytes()};
        comms_status_t st = on.wait(in.csi);   // the weights' producer, beside the symbols' (submit waits for that one)
        if (st == COMMS_OK)
            st = on.submit(in.frames.data, out.data, [&](void* s) {
                return comms_demap_run_weighted_dev(h_.get(), reinterpret_cast<const comms_c32*>(in.frames.data.ptr()), in.csi.ptr(), in.csi_period,
                                                    in.size(), out.data.ptr(), s);
            });
        if (st == COMMS_OK) st = comms_buf_record_use(in.csi.raw(), on.get());
        return ok_or(st, out);
    }
};
class WeightedDemapNode : public DeriveNode<WeightedDemapNode>, public Ports<WeightedDemapOp::Equalised, WeightedDemapOp::Frames>, public WeightedDemapOp {
public:
    explicit WeightedDemapNode(const DemapSpec& format, int device = 0) : WeightedDemapOp("WeightedDemapNode::new", format, device) {}
    Result<Frames> run(const Equalised& in) { return demap_weighted(in); }
};
class WeightedDemapNodeDev : public DeriveNode<WeightedDemapNodeDev>, public Ports<WeightedDemapOp::EqualisedDev, WeightedDemapOp::FramesDev>, public OnStream<WeightedDemapOp> {
public:
    explicit WeightedDemapNodeDev(const DemapSpec& format, int device = 0) : OnStream(device, "WeightedDemapNodeDev::new", format, device) {}
    Result<FramesDev> run(const EqualisedDev& in) { return demap_weighted_dev(in, *this); }
};

// OFDM stream synchroniser (comms_ofdmsync_*; additional nodes): what stands between a received sample stream and OfdmDemodNode.
//   stream -> OfdmSyncNode -+- detections -> DeframeNode (COMMS_SYM_C32, n_payload = frame_samples, offset 0, lookback())
//                            +- output ----------------------+-> OfdmCfoCorrectNode -> OfdmDemodNode
// OfdmSyncNode takes the sample blocks and sends, per block, the frame starts that the block decides -- possibly none -- with
// the carrier-frequency offset of each (rad / sample): the whole message on `output`, the detections alone on `detections`,
// which is what DeframeNode's second receiver takes.  A block of n samples decides n positions; flush() ends a stream; the
// message does not depend on how the stream is cut into blocks.  It is a host value on either message kind (the call
// synchronises its stream): run() bodies of their own, as the frame synchroniser's.
struct OfdmSyncSpec {
    size_t lag;            // 1 ... 2048: distance of the two correlated windows
    size_t window;         // 2 ... 2048: their length
    double threshold;      // 0 < threshold <= 1
    size_t guard;          // <= 512: half-width of the peak search
    size_t advance = 0;    // <= 2048: samples by which `index` lies ahead of the peak, into the prefix
    // the frames of an OfdmModNode / OfdmDemodNode format with n_train >= 2: lag = window = n_fft + n_cp
    static OfdmSyncSpec for_format(const OfdmSpec& f, double threshold, size_t guard, size_t advance = 0) {
        const size_t sym = static_cast<size_t>(f.n_fft) + static_cast<size_t>(f.n_cp);
        return OfdmSyncSpec{sym, sym, threshold, guard, advance};
    }
    size_t lookback() const { return window + lag + guard + advance - 1; }  // the least `lookback` of the DeframeNode behind
};
struct OfdmSyncFound {
    FrameSyncOp::Detections detections;  // ascending index
    std::vector<double> cfo;             // one per detection: atan2(corr_im, corr_re) / lag
    size_t size() const { return detections.size(); }
    operator FrameSyncOp::Detections() const { return detections; }
};
struct OfdmSyncOp {
    OfdmSyncOp(const char* who, const OfdmSyncSpec& f, int device)
        : h_(create<decltype(h_)>(who, comms_ofdmsync_create, f.lag, f.window, f.threshold, f.guard, f.advance, size_t(0), static_cast<int32_t>(device))),
          spec_(f) {}
    Result<OfdmSyncFound> flush() {  // a flush decides window + lag + guard positions
        return collect(spec_.window + spec_.lag + spec_.guard,
                       [&](auto* out, double* cfo, size_t cap, size_t* found) { return comms_ofdmsync_flush(h_.get(), out, cfo, cap, found); });
    }
    size_t lookback() const { return spec_.lookback(); }
    uint64_t position() const {  // stream index of the next sample
        uint64_t t = 0;
        throw_on(comms_ofdmsync_get_position(h_.get(), &t), "OfdmSyncNode::position");
        return t;
    }
    std::string kernel(size_t n) const { return kernel_name(comms_ofdmsync_get_kernel, h_.get(), n); }  // "ofdmsync_detect_kernel ..."

protected:
    Result<OfdmSyncFound> detect(const Complex32* in, size_t n) {
        return collect(n, [&](auto* out, double* cfo, size_t cap, size_t* found) { return comms_ofdmsync_run(h_.get(), c32(in), n, out, cfo, cap, found); });
    }
    Result<OfdmSyncFound> detect_dev(const Complex32* in, size_t n, void* s) {
        return collect(n, [&](auto* out, double* cfo, size_t cap, size_t* found) {
            return comms_ofdmsync_run_dev(h_.get(), c32(in), n, out, cfo, cap, found, s);
        });
    }

private:
    // no call that decides n positions has more than (n + guard) / (guard + 1) detections: they are more than `guard` apart
    template <class F>
    Result<OfdmSyncFound> collect(size_t n, F&& call) {
        const size_t cap = (n + spec_.guard) / (spec_.guard + 1);
        OfdmSyncFound out{FrameSyncOp::Detections(cap), std::vector<double>(cap)};
        size_t found = 0;
        comms_status_t st = call(out.detections.data(), out.cfo.data(), cap, &found);
        if (st != COMMS_OK) return to_node_error(st);
        out.detections.resize(found);
        out.cfo.resize(found);
        return out;
    }
    Owned<comms_ofdmsync_t, comms_ofdmsync_destroy> h_;
    OfdmSyncSpec spec_;
};
template <class In>
struct OfdmSyncPorts {  // as Ports, with the second sender
    NodeReceiver<In> input;
    NodeSender<OfdmSyncFound> output;
    NodeSender<FrameSyncOp::Detections> detections;
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output, detections); }
};
class OfdmSyncNode : public DeriveNode<OfdmSyncNode>, public OfdmSyncPorts<std::vector<Complex32>>, public OfdmSyncOp {
public:
    explicit OfdmSyncNode(const OfdmSyncSpec& spec, int device = 0) : OfdmSyncOp("OfdmSyncNode::new", spec, device) {}
    Result<OfdmSyncFound> run(const std::vector<Complex32>& samples) { return detect(samples.data(), samples.size()); }
};
class OfdmSyncNodeDev : public DeriveNode<OfdmSyncNodeDev>, public OfdmSyncPorts<DeviceBuf<Complex32>>, public OnStream<OfdmSyncOp> {
public:
    explicit OfdmSyncNodeDev(const OfdmSyncSpec& spec, int device = 0) : OnStream(device, "OfdmSyncNodeDev::new", spec, device) {}
    Result<OfdmSyncFound> run(const DeviceBuf<Complex32>& in) {
        comms_status_t st = wait(in);
        if (st != COMMS_OK) return to_node_error(st);
        return detect_dev(in.ptr(), in.size(), get());
    }
};

// The correct stage (comms_ofdmsync_correct_*): takes DeframeNode's message in the COMMS_SYM_C32 format (records of n_frame
// samples) and, on a second receiver, what OfdmSyncNode sent on `output` for the same block; sends record f times
// exp(-i cfo n) under the same headers, all records of a message by one launch -- OfdmDemodNode's input once `data` is read as
// samples.  A frame's offset arrives with its detection and is kept until its record does (a record ends in a later block than
// its detection); a record whose detection was never seen is a DataError.  A message without frames passes through empty.
struct OfdmCfoCorrectOp {
    using Frames = DeframeOp::Frames;
    using FramesDev = DeframeOp::FramesDev;
    OfdmCfoCorrectOp(const char* who, size_t n_frame, int device) : n_frame_(n_frame) {
        if (n_frame == 0) throw std::runtime_error(std::string(who) + ": n_frame is 1 ... 2^20");
        // the handle's detect stage is not used: the least lag and window
        h_ = create<decltype(h_)>(who, comms_ofdmsync_create, size_t(1), size_t(2), 1.0, size_t(0), size_t(0), n_frame, static_cast<int32_t>(device));
    }
    size_t frame_bytes() const { return n_frame_ * sizeof(Complex32); }

protected:
    Result<Frames> correct(const Frames& in, const OfdmSyncFound& found) {
        std::vector<double> cfo;
        if (!match(in.headers, in.frame_bytes, in.data.size(), found, cfo)) return NodeError::DataError;
        Frames out{std::vector<uint8_t>(in.size() * frame_bytes()), in.headers, frame_bytes()};
        return ok_or(comms_ofdmsync_correct_run(h_.get(), reinterpret_cast<const comms_c32*>(in.data.data()), in.size(), cfo.data(),
                                                reinterpret_cast<comms_c32*>(out.data.data())), out);
    }
    Result<FramesDev> correct_dev(const FramesDev& in, const OfdmSyncFound& found, const DevStream& on) {
        std::vector<double> cfo;
        if (!match(in.headers, in.frame_bytes, in.data.size(), found, cfo)) return NodeError::DataError;
        FramesDev out{DeviceBuf<uint8_t>(in.size() ? in.size() * frame_bytes() : 16, on.device()), in.headers, frame_bytes()};
        return ok_or(on.submit(in.data, out.data, [&](void* s) {
            return comms_ofdmsync_correct_run_dev(h_.get(), reinterpret_cast<const comms_c32*>(in.data.ptr()), in.size(), cfo.data(),
                                                  reinterpret_cast<comms_c32*>(out.data.ptr()), s);
        }), out);
    }

private:
    // the offsets of the message's records, by index; records come in ascending index, so what lies before a matched
    // detection belongs to frames that the deframer dropped
    bool match(const std::vector<comms_deframe_header_t>& headers, size_t in_frame_bytes, size_t bytes, const OfdmSyncFound& found,
               std::vector<double>& cfo) {
        if (found.cfo.size() != found.detections.size() || in_frame_bytes != frame_bytes() || bytes < headers.size() * in_frame_bytes) return false;
        for (size_t i = 0; i < found.size(); ++i) pending_.emplace_back(found.detections[i].index, found.cfo[i]);
        cfo.reserve(headers.size());
        for (const comms_deframe_header_t& hd : headers) {
            size_t at = 0;
            while (at < pending_.size() && pending_[at].first != hd.index) ++at;
            if (at == pending_.size()) return false;
            cfo.push_back(pending_[at].second);
            pending_.erase(pending_.begin(), pending_.begin() + static_cast<std::ptrdiff_t>(at) + 1);
        }
        return true;
    }
    Owned<comms_ofdmsync_t, comms_ofdmsync_destroy> h_;
    size_t n_frame_;
    std::vector<std::pair<uint64_t, double>> pending_;  // (index, cfo) of the detections whose records are still to come
};
template <class FramesT>
struct OfdmCfoCorrectPorts {  // as Ports, with the second receiver
    NodeReceiver<FramesT> input;          // DeframeNode's message
    NodeReceiver<OfdmSyncFound> found;    // OfdmSyncNode's message for the same block
    NodeSender<FramesT> output;
    auto receivers() { return std::tie(input, found); }
    auto senders() { return std::tie(output); }
};
class OfdmCfoCorrectNode : public DeriveNode<OfdmCfoCorrectNode>, public OfdmCfoCorrectPorts<OfdmCfoCorrectOp::Frames>, public OfdmCfoCorrectOp {
public:
    explicit OfdmCfoCorrectNode(size_t n_frame, int device = 0) : OfdmCfoCorrectOp("OfdmCfoCorrectNode::new", n_frame, device) {}
    Result<Frames> run(const Frames& in, const OfdmSyncFound& found) { return correct(in, found); }
};
// on device-resident messages: DeframeNodeDev's records in, the corrected records in a DeviceBuf out (headers on the host)
class OfdmCfoCorrectNodeDev : public DeriveNode<OfdmCfoCorrectNodeDev>, public OfdmCfoCorrectPorts<OfdmCfoCorrectOp::FramesDev>, public OnStream<OfdmCfoCorrectOp> {
public:
    explicit OfdmCfoCorrectNodeDev(size_t n_frame, int device = 0) : OnStream(device, "OfdmCfoCorrectNodeDev::new", n_frame, device) {}
    Result<FramesDev> run(const FramesDev& in, const OfdmSyncFound& found) { return correct_dev(in, found, *this); }
};

// NcoNode::new(dphase, Option<phase>) (src/demodulation/nco.rs:118-133) in block form: one
// message is a vector of phase errors, the output is exp(i*phase) per sample.  (The reference
// node is per sample, f64 -> Complex<f64>; a closed loop runs it at block rate here.)
struct NcoOp : protected SameLength {
    using In = double;
    using Out = Complex64;
    NcoOp(const char* who, double dphase, double phase, int device) : h_(create<decltype(h_)>(who, comms_nco_create, dphase, phase, device)) {}

protected:
    comms_status_t launch(const double* perr, size_t n, Complex64* out) { return comms_nco_run(h_.get(), perr, n, reinterpret_cast<double*>(out)); }
    Owned<comms_nco_t, comms_nco_destroy> h_;
};
class BatchNcoNode : public HostNode<BatchNcoNode, NcoOp> {
public:
    explicit BatchNcoNode(double dphase, double phase = 0.0, int device = 0) : HostNode("NcoNode::new", dphase, phase, device) {}
};

inline std::vector<double> qfilt_taps(uint32_t n_taps, double alpha, uint32_t sam_per_sym) {
    std::vector<double> t(comms_qfilt_len(n_taps));
    throw_on(comms_qfilt_taps(n_taps, alpha, sam_per_sym, t.data()), "qfilt_taps");
    return t;
}

// ---------------------------------------------------------------- stream shards
// One long stream over several GPUs, one node set per GPU: contiguous shards and one hand-over of the raw samples
// in front of each shard.  Thin wrappers of the C entries (csrc/shard.cpp), so that a C++ host cuts a stream exactly
// as bench.py / sharding.py do.
inline std::pair<size_t, size_t> shard_range(size_t total, unsigned world, unsigned rank) {
    size_t a = 0, b = 0;
    throw_on(comms_shard_range(total, world, rank, &a, &b), "shard_range");
    return {a, b};
}
// the n samples before a shard, time order -> BatchFirNode::new(taps, Some(state)) (fir_node.rs:193-211)
inline std::vector<Complex32> state_from_halo(const std::vector<Complex32>& halo) {
    std::vector<Complex32> st(halo.size());
    throw_on(comms_state_from_halo(c32(halo.data()), halo.size(), c32(st.data())), "state_from_halo");
    return st;
}
// oscillator phase of stream sample first_index: MixerNode::new(dphase, Some(phase)) of the shard's node
inline double shard_mixer_phase(double phase0, double dphase, long long first_index) {
    double ph = 0.0;
    throw_on(comms_shard_mixer_phase(phase0, dphase, first_index, &ph), "shard_mixer_phase");
    return ph;
}
// raw samples a chain shard runs through first (outputs dropped): FIR history + the sample FM.prev comes from
inline size_t chain_prefix_len(size_t n_taps, size_t rate, bool fm_demod) {
    size_t n = 0;
    throw_on(comms_chain_prefix_len(n_taps, rate, fm_demod ? 1 : 0, &n), "chain_prefix_len");
    return n;
}

// mixer / FIR / decimate [/ FM demod] as ONE node on device-resident messages.  Out = Complex32 without FM demod, float with it.
template <class Out>
class ChainNodeDev : public DevNode<ChainNodeDev<Out>, ChainOp<Complex32, Out>> {
public:
    static constexpr bool kFm = std::is_same<Out, float>::value;
    ChainNodeDev(double dphase, double phase, const std::vector<Complex32>& taps, size_t rate, bool mixer_after_fir = false, int device = 0)
        : ChainNodeDev::DevNode(device, "ChainNodeDev::new", dphase, phase, taps, rate,
                                (kFm ? COMMS_CHAIN_FM_DEMOD : 0) | (mixer_after_fir ? COMMS_CHAIN_MIXER_AFTER_FIR : 0), device) {}
};

}  // namespace comms
