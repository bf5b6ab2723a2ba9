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
// Messages are host vectors (std::vector<Complex>), moved through the channels by
// value as in the reference; every run() goes H2D -> kernel -> D2H through the C
// ABI.  The *Dev variants at the bottom keep messages device-resident
// (DeviceBuf<T>, clone = refcount bump) -- what the roofline numbers use.
//
// Error convention: comms_status_t 1 -> NodeError::DataError, 2 -> PermanentError.
// Constructors throw std::runtime_error when a handle cannot be created (the
// reference panics in the same places); there is no CPU fallback.
#pragma once

#include <cmath>
#include <limits>
#include <complex>
#include <cstring>
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

// ---------------------------------------------------------------- sample types
// What the C ABI offers per sample type, as the Rust shim's FirSample / MixSample / SpectralSample traits have it: the
// interleaved {re, im} struct, the handle types and the entry points.  Complex<i16> (wrapping arithmetic) has the FIR and
// the pulse shaper only.
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
    static constexpr auto fir_destroy = comms_fir_destroy;
    static constexpr auto pulse_create = comms_pulse_create;
    static constexpr auto pulse_run = comms_pulse_run;
    static constexpr auto pulse_destroy = comms_pulse_destroy;
    static constexpr auto mixer_run = comms_mixer_run;
    static constexpr auto fft_create = comms_fft_create;
    static constexpr auto fft_run = comms_fft_run;
    static constexpr auto fft_destroy = comms_fft_destroy;
    static constexpr auto fm_create = comms_fmdemod_create;
    static constexpr auto fm_run = comms_fmdemod_run;
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
template <class D, class T>
class BatchFirNodeOf : public DeriveNode<D> {
    using S = Sample<T>;

public:
    NodeReceiver<std::vector<T>> input;
    NodeSender<std::vector<T>> output;

    BatchFirNodeOf(const std::vector<T>& taps, const std::optional<std::vector<T>>& state = std::nullopt, int device = 0) {
        throw_on(S::fir_create(abi(taps.data()), taps.size(), state ? abi(state->data()) : nullptr, state ? state->size() : 0, device, &h_),
                 D::kNew);
    }
    BatchFirNodeOf(BatchFirNodeOf&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~BatchFirNodeOf() { S::fir_destroy(h_); }

    Result<std::vector<T>> run(const std::vector<T>& in) {
        std::vector<T> out(in.size());
        comms_status_t st = S::fir_run(h_, abi(in.data()), in.size(), abi(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }
    typename S::Fir* handle() const { return h_; }

private:
    typename S::Fir* h_ = nullptr;
};

template <class D, class T>
class FirNodeOf : public DeriveNode<D> {
    using S = Sample<T>;

public:
    NodeReceiver<T> input;
    NodeSender<T> output;

    FirNodeOf(const std::vector<T>& taps, const std::optional<std::vector<T>>& state = std::nullopt, int device = 0) {
        throw_on(S::fir_create(abi(taps.data()), taps.size(), state ? abi(state->data()) : nullptr, state ? state->size() : 0, device, &h_),
                 D::kNew);
    }
    FirNodeOf(FirNodeOf&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~FirNodeOf() { S::fir_destroy(h_); }

    Result<T> run(const T& in) {
        T out;
        comms_status_t st = S::fir_run(h_, abi(&in), 1, abi(&out));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    // the samples already queued behind the first one, in one launch (DeriveNode::call): the
    // filter's state runs through the block exactly as through the same samples one by one
    Result<std::vector<T>> run_block(const std::vector<T>& ins) {
        std::vector<T> out(ins.size());
        comms_status_t st = S::fir_run(h_, abi(ins.data()), ins.size(), abi(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    typename S::Fir* h_ = nullptr;
};

// ---------------------------------------------------------------- pulse shaping
template <class D, class T>
class PulseNodeOf : public DeriveNode<D> {
    using S = Sample<T>;

public:
    NodeReceiver<T> input;
    NodeSender<std::vector<T>> output;

    PulseNodeOf(const std::vector<T>& taps, size_t sam_per_sym, int device = 0) : sps_(sam_per_sym) {
        throw_on(S::pulse_create(abi(taps.data()), taps.size(), sam_per_sym, device, &h_), D::kNew);
    }
    PulseNodeOf(PulseNodeOf&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), sps_(o.sps_) { o.h_ = nullptr; }
    ~PulseNodeOf() { S::pulse_destroy(h_); }

    Result<std::vector<T>> run(const T& sym) {
        std::vector<T> out(sps_);
        comms_status_t st = S::pulse_run(h_, abi(&sym), 1, abi(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    // queued symbols in one launch; still one Vec of sam_per_sym samples per symbol downstream
    Result<std::vector<std::vector<T>>> run_block(const std::vector<T>& syms) {
        std::vector<T> flat(syms.size() * sps_);
        comms_status_t st = S::pulse_run(h_, abi(syms.data()), syms.size(), abi(flat.data()));
        if (st != COMMS_OK) return to_node_error(st);
        std::vector<std::vector<T>> out(syms.size());
        for (size_t i = 0; i < syms.size(); ++i) out[i].assign(flat.begin() + i * sps_, flat.begin() + (i + 1) * sps_);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

protected:
    typename S::Pulse* h_ = nullptr;

private:
    size_t sps_;
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
        throw_on(comms_pulse_set_mixer(h_, dphase, phase.value_or(0.0)), "PulseNode::with_mixer");
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

    PrnsNode(uint64_t poly_mask, uint64_t state, int width = 8, int device = 0) : start_(state) {
        throw_on(comms_prns_create(poly_mask, state, width, device, &h_), "PrnsNode::new");
    }
    PrnsNode(PrnsNode&& o) noexcept
        : output(std::move(o.output)), h_(o.h_), buf_(std::move(o.buf_)), pos_(o.pos_), start_(o.start_) { o.h_ = nullptr; }
    ~PrnsNode() { comms_prns_destroy(h_); }

    Result<uint8_t> run() {
        if (pos_ == buf_.size()) {
            uint64_t s = 0;
            comms_status_t st = comms_prns_get_state(h_, &s);
            buf_.resize(kBlock);
            if (st == COMMS_OK) st = comms_prns_run(h_, kBlock, COMMS_BITS_U8, buf_.data());
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
        throw_on(comms_prns_get_state(h_, &ahead), "PrnsNode::state");
        throw_on(comms_prns_set_state(h_, start_), "PrnsNode::state");
        throw_on(comms_prns_skip(h_, pos_), "PrnsNode::state");
        throw_on(comms_prns_get_state(h_, &s), "PrnsNode::state");
        throw_on(comms_prns_set_state(h_, ahead), "PrnsNode::state");
        return s;
    }
    auto receivers() { return std::tie(); }
    auto senders() { return std::tie(output); }

private:
    comms_prns_t* h_ = nullptr;
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

// CRTP base: D::draw(handle, n, out) draws n values (n a multiple of D::kGrain) from the stream position
template <class D, class T>
class NoiseSourceNode : public DeriveNode<D> {
public:
    NodeSender<T> output;
    static constexpr size_t kBlock = 4096;

    NoiseSourceNode(std::optional<uint64_t> seed, int device, const char* what) : seed_(seed ? *seed : entropy_seed()) {
        throw_on(comms_noise_create(seed_, 0, device, &h_), what);
    }
    NoiseSourceNode(NoiseSourceNode&& o) noexcept
        : output(std::move(o.output)), h_(o.h_), seed_(o.seed_), buf_(std::move(o.buf_)), pos_(o.pos_) { o.h_ = nullptr; }
    ~NoiseSourceNode() { comms_noise_destroy(h_); }

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

protected:
    comms_noise_t* h_ = nullptr;

private:
    comms_status_t refill(size_t n) {
        buf_.resize(n);
        pos_ = 0;
        comms_status_t st = static_cast<D&>(*this).draw(n, buf_.data());
        if (st != COMMS_OK) buf_.clear();
        return st;
    }
    uint64_t seed_;
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
    comms_status_t draw(size_t n, double* out) { return comms_noise_normal_f64_run(h_, n, mu_, sd_, out); }

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
    comms_status_t draw(size_t n, float* out) { return comms_noise_uniform_run(h_, n, lo_, hi_, out); }

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
    comms_status_t draw(size_t n, uint8_t* out) { return comms_noise_bits_run(h_, n, COMMS_BITS_U8, out); }
};

inline UniformNode<uint8_t> random_bit(std::optional<uint64_t> seed = std::nullopt, int device = 0) {
    return UniformNode<uint8_t>(0, 2, seed, device);
}

// AWGN channel (an additional node): out = in + sigma * (z + i z'), one complex standard pair per sample, the pairs of
// consecutive messages consecutive in the source's stream (comms_awgn_run)
class AwgnNode : public DeriveNode<AwgnNode> {
public:
    NodeReceiver<std::vector<Complex32>> input;
    NodeSender<std::vector<Complex32>> output;
    AwgnNode(float sigma, std::optional<uint64_t> seed = std::nullopt, uint64_t stream = 0, int device = 0) : sigma_(sigma) {
        throw_on(comms_noise_create(seed ? *seed : entropy_seed(), stream, device, &h_), "AwgnNode::new");
    }
    AwgnNode(AwgnNode&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), sigma_(o.sigma_) { o.h_ = nullptr; }
    ~AwgnNode() { comms_noise_destroy(h_); }
    Result<std::vector<Complex32>> run(const std::vector<Complex32>& in) {
        std::vector<Complex32> out(in.size());
        comms_status_t st = comms_awgn_run(h_, in.data(), in.size(), sigma_, c32(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_noise_t* h_ = nullptr;
    float sigma_;
};

// ---------------------------------------------------------------- a digital link from bits to bits (additional nodes)
// Transmit: packed bits (LSB first, bits_per_sym = 1 or 2 per symbol, whole bytes per message) -> constellation -> pulse
// shaping -> mixer -> (scale * y) as i16, one launch per message (comms_pulse_set_input_format / _set_output_format).
class PulseBitsNode : public DeriveNode<PulseBitsNode> {
public:
    NodeReceiver<std::vector<uint8_t>> input;
    NodeSender<std::vector<Complex16>> output;
    PulseBitsNode(const std::vector<Complex32>& taps, size_t sam_per_sym, int bits_per_sym, double dphase, float scale,
                  const std::vector<Complex32>& constellation = {}, int device = 0)
        : sps_(sam_per_sym), k_(bits_per_sym) {
        throw_on(comms_pulse_create(c32(taps.data()), taps.size(), sam_per_sym, device, &h_), "PulseBitsNode::new");
        try {
            throw_on(comms_pulse_set_mixer(h_, dphase, 0.0), "PulseBitsNode::new");
            throw_on(comms_pulse_set_input_format(h_, COMMS_SYM_BITS, bits_per_sym, constellation.empty() ? nullptr : c32(constellation.data())),
                     "PulseBitsNode::new");
            throw_on(comms_pulse_set_output_format(h_, COMMS_IQ_I16, scale), "PulseBitsNode::new");
        } catch (...) {
            comms_pulse_destroy(h_);
            throw;
        }
    }
    PulseBitsNode(PulseBitsNode&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), sps_(o.sps_), k_(o.k_) { o.h_ = nullptr; }
    ~PulseBitsNode() { comms_pulse_destroy(h_); }
    Result<std::vector<Complex16>> run(const std::vector<uint8_t>& packed) {
        const size_t n_sym = packed.size() * 8 / static_cast<size_t>(k_);
        std::vector<Complex16> out(n_sym * sps_);
        comms_status_t st = comms_pulse_run(h_, reinterpret_cast<const comms_c32*>(packed.data()), n_sym, c32_as(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    static comms_c32* c32_as(Complex16* p) { return reinterpret_cast<comms_c32*>(p); }
    comms_pulse_t* h_ = nullptr;
    size_t sps_;
    int k_;
};

// Receive: i16 samples -> mixer -> matched FIR -> keep every rate-th -> hard decisions -> packed bits (LSB first), one chain
// (comms_chain_set_input_format / _set_output_format): ceil(n / rate * bits_per_sym / 8) bytes per message, each message
// from bit 0 of its first byte -- whole bytes when n is a multiple of 8 * rate / bits_per_sym.
class ChainBitsNode : public DeriveNode<ChainBitsNode> {
public:
    NodeReceiver<std::vector<Complex16>> input;
    NodeSender<std::vector<uint8_t>> output;
    ChainBitsNode(double dphase, double phase, const std::vector<Complex32>& taps, size_t rate, int bits_per_sym, float in_scale,
                  const std::vector<Complex32>& constellation = {}, bool mixer_after_fir = false, int device = 0)
        : rate_(rate), k_(bits_per_sym) {
        throw_on(comms_chain_create_ex(dphase, phase, c32(taps.data()), taps.size(), rate, mixer_after_fir ? COMMS_CHAIN_MIXER_AFTER_FIR : 0,
                                       device, &h_),
                 "ChainBitsNode::new");
        try {
            throw_on(comms_chain_set_input_format(h_, COMMS_IQ_I16, in_scale), "ChainBitsNode::new");
            throw_on(comms_chain_set_output_format(h_, COMMS_SYM_BITS, bits_per_sym, constellation.empty() ? nullptr : c32(constellation.data())),
                     "ChainBitsNode::new");
        } catch (...) {
            comms_chain_destroy(h_);
            throw;
        }
    }
    ChainBitsNode(ChainBitsNode&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), rate_(o.rate_), k_(o.k_) { o.h_ = nullptr; }
    ~ChainBitsNode() { comms_chain_destroy(h_); }
    Result<std::vector<uint8_t>> run(const std::vector<Complex16>& in) {
        if (rate_ == 0 || in.size() % rate_) return NodeError::DataError;
        std::vector<uint8_t> out((in.size() / rate_ * static_cast<size_t>(k_) + 7) / 8);
        comms_status_t st = comms_chain_run(h_, reinterpret_cast<const comms_c32*>(in.data()), in.size(), out.data());
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    int fused_kind() const {  // as ChainNodeDev::fused_kind
        int32_t f = 0;
        comms_chain_is_fused(h_, &f);
        return f;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_chain_t* h_ = nullptr;
    size_t rate_;
    int k_;
};

// Real FIR + decimator over an f32 stream as ONE node (comms_rfir_*; an additional node): the results of the audio stage of
// examples/fm_radio.rs:98-164 -- Convert2Node -> BatchFirNode<f32> -> Convert3Node -> DecimateNode<f32>(rate) -- for real
// taps.  Any message length: ceil(n / rate) outputs, the decimator restarting with every message as DecimateNode does.
class RealFirDecimNode : public DeriveNode<RealFirDecimNode> {
public:
    NodeReceiver<std::vector<float>> input;
    NodeSender<std::vector<float>> output;
    RealFirDecimNode(const std::vector<float>& taps, size_t rate, const std::optional<std::vector<float>>& state = std::nullopt,
                     int device = 0)
        : rate_(rate) {
        throw_on(comms_rfir_create(taps.data(), taps.size(), state ? state->data() : nullptr, state ? state->size() : 0, rate,
                                   device, &h_),
                 "RealFirDecimNode::new");
    }
    RealFirDecimNode(RealFirDecimNode&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), rate_(o.rate_) { o.h_ = nullptr; }
    ~RealFirDecimNode() { comms_rfir_destroy(h_); }
    Result<std::vector<float>> run(const std::vector<float>& in) {
        size_t m = 0;
        comms_rfir_out_len(in.size(), rate_, &m);
        std::vector<float> out(m);
        comms_status_t st = comms_rfir_run(h_, in.data(), in.size(), out.data());
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    std::string kernel(size_t n) const {  // "rfir_decim_kernel<..>", or "series: ..." (the four launches)
        char name[160] = {0};
        comms_rfir_get_kernel(h_, n, name, sizeof name);
        return name;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_rfir_t* h_ = nullptr;
    size_t rate_;
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
class ResampleNode : public DeriveNode<ResampleNode<T>> {
public:
    NodeReceiver<std::vector<T>> input;
    NodeSender<std::vector<T>> output;
    ResampleNode(const std::vector<float>& taps, size_t up, size_t down, int device = 0) : up_(up), down_(down) {
        throw_on(comms_resample_create(taps.data(), taps.size(), up, down, ResampleElem<T>::value, device, &h_), "ResampleNode::new");
    }
    ResampleNode(ResampleNode&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), up_(o.up_), down_(o.down_) { o.h_ = nullptr; }
    ~ResampleNode() { comms_resample_destroy(h_); }
    Result<std::vector<T>> run(const std::vector<T>& in) {
        size_t m = 0;
        if (comms_resample_out_len(in.size(), up_, down_, &m) != COMMS_OK) return NodeError::DataError;
        std::vector<T> out(m);
        comms_status_t st = comms_resample_run(h_, in.data(), in.size(), out.data());
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    std::string kernel(size_t n) const {  // "resample_kernel<..> ...", or "series: ..." (the launches)
        char name[200] = {0};
        comms_resample_get_kernel(h_, n, name, sizeof name);
        return name;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_resample_t* h_ = nullptr;
    size_t up_, down_;
};

// Polyphase channelizer as ONE node (comms_channelizer_*; an additional node): the results of M chains
// MixerNode(0, -2 pi k / M) -> BatchFirNode(Complex(taps, 0)) -> DecimateNode(down) over one Complex32 stream.  Any message
// length: ceil(n / down) frames.  One sender carries a message's frames x M outputs in the node's layout
// (COMMS_CHANNELIZER_CHANNEL_MAJOR: channel k is out[k frames .. (k + 1) frames)); connect it to as many receivers as there
// are consumers.
class ChannelizerNode : public DeriveNode<ChannelizerNode> {
public:
    NodeReceiver<std::vector<Complex32>> input;
    NodeSender<std::vector<Complex32>> output;
    ChannelizerNode(const std::vector<float>& taps, size_t channels, size_t down, int32_t layout = COMMS_CHANNELIZER_CHANNEL_MAJOR, int device = 0)
        : channels_(channels), down_(down) {
        throw_on(comms_channelizer_create(taps.data(), taps.size(), channels, down, layout, device, &h_), "ChannelizerNode::new");
    }
    ChannelizerNode(ChannelizerNode&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), channels_(o.channels_), down_(o.down_) {
        o.h_ = nullptr;
    }
    ~ChannelizerNode() { comms_channelizer_destroy(h_); }
    Result<std::vector<Complex32>> run(const std::vector<Complex32>& in) {
        size_t frames = 0;
        if (comms_channelizer_out_len(in.size(), down_, &frames) != COMMS_OK) return NodeError::DataError;
        std::vector<Complex32> out(frames * channels_);
        comms_status_t st = comms_channelizer_run(h_, reinterpret_cast<const comms_c32*>(in.data()), in.size(), reinterpret_cast<comms_c32*>(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    size_t channels() const { return channels_; }
    std::string kernel(size_t n) const {  // "channelizer_kernel<..> ...", or "series: ..." (the launches)
        char name[240] = {0};
        comms_channelizer_get_kernel(h_, n, name, sizeof name);
        return name;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_channelizer_t* h_ = nullptr;
    size_t channels_, down_;
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
namespace detail {
class SymbolSyncCore {
public:
    SymbolSyncCore(const std::vector<float>& taps, size_t phases, size_t sps, double dphase, int bits_per_sym, int device, const char* who)
        : sps_(sps < 1 ? 1 : sps), dphase_(dphase), bits_(bits_per_sym) {
        throw_on(comms_symsync_create(taps.data(), taps.size(), phases, sps, device, &h_), who);
        comms_status_t st = comms_symsync_set_rotation(h_, dphase, 0.0);
        if (st == COMMS_OK && bits_) st = comms_symsync_set_output_format(h_, COMMS_SYM_BITS, bits_, nullptr);
        if (st != COMMS_OK) {
            comms_symsync_destroy(h_);
            throw_on(st, who);
        }
    }
    SymbolSyncCore(SymbolSyncCore&& o) noexcept : h_(o.h_), sps_(o.sps_), dphase_(o.dphase_), bits_(o.bits_) { o.h_ = nullptr; }
    ~SymbolSyncCore() { comms_symsync_destroy(h_); }
    comms_status_t drain(NodeReceiver<SymbolSyncUpdate>& update) {
        while (update) {
            const std::optional<SymbolSyncUpdate> u = update->try_recv();
            if (!u) break;
            comms_status_t st = COMMS_OK;
            if (!std::isnan(u->tau)) st = comms_symsync_set_timing(h_, u->tau);
            if (st == COMMS_OK && !std::isnan(u->phase)) st = comms_symsync_set_rotation(h_, dphase_, u->phase);
            if (st != COMMS_OK) return st;
        }
        return COMMS_OK;
    }
    // elements of a message's output: symbols, or bytes of packed bits
    size_t out_len(size_t n) const {
        const size_t n_sym = n / sps_;
        return bits_ ? (n_sym * static_cast<size_t>(bits_) + 7) / 8 : n_sym;
    }
    comms_symsync_t* h() const { return h_; }

private:
    comms_symsync_t* h_ = nullptr;
    size_t sps_;
    double dphase_;
    int bits_;
};
}  // namespace detail

template <class Out = Complex32>
class SymbolSyncNode : public DeriveNode<SymbolSyncNode<Out>> {
    static_assert(std::is_same_v<Out, Complex32> || std::is_same_v<Out, uint8_t>, "symbols (Complex32) or packed bits (uint8_t)");

public:
    NodeReceiver<std::vector<Complex32>> input;
    NodeReceiver<SymbolSyncUpdate> update;  // optional; drained before each block
    NodeSender<std::vector<Out>> output;
    SymbolSyncNode(const std::vector<float>& taps, size_t phases, size_t sps, double dphase = 0.0, int bits_per_sym = 2, int device = 0)
        : core_(taps, phases, sps, dphase, std::is_same_v<Out, uint8_t> ? bits_per_sym : 0, device, "SymbolSyncNode::new") {}
    SymbolSyncNode(SymbolSyncNode&&) noexcept = default;
    Result<std::vector<Out>> run(const std::vector<Complex32>& in) {
        comms_status_t st = core_.drain(update);
        if (st != COMMS_OK) return to_node_error(st);
        std::vector<Out> out(core_.out_len(in.size()));
        st = comms_symsync_run(core_.h(), reinterpret_cast<const comms_c32*>(in.data()), in.size(), out.data());
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    std::string kernel(size_t n) const {  // "symsync_kernel<..> ..."
        char name[240] = {0};
        comms_symsync_get_kernel(core_.h(), n, name, sizeof name);
        return name;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    detail::SymbolSyncCore core_;
};

// ---------------------------------------------------------------- mixer
template <class D, class T>
class MixerNodeOf : public DeriveNode<D> {
public:
    NodeReceiver<T> input;
    NodeSender<T> output;

    // NB (dphase, phase): the node's order, not Mixer::new's (mixer.rs:128 vs :43)
    explicit MixerNodeOf(double dphase, std::optional<double> phase = std::nullopt, int device = 0) {
        throw_on(comms_mixer_create(dphase, phase.value_or(0.0), device, &h_), D::kNew);
    }
    MixerNodeOf(MixerNodeOf&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~MixerNodeOf() { comms_mixer_destroy(h_); }

    Result<T> run(const T& in) {
        T out;
        comms_status_t st = Sample<T>::mixer_run(h_, abi(&in), 1, abi(&out));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    Result<std::vector<T>> run_block(const std::vector<T>& ins) {  // see FirNodeOf::run_block
        std::vector<T> out(ins.size());
        comms_status_t st = Sample<T>::mixer_run(h_, abi(ins.data()), ins.size(), abi(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_mixer_t* h_ = nullptr;
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
class BatchMixerNode : public DeriveNode<BatchMixerNode> {
public:
    NodeReceiver<std::vector<Complex32>> input;
    NodeSender<std::vector<Complex32>> output;

    explicit BatchMixerNode(double dphase, std::optional<double> phase = std::nullopt, int device = 0) {
        throw_on(comms_mixer_create(dphase, phase.value_or(0.0), device, &h_), "BatchMixerNode::new");
    }
    BatchMixerNode(BatchMixerNode&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~BatchMixerNode() { comms_mixer_destroy(h_); }

    Result<std::vector<Complex32>> run(const std::vector<Complex32>& in) {
        std::vector<Complex32> out(in.size());
        comms_status_t st = comms_mixer_run(h_, c32(in.data()), in.size(), c32(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_mixer_t* h_ = nullptr;
};

// ---------------------------------------------------------------- decimate / upsample (T: Copy)
template <class T>
class DecimateNode : public DeriveNode<DecimateNode<T>> {
public:
    NodeReceiver<std::vector<T>> input;
    NodeSender<std::vector<T>> output;
    explicit DecimateNode(size_t dec_rate, int device = 0) : rate_(dec_rate), device_(device) {}

    Result<std::vector<T>> run(const std::vector<T>& signal) {
        std::vector<T> out;
        comms_status_t st = decimate(signal, out);
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    comms_status_t decimate(const std::vector<T>& data, std::vector<T>& out) const {
        size_t n_out = 0;
        comms_decimate_out_len(data.size(), rate_, &n_out);
        out.resize(n_out);
        return comms_decimate_run(data.data(), data.size(), sizeof(T), rate_, out.data(), nullptr, device_);
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    size_t rate_;
    int device_;
};

template <class T>
class UpsampleNode : public DeriveNode<UpsampleNode<T>> {
public:
    NodeReceiver<std::vector<T>> input;
    NodeSender<std::vector<T>> output;
    explicit UpsampleNode(size_t ups_rate, int device = 0) : rate_(ups_rate), device_(device) {}

    Result<std::vector<T>> run(const std::vector<T>& signal) {
        std::vector<T> out;
        comms_status_t st = upsample(signal, out);
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    comms_status_t upsample(const std::vector<T>& data, std::vector<T>& out) const {
        size_t n_out = 0;
        comms_status_t st = comms_upsample_out_len(data.size(), rate_, &n_out);
        if (st != COMMS_OK) return st;
        out.resize(n_out);
        return comms_upsample_run(data.data(), data.size(), sizeof(T), rate_, out.data(), nullptr, device_);
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    size_t rate_;
    int device_;
};

// ---------------------------------------------------------------- FM demod
template <class D, class T>
class FMDemodNodeOf : public DeriveNode<D> {
    using S = Sample<T>;

public:
    NodeReceiver<std::vector<T>> input;
    NodeSender<std::vector<typename S::Real>> output;

    explicit FMDemodNodeOf(int device = 0) { throw_on(S::fm_create(device, &h_), D::kNew); }
    FMDemodNodeOf(FMDemodNodeOf&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~FMDemodNodeOf() { S::fm_destroy(h_); }

    Result<std::vector<typename S::Real>> run(const std::vector<T>& samples) {
        std::vector<typename S::Real> out(samples.size());
        comms_status_t st = S::fm_run(h_, abi(samples.data()), samples.size(), out.data());
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    typename S::Fm* h_ = nullptr;
};

// ---------------------------------------------------------------- FFT
template <class D, class T>
class FFTBatchNodeOf : public DeriveNode<D> {
    using S = Sample<T>;

public:
    NodeReceiver<std::vector<T>> input;
    NodeSender<std::vector<T>> output;

    FFTBatchNodeOf(size_t fft_size, bool ifft, int device = 0) {
        throw_on(S::fft_create(fft_size, ifft ? 1 : 0, device, &h_), D::kNew);
    }
    FFTBatchNodeOf(FFTBatchNodeOf&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~FFTBatchNodeOf() { S::fft_destroy(h_); }

    Result<std::vector<T>> run(const std::vector<T>& data) {
        std::vector<T> out(data.size());
        // a wrong length panics inside rustfft in the reference; here it is DataError
        comms_status_t st = S::fft_run(h_, abi(data.data()), data.size(), abi(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    typename S::Fft* h_ = nullptr;
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

// #[aggregate]: run returns Some(vec) every fft_size pushes, None otherwise
class FFTSampleNode : public DeriveNode<FFTSampleNode> {
public:
    NodeReceiver<Complex32> input;
    NodeSender<std::vector<Complex32>> output;

    FFTSampleNode(size_t fft_size, bool ifft, int device = 0) : n_(fft_size) {
        throw_on(comms_fft_create(fft_size, ifft ? 1 : 0, device, &h_), "FFTSampleNode::new");
    }
    FFTSampleNode(FFTSampleNode&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), n_(o.n_), samples_(std::move(o.samples_)) {
        o.h_ = nullptr;
    }
    ~FFTSampleNode() { comms_fft_destroy(h_); }

    Result<std::optional<std::vector<Complex32>>> run(const Complex32& sample) {
        samples_.push_back(sample);
        if (samples_.size() != n_) return std::optional<std::vector<Complex32>>(std::nullopt);
        std::vector<Complex32> out(n_);
        comms_status_t st = comms_fft_run(h_, c32(samples_.data()), n_, c32(out.data()));
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
        comms_status_t st = comms_fft_run(h_, c32(samples_.data()), k * n_, c32(flat.data()));
        samples_.erase(samples_.begin(), samples_.begin() + k * n_);
        if (st != COMMS_OK) return to_node_error(st);
        outs.resize(k);
        for (size_t i = 0; i < k; ++i) outs[i].assign(flat.begin() + i * n_, flat.begin() + (i + 1) * n_);
        return outs;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_fft_t* h_ = nullptr;
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
using Complex64 = std::complex<double>;

// TimingEstimatorNode::new(n, d, alpha) -> Result<Self, MathError>; run(&[Complex<f64>]) -> f64
// (src/demodulation/timing_estimator.rs:116-136).  A bad alpha throws (the reference returns Err).
class TimingEstimatorNode : public DeriveNode<TimingEstimatorNode> {
public:
    NodeReceiver<std::vector<Complex64>> input;
    NodeSender<double> output;

    TimingEstimatorNode(uint32_t n, uint32_t d, double alpha, int device = 0) {
        throw_on(comms_timing_create(n, d, alpha, device, &h_), "TimingEstimatorNode::new");
    }
    TimingEstimatorNode(TimingEstimatorNode&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~TimingEstimatorNode() { comms_timing_destroy(h_); }

    Result<double> run(const std::vector<Complex64>& samples) {
        double est = 0.0;
        comms_status_t st = comms_timing_push(h_, reinterpret_cast<const double*>(samples.data()), samples.size(), &est);
        if (st != COMMS_OK) return to_node_error(st);
        return est;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_timing_t* h_ = nullptr;
};

// Timing and frequency estimates of a Complex<f32> block from one read of it (comms_syncest_*; an additional node):
// TimingEstimator::push at (n, d, alpha) and frequency_offset_estimate of the widened samples.  Two outputs per block:
// `output` carries the whole comms_sync_estimate_t, `update` the SymbolSyncUpdate{tau, NaN} that puts a SymbolSyncNode of
// (n_taps, phases) -- its sps = n -- on the symbol centres: tau = timing + (n_taps - 1) / (2 phases) (mod n); the NaN leaves
// the synchroniser's phase alone.  `update` plugs straight into SymbolSyncNode::update.
struct SyncEstimate {
    comms_sync_estimate_t estimate;
    SymbolSyncUpdate update;
    operator comms_sync_estimate_t() const { return estimate; }
    operator SymbolSyncUpdate() const { return update; }
};
namespace detail {
class SyncEstimatorCore {
public:
    SyncEstimatorCore(uint32_t n, uint32_t d, double alpha, size_t n_taps, size_t phases, int device, const char* who)
        : n_(n), delay_(n_taps ? static_cast<double>(n_taps - 1) / (2.0 * static_cast<double>(phases < 1 ? 1 : phases)) : 0.0) {
        throw_on(comms_syncest_create(n, d, alpha, device, &h_), who);
    }
    SyncEstimatorCore(SyncEstimatorCore&& o) noexcept : h_(o.h_), n_(o.n_), delay_(o.delay_) { o.h_ = nullptr; }
    ~SyncEstimatorCore() { comms_syncest_destroy(h_); }
    SyncEstimate message(const comms_sync_estimate_t& e) const {
        double tau = std::fmod(e.timing + delay_, static_cast<double>(n_));
        if (tau < 0) tau += static_cast<double>(n_);
        return SyncEstimate{e, SymbolSyncUpdate{tau, std::numeric_limits<double>::quiet_NaN()}};
    }
    comms_syncest_t* h() const { return h_; }

private:
    comms_syncest_t* h_ = nullptr;
    uint32_t n_;
    double delay_;
};
}  // namespace detail

class SyncEstimatorNode : public DeriveNode<SyncEstimatorNode> {
public:
    NodeReceiver<std::vector<Complex32>> input;
    NodeSender<comms_sync_estimate_t> output;
    NodeSender<SymbolSyncUpdate> update;
    SyncEstimatorNode(uint32_t n, uint32_t d, double alpha, size_t n_taps, size_t phases, int device = 0)
        : core_(n, d, alpha, n_taps, phases, device, "SyncEstimatorNode::new") {}
    SyncEstimatorNode(SyncEstimatorNode&&) noexcept = default;
    Result<SyncEstimate> run(const std::vector<Complex32>& samples) {
        comms_sync_estimate_t e{};
        comms_status_t st = comms_syncest_run(core_.h(), reinterpret_cast<const comms_c32*>(samples.data()), samples.size(), &e);
        if (st != COMMS_OK) return to_node_error(st);
        return core_.message(e);
    }
    std::string kernel(size_t n) const {  // "syncest_kernel ..."
        char name[240] = {0};
        comms_syncest_get_kernel(core_.h(), n, name, sizeof name);
        return name;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output, update); }

private:
    detail::SyncEstimatorCore core_;
};

// Frame synchroniser (comms_framesync_*; an additional node): takes SymbolSyncNode<Complex32>'s symbol output and sends, per
// block, the detections of a known word that the block decides -- possibly none -- as a vector ordered by stream index.
// index + word.size() is the first payload symbol, atan2(corr_im, corr_re) the rotation to take out.  A block of n symbols
// decides n positions, so a word is reported by the block that brings the last symbol of its guard window; flush() ends a
// stream.  The detections do not depend on how the stream is cut into blocks.
namespace detail {
class FrameSyncCore {
public:
    FrameSyncCore(const std::vector<Complex32>& word, double threshold, size_t guard, int device, const char* who)
        : n_word_(word.size()), guard_(guard) {
        throw_on(comms_framesync_create(reinterpret_cast<const comms_c32*>(word.data()), word.size(), threshold, guard, device, &h_), who);
    }
    FrameSyncCore(FrameSyncCore&& o) noexcept : h_(o.h_), n_word_(o.n_word_), guard_(o.guard_) { o.h_ = nullptr; }
    ~FrameSyncCore() { comms_framesync_destroy(h_); }
    // no call on n symbols has more detections: they are more than `guard` apart
    size_t bound(size_t n) const { return (n + guard_) / (guard_ + 1); }
    Result<std::vector<comms_frame_detection_t>> flush() {
        size_t found = 0;
        std::vector<comms_frame_detection_t> out(bound(n_word_ + guard_));  // a flush decides word + guard positions
        comms_status_t st = comms_framesync_flush(h_, out.data(), out.size(), &found);
        if (st != COMMS_OK) return to_node_error(st);
        out.resize(found);
        return out;
    }
    comms_framesync_t* h() const { return h_; }

private:
    comms_framesync_t* h_ = nullptr;
    size_t n_word_, guard_;
};
}  // namespace detail

class FrameSyncNode : public DeriveNode<FrameSyncNode> {
public:
    NodeReceiver<std::vector<Complex32>> input;
    NodeSender<std::vector<comms_frame_detection_t>> output;
    FrameSyncNode(const std::vector<Complex32>& word, double threshold, size_t guard, int device = 0)
        : core_(word, threshold, guard, device, "FrameSyncNode::new") {}
    FrameSyncNode(FrameSyncNode&&) noexcept = default;
    Result<std::vector<comms_frame_detection_t>> run(const std::vector<Complex32>& symbols) {
        std::vector<comms_frame_detection_t> out(core_.bound(symbols.size()));
        size_t found = 0;
        comms_status_t st = comms_framesync_run(core_.h(), reinterpret_cast<const comms_c32*>(symbols.data()), symbols.size(), out.data(),
                                                out.size(), &found);
        if (st != COMMS_OK) return to_node_error(st);
        out.resize(found);
        return out;
    }
    Result<std::vector<comms_frame_detection_t>> flush() { return core_.flush(); }
    std::string kernel(size_t n) const {  // "framesync_kernel ..."
        char name[240] = {0};
        comms_framesync_get_kernel(core_.h(), n, name, sizeof name);
        return name;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    detail::FrameSyncCore core_;
};

// NcoNode::new(dphase, Option<phase>) (src/demodulation/nco.rs:118-133) in block form: one
// message is a vector of phase errors, the output is exp(i*phase) per sample.  (The reference
// node is per sample, f64 -> Complex<f64>; a closed loop runs it at block rate here.)
class BatchNcoNode : public DeriveNode<BatchNcoNode> {
public:
    NodeReceiver<std::vector<double>> input;
    NodeSender<std::vector<Complex64>> output;

    explicit BatchNcoNode(double dphase, double phase = 0.0, int device = 0) {
        throw_on(comms_nco_create(dphase, phase, device, &h_), "NcoNode::new");
    }
    BatchNcoNode(BatchNcoNode&& o) noexcept : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_) { o.h_ = nullptr; }
    ~BatchNcoNode() { comms_nco_destroy(h_); }

    Result<std::vector<Complex64>> run(const std::vector<double>& perr) {
        std::vector<Complex64> out(perr.size());
        comms_status_t st = comms_nco_run(h_, perr.data(), perr.size(), reinterpret_cast<double*>(out.data()));
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_nco_t* h_ = nullptr;
};

inline std::vector<double> qfilt_taps(uint32_t n_taps, double alpha, uint32_t sam_per_sym) {
    std::vector<double> t(comms_qfilt_len(n_taps));
    throw_on(comms_qfilt_taps(n_taps, alpha, sam_per_sym, t.data()), "qfilt_taps");
    return t;
}

// ---------------------------------------------------------------- device-resident nodes
// Messages are DeviceBuf<T>: nothing crosses PCIe between nodes and nothing ever synchronises
// the device.  Every node owns a stream (DevStream); run() is
//     wait_ready(in)  ->  one asynchronous launch on the node's stream  ->  record_use(in),
//     record_ready(out)  ->  send(out)
// so the consumer's stream starts its own launch only after the producer's has finished, while the
// node threads themselves run ahead of the device.  An edge stays on ONE GPU: the buffer's events
// belong to its device and the kernels read it directly, so a message whose device is not the node's is a
// DataError (COMMS_ERR_ARG) -- between GPUs the host copies or sends the samples itself (sharding, above).  Output
// buffers come from the library's cache (no hipMalloc / hipFree in steady state); a buffer's
// memory is recycled only after the launches that read it.  to_host() waits for the producer.
class DevStream {
public:
    explicit DevStream(int device) : device_(device) { throw_on(comms_stream_create(device, &s_), "comms_stream_create"); }
    DevStream(DevStream&& o) noexcept : s_(o.s_), device_(o.device_) { o.s_ = nullptr; }
    DevStream(const DevStream&) = delete;
    ~DevStream() {
        if (!s_) return;
        comms_stream_synchronize(device_, s_);
        comms_stream_destroy(device_, s_);
    }
    // `launch(stream)` is the node's *_run_dev call
    template <class TI, class TO, class F>
    comms_status_t run(const DeviceBuf<TI>& in, DeviceBuf<TO>& out, F&& launch) {
        if (in.device() != device_ || out.device() != device_) return COMMS_ERR_ARG;  // no cross-device edges (see above)
        comms_status_t st = comms_buf_wait_ready(in.raw(), s_);
        if (st == COMMS_OK) st = launch(s_);
        if (st == COMMS_OK) st = comms_buf_record_use(in.raw(), s_);
        if (st == COMMS_OK) st = comms_buf_record_ready(out.raw(), s_);
        return st;
    }
    int device() const { return device_; }

private:
    void* s_ = nullptr;
    int device_;
};

class BatchFirNodeDev : public DeriveNode<BatchFirNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    BatchFirNodeDev(const std::vector<Complex32>& taps, const std::optional<std::vector<Complex32>>& state = std::nullopt,
                    int device = 0)
        : device_(device), st_(device) {
        throw_on(comms_fir_create(c32(taps.data()), taps.size(), state ? c32(state->data()) : nullptr,
                                  state ? state->size() : 0, device, &h_),
                 "BatchFirNodeDev::new");
    }
    BatchFirNodeDev(BatchFirNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~BatchFirNodeDev() { comms_fir_destroy(h_); }
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& in) {
        DeviceBuf<Complex32> out(in.size(), device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_fir_run_dev(h_, c32(in.ptr()), in.size(), c32(out.ptr()), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_fir_t* h_ = nullptr;
    int device_;
    DevStream st_;
};

class BatchMixerNodeDev : public DeriveNode<BatchMixerNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    explicit BatchMixerNodeDev(double dphase, std::optional<double> phase = std::nullopt, int device = 0) : device_(device), st_(device) {
        throw_on(comms_mixer_create(dphase, phase.value_or(0.0), device, &h_), "BatchMixerNodeDev::new");
    }
    BatchMixerNodeDev(BatchMixerNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~BatchMixerNodeDev() { comms_mixer_destroy(h_); }
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& in) {
        DeviceBuf<Complex32> out(in.size(), device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_mixer_run_dev(h_, c32(in.ptr()), in.size(), c32(out.ptr()), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_mixer_t* h_ = nullptr;
    int device_;
    DevStream st_;
};

class DecimateNodeDev : public DeriveNode<DecimateNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    explicit DecimateNodeDev(size_t dec_rate, int device = 0) : rate_(dec_rate), device_(device), st_(device) {}
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& in) {
        size_t n_out = 0;
        comms_decimate_out_len(in.size(), rate_, &n_out);
        DeviceBuf<Complex32> out(n_out, device_);
        comms_status_t st = st_.run(in, out, [&](void* s) {
            return comms_decimate_run_dev(in.ptr(), in.size(), sizeof(Complex32), rate_, out.ptr(), nullptr, device_, s);
        });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    size_t rate_;
    int device_;
    DevStream st_;
};

// One macro-free pattern for the remaining device-resident nodes: own the C handle, move-only,
// run() takes the output DeviceBuf from the cache and launches on the node's stream.
class FFTBatchNodeDev : public DeriveNode<FFTBatchNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    FFTBatchNodeDev(size_t fft_size, bool ifft, int device = 0) : device_(device), st_(device) {
        throw_on(comms_fft_create(fft_size, ifft ? 1 : 0, device, &h_), "FFTBatchNodeDev::new");
    }
    FFTBatchNodeDev(FFTBatchNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~FFTBatchNodeDev() { comms_fft_destroy(h_); }
    // the message may hold any whole number of transforms (the reference: exactly one)
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& in) {
        DeviceBuf<Complex32> out(in.size(), device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_fft_run_dev(h_, c32(in.ptr()), in.size(), c32(out.ptr()), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_fft_t* h_ = nullptr;
    int device_;
    DevStream st_;
};

class FMDemodNodeDev : public DeriveNode<FMDemodNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<float>> output;
    explicit FMDemodNodeDev(int device = 0) : device_(device), st_(device) {
        throw_on(comms_fmdemod_create(device, &h_), "FMDemodNodeDev::new");
    }
    FMDemodNodeDev(FMDemodNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~FMDemodNodeDev() { comms_fmdemod_destroy(h_); }
    Result<DeviceBuf<float>> run(const DeviceBuf<Complex32>& in) {
        DeviceBuf<float> out(in.size(), device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_fmdemod_run_dev(h_, c32(in.ptr()), in.size(), out.ptr(), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_fmdemod_t* h_ = nullptr;
    int device_;
    DevStream st_;
};

// PulseNode over whole symbol blocks: n symbols in, n * sam_per_sym samples out
class BatchPulseNodeDev : public DeriveNode<BatchPulseNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    BatchPulseNodeDev(const std::vector<Complex32>& taps, size_t sam_per_sym, int device = 0)
        : sps_(sam_per_sym), device_(device), st_(device) {
        throw_on(comms_pulse_create(c32(taps.data()), taps.size(), sam_per_sym, device, &h_), "BatchPulseNodeDev::new");
    }
    BatchPulseNodeDev(BatchPulseNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), sps_(o.sps_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~BatchPulseNodeDev() { comms_pulse_destroy(h_); }
    BatchPulseNodeDev& with_mixer(double dphase, std::optional<double> phase = std::nullopt) {
        throw_on(comms_pulse_set_mixer(h_, dphase, phase.value_or(0.0)), "BatchPulseNodeDev::with_mixer");
        return *this;
    }
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& sym) {
        DeviceBuf<Complex32> out(sym.size() * sps_, device_);
        comms_status_t st = st_.run(sym, out, [&](void* s) { return comms_pulse_run_dev(h_, c32(sym.ptr()), sym.size(), c32(out.ptr()), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_pulse_t* h_ = nullptr;
    size_t sps_;
    int device_;
    DevStream st_;
};

class UpsampleNodeDev : public DeriveNode<UpsampleNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    explicit UpsampleNodeDev(size_t ups_rate, int device = 0) : rate_(ups_rate), device_(device), st_(device) {}
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& in) {
        size_t n_out = 0;
        comms_upsample_out_len(in.size(), rate_, &n_out);
        DeviceBuf<Complex32> out(n_out, device_);
        comms_status_t st = st_.run(in, out, [&](void* s) {
            return comms_upsample_run_dev(in.ptr(), in.size(), sizeof(Complex32), rate_, out.ptr(), nullptr, device_, s);
        });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    size_t rate_;
    int device_;
    DevStream st_;
};

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

// mixer / FIR / decimate [/ FM demod] as ONE node (comms_chain_*; an additional node, the results of
// the reference nodes in series).  Out = Complex32 without FM demod, float with it.
template <class Out>
class ChainNodeDev : public DeriveNode<ChainNodeDev<Out>> {
public:
    static constexpr bool kFm = std::is_same<Out, float>::value;
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Out>> output;
    ChainNodeDev(double dphase, double phase, const std::vector<Complex32>& taps, size_t rate, bool mixer_after_fir = false,
                 int device = 0)
        : rate_(rate), device_(device), st_(device) {
        const int32_t flags = (kFm ? COMMS_CHAIN_FM_DEMOD : 0) | (mixer_after_fir ? COMMS_CHAIN_MIXER_AFTER_FIR : 0);
        throw_on(comms_chain_create_ex(dphase, phase, c32(taps.data()), taps.size(), rate, flags, device, &h_),
                 "ChainNodeDev::new");
    }
    ChainNodeDev(ChainNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), rate_(o.rate_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~ChainNodeDev() { comms_chain_destroy(h_); }
    Result<DeviceBuf<Out>> run(const DeviceBuf<Complex32>& in) {
        if (rate_ == 0 || in.size() % rate_) return NodeError::DataError;
        DeviceBuf<Out> out(in.size() / rate_, device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_chain_run_dev(h_, c32(in.ptr()), in.size(), out.ptr(), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    int fused_kind() const {  // 0 four kernels, 1 overlap-save fusion, 2 time-domain decimating kernel, 3 its any-rate form, 4 the polyphase
                              // frequency-domain kernel (what the last call ran on: rates 4, 8, 12 ... 64)
        int32_t f = 0;
        comms_chain_is_fused(h_, &f);
        return f;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_chain_t* h_ = nullptr;
    size_t rate_;
    int device_;
    DevStream st_;
};

// The real FIR + decimator on device-resident messages (the angles a ChainNodeDev<float> sends never leave the device)
class RealFirDecimNodeDev : public DeriveNode<RealFirDecimNodeDev> {
public:
    NodeReceiver<DeviceBuf<float>> input;
    NodeSender<DeviceBuf<float>> output;
    RealFirDecimNodeDev(const std::vector<float>& taps, size_t rate, const std::optional<std::vector<float>>& state = std::nullopt,
                        int device = 0)
        : rate_(rate), device_(device), st_(device) {
        throw_on(comms_rfir_create(taps.data(), taps.size(), state ? state->data() : nullptr, state ? state->size() : 0, rate,
                                   device, &h_),
                 "RealFirDecimNodeDev::new");
    }
    RealFirDecimNodeDev(RealFirDecimNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), rate_(o.rate_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~RealFirDecimNodeDev() { comms_rfir_destroy(h_); }
    Result<DeviceBuf<float>> run(const DeviceBuf<float>& in) {
        size_t m = 0;
        comms_rfir_out_len(in.size(), rate_, &m);
        DeviceBuf<float> out(m, device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_rfir_run_dev(h_, in.ptr(), in.size(), out.ptr(), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_rfir_t* h_ = nullptr;
    size_t rate_;
    int device_;
    DevStream st_;
};

// The rational resampler on device-resident messages
template <class T>
class ResampleNodeDev : public DeriveNode<ResampleNodeDev<T>> {
public:
    NodeReceiver<DeviceBuf<T>> input;
    NodeSender<DeviceBuf<T>> output;
    ResampleNodeDev(const std::vector<float>& taps, size_t up, size_t down, int device = 0)
        : up_(up), down_(down), device_(device), st_(device) {
        throw_on(comms_resample_create(taps.data(), taps.size(), up, down, ResampleElem<T>::value, device, &h_), "ResampleNodeDev::new");
    }
    ResampleNodeDev(ResampleNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), up_(o.up_), down_(o.down_), device_(o.device_), st_(std::move(o.st_)) {
        o.h_ = nullptr;
    }
    ~ResampleNodeDev() { comms_resample_destroy(h_); }
    Result<DeviceBuf<T>> run(const DeviceBuf<T>& in) {
        size_t m = 0;
        if (comms_resample_out_len(in.size(), up_, down_, &m) != COMMS_OK) return NodeError::DataError;
        DeviceBuf<T> out(m, device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_resample_run_dev(h_, in.ptr(), in.size(), out.ptr(), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_resample_t* h_ = nullptr;
    size_t up_, down_;
    int device_;
    DevStream st_;
};

// The channelizer on device-resident messages: channel k of a channel-major message is a contiguous device stream
class ChannelizerNodeDev : public DeriveNode<ChannelizerNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    ChannelizerNodeDev(const std::vector<float>& taps, size_t channels, size_t down, int32_t layout = COMMS_CHANNELIZER_CHANNEL_MAJOR, int device = 0)
        : channels_(channels), down_(down), device_(device), st_(device) {
        throw_on(comms_channelizer_create(taps.data(), taps.size(), channels, down, layout, device, &h_), "ChannelizerNodeDev::new");
    }
    ChannelizerNodeDev(ChannelizerNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), channels_(o.channels_), down_(o.down_), device_(o.device_),
          st_(std::move(o.st_)) {
        o.h_ = nullptr;
    }
    ~ChannelizerNodeDev() { comms_channelizer_destroy(h_); }
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& in) {
        size_t frames = 0;
        if (comms_channelizer_out_len(in.size(), down_, &frames) != COMMS_OK) return NodeError::DataError;
        DeviceBuf<Complex32> out(frames * channels_, device_);
        comms_status_t st = st_.run(in, out, [&](void* s) {
            return comms_channelizer_run_dev(h_, reinterpret_cast<const comms_c32*>(in.ptr()), in.size(), reinterpret_cast<comms_c32*>(out.ptr()), s);
        });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_channelizer_t* h_ = nullptr;
    size_t channels_, down_;
    int device_;
    DevStream st_;
};

// The symbol synchroniser on device-resident messages (`update` as SymbolSyncNode's: host values, drained before each block)
template <class Out = Complex32>
class SymbolSyncNodeDev : public DeriveNode<SymbolSyncNodeDev<Out>> {
    static_assert(std::is_same_v<Out, Complex32> || std::is_same_v<Out, uint8_t>, "symbols (Complex32) or packed bits (uint8_t)");

public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeReceiver<SymbolSyncUpdate> update;
    NodeSender<DeviceBuf<Out>> output;
    SymbolSyncNodeDev(const std::vector<float>& taps, size_t phases, size_t sps, double dphase = 0.0, int bits_per_sym = 2, int device = 0)
        : core_(taps, phases, sps, dphase, std::is_same_v<Out, uint8_t> ? bits_per_sym : 0, device, "SymbolSyncNodeDev::new"),
          device_(device), st_(device) {}
    SymbolSyncNodeDev(SymbolSyncNodeDev&&) noexcept = default;
    Result<DeviceBuf<Out>> run(const DeviceBuf<Complex32>& in) {
        comms_status_t st = core_.drain(update);
        if (st != COMMS_OK) return to_node_error(st);
        DeviceBuf<Out> out(core_.out_len(in.size()), device_);
        st = st_.run(in, out, [&](void* s) {
            return comms_symsync_run_dev(core_.h(), reinterpret_cast<const comms_c32*>(in.ptr()), in.size(), out.ptr(), s);
        });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    detail::SymbolSyncCore core_;
    int device_;
    DevStream st_;
};

// The synchronisation estimator on device-resident messages: the estimates themselves are host values (the call
// synchronises its stream), so the outputs are SyncEstimatorNode's
class SyncEstimatorNodeDev : public DeriveNode<SyncEstimatorNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<comms_sync_estimate_t> output;
    NodeSender<SymbolSyncUpdate> update;
    SyncEstimatorNodeDev(uint32_t n, uint32_t d, double alpha, size_t n_taps, size_t phases, int device = 0)
        : core_(n, d, alpha, n_taps, phases, device, "SyncEstimatorNodeDev::new"), device_(device) {
        throw_on(comms_stream_create(device, &s_), "comms_stream_create");
    }
    SyncEstimatorNodeDev(SyncEstimatorNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), update(std::move(o.update)), core_(std::move(o.core_)),
          device_(o.device_), s_(o.s_) { o.s_ = nullptr; }
    ~SyncEstimatorNodeDev() {
        if (s_) comms_stream_destroy(device_, s_);   // every run ends synchronised
    }
    Result<SyncEstimate> run(const DeviceBuf<Complex32>& in) {
        if (in.device() != device_) return to_node_error(COMMS_ERR_ARG);
        comms_sync_estimate_t e{};
        comms_status_t st = comms_buf_wait_ready(in.raw(), s_);
        if (st == COMMS_OK) st = comms_syncest_run_dev(core_.h(), reinterpret_cast<const comms_c32*>(in.ptr()), in.size(), &e, s_);
        if (st != COMMS_OK) return to_node_error(st);
        return core_.message(e);
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output, update); }

private:
    detail::SyncEstimatorCore core_;
    int device_;
    void* s_ = nullptr;
};

// The frame synchroniser on device-resident messages (SymbolSyncNodeDev<Complex32>'s output): the detections are host
// values (the call synchronises its stream), so the output is FrameSyncNode's
class FrameSyncNodeDev : public DeriveNode<FrameSyncNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<std::vector<comms_frame_detection_t>> output;
    FrameSyncNodeDev(const std::vector<Complex32>& word, double threshold, size_t guard, int device = 0)
        : core_(word, threshold, guard, device, "FrameSyncNodeDev::new"), device_(device) {
        throw_on(comms_stream_create(device, &s_), "comms_stream_create");
    }
    FrameSyncNodeDev(FrameSyncNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), core_(std::move(o.core_)), device_(o.device_), s_(o.s_) { o.s_ = nullptr; }
    ~FrameSyncNodeDev() {
        if (s_) comms_stream_destroy(device_, s_);   // every run ends synchronised
    }
    Result<std::vector<comms_frame_detection_t>> run(const DeviceBuf<Complex32>& in) {
        if (in.device() != device_) return to_node_error(COMMS_ERR_ARG);
        std::vector<comms_frame_detection_t> out(core_.bound(in.size()));
        size_t found = 0;
        comms_status_t st = comms_buf_wait_ready(in.raw(), s_);
        if (st == COMMS_OK)
            st = comms_framesync_run_dev(core_.h(), reinterpret_cast<const comms_c32*>(in.ptr()), in.size(), out.data(), out.size(), &found, s_);
        if (st != COMMS_OK) return to_node_error(st);
        out.resize(found);
        return out;
    }
    Result<std::vector<comms_frame_detection_t>> flush() { return core_.flush(); }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    detail::FrameSyncCore core_;
    int device_;
    void* s_ = nullptr;
};

// AWGN channel on device-resident messages: wait_ready(in) -> comms_awgn_run_dev on the node's stream -> record_use(in),
// record_ready(out) -> send(out), the ordering of every *Dev node
class AwgnNodeDev : public DeriveNode<AwgnNodeDev> {
public:
    NodeReceiver<DeviceBuf<Complex32>> input;
    NodeSender<DeviceBuf<Complex32>> output;
    AwgnNodeDev(float sigma, std::optional<uint64_t> seed = std::nullopt, uint64_t stream = 0, int device = 0)
        : sigma_(sigma), device_(device), st_(device) {
        throw_on(comms_noise_create(seed ? *seed : entropy_seed(), stream, device, &h_), "AwgnNodeDev::new");
    }
    AwgnNodeDev(AwgnNodeDev&& o) noexcept
        : input(std::move(o.input)), output(std::move(o.output)), h_(o.h_), sigma_(o.sigma_), device_(o.device_), st_(std::move(o.st_)) { o.h_ = nullptr; }
    ~AwgnNodeDev() { comms_noise_destroy(h_); }
    Result<DeviceBuf<Complex32>> run(const DeviceBuf<Complex32>& in) {
        DeviceBuf<Complex32> out(in.size(), device_);
        comms_status_t st = st_.run(in, out, [&](void* s) { return comms_awgn_run_dev(h_, in.ptr(), in.size(), sigma_, c32(out.ptr()), s); });
        if (st != COMMS_OK) return to_node_error(st);
        return out;
    }
    auto receivers() { return std::tie(input); }
    auto senders() { return std::tie(output); }

private:
    comms_noise_t* h_ = nullptr;
    float sigma_;
    int device_;
    DevStream st_;
};

}  // namespace comms
