// common.hpp -- shared plumbing of libcomms_hip.so (gfx950 only; no CPU fallback).
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/comms_hip.h"
#include "history_order.hpp"

// fused-chain stage bits shared by fir.hip and chain.hip (internal)
#define COMMS_CHAIN_PRE 1  /* mixer before the FIR */
#define COMMS_CHAIN_POST 2 /* mixer after the FIR */
#define COMMS_CHAIN_DEC 4
#define COMMS_CHAIN_FM 8
#ifdef COMMS_DIAG  // the diagnostic build lets scripts/trace_fir.py, stamp_fir.py reach these
#define COMMS_INTERNAL
#else
#define COMMS_INTERNAL __attribute__((visibility("hidden")))
#endif
extern "C" COMMS_INTERNAL int32_t comms_fir_os4096_decim_supported(const comms_fir_t* h, uint32_t rate);
extern "C" COMMS_INTERNAL int32_t comms_fir_os16k_decim_supported(const comms_fir_t* h, uint32_t rate);
extern "C" COMMS_INTERNAL comms_status_t comms_fir_run_os16k_decim_dev(comms_fir_t* h, const comms_c32* d_in, size_t n, void* d_out, uint64_t turns0,
                                                                      uint64_t frac, uint32_t rate, void* stream);
extern "C" COMMS_INTERNAL comms_status_t comms_fir_run_os4096_decim_dev(comms_fir_t* h, const void* d_in, size_t n, void* d_out, uint64_t turns0,
                                                                       uint64_t frac, uint32_t rate, void* stream);
extern "C" COMMS_INTERNAL comms_status_t comms_fir_run_fused_dev(comms_fir_t* h, const comms_c32* d_in, size_t n, void* d_out,
                                                  int32_t mode, uint64_t turns0, uint64_t frac, uint32_t rate,
                                                  const void* fm_prev, void* fm_prev_new, void* stream);

// the same chain on the time-domain decimating kernel (fir_decim.hip), where it applies
extern "C" COMMS_INTERNAL comms_status_t comms_mixer_run_decim_dev(comms_mixer_t* h, const comms_c32* d_in, size_t n, size_t rate,
                                                                 comms_c32* d_out, void* stream);
extern "C" COMMS_INTERNAL int32_t comms_fir_decim_supported(const comms_fir_t* h, uint32_t rate);
extern "C" COMMS_INTERNAL int32_t comms_fir_decim_supported_for(const comms_fir_t* h, uint32_t rate, int32_t fm_demod, int32_t can_fuse);
extern "C" COMMS_INTERNAL comms_status_t comms_fir_run_decim_dev(comms_fir_t* h, const void* d_in, size_t n, void* d_out,
                                                  int32_t mode, uint64_t turns0, uint64_t frac, uint32_t rate,
                                                  const void* fm_prev, void* fm_prev_new, void* stream);
// ... the same with hard-decision bits out of its store stage (comms_chain_set_output_format; no FM demod): ceil(n/rate * k / 8)
// bytes at d_out (4-byte aligned).  A call the wave-private form takes (it has no decision stage) writes its Complex<f32>
// outputs to c32_scratch (n/rate of them) and the decision pass follows, so that the bits are always those of the c32 form.
extern "C" COMMS_INTERNAL comms_status_t comms_fir_run_decim_bits_dev(comms_fir_t* h, const void* d_in, size_t n, void* d_out,
                                                  int32_t mode, uint64_t turns0, uint64_t frac, uint32_t rate,
                                                  const void* sym_table, void* c32_scratch, void* stream);

// ... and on the any-rate time-domain kernel (fir_decim_any.hip): mixer behind the FIR only
extern "C" COMMS_INTERNAL int32_t comms_fir_decim_any_supported(const comms_fir_t* h, uint32_t rate);
extern "C" COMMS_INTERNAL comms_status_t comms_fir_run_decim_any_dev(comms_fir_t* h, const void* d_in, size_t n, void* d_out,
                                                  int32_t mode, uint64_t turns0, uint64_t frac, uint32_t rate,
                                                  const void* fm_prev, void* fm_prev_new, void* stream);

// ... and, at rate 8, as eight polyphase branches in the frequency domain (fir_poly8.hip): long filters on long batches
extern "C" COMMS_INTERNAL int32_t comms_fir_poly8_supported(const comms_fir_t* h, uint32_t rate, int32_t mode, size_t n);
extern "C" COMMS_INTERNAL comms_status_t comms_fir_run_poly8_dev(comms_fir_t* h, const void* d_in, size_t n, void* d_out,
                                                  int32_t mode, uint64_t turns0, uint64_t frac, uint32_t rate,
                                                  const void* fm_prev, void* fm_prev_new, void* stream);

namespace comms {

// ---- tuning knobs ------------------------------------------------------------
// Kernel selectors and sweep parameters (COMMS_OS1024_*, COMMS_DECIM_*, COMMS_FFT_*, ...) exist in the DIAGNOSTIC build
// only (`make diag`, -DCOMMS_DIAG: scripts/ load it through scripts/with_lib.py), where they are read once from the
// environment.  In the product build every knob is its default at compile time: no getenv on any launch path, nothing
// in the environment changes which kernel runs or what it computes.  (The two documented runtime limits,
// COMMS_ZERO_COPY_BYTES and COMMS_BUF_POOL_MB in runtime.hip, are resources, not kernel selectors.)
#ifdef COMMS_DIAG
inline int diag_knob(const char* name, int dflt) {
    const char* v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
#else
constexpr int diag_knob(const char*, int dflt) { return dflt; }
#endif

// ---- thread-local last error -------------------------------------------------
inline char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
inline comms_status_t fail(comms_status_t code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define COMMS_HIP_TRY(expr)                                                              \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess)                                                            \
            return ::comms::fail(COMMS_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr,       \
                                 hipGetErrorString(_e), __FILE__, __LINE__);             \
    } while (0)

#define COMMS_TRY(expr)                       \
    do {                                      \
        comms_status_t _s = (expr);           \
        if (_s != COMMS_OK) return _s;        \
    } while (0)

#define COMMS_ARG(cond, ...)                                             \
    do {                                                                 \
        if (!(cond)) return ::comms::fail(COMMS_ERR_ARG, __VA_ARGS__);   \
    } while (0)

// Every entry point runs on the handle's device: the current device is
// thread-local in HIP and a node is created on one thread and run on another
// (src/node/mod.rs:279-281 in the reference).
comms_status_t use_device(int32_t device);

// Kernel launch check (launch-time errors only; execution stays async).
inline comms_status_t launch_ok(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(COMMS_ERR_DEVICE, "launch of %s failed: %s", what, hipGetErrorString(e));
    return COMMS_OK;
}

// The event pair of a timed launch (Handle::take_events): both events or neither.
struct EventPair {
    hipEvent_t start = nullptr, stop = nullptr;
};

// Dynamic LDS that `Kernel` may ask for, per device, in bytes: what launch_kernel has set
// hipFuncAttributeMaxDynamicSharedMemorySize to there (0: never set).  The attribute applies to the current device only,
// and a process may drive several GPUs through the C ABI.
template <auto Kernel>
struct LdsGranted {
    static inline std::atomic<unsigned> bytes[64] = {};
    static inline std::mutex grow;  // held while the limit is raised, never by a launch that fits
};

// The one way to launch a kernel: LDS opt-in, launch, check.
//   launch_kernel<fir_decim_kernel<R, REAL, PRE, A>>("fir_decim_kernel", grid, block, lds, s, h->take_events(), args);
// 1. A launch that asks for more dynamic LDS than the kernel has been granted on the current device raises the limit to
//    what it asks for and remembers that; a failed hipFuncSetAttribute is not remembered.  Every other launch pays one
//    hipGetDevice and one atomic load (nothing without dynamic LDS).  Node threads of one process reach the same kernel
//    concurrently, hence the atomics; the limit is raised under the kernel's mutex, so that of two threads that first ask
//    for different sizes the smaller one cannot be the last to set the attribute.
// 2. With an event pair the launch is hipExtLaunchKernelGGL's: the pair takes the kernel's own begin / end timestamps (no
//    dispatch gap), which is what rocprofv3 reports as its duration.  Without one it is a plain launch.
// 3. launch_ok under `name`.
// The arguments reach the launch expression by reference: no copy of a large argument block (PulseArgs, DecimArgs) is made
// in front of the runtime's own.
template <auto Kernel, class... Args>
comms_status_t launch_kernel(const char* name, dim3 grid, dim3 block, size_t lds, hipStream_t s, EventPair ev, const Args&... args) {
    if (lds) {
        using G = LdsGranted<Kernel>;
        int dev = 0;
        COMMS_HIP_TRY(hipGetDevice(&dev));
        COMMS_ARG(dev >= 0 && dev < 64, "device index out of range");
        if (lds > G::bytes[dev].load(std::memory_order_acquire)) {
            std::lock_guard<std::mutex> lk(G::grow);
            if (lds > G::bytes[dev].load(std::memory_order_relaxed)) {
                COMMS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                  static_cast<int>(lds)));
                G::bytes[dev].store(static_cast<unsigned>(lds), std::memory_order_release);
            }
        }
    }
    if (ev.start)
        hipExtLaunchKernelGGL(Kernel, grid, block, static_cast<uint32_t>(lds), s, ev.start, ev.stop, 0u, args...);
    else
        Kernel<<<grid, block, lds, s>>>(args...);
    return launch_ok(name);
}

// ---- owners of device and pinned memory -----------------------------------------------------------------------------
// Every allocation of a handle is a member of one of these types (Scratch, Pinned, DevBuf, History): freed by its
// destructor, never copied.  They are the only places of the library (runtime.hip's pools aside) that free memory.

// Grow-only device scratch used by the host-pointer (`*_run`) entry points.
struct Scratch {
    void* p = nullptr;
    size_t cap = 0;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { release(); }
    comms_status_t reserve(size_t bytes) {
        if (bytes <= cap) return COMMS_OK;
        if (p) {
            COMMS_HIP_TRY(hipFree(p));
            p = nullptr;
            cap = 0;
        }
        size_t want = bytes + bytes / 4 + 256;
        COMMS_HIP_TRY(hipMalloc(&p, want));
        cap = want;
        return COMMS_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// Host-mapped pinned staging for SHORT host-pointer calls: the kernel reads its input from, and
// writes its output to, pinned host memory directly, which replaces two DMA submissions by two
// small CPU copies (mixer: 32 -> 18 us per call at 64 samples, 44 -> 31 us at 16384; measured
// crossover with the DMA route between 512 KiB and 2 MiB per direction).
struct Pinned {
    void* h = nullptr;  // host address
    void* d = nullptr;  // the same memory as the device sees it
    size_t cap = 0;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { release(); }
    comms_status_t reserve(size_t bytes) {
        if (bytes <= cap) return COMMS_OK;
        release();
        const size_t want = bytes < 65536 ? 65536 : bytes;
        // coherent (fine-grained) on purpose, not by the HIP_HOST_COHERENT default: the GPU must not keep lines of a
        // staging buffer in its L2 from one call to the next, the CPU rewrites the buffer between them
        COMMS_HIP_TRY(hipHostMalloc(&h, want, hipHostMallocMapped | hipHostMallocCoherent));
        hipError_t e = hipHostGetDevicePointer(&d, h, 0);
        if (e != hipSuccess) {
            (void)hipHostFree(h);
            h = d = nullptr;
            return fail(COMMS_ERR_DEVICE, "hipHostGetDevicePointer failed: %s", hipGetErrorString(e));
        }
        cap = want;
        return COMMS_OK;
    }
    void release() {
        if (h) (void)hipHostFree(h);
        h = d = nullptr;
        cap = 0;
    }
};
// Create-time zeroing of device state (FIR history, FM.prev).  hipMemset on device memory returns before the fill
// has run, on the legacy stream -- which the handles' own non-blocking streams (and PyTorch's side streams) do not
// wait for: a first launch could read the allocation's old bytes.  So the fill is waited for here, once per create.
inline hipError_t zero_device(void* p, size_t bytes) {
    hipError_t e = hipMemsetAsync(p, 0, bytes, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    return e;
}

// A device array of n elements of T, fixed once allocated (alloc again replaces it).  The three ways a create fills
// one: left as allocated, zero-filled and waited for (zero_device), or uploaded from a host array (synchronous).
template <class T>
struct DevBuf {
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    T* get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    hipError_t alloc(size_t n) {
        reset();
        return hipMalloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
    }
    hipError_t alloc_zero(size_t n) {
        hipError_t e = alloc(n);
        if (e == hipSuccess) e = zero_device(p_, n * sizeof(T));
        return e;
    }
    hipError_t upload(const T* host, size_t n) {
        hipError_t e = alloc(n);
        if (e == hipSuccess) e = hipMemcpy(p_, host, n * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
    hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }

private:
    T* p_ = nullptr;
};

// The sample history every stateful node carries from one launch to the next: the last `len` samples in time order
// (the "ring" of history_order.hpp), twice.  A launch reads cur() and writes the advanced history to next() -- all
// `len` entries of it, so next() never needs a defined content -- and the host calls flip() once the launch is queued.
// upload / download exchange the reference's newest-first state with cur(); they are synchronous and do NOT wait for
// the node's stream: the caller quiesces its handle first.
struct History {
    void* buf[2] = {nullptr, nullptr};
    size_t len = 0, elem = 0;  // samples kept, bytes per sample
    int idx = 0;
    History() = default;
    History(const History&) = delete;
    History& operator=(const History&) = delete;
    ~History() { release(); }
    // both buffers zero-filled (at least one sample each: an empty history still hands the kernels a valid address)
    hipError_t alloc(size_t n_elems, size_t elem_bytes) {
        len = n_elems;
        elem = elem_bytes;
        const size_t bytes = (len ? len : 1) * elem;
        hipError_t e = hipSuccess;
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            e = hipMalloc(&buf[i], bytes);
            if (e == hipSuccess) e = zero_device(buf[i], bytes);
        }
        return e;
    }
    void release() {
        for (void*& b : buf) {
            if (b) (void)hipFree(b);
            b = nullptr;
        }
    }
    template <class T = void>
    T* cur() const { return static_cast<T*>(buf[idx]); }
    template <class T = void>
    T* next() const { return static_cast<T*>(buf[idx ^ 1]); }
    void flip() { idx ^= 1; }
    // state (newest first; entries beyond `len` ignored, missing ones zero) -> cur()
    hipError_t upload(const void* state, size_t n_state) {
        std::vector<char> ring(len * elem);
        state_to_ring(ring.data(), len, state, n_state, elem);
        return len ? hipMemcpy(buf[idx], ring.data(), ring.size(), hipMemcpyHostToDevice) : hipSuccess;
    }
    // cur() -> its newest min(len, n_state) samples, newest first
    hipError_t download(void* state, size_t n_state) const {
        std::vector<char> ring(len * elem);
        hipError_t e = len ? hipMemcpy(ring.data(), buf[idx], ring.size(), hipMemcpyDeviceToHost) : hipSuccess;
        if (e == hipSuccess) ring_to_state(state, n_state, ring.data(), len, elem);
        return e;
    }
};
static_assert(!std::is_copy_constructible_v<Scratch> && !std::is_copy_constructible_v<Pinned> &&
                  !std::is_copy_constructible_v<DevBuf<float>> && !std::is_copy_constructible_v<History>,
              "the owners of device memory are never copied");

// calls moving at most this many bytes each way take the zero-copy route (COMMS_ZERO_COPY_BYTES)
size_t zero_copy_limit();

}  // namespace comms

// Kernel timer: a pool of hipEvent pairs recorded around a node's dominant kernel, device slots that the kernels
// themselves stamp (below), or both (bench / profiling).
struct comms_timer {
    int32_t device = 0;
    size_t n = 0;        // event pairs (0: a stamps-only timer)
    size_t next = 0;     // bracketed launches so far (the pairs wrap modulo n)
    size_t stride = 1;   // events bracket every stride-th launch of the attached node
    size_t seq = 0;      // launches seen since the last reset
    hipEvent_t* start = nullptr;
    hipEvent_t* stop = nullptr;
    size_t ns = 0;       // launches with stamp slots (stamping stops there until the next reset)
    size_t snext = 0;
    unsigned long long* d_begin = nullptr;  // [ns][kStampSlots], initialised to ~0
    unsigned long long* d_end = nullptr;    // [ns][kStampSlots], initialised to 0
};

// In-kernel begin / end stamps of a launch: s_memrealtime (the 100 MHz counter every CU reads alike) taken by the
// first thread of every workgroup when it starts and by every wave once its last store has been acknowledged,
// reduced into kStampSlots slots per launch by atomic min / max (workgroups b and b + kStampSlots share a slot; the
// host reduces the slots).  Unlike an event pair this idles nothing: the launch is an ordinary one, back to back with
// its neighbours in the stream, so the figure is the kernel's duration IN the stream (first wave in to last wave
// out), measured on every launch.  A null KStamp costs a scalar compare at either end of the kernel.
constexpr int kStampSlots = 256;
struct KStamp {
    unsigned long long* begin;
    unsigned long long* end;
};
__device__ __forceinline__ void kstamp_begin(const KStamp& k) {
    if (k.begin != nullptr && threadIdx.x == 0)
        atomicMin(k.begin + (blockIdx.x & (kStampSlots - 1)), static_cast<unsigned long long>(__builtin_amdgcn_s_memrealtime()));
}
__device__ __forceinline__ void kstamp_end(const KStamp& k) {
    if (k.end != nullptr) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if ((threadIdx.x & 63) == 0)
            atomicMax(k.end + (blockIdx.x & (kStampSlots - 1)), static_cast<unsigned long long>(__builtin_amdgcn_s_memrealtime()));
    }
}

namespace comms {

// ---- hard decisions (receive side: comms_chain_set_output_format, comms_sym_to_bits) ---------------------------------
// The contract of include/comms_hip.h: nearest point by d_i = dx*dx + dy*dy, every operation rounded on its own (no FMA),
// i scanned ascending and replaced on a strictly smaller d only -- ties to the lowest index, NaN to index 0.
struct SymTable {
    float2 c[4];  // 2^k points (k = 1: c[0], c[1])
    int k;        // bits per symbol, 1 or 2
};
__device__ __forceinline__ float sym_dist(float2 y, float2 c) {
    const float dx = __fsub_rn(y.x, c.x), dy = __fsub_rn(y.y, c.y);
    return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
}
template <int K>
__device__ __forceinline__ unsigned sym_decide(float2 y, const float2 (&c)[4]) {
    unsigned v = 0;
    float best = sym_dist(y, c[0]);
#pragma unroll
    for (int i = 1; i < (1 << K); ++i) {
        const float d = sym_dist(y, c[i]);
        if (d < best) {
            best = d;
            v = static_cast<unsigned>(i);
        }
    }
    return v;
}
// 32 stream bits made by the lanes of one group (lane l holds `bits` = its `nb` bits at stream offset nb * (l % G),
// G = 32 / nb lanes per group, groups aligned in the wave): OR-ed across the group, the sum lands in every lane of it
template <int G>
__device__ __forceinline__ unsigned bits_gather(unsigned bits) {
#pragma unroll
    for (int s = G / 2; s >= 1; s >>= 1) bits |= static_cast<unsigned>(__shfl_xor(static_cast<int>(bits), s));
    return bits;
}
// One packed 32-bit word at byte offset `byte` of an output of `n_bytes` bytes: whole when it fits, otherwise only the
// bytes before the end (the caller zeroed the bits past the last symbol) -- no byte past the end is written.
__device__ __forceinline__ void bits_store_word(uint8_t* out, size_t byte, size_t n_bytes, unsigned word) {
    if (byte + 4 <= n_bytes) {
        *reinterpret_cast<unsigned*>(out + byte) = word;
    } else {
        for (int i = 0; i < 3; ++i)
            if (byte + i < n_bytes) out[byte + i] = static_cast<uint8_t>(word >> (8 * i));
    }
}
// COMMS_SYM_BITS table of a receiver: the caller's points, or digital.rs's (the pulse node's defaults)
COMMS_INTERNAL comms_status_t sym_table(int32_t bits_per_sym, const comms_c32* constellation, SymTable* out);
// n_sym symbols (device) -> packed bits (device, 4-byte aligned), the pass behind the chain kinds without a fused store stage
COMMS_INTERNAL comms_status_t sym_to_bits_launch(const comms_c32* d_sym, size_t n_sym, const SymTable& t, uint8_t* d_out, hipStream_t s);

// Base of every node handle: device + own stream + scratch for host-pointer runs.
// Streams of handles and host-graph nodes come from a per-device pool and go back to it instead of being destroyed
// (runtime.hip): a HIP event keeps referring to the stream it was last recorded on, and the events that travel with
// pooled buffers outlive the node -- and so the stream -- that recorded them.  On this runtime, synchronising such an
// event after hipStreamDestroy intermittently failed with "operation not permitted when stream is capturing".
COMMS_INTERNAL comms_status_t stream_acquire(int32_t device, hipStream_t* out);
COMMS_INTERNAL void stream_release(int32_t device, hipStream_t s);
// Node handles alive per device (the per-thread handles of the handle-less entry points excepted: they only ever
// follow their own stream).  A handle remembers the last stream it launched on, possibly a pooled one that its owner
// has since released: comms_stream_pool_trim must not destroy streams while such a handle exists.
COMMS_INTERNAL void handle_count(int32_t device, int delta);
// Handles that currently FOLLOW a stream of the device's pool other than their own (a node thread's stream, handed to
// run_dev): comms_stream_pool_trim refuses while there is one -- its owner may have released that stream to the pool,
// and the handle's next drain would synchronise a destroyed stream.  pool_owns: did the pool create `s`?
COMMS_INTERNAL void follower_count(int32_t device, int delta);
COMMS_INTERNAL bool pool_owns(int32_t device, hipStream_t s);
// in + out bytes from which a host-pointer call is pipelined in chunks (COMMS_HOST_PIPE_BYTES, a documented runtime limit
// like COMMS_ZERO_COPY_BYTES; 0 = never)
COMMS_INTERNAL size_t host_pipe_bytes();
COMMS_INTERNAL size_t host_chunk_bytes();  // COMMS_HOST_CHUNK_BYTES: bytes of the larger side per chunk (default 8 MiB)

struct Handle {
    int32_t device = 0;
    hipStream_t stream = nullptr;
    Scratch in_scratch, out_scratch;
    Pinned pin_in, pin_out;
    comms_timer* timer = nullptr;

    // Event bracketing of the dominant kernel launch (no-ops without an attached timer that holds event pairs).
    // Every timed launch site runs exactly one of: tic ... toc, or take_events; each counts the launch once and
    // brackets it only when it is the timer's stride-th.
    bool has_events() const { return timer && timer->n; }
    bool timed() const { return has_events() && timer->seq % timer->stride == 0; }
    void tic(hipStream_t s) {
        if (timed()) (void)hipEventRecord(timer->start[timer->next % timer->n], s);
    }
    void toc(hipStream_t s) {
        if (!has_events()) return;
        if (timed()) {
            (void)hipEventRecord(timer->stop[timer->next % timer->n], s);
            ++timer->next;
        }
        ++timer->seq;
    }
    // For launch_kernel's timed form: the pair that takes the kernel's own begin / end timestamps, or an empty one
    // (launch plainly).
    EventPair take_events() {
        EventPair ev;
        if (!has_events()) return ev;
        if (timed()) {
            ev = EventPair{timer->start[timer->next % timer->n], timer->stop[timer->next % timer->n]};
            ++timer->next;
        }
        ++timer->seq;
        return ev;
    }
    // In-kernel stamps: the slots of the launch about to be made, or a null KStamp when the attached timer has none
    // (left).  Only kernels that take a KStamp are timed this way.
    KStamp next_stamp() {
        if (!timer || !timer->d_begin || timer->snext >= timer->ns) return KStamp{nullptr, nullptr};
        const size_t i = timer->snext++;
        return KStamp{timer->d_begin + i * kStampSlots, timer->d_end + i * kStampSlots};
    }

    bool counted = false;
    comms_status_t init(int32_t dev, bool count_me = true) {
        COMMS_TRY(use_device(dev));
        device = dev;
        COMMS_TRY(stream_acquire(dev, &stream));
        counted = count_me;
        if (counted) handle_count(dev, +1);
        return COMMS_OK;
    }
    // `stream` arguments of the C ABI are passed through as HIP does: NULL is the
    // legacy default stream; COMMS_STREAM_HANDLE selects the handle's own stream.
    hipStream_t pick(void* s) const {
        return s == COMMS_STREAM_HANDLE ? stream : reinterpret_cast<hipStream_t>(s);
    }
    // Device-resident node state (FIR history ping-pong, FM prev, FFT work buffers) is advanced by
    // the launches themselves, in stream order.  A handle therefore follows ONE stream at a time:
    // `enter` is the stream pick of every stateful run_dev -- when the caller moves the node to a
    // different stream, the work still pending on the previous one is drained first (host wait,
    // rare) so that launches on the two streams can never race on the state; `quiesce` is what
    // the state getters / setters call before touching the state from the host.
    hipStream_t last_stream = nullptr;
    bool launched = false;
    bool follows_pooled = false;  // last_stream is a pooled stream that is not this handle's own
    void set_following(hipStream_t s) {
        const bool f = s != nullptr && s != stream && pool_owns(device, s);  // (looked up on a CHANGE of stream only)
        if (f != follows_pooled) follower_count(device, f ? +1 : -1);
        follows_pooled = f;
    }
    comms_status_t enter(void* s_arg, hipStream_t* out) {
        hipStream_t s = pick(s_arg);
        if (launched && s != last_stream) COMMS_TRY(drain());
        if (s != last_stream) set_following(s);
        last_stream = s;
        launched = true;
        *out = s;
        return COMMS_OK;
    }
    comms_status_t quiesce() {
        if (launched) COMMS_TRY(drain());
        return COMMS_OK;
    }
    // Host wait for the launches pending on the stream the handle followed last.  Whatever the outcome the handle
    // forgets that stream: a caller-owned stream that was destroyed meanwhile (against the header's lifetime rule)
    // fails this ONE call and the handle goes on with the next stream it is given.
    comms_status_t drain() {
        hipStream_t s = last_stream;
        launched = false;
        last_stream = nullptr;
        hipError_t e = hipStreamSynchronize(s);
        set_following(nullptr);
        if (e != hipSuccess)
            return fail(COMMS_ERR_DEVICE, "draining the handle's previous stream: %s", hipGetErrorString(e));
        return COMMS_OK;
    }
    // The host-pointer form of a node: `launch(d_in, d_out)` runs the device form on this handle's
    // stream.  Short calls work on host-mapped pinned staging (two CPU copies instead of two DMA
    // submissions), longer ones go through device scratch.  Synchronous.
    template <class F>
    comms_status_t run_host(const void* in, size_t in_bytes, void* out, size_t out_bytes, F&& launch) {
        if (in_bytes <= zero_copy_limit() && out_bytes <= zero_copy_limit()) {
            COMMS_TRY(pin_in.reserve(in_bytes));
            COMMS_TRY(pin_out.reserve(out_bytes));
            std::memcpy(pin_in.h, in, in_bytes);
            COMMS_TRY(launch(pin_in.d, pin_out.d));
            COMMS_HIP_TRY(hipStreamSynchronize(stream));
            std::memcpy(out, pin_out.h, out_bytes);
            return COMMS_OK;
        }
        COMMS_TRY(in_scratch.reserve(in_bytes));
        COMMS_TRY(out_scratch.reserve(out_bytes));
        COMMS_HIP_TRY(hipMemcpyAsync(in_scratch.p, in, in_bytes, hipMemcpyHostToDevice, stream));
        COMMS_TRY(launch(in_scratch.p, out_scratch.p));
        COMMS_HIP_TRY(hipMemcpyAsync(out, out_scratch.p, out_bytes, hipMemcpyDeviceToHost, stream));
        COMMS_HIP_TRY(hipStreamSynchronize(stream));
        return COMMS_OK;
    }

    // ---- long host-pointer calls, pipelined (round 5) ----------------------------------------------------------------
    // The drop-in path of a comms-rs graph is `run(&[Complex<T>]) -> Vec<Complex<T>>` (src/filter/fir_node.rs:215-220):
    // host memory in, host memory out.  Until round 4 that was one copy in, the launch, one copy out, one direction of
    // the PCIe link at a time.  Above kHostPipeBytes (and where both directions carry bytes) the batch is now cut into chunks of whole UNITS (a unit = in_u input
    // bytes that yield out_u output bytes: a sample, `rate` samples of a decimator, one transform): the calling thread
    // feeds chunk after chunk -- copy in, launch(es), an event -- and a helper thread copies each chunk's outputs back
    // on a second stream as soon as its event has fired, so that the two directions of the link run together.  Stateful
    // nodes stream across the chunks exactly as they stream across calls (same launches, same order, one stream), so the
    // samples are bit-identical to the single-shot path (tests/test_gpu_host_pipeline.py).
    hipStream_t out_stream = nullptr;
    std::vector<hipEvent_t> pipe_events;
    static constexpr size_t kHostPipeBytes = 64u << 20;   // in + out bytes from which a call is pipelined
    static constexpr size_t kHostChunkBytes = 16u << 20;  // of the larger side, per chunk
    template <class F>
    comms_status_t run_host_units(const void* in, size_t in_bytes, size_t in_u, void* out, size_t out_bytes, size_t out_u, F&& launch) {
        const size_t big_u = in_u > out_u ? in_u : out_u;
        size_t per = big_u ? host_chunk_bytes() / big_u : 0;
        if (per < 1) per = 1;
        const size_t n_units = in_u ? (in_bytes + in_u - 1) / in_u : 1;
        const size_t n_chunks = (n_units + per - 1) / per;
        // Only where BOTH directions carry a real share of the bytes: what the pipeline buys is the two directions of the
        // link at once (2^24 samples through the FIR node: 4.84 -> 3.26 ms); a decimating chain's output is an eighth of
        // its input, and its one big copy in is faster whole than in chunks (2.74 against 2.82 - 3.20 ms) --
        // scripts/bench_host_path.py, profiles/r05_host_pipeline.txt
        const bool both_ways = out_bytes * 4 >= in_bytes && in_bytes * 4 >= out_bytes;
        if (in_bytes + out_bytes < host_pipe_bytes() || n_chunks < 2 || !in_u || !out_u || !both_ways)
            return run_host(in, in_bytes, out, out_bytes, [&](void* d_in, void* d_out) { return launch(d_in, d_out, in_bytes, out_bytes); });
        COMMS_TRY(in_scratch.reserve(in_bytes));
        COMMS_TRY(out_scratch.reserve(out_bytes));
        if (!out_stream) COMMS_TRY(stream_acquire(device, &out_stream));
        while (pipe_events.size() < n_chunks) {
            hipEvent_t e = nullptr;
            COMMS_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            pipe_events.push_back(e);
        }
        struct Shared {
            std::mutex m;
            std::condition_variable cv;
            size_t recorded = 0;   // chunks whose event has been recorded
            bool abort = false;
            hipError_t err = hipSuccess;
        } sh;
        const char* cin = static_cast<const char*>(in);
        char* cout_ = static_cast<char*>(out);
        char* din = static_cast<char*>(in_scratch.p);
        char* dout = static_cast<char*>(out_scratch.p);
        auto out_range = [&](size_t k, size_t& o0, size_t& o1) {
            o0 = k * per * out_u;
            o1 = (k + 1) * per * out_u;
            if (o0 > out_bytes) o0 = out_bytes;
            if (o1 > out_bytes || k + 1 == n_chunks) o1 = out_bytes;
        };
        std::thread back([&] {
            if (hipSetDevice(device) != hipSuccess) {
                std::lock_guard<std::mutex> lk(sh.m);
                sh.err = hipErrorInvalidDevice;
                return;
            }
            for (size_t k = 0; k < n_chunks; ++k) {
                {
                    std::unique_lock<std::mutex> lk(sh.m);
                    sh.cv.wait(lk, [&] { return sh.recorded > k || sh.abort; });
                    if (sh.abort) return;
                }
                size_t o0, o1;
                out_range(k, o0, o1);
                hipError_t e = hipStreamWaitEvent(out_stream, pipe_events[k], 0);
                if (e == hipSuccess && o1 > o0) e = hipMemcpyAsync(cout_ + o0, dout + o0, o1 - o0, hipMemcpyDeviceToHost, out_stream);
                if (e != hipSuccess) {
                    std::lock_guard<std::mutex> lk(sh.m);
                    sh.err = e;
                    return;
                }
            }
            hipError_t e = hipStreamSynchronize(out_stream);
            if (e != hipSuccess) {
                std::lock_guard<std::mutex> lk(sh.m);
                sh.err = e;
            }
        });
        comms_status_t st = COMMS_OK;
        for (size_t k = 0; k < n_chunks && st == COMMS_OK; ++k) {
            size_t i0 = k * per * in_u, i1 = (k + 1) * per * in_u;
            if (i1 > in_bytes || k + 1 == n_chunks) i1 = in_bytes;
            size_t o0, o1;
            out_range(k, o0, o1);
            hipError_t e = hipMemcpyAsync(din + i0, cin + i0, i1 - i0, hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) st = fail(COMMS_ERR_DEVICE, "host pipeline: copy in failed: %s", hipGetErrorString(e));
            if (st == COMMS_OK) st = launch(din + i0, dout + o0, i1 - i0, o1 - o0);
            if (st == COMMS_OK && (e = hipEventRecord(pipe_events[k], stream)) != hipSuccess)
                st = fail(COMMS_ERR_DEVICE, "host pipeline: event record failed: %s", hipGetErrorString(e));
            std::lock_guard<std::mutex> lk(sh.m);
            if (st == COMMS_OK) sh.recorded = k + 1;
            else sh.abort = true;
            sh.cv.notify_all();
        }
        back.join();
        if (st != COMMS_OK) {
            (void)hipStreamSynchronize(stream);  // nothing of this call stays in flight behind an error
            return st;
        }
        if (sh.err != hipSuccess) return fail(COMMS_ERR_DEVICE, "host pipeline: copy out failed: %s", hipGetErrorString(sh.err));
        COMMS_HIP_TRY(hipStreamSynchronize(stream));
        return COMMS_OK;
    }

    // Runs after the members of the derived handle have gone (their device memory is freed first), on the handle's
    // device (HandleDelete): staging freed, the streams back to the device's pool.
    Handle() = default;
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() {
        set_following(nullptr);
        for (hipEvent_t e : pipe_events) (void)hipEventDestroy(e);
        if (out_stream) stream_release(device, out_stream);
        in_scratch.release();
        out_scratch.release();
        pin_in.release();
        pin_out.release();
        if (stream) stream_release(device, stream);
        if (counted) handle_count(device, -1);
    }
};

// The one owner of a handle: its deleter selects the handle's device (the current device is thread-local, and the
// members' destructors free device memory), then deletes.  Creates hold their handle in one until `*out = h.release()`,
// so every failure exit is a plain return; inner handles of a handle (the chain's FIR, a channelizer's chains) are
// members of this type.
struct HandleDelete {
    template <class H>
    void operator()(H* h) const {
        if (h->stream) (void)use_device(h->device);  // (no stream: init failed, nothing on any device yet)
        delete h;
    }
};
template <class H>
using HandlePtr = std::unique_ptr<H, HandleDelete>;

// What every *_create starts with: a handle of its own stream on `device`, or the error and no handle
template <class H>
comms_status_t make_handle(int32_t device, HandlePtr<H>* out, bool count_me = true) {
    HandlePtr<H> h(new (std::nothrow) H);
    COMMS_ARG(h != nullptr, "out of host memory");
    COMMS_TRY(h->init(device, count_me));
    *out = std::move(h);
    return COMMS_OK;
}
// ... and the body of every *_destroy: the handle drained (the launches pending on the stream it followed last may
// still touch its memory; a failure to wait changes nothing about what follows), then deleted.  NULL is fine.
template <class H>
comms_status_t destroy_handle(H* h) {
    if (!h) return COMMS_OK;
    (void)use_device(h->device);
    (void)h->quiesce();
    HandleDelete{}(h);
    return COMMS_OK;
}
// An inner handle whose type is opaque where it is held (the chain's mixer): made by its public create, ended by its
// public destroy -- which is destroy_handle again
template <auto Destroy>
struct DestroyWith {
    template <class H>
    void operator()(H* h) const {
        (void)Destroy(h);
    }
};
template <class H, auto Destroy>
using InnerHandle = std::unique_ptr<H, DestroyWith<Destroy>>;

// Handle-less host-pointer entry points (resampling, IQ formats, estimators) borrow a per-thread,
// per-device handle (stream + staging), created on first use and kept for the thread's life:
// no hipMalloc / hipFree -- which also synchronise the device -- per call.  The handles END with their thread
// (comms-rs starts one thread per node, src/node/mod.rs:276-284: a graph that is torn down and rebuilt must not leave
// a pooled stream, device scratch and pinned staging behind per retired node thread).
inline comms_status_t thread_handle(int32_t device, Handle** out) {
    static thread_local HandlePtr<Handle> th[64];
    COMMS_ARG(device >= 0 && device < 64, "device index out of range");
    if (!th[device]) COMMS_TRY(make_handle(device, &th[device], false));
    *out = th[device].get();
    return COMMS_OK;
}

inline bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char* pa = static_cast<const char*>(a);
    const char* pb = static_cast<const char*>(b);
    return pa < pb + nb && pb < pa + na;
}
inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// A record of `bits` packed bits: whole bytes, rounded up to 4
inline size_t bit_record_bytes(size_t bits) { return ((bits + 7) / 8 + 3) / 4 * 4; }

// The quantiser of the soft-input decoders (Viterbi, LDPC): q = clamp(rint(L * qscale), -127, 127), the product rounded to
// f32 (no FMA), halves to even, NaN -> 0
__device__ __forceinline__ int quantise_llr(float L, float qscale) {
    const float x = __fmul_rn(L, qscale);
    float r = rintf(x);                       // to nearest, halves to even
    r = x != x ? 0.f : r;                     // NaN: an erasure
    r = r < -127.f ? -127.f : r > 127.f ? 127.f : r;
    return static_cast<int>(r);
}

// The body of every *_set_timer that only attaches the timer
template <class H>
comms_status_t set_handle_timer(H* h, comms_timer_t* t) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    h->timer = t;
    return COMMS_OK;
}

// ---- the call shell of the per-frame nodes (encoder ... OFDM): n_frames input records in, n_frames output records out -------
struct FrameCall {
    size_t in_bytes, out_bytes;     // per frame (out_bytes = 0: the call writes no such output, and `out` may be NULL)
    uintptr_t in_align, out_align;  // of the device pointers
    size_t max_frames;              // the node's own limit
};
// What every frame call checks, in this order: the handle, NULL pointers only with n_frames = 0, the node's limit and the byte
// counts, and -- for device pointers -- their alignment and that the input and output records do not overlap.  `call(h)`
// describes the handle's records; it is asked once h is known not to be NULL.  A device form goes on with
// `if (!n_frames) return COMMS_OK;` and use_device.  (static: the instantiations are no symbols of the library.)
template <class H, class D>
static comms_status_t check_frame_call(const H* h, D&& call, const void* in, size_t n_frames, const void* out, bool device) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    const FrameCall c = call(h);
    COMMS_ARG(!n_frames || (in && (out || !c.out_bytes)), "NULL pointer");
    COMMS_ARG(n_frames <= c.max_frames, "n_frames must be at most %zu (got %zu)", c.max_frames, n_frames);
    COMMS_ARG(!n_frames || (c.in_bytes <= SIZE_MAX / 2 / n_frames && c.out_bytes <= SIZE_MAX / 2 / n_frames), "n_frames overflows");
    if (device) {
        COMMS_ARG(aligned(in, c.in_align) && aligned(out, c.out_align), "the input must be aligned to %zu bytes and the output to %zu",
                  static_cast<size_t>(c.in_align), static_cast<size_t>(c.out_align));
        COMMS_ARG(!n_frames || !ranges_overlap(in, n_frames * c.in_bytes, out, n_frames * c.out_bytes), "the input and output records overlap");
    }
    return COMMS_OK;
}
// The host-pointer form: the same checks, then Handle::run_host around `run_dev(d_in, d_out)`, which forwards to the node's
// device form on COMMS_STREAM_HANDLE
template <class H, class D, class F>
static comms_status_t run_frame_call(H* h, D&& call, const void* in, size_t n_frames, void* out, F&& run_dev) {
    COMMS_TRY(check_frame_call(h, call, in, n_frames, out, false));
    if (!n_frames) return COMMS_OK;
    COMMS_TRY(use_device(h->device));
    const FrameCall c = call(h);
    return h->run_host(in, n_frames * c.in_bytes, out, n_frames * c.out_bytes, run_dev);
}

// Stride (in elements, >= len) of R phase arrays that a staging row scatters over: sample s goes to [s mod R][s div R].
// The LDS serves a row `lanes` lanes at a time over as many element-wide banks (32 for a ds_write_b32, 16 for a
// ds_write_b64); a group holds consecutive samples, i.e. up to R phases x ~lanes / R consecutive elements, at banks
// (phase * stride + element) mod lanes.  Two lanes on a bank cost nothing (the instruction takes its cycles anyway), more
// do: count the lanes beyond two per bank over every alignment of the group and take the residue with the fewest.
inline int plan_stride(int R, int len, int lanes = 32) {
    int best = len, best_cost = -1;
    for (int c = 0; c < lanes; ++c) {
        const int stride = len + c;
        int cost = 0;
        for (int s0 = 0; s0 < R * lanes; s0 += lanes) {  // every phase alignment of a group (period R groups)
            int banks[32] = {0};
            for (int l = 0; l < lanes; ++l) {
                const int s = s0 + l;
                ++banks[((s % R) * stride + s / R) & (lanes - 1)];
            }
            int worst = 0;
            for (int b = 0; b < lanes; ++b) worst = banks[b] > worst ? banks[b] : worst;
            cost += worst > 2 ? worst - 2 : 0;
        }
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = stride;
        }
    }
    return best;
}

constexpr int kNumCU = 256;  // MI355X: 8 XCD x 32 CU
// Grid cap of a persistent kernel that uses `lds` bytes per workgroup: the workgroups the chip holds at once, at most
// eight per CU and as many as fit the CU's 160 KiB of LDS (a kernel below 1 KiB counts as 1 KiB).  The diagnostic build's
// COMMS_GRID_CAP = c > 0 lowers it to at most c, so that every persistent loop makes many passes over a small call
// (tests/test_gpu_small_grids.py); it is read at each call: a handle takes its cap at create, one process makes handles
// under several.  grid_cap() is the one place that reads the knob: the handles that size their grid by hand (demod.hip's
// 4 and 8 workgroups per CU) pass their own `chip`.
inline unsigned grid_cap(unsigned chip) {
    const int cap = diag_knob("COMMS_GRID_CAP", 0);
    return cap > 0 && static_cast<unsigned>(cap) < chip ? static_cast<unsigned>(cap) : chip;
}
inline unsigned resident_workgroups(size_t lds) {
    const size_t per_cu = (160 * 1024) / (lds < 1024 ? 1024 : lds);
    return grid_cap(static_cast<unsigned>(kNumCU * (per_cu > 8 ? 8 : per_cu < 1 ? 1 : per_cu)));
}
// The grid of a persistent launch with `blocks` workgroups' worth of work: at least one, at most the handle's cap
inline size_t capped_grid(size_t blocks, unsigned max_grid) { return blocks < 1 ? 1 : blocks < max_grid ? blocks : max_grid; }

// ---- 16-byte output stores of the streaming kernels: plain, or written through the L2 ----------------------------------
// A plain store leaves its line dirty in the XCD's L2; what is still dirty when the kernel ends is written back behind its
// last wave, in front of the next kernel of the stream.  An `sc1` store writes through and drops the line, so the bytes
// leave while the kernel is still streaming -- at 16 bytes per lane at the price of a plain store (narrower ones pay per
// byte: the 8-byte kernels keep plain stores).  WT = false is the plain twin: both forms of a kernel come from one body.
// `p` is 16-byte aligned.  (A vector store; the string ends in `s_nop 1`: the compiler's next instruction must not
// overwrite the data registers before the store has read them.)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <bool WT>
__device__ __forceinline__ void store16(void* p, uint4 v) {
    if constexpr (WT) {
        const u32x4 d = {v.x, v.y, v.z, v.w};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(d) : "memory");
    } else {
        *static_cast<uint4*>(p) = v;
    }
}
template <bool WT>
__device__ __forceinline__ void store16(void* p, float4 v) {
    store16<WT>(p, make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)));
}
// Which form a call takes is decided here, for the mixer and the decimator alike: write-through only when the call's output
// exceeds the chip's L2 (8 XCDs x 4 MiB) -- a smaller output is better left there for the next kernel's first reads.
// COMMS_WT_MIN_BYTES (the diagnostic build, read once) moves the threshold: 0 = every call that can (tests/test_gpu_store_forms.py).
constexpr size_t kWriteThroughMinBytes = 32u << 20;
inline bool write_through(size_t out_bytes) {
    static const size_t min_bytes = static_cast<size_t>(diag_knob("COMMS_WT_MIN_BYTES", static_cast<int>(kWriteThroughMinBytes)));
    return out_bytes > min_bytes;
}

// Mixer phase bookkeeping shared by the mixer node and the fused chain: phases are
// 64-bit fixed-point fractions ("turns") of T = fl(2*pi), the constant the reference
// wraps with (src/mixer.rs:79-82).
constexpr double kMixT = 2.0 * 3.14159265358979323846264338327950288;
inline uint64_t mix_to_turns(double angle) {
    long double r = fmodl(static_cast<long double>(angle), static_cast<long double>(kMixT));
    if (r < 0) r += static_cast<long double>(kMixT);
    long double t = r / static_cast<long double>(kMixT) * 18446744073709551616.0L;
    if (t >= 18446744073709551616.0L) return 0;
    return static_cast<uint64_t>(t);
}
inline void mix_host_rotor(uint64_t turns, double& c, double& s) {
    double ang = static_cast<double>(turns >> 11) * (kMixT * 0x1.0p-53);
    c = cos(ang);
    s = sin(ang);
}
// The mixer's device arithmetic (pointwise.hip's kernels, the symbol synchroniser's store stage): the rotor of a phase in
// turns, and Mixer::mix of one sample -- (xr + i xi) * (c + i s) in num-complex's form, f64, then `as f32`
__device__ inline void mix_rotor_at(uint64_t turns, double& c, double& s) {
    double ang = static_cast<double>(turns >> 11) * (kMixT * 0x1.0p-53);
    sincos(ang, &s, &c);
}
__device__ inline float2 mix_one(float2 x, double c, double s) {
    double xr = static_cast<double>(x.x), xi = static_cast<double>(x.y);
    return make_float2(static_cast<float>(xr * c - xi * s), static_cast<float>(xr * s + xi * c));
}
// Mixer::new (src/mixer.rs:43-51): dphase wrapped into [0, 2pi)
inline double mix_wrap_dphase(double dphase) {
    if (fabs(dphase) > 64.0 * kMixT) dphase = fmod(dphase, kMixT);
    while (dphase >= kMixT) dphase -= kMixT;
    while (dphase < 0.0) dphase += kMixT;
    return dphase;
}

}  // namespace comms
