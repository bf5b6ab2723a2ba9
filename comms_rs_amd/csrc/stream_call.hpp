// stream_call.hpp -- the host shell of the stream nodes (rfir_decim ... ofdmsync): what a node with a History, a stream
// position or a detection list does around its own kernel.  A new stream node gets from here
//   * its state accessors: get_history_state / set_history_state (state_access alone in front of a series fallback);
//   * its position accessors and the threshold check: get_position / set_position, check_threshold / set_threshold;
//   * the input-only host staging of a node that returns no sample stream: stage_input;
//   * the whole detection step of a synchroniser: detect_prologue, detection_bound, detection_step;
//   * the grid of its persistent kernel (tile_grid, persistent_cap) and, for a polyphase filter, polyphase_rows and tile_workgroup.
// (Everything here is static: no function or instantiation of this header is a symbol of the library.)
#pragma once

#include <algorithm>
#include <vector>

#include "common.hpp"

namespace comms {

// ---- state ------------------------------------------------------------------------------------------------------------
// What every state accessor checks and does before it touches the state: `state` may be NULL only with n_state == 0; a
// getter (exact = false) takes n_state <= len, a setter exactly len.  Then the handle's device, and its stream drained:
// the history is advanced by the launches, on whatever stream they ran, and no pending launch may still read a buffer
// that is overwritten.  `what` names the entries ("samples", "symbols").
static inline comms_status_t state_access(Handle* h, size_t len, const void* state, size_t n_state, bool exact, const char* what) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    if (exact)
        COMMS_ARG(n_state == len, "n_state must be exactly the %zu %s of the state (got %zu)", len, what, n_state);
    else
        COMMS_ARG(n_state <= len, "n_state %zu exceeds the %zu %s of the state", n_state, len, what);
    COMMS_ARG(state != nullptr || !n_state, "state is NULL");
    COMMS_TRY(use_device(h->device));
    return h->quiesce();
}
// The newest n_state entries of h->hist, newest first ...
template <class H>
static comms_status_t get_history_state(H* h, void* state, size_t n_state, const char* what) {
    COMMS_TRY(state_access(h, h ? h->hist.len : 0, state, n_state, false, what));
    if (!n_state) return COMMS_OK;
    COMMS_HIP_TRY(h->hist.download(state, n_state));
    return COMMS_OK;
}
// ... and all of them written
template <class H>
static comms_status_t set_history_state(H* h, const void* state, size_t n_state, const char* what) {
    COMMS_TRY(state_access(h, h ? h->hist.len : 0, state, n_state, true, what));
    COMMS_HIP_TRY(h->hist.upload(state, n_state));
    return COMMS_OK;
}

// ---- position and threshold (a handle with a stream index T) -------------------------------------------------------------
template <class H>
static comms_status_t get_position(const H* h, uint64_t* out_position) {
    COMMS_ARG(h && out_position, "NULL argument");
    *out_position = h->T;
    return COMMS_OK;
}
// reset(): what the node forgets when its stream moves (the origin of a flush, the pending frames)
template <class H, class R>
static comms_status_t set_position(H* h, uint64_t position, R&& reset) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(position <= (1ull << 62), "position is out of range");
    h->T = position;
    reset();
    return COMMS_OK;
}
static inline comms_status_t check_threshold(double thr) {
    COMMS_ARG(thr > 0.0 && thr <= 1.0, "threshold must lie in (0, 1] (got %g)", thr);  // a NaN fails both
    return COMMS_OK;
}
template <class H>
static comms_status_t set_threshold(H* h, double thr) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_TRY(check_threshold(thr));
    h->thr = static_cast<float>(thr);
    return COMMS_OK;
}

// ---- input-only host staging -----------------------------------------------------------------------------------------------
// `bytes` > 0 of host input where a launch on the handle's own stream can read them: short blocks straight from pinned host
// memory, long ones uploaded (Handle::run_host without the output side)
static inline comms_status_t stage_input(Handle* h, const void* in, size_t bytes, const void** d) {
    if (bytes <= zero_copy_limit()) {
        COMMS_TRY(h->pin_in.reserve(bytes));
        std::memcpy(h->pin_in.h, in, bytes);
        *d = h->pin_in.d;
    } else {
        COMMS_TRY(h->in_scratch.reserve(bytes));
        COMMS_HIP_TRY(hipMemcpyAsync(h->in_scratch.p, in, bytes, hipMemcpyHostToDevice, h->stream));
        *d = h->in_scratch.p;
    }
    return COMMS_OK;
}

// ---- the detection step of the synchronisers ---------------------------------------------------------------------------
constexpr size_t kDetFirst = 16;  // detections copied back together with the count

// The argument checks of run_dev (device = true: `in` is a device pointer), run and flush, in this order; then no
// detections yet and the handle's device.  The caller goes on with `if (!n) return COMMS_OK;`.
static inline comms_status_t detect_prologue(Handle* h, const void* in, size_t n, bool device, const comms_frame_detection_t* out, size_t cap,
                                      size_t* n_found) {
    COMMS_ARG(h != nullptr, "handle is NULL");
    COMMS_ARG(n_found != nullptr, "n_found is NULL");
    COMMS_ARG(out != nullptr || !cap, "out is NULL with cap > 0");
    COMMS_ARG(in || !n, "%s is NULL", device ? "d_in" : "in");
    COMMS_ARG(!device || aligned(in, 8), "d_in must be aligned to one sample (8 bytes)");
    COMMS_ARG(n <= SIZE_MAX / 8, "n overflows");
    *n_found = 0;
    return use_device(h->device);
}
// Detections are more than `guard` positions apart: a call on n positions has at most ceil(n / (guard + 1))
static inline size_t detection_bound(size_t n, size_t guard) { return n / (guard + 1) + (n % (guard + 1) ? 1 : 0); }

// One detection launch on stream s and its results.  The list scratch is sized to `bound` entries behind an 8-byte counter,
// which is cleared; `launch(count, entries, list_cap)` fills the node's arguments, launches `kernel`, flips the history and
// advances the position; the count and the first kDetFirst entries come back in one copy, the rest, rarely, in a second;
// the entries are sorted by index (the order of arrival does not show), the first min(count, cap) go to `out` and the true
// count to *n_found.  Ends synchronised.
template <class L>
static comms_status_t detection_step(Scratch& list, size_t bound, hipStream_t s, const char* kernel, L&& launch,
                                     comms_frame_detection_t* out, size_t cap, size_t* n_found) {
    constexpr size_t kDet = sizeof(comms_frame_detection_t);
    COMMS_ARG(bound <= 0xFFFFFFFFull / kDet, "n is too long for one call");
    COMMS_TRY(list.reserve(8 + bound * kDet));
    char* d_list = static_cast<char*>(list.p);
    COMMS_HIP_TRY(hipMemsetAsync(d_list, 0, 8, s));
    COMMS_TRY(launch(reinterpret_cast<unsigned*>(d_list), reinterpret_cast<comms_frame_detection_t*>(d_list + 8), static_cast<unsigned>(bound)));
    const size_t first = bound < kDetFirst ? bound : kDetFirst;
    char head[8 + kDetFirst * kDet];
    hipError_t e = hipMemcpyAsync(head, d_list, 8 + first * kDet, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(COMMS_ERR_DEVICE, "%s: copy-back: %s", kernel, hipGetErrorString(e));
    unsigned count = 0;
    std::memcpy(&count, head, sizeof count);
    if (count > bound) return fail(COMMS_ERR_DEVICE, "%s reported %u detections, more than the bound %zu", kernel, count, bound);
    std::vector<comms_frame_detection_t> det(count);
    if (count) std::memcpy(det.data(), head + 8, (count < first ? count : first) * kDet);
    if (count > first) {
        e = hipMemcpyAsync(det.data() + first, d_list + 8 + first * kDet, (count - first) * kDet, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(COMMS_ERR_DEVICE, "%s: copy-back: %s", kernel, hipGetErrorString(e));
    }
    std::sort(det.begin(), det.end(), [](const comms_frame_detection_t& x, const comms_frame_detection_t& y) { return x.index < y.index; });
    const size_t take = count < cap ? count : cap;
    if (take) std::memcpy(out, det.data(), take * kDet);
    *n_found = count;
    return COMMS_OK;
}

// ---- grids and polyphase tables ------------------------------------------------------------------------------------------
// The grid of a persistent kernel that walks `tiles` tiles: capped_grid, except that an empty call has no grid (nothing is
// launched for it, and get_kernel reports grid=0)
static inline size_t tile_grid(size_t tiles, unsigned max_grid) { return tiles ? capped_grid(tiles, max_grid) : 0; }
// The cap itself, from the LDS bytes of a workgroup (0: a kernel without LDS): the workgroups the chip holds at once, lowered by the
// diagnostic build's COMMS_GRID_CAP.  A node that takes its cap here has its capped-grid cases in a test file of its own
// (tests/test_gpu_spectrum_grids.py); tests/grid_cases.py lists the .hip files that ask common.hpp directly.
static inline unsigned persistent_cap(size_t lds) { return resident_workgroups(lds); }

// Polyphase row table of `taps` over L phases, rows of RS floats padded with zeros: tab[p * RS + q] = taps[p + L * q]
static inline std::vector<float> polyphase_rows(const float* taps, size_t n_taps, size_t L, size_t RS) {
    std::vector<float> tab(L * RS, 0.0f);
    for (size_t p = 0; p < L; ++p)
        for (size_t q = 0; p + L * q < n_taps; ++q) tab[p * RS + q] = taps[p + L * q];
    return tab;
}
// Lanes of the workgroup that takes a tile of TO outputs: one per output, between one wave and four
static inline int tile_workgroup(int TO) { return TO >= 256 ? 256 : TO < 64 ? 64 : TO; }

}  // namespace comms
