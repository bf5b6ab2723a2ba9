// history_order.hpp -- the two layouts of a node's sample history, and the one conversion between them.
// Host-only on purpose (no HIP header): tests/history_order_test.cpp compiles it alone, under the sanitizers.
//
//   ring  : what the kernels read and write -- the last `hist_len` samples in TIME order, oldest first
//   state : what the reference keeps and the C ABI exchanges -- NEWEST first, of any length n_state: only
//           min(hist_len, n_state) entries take part (zip(taps, state), fir.rs:53)
//
// Elements are opaque blocks of `elem` bytes (float, float2, short2, double2; comms_c16 / c32 / c64 are laid out alike).
#pragma once

#include <cstddef>
#include <cstring>

namespace comms {

// ring[hist_len - 1 - k] = state[k] for k < min(hist_len, n_state); every other ring entry is zero
inline void state_to_ring(void* ring, size_t hist_len, const void* state, size_t n_state, size_t elem) {
    char* r = static_cast<char*>(ring);
    const char* s = static_cast<const char*>(state);
    if (hist_len) std::memset(r, 0, hist_len * elem);
    for (size_t k = 0; k < hist_len && k < n_state; ++k) std::memcpy(r + (hist_len - 1 - k) * elem, s + k * elem, elem);
}

// state[k] = ring[hist_len - 1 - k] for k < min(hist_len, n_state): the newest n_state samples
inline void ring_to_state(void* state, size_t n_state, const void* ring, size_t hist_len, size_t elem) {
    char* s = static_cast<char*>(state);
    const char* r = static_cast<const char*>(ring);
    for (size_t k = 0; k < hist_len && k < n_state; ++k) std::memcpy(s + k * elem, r + (hist_len - 1 - k) * elem, elem);
}

}  // namespace comms
