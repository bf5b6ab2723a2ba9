// Stand-alone check of comms_rs_amd/csrc/history_order.hpp (the only project header included): built and run by
// tests/test_history_order.py under AddressSanitizer and UBSan.  Exit status 0 = every case holds.
//
// Cases: element sizes 4 / 8 / 16 bytes x hist_len 0 / 1 / 2 / 7 x n_state 0 / 1 / hist_len - 1 / hist_len, and
// n_state = hist_len + 3 on the state -> ring side (the extra entries are ignored).  Every buffer is a heap allocation
// of its exact size plus a sentinel byte on either side: a stray byte shows in a sentinel, anything longer to the sanitizer.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "history_order.hpp"

namespace {

constexpr unsigned char kGuard = 0xA5;
int failures = 0;

void expect(bool ok, const char* what, size_t elem, size_t hist_len, size_t n_state) {
    if (ok) return;
    ++failures;
    std::fprintf(stderr, "FAIL %s: elem %zu hist_len %zu n_state %zu\n", what, elem, hist_len, n_state);
}

// `bytes` payload bytes between two sentinels
struct Guarded {
    std::vector<unsigned char> v;
    explicit Guarded(size_t bytes, unsigned char fill) : v(bytes + 2, fill) { v.front() = v.back() = kGuard; }
    unsigned char* p() { return v.data() + 1; }
    bool intact() const { return v.front() == kGuard && v.back() == kGuard; }
};

// byte b of state entry k: never zero, different for every (k, b) in range
unsigned char pattern(size_t k, size_t b) { return static_cast<unsigned char>(1 + (k * 16 + b) % 251); }

void one_case(size_t elem, size_t hist_len, size_t n_state) {
    Guarded state(n_state * elem, 0), ring(hist_len * elem, 0xEE);
    for (size_t k = 0; k < n_state; ++k)
        for (size_t b = 0; b < elem; ++b) state.p()[k * elem + b] = pattern(k, b);

    comms::state_to_ring(ring.p(), hist_len, state.p(), n_state, elem);
    const size_t used = n_state < hist_len ? n_state : hist_len;
    bool placed = true, zero = true;
    for (size_t k = 0; k < used; ++k)  // ring entry hist_len - 1 - k is state entry k
        placed = placed && std::memcmp(ring.p() + (hist_len - 1 - k) * elem, state.p() + k * elem, elem) == 0;
    for (size_t i = 0; i < (hist_len - used) * elem; ++i) zero = zero && ring.p()[i] == 0;  // the older entries
    expect(placed, "state -> ring placement", elem, hist_len, n_state);
    expect(zero, "state -> ring zero fill", elem, hist_len, n_state);
    expect(state.intact() && ring.intact(), "state -> ring sentinels", elem, hist_len, n_state);

    if (n_state > hist_len) return;  // the getters never ask for more than the history
    // the inverse, from a FULL ring (entry j of time order carries pattern(hist_len - 1 - j, .)): the newest n_state
    Guarded full(hist_len * elem, 0), back(n_state * elem, 0xEE);
    for (size_t j = 0; j < hist_len; ++j)
        for (size_t b = 0; b < elem; ++b) full.p()[j * elem + b] = pattern(hist_len - 1 - j, b);
    comms::ring_to_state(back.p(), n_state, full.p(), hist_len, elem);
    expect(std::memcmp(back.p(), state.p(), n_state * elem) == 0, "ring -> state", elem, hist_len, n_state);
    expect(full.intact() && back.intact(), "ring -> state sentinels", elem, hist_len, n_state);
    // ... and the round trip of the ring made above
    Guarded again(n_state * elem, 0xEE);
    comms::ring_to_state(again.p(), n_state, ring.p(), hist_len, elem);
    expect(std::memcmp(again.p(), state.p(), n_state * elem) == 0, "round trip", elem, hist_len, n_state);
    expect(again.intact() && ring.intact(), "round trip sentinels", elem, hist_len, n_state);
}

}  // namespace

int main() {
    int cases = 0;
    for (size_t elem : {4u, 8u, 16u})
        for (size_t hist_len : {0u, 1u, 2u, 7u}) {
            std::set<size_t> ns = {0, 1, hist_len, hist_len + 3};
            if (hist_len) ns.insert(hist_len - 1);
            for (size_t n_state : ns) {  // (n_state 1 at hist_len 0 is an excess too)
                one_case(elem, hist_len, n_state);
                ++cases;
            }
        }
    std::printf("%d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
