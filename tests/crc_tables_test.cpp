// The host arithmetic of the frame check (comms_rs_amd/csrc/crc_tables.hpp) against the bit-serial register of the contract:
// the word-parallel combination crc_combine -- lane by lane, round by round, as crc.hip's kernels form it -- must equal the
// register for every width, every length that takes another path, and a non-zero init.  Includes only that header; built with
// AddressSanitizer and UBSan by tests/test_crc_tables.py and run as a program of its own.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "crc_tables.hpp"

using namespace comms;

static int failures = 0, checks = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return static_cast<uint32_t>(rng_state >> 16);
}

struct Params {
    unsigned W;
    uint32_t poly, init, xorout;
};

static void check_length(const Params& q, unsigned T) {
    const CrcPlan p = crc_plan(q.W, q.poly, q.init, q.xorout, T);
    // a checked record, dirty from T on: the combination must ignore everything but the first T bits
    std::vector<uint32_t> rec(p.cw);
    for (uint32_t& w : rec) w = rnd();
    std::vector<uint8_t> bits(T);
    for (unsigned i = 0; i < T; ++i) bits[i] = (rec[i / 32] >> (i % 32)) & 1u;
    const uint32_t want = crc_bit_serial(q.W, q.poly, q.init, bits.data(), T) ^ q.xorout;
    const uint32_t got = crc_combine(p, rec.data());
    ++checks;
    if (got != want) {
        ++failures;
        std::printf("W=%u poly=%08X init=%08X T=%u: bit-serial %08X, combined %08X\n", q.W, q.poly, q.init, T, want, got);
    }
    // the plan's shape
    unsigned g = 1;
    while (g < p.np && g < 64) g *= 2;
    if (p.group != g || p.rounds != (p.np + g - 1) / g || p.np != (T + 31) / 32 || p.cw != (T + q.W + 31) / 32) {
        ++failures;
        std::printf("W=%u T=%u: plan group=%u rounds=%u np=%u cw=%u\n", q.W, T, p.group, p.rounds, p.np, p.cw);
    }
}

int main() {
    const Params sets[] = {
        {1, 0x1, 0, 0},           {1, 0x1, 1, 1},           {5, 0x05, 0x1F, 0x1F},        {5, 0x15, 0, 0},
        {8, 0x07, 0, 0},          {8, 0x9B, 0xA5, 0x55},    {16, 0x1021, 0, 0},           {16, 0x1021, 0xFFFF, 0xFFFF},
        {24, 0x864CFB, 0, 0},     {24, 0x800063, 0x123456, 0}, {32, 0x04C11DB7, 0, 0},    {32, 0x04C11DB7, 0xFFFFFFFFu, 0xFFFFFFFFu},
    };
    for (const Params& q : sets) {
        for (unsigned T = 1; T <= 200; ++T) check_length(q, T);
        for (unsigned T : {2047u, 2048u, 2049u, 65504u, 65535u})
            if (T + q.W <= CRC_MAX_BITS) check_length(q, T);
        check_length(q, static_cast<unsigned>(CRC_MAX_BITS) - q.W);   // the limit
    }
    // x^n mod P and the word remainder against the register: x^n is the register over a 1 followed by n - W zeros ...
    for (const Params& q : sets) {
        for (unsigned n : {0u, 1u, 31u, 32u, 33u, 100u, 2048u}) {
            uint32_t want;
            if (n < q.W) {
                want = 1u << n;
            } else {
                std::vector<uint8_t> bits(n - q.W + 1, 0);
                bits[0] = 1;
                want = crc_bit_serial(q.W, q.poly, 0, bits.data(), bits.size());
            }
            ++checks;
            if ((crc_xpow(q.W, q.poly, n) >> (32 - q.W)) != want) {
                ++failures;
                std::printf("W=%u poly=%08X: x^%u mod P = %08X, want %08X\n", q.W, q.poly, n, crc_xpow(q.W, q.poly, n) >> (32 - q.W), want);
            }
        }
        // ... and v mod P is the register over the 32 bits of v from the top, followed by nothing: reg(v) = v * x^W mod P, so
        // compare (v mod P) * x^W instead
        for (int k = 0; k < 8; ++k) {
            const uint32_t v = rnd();
            uint8_t bits[32];
            for (int i = 0; i < 32; ++i) bits[i] = (v >> (31 - i)) & 1u;
            const uint32_t want = crc_bit_serial(q.W, q.poly, 0, bits, 32);
            const uint32_t rem = crc_word_rem(q.W, q.poly, v) >> (32 - q.W);
            const uint32_t got = crc_mul(rem, crc_xpow(q.W, q.poly, q.W), q.poly << (32 - q.W)) >> (32 - q.W);
            ++checks;
            if (got != want) {
                ++failures;
                std::printf("W=%u poly=%08X: (%08X mod P) x^W = %08X, want %08X\n", q.W, q.poly, v, got, want);
            }
        }
    }
    std::printf("crc_tables: %d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
