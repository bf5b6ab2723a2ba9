// crc_tables.hpp -- the host arithmetic of the frame check (crc.hip): x^n mod P, the word remainder, the multiply mod P, and
// the per-handle constants the kernels read.  It includes nothing of HIP, so that tests/crc_tables_test.cpp builds it with a
// plain C++ compiler and holds the word-parallel combination to the bit-serial register of include/comms_hip.h.
//
// P(x) = x^W + poly, 1 <= W <= 32.  A residue is kept LEFT-ALIGNED in 32 bits ("L" in a name): the coefficient of x^(W-1) in
// bit 31, the 32 - W low bits zero.  Then a step of the register is the same three operations for every W (crc_mul), W = 32
// needs no 33rd bit, and the bit-reversed residue is the W attached bits in stream order.
//
// The combination.  With b_0 ... b_{T-1} the payload in stream order and M(x) = sum b_i x^(T-1-i), the register of the contract
// ends at  (init * x^T + M(x) * x^W) mod P.  Record word w holds b_{32w} ... b_{32w+31} LSB first, so its bit reversal V_w is
// that slice of M as a polynomial, and  M * x^W = sum_w V_w * x^(W + e_w), where e_w = T - 32 (w + 1) for every word but the
// last.  The last word holds nb = T - 32 (np - 1) bits; its reversal is shifted right by 32 - nb and e = 0.  The multiplier of a
// word depends only on its distance d = np - 1 - w from the last payload word: mult[d].  A frame of more than 64 words is
// walked in chunks of 64 words that END at the last payload word, first chunk first.  The last chunk takes mult[0 ... 63]; every
// earlier one takes mult[64 ... 127], as if it were the last but one, and is carried to its place by acc = acc * x^(32 * 64) +
// chunk: the last word's exponent is short of a multiple of 32, and x has no inverse mod P in general, so the last chunk cannot
// be part of the same recurrence.  The word behind the payload, where a checked record has one, holds attached bits only and
// takes no part in this.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define CRC_HD __host__ __device__ __forceinline__
#else
#define CRC_HD inline
#endif

namespace comms {

constexpr unsigned CRC_MAX_GROUP = 64;           // lanes that serve one frame at most: a wave
constexpr size_t CRC_MAX_BITS = size_t(1) << 16; // T + W at most: a checked record is a valid comms_viterbi output

// (v * m) mod P: v any polynomial of degree <= 31 (bit k = coefficient of x^k), m and the result left-aligned residues.
// Horner over the bits of v from the top: one shift-and-reduce and one conditional add of m per bit.
CRC_HD uint32_t crc_mul(uint32_t v, uint32_t mL, uint32_t polyL) {
    uint32_t acc = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < 32; ++k) {
        acc = (acc << 1) ^ (polyL & (0u - (acc >> 31)));
        acc ^= mL & (0u - (v >> 31));
        v <<= 1;
    }
    return acc;
}

// bit reversal of a 32-bit word (the device has an instruction for it)
inline uint32_t crc_brev(uint32_t v) {
    v = (v >> 16) | (v << 16);
    v = ((v & 0xFF00FF00u) >> 8) | ((v & 0x00FF00FFu) << 8);
    v = ((v & 0xF0F0F0F0u) >> 4) | ((v & 0x0F0F0F0Fu) << 4);
    v = ((v & 0xCCCCCCCCu) >> 2) | ((v & 0x33333333u) << 2);
    v = ((v & 0xAAAAAAAAu) >> 1) | ((v & 0x55555555u) << 1);
    return v;
}

// the word remainder: v mod P, left-aligned (1 mod P = 1, for every W >= 1)
inline uint32_t crc_word_rem(unsigned W, uint32_t poly, uint32_t v) { return crc_mul(v, 1u << (32 - W), poly << (32 - W)); }

// x^n mod P, left-aligned, by square and multiply
inline uint32_t crc_xpow(unsigned W, uint32_t poly, uint64_t n) {
    const unsigned sh = 32 - W;
    const uint32_t polyL = poly << sh;
    uint32_t result = 1u << sh;                              // x^0
    uint32_t sq = W == 1 ? polyL : 2u << sh;                 // x^1 (x mod (x + poly) = poly where W = 1)
    for (; n; n >>= 1) {
        if (n & 1) result = crc_mul(result >> sh, sq, polyL);
        sq = crc_mul(sq >> sh, sq, polyL);
    }
    return result;
}

// the bit-serial register of the contract over `bits` (one bit per byte), from `init`: the definition, right-aligned
inline uint32_t crc_bit_serial(unsigned W, uint32_t poly, uint32_t init, const uint8_t* bits, size_t n) {
    const uint32_t mask = W == 32 ? 0xFFFFFFFFu : (1u << W) - 1u;
    uint32_t reg = init;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t top = ((reg >> (W - 1)) & 1u) ^ (bits[i] & 1u);
        reg = (reg << 1) & mask;
        if (top) reg ^= poly;
    }
    return reg;
}

// What a handle fixes at create.  Words are the 32-bit words of a record.
struct CrcPlan {
    unsigned W = 0, T = 0;
    unsigned np = 0;          // words of a payload record, ceil(T / 32)
    unsigned cw = 0;          // words of a checked record, ceil((T + W) / 32): np or np + 1
    unsigned group = 1;       // lanes per frame: the smallest power of two >= np, at most 64
    unsigned rounds = 1;      // chunks of `group` words a frame is walked in (more than one only at group = 64)
    unsigned s = 0;           // T mod 32: the attached bits start at bit s of word T / 32
    unsigned tail_shift = 0;  // 32 - (payload bits of the last payload word)
    unsigned sh = 0;          // 32 - W
    uint32_t polyL = 0, strideL = 0, finalL = 0;   // P, x^(32 * 64) mod P, (init * x^T mod P) ^ xorout
    uint32_t mask = 0;        // the low W bits
    // mult[d]: the multiplier of the word at distance d = 0 ... 127 from the last payload word.  Lane j of a group reads
    // mult[group - 1 - j] for the last chunk and mult[64 + 63 - j] for the earlier ones.
    uint32_t mult[2 * CRC_MAX_GROUP] = {0};
};

inline CrcPlan crc_plan(unsigned W, uint32_t poly, uint32_t init, uint32_t xorout, unsigned T) {
    CrcPlan p;
    p.W = W;
    p.T = T;
    p.np = (T + 31) / 32;
    p.cw = (T + W + 31) / 32;
    while (p.group < p.np && p.group < CRC_MAX_GROUP) p.group *= 2;
    p.rounds = (p.np + p.group - 1) / p.group;
    p.s = T % 32;
    const unsigned nb = T - 32 * (p.np - 1);   // 1 ... 32
    p.tail_shift = 32 - nb;
    p.sh = 32 - W;
    p.polyL = poly << p.sh;
    p.mask = W == 32 ? 0xFFFFFFFFu : (1u << W) - 1u;
    p.strideL = crc_xpow(W, poly, 32 * CRC_MAX_GROUP);
    p.finalL = crc_mul(init, crc_xpow(W, poly, T), p.polyL) ^ (xorout << p.sh);
    p.mult[0] = crc_xpow(W, poly, W);
    for (unsigned d = 1; d < 2 * CRC_MAX_GROUP; ++d) p.mult[d] = crc_xpow(W, poly, W + 32ull * (d - 1) + nb);
    return p;
}

// the payload bits of record word w: everything below T
inline uint32_t crc_payload_mask(const CrcPlan& p, long w) {
    const long nbits = static_cast<long>(p.T) - 32 * w;
    return nbits >= 32 ? 0xFFFFFFFFu : nbits <= 0 ? 0u : (1u << nbits) - 1u;
}

// crc of a record (its first T bits) the way crc.hip's kernels form it: lane by lane, chunk by chunk
inline uint32_t crc_combine(const CrcPlan& p, const uint32_t* rec) {
    uint32_t acc = 0;
    for (unsigned c = p.rounds; c-- > 0;) {
        uint32_t chunk = 0;
        for (unsigned j = 0; j < p.group; ++j) {
            const long w = static_cast<long>(p.np) - static_cast<long>(p.group) * (c + 1) + j;
            const uint32_t word = w >= 0 ? rec[w] : 0u;
            uint32_t v = crc_brev(word & crc_payload_mask(p, w));
            if (w == static_cast<long>(p.np) - 1) v >>= p.tail_shift;
            chunk ^= crc_mul(v, p.mult[(c ? CRC_MAX_GROUP : 0) + p.group - 1 - j], p.polyL);
        }
        acc = (c && c + 1 < p.rounds ? crc_mul(acc >> p.sh, p.strideL, p.polyL) : acc) ^ chunk;
    }
    return (acc ^ p.finalL) >> p.sh;
}

}  // namespace comms
