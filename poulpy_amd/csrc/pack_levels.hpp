// pack_levels.hpp — the level map of FheUint::pack (pz_fhe_uint_pack_batched): which two slots of the dense bit buffer
// every merge of glwe_pack takes when all word_bits indices bit_index(s) << log_gap are occupied.  Plain C++, no HIP: pack_levels.cpp links
// into host-only programs (tests/cpp/test_pack_levels.cpp), and every slot a kernel argument will ever hold is checked here, on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace pz {

constexpr size_t kPackMaxPairs = 64;   // word_bits <= 128

// bdd_arithmetic/mod.rs:97-99: bit i of the integer lies at index ((i & 7) << LOG_BYTES) | (i >> 3) of the word, LOG_BYTES = log2(word_bits / 8)
inline uint32_t fhe_uint_bit_index(uint32_t i, uint32_t log_bytes) { return ((i & 7u) << log_bytes) | (i >> 3); }
// its inverse: the bit (= the slot of the dense buffer) that lies at index q
inline uint32_t fhe_uint_slot_of_index(uint32_t q, uint32_t log_bytes) { return ((q & ((1u << log_bytes) - 1u)) << 3) | (q >> log_bytes); }

// One level of glwe_pack_default's loop (glwe_packing.rs:147-168) restricted to the occupied indices: pair k merges the ciphertext at index
// q = k (slot lo[k], the survivor) with the one at index q + pairs (slot hi[k]); t = n >> (level + 1) = pairs << log_gap.
struct PackLevel {
    uint32_t t = 0;
    std::vector<uint8_t> lo, hi;
    size_t pairs() const { return lo.size(); }
};

// word_bits one of 8 / 16 / 32 / 64 / 128, n a power of two and a multiple of it: the log2(word_bits) levels; false + *err otherwise
bool fhe_uint_pack_levels(size_t n, size_t word_bits, std::vector<PackLevel>* out, std::string* err);
// Re-checks what the kernels rely on, from the tables alone: every slot below word_bits; inside a level no slot named twice (the survivors'
// slots, which the post-kernel writes, are disjoint from the slots it reads); a level reads only survivors of the level before; the last
// survivor is slot 0; t halves from n / 2.  false + *err on a violation.
bool fhe_uint_pack_check(size_t n, size_t word_bits, const std::vector<PackLevel>& levels, std::string* err);

}  // namespace pz
