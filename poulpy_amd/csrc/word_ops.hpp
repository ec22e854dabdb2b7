// word_ops.hpp — the stage plan of the FheUint byte operations (pz_fhe_uint_get_batched / _zero_byte_ / _splice_ / _sext_):
// get_bit_glwe, get_byte, zero_byte, splice_u8, splice_u16 and sext of bdd_arithmetic/ciphertexts/fhe_uint.rs:259-524 regrouped around their
// partial traces.  Rotations are signed permutations and everything around the traces is wrapping arithmetic, so, bit for bit on every limb,
//   zero_byte:  res = a - X^r T_a                T_a = trace_ts(X^-r a)
//   splice_u8:  res = a + X^rd (T_b - T_a)       T_a = trace_ts(X^-rd a), T_b = trace_ts(X^-rs b)
//   replicate:  s'  = sum_{m < 8} X^(m n / 8) s
// and the traces of one stage are independent and share their keys: a stage is ONE trace call on items * batch ciphertexts.
// Plain C++, no HIP: word_ops.cpp links into host-only programs (tests/cpp/test_word_ops.cpp), and every exponent and slot a kernel argument
// will ever hold is checked here, on the CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace pz {

constexpr size_t kWordMaxItems = 128;   // a get of every bit of a u128
constexpr size_t kWordSlots = 6;        // ciphertext arrays [batch] of tmp that the operations other than get use (either route)
constexpr uint32_t kWordNone = 0xFFFFFFFFu;

enum WordOp : uint32_t { WORD_GET_BIT = 0, WORD_GET_BYTE = 1, WORD_ZERO_BYTE = 2, WORD_SPLICE_U8 = 3, WORD_SPLICE_U16 = 4, WORD_SEXT = 5 };
// where a traced item (or the closing step's first operand) is read: the call's a, its b, the running word (res; sext: the word), s' (slot 1)
enum WordSrc : uint32_t { WORD_SRC_A = 0, WORD_SRC_B = 1, WORD_SRC_RES = 2, WORD_SRC_S = 3 };
// what follows the stage's trace: nothing (a get: the traced items are the result), res = base + X^r (T[plus] - T[minus]), or the eight-term
// sum of sext from slot 0 into slot 1
enum WordClose : uint32_t { WORD_CLOSE_NONE = 0, WORD_CLOSE_COMBINE = 1, WORD_CLOSE_REPLICATE = 2 };

struct WordItem {
    uint32_t src;    // WordSrc
    uint32_t exp;    // the item is X^-exp src, exp < n
    uint32_t slot;   // where it is traced: ciphertext array `slot` of the stage's dense array (a get: of res; else of tmp)
};
struct WordStage {
    uint32_t skip = 0;                 // glwe_trace_assign(.., skip): steps skip .. log2(n)
    std::vector<WordItem> items;       // at consecutive slots
    uint32_t close = WORD_CLOSE_NONE;
    uint32_t base = WORD_SRC_A;        // COMBINE: res[j] = base[j] + (X^r (T[plus] - T[minus]))[j]; a missing T is zero
    uint32_t plus = kWordNone, minus = kWordNone;
    uint32_t r = 0;
};

// bdd_arithmetic/mod.rs:97-99 and fhe_uint.rs:384: the coefficient of bit `bit` of a word of word_bits bits in a ring of degree n
inline uint32_t fhe_uint_word_coefficient(size_t n, size_t word_bits, uint32_t bit) {
    uint32_t log_bytes = 0;
    while (((size_t)8 << log_bytes) < word_bits) ++log_bytes;
    return (uint32_t)((size_t)(((bit & 7u) << log_bytes) | (bit >> 3)) * (n / word_bits));
}

// The stages of `op` on words of word_bits bits (8 / 16 / 32 / 64 / 128) in a ring of degree n (a power of two that word_bits divides).
//   args: get: the nargs <= 128 bit / byte indices; zero_byte: {byte}; splice: {dst, src}; sext: {byte}
// sext of the last byte is the empty plan.  false + *err for anything out of range.
bool fhe_uint_word_plan(size_t n, size_t word_bits, uint32_t op, const uint32_t* args, size_t nargs, std::vector<WordStage>* out, std::string* err);
// Re-checks what the kernels rely on, from the plan alone: every exponent below n, the items of a stage at consecutive slots below `slots`,
// every T a closing step names written by this or an earlier stage and not overwritten since, s' read only after a replicate.
bool fhe_uint_word_plan_check(size_t n, size_t slots, const std::vector<WordStage>& plan, std::string* err);
// the plan as plain words: per stage  skip, nitems, nitems x (src, exp, slot), close, base, plus, minus, r
std::vector<uint32_t> fhe_uint_word_plan_words(const std::vector<WordStage>& plan);

}  // namespace pz
