// dot_form.hpp — which form the accumulated GLWETensor of pz_glwe_tensor_dot_relinearize_batched takes in the workspace, and how many 16-bit
// term tensors one summing launch takes.  Plain C++ with no HIP header: api_cnv.hip calls these, tests/cpp/test_dot_form.cpp compiles them
// with the host compiler.
#pragma once
#include <cstddef>

namespace pz {

constexpr size_t kDotMaxPairs = 64;   // pairs of one call (as the terms of one pz_glwe_sum_batched)

enum DotTensorForm : int { DOT_TENSOR_I64 = 0, DOT_TENSOR_T16 = 1 };

// The largest |value| a limb of ONE pair's GLWETensor takes at one base2k = k.  The tensoring tails end in the normalizing carry step
// (znx_digit: digit(x) = ((x + 2^(k-1)) mod 2^k) - 2^(k-1), in [-2^(k-1), 2^(k-1)); the reference's other rounding convention gives
// (-2^(k-1), 2^(k-1)]): |digit| <= 2^(k-1) either way.  A diagonal column (i, i) holds such digits.  A pairwise column (i, j) holds
// pair - d_i - d_j (glwe_tensor_apply, poulpy-core operations/glwe.rs:762-805: the pairwise product's digits minus the two diagonal columns'
// digits, element-wise, NOT normalized again) - three digits: |value| <= 3 * 2^(k-1).  Every GLWETensor has a pairwise column (rank >= 1).
constexpr long long dot_term_bound(size_t base2k) { return 3ll << (base2k - 1); }

// glwe_tensor_apply_add_assign adds a pair's values to the running columns element-wise (:870-890), so after npairs pairs a limb holds at
// most npairs * dot_term_bound.  The 16-bit form keeps that sum in an int16 and the relinearization sign-extends it: it applies where the one-call
// product is compact (mul_relin_plan: pipeline plans, one base2k <= 14, glwe_relin_t16) AND npairs * 3 * 2^(base2k-1) <= 2^15 - 1:
//   base2k 12: 5 pairs (30 720)    13: 2 pairs (24 576)    14: 1 pair (24 576; one pair is the existing one-call product)    <= 11: 10 and more
// (The diagonal columns alone would admit npairs * 2^(base2k-1) <= 2^15 - 1 - 15 pairs at base2k 12 - but the pairwise columns overflow there.)
// Beyond the bound: the i64 tensor.
inline DotTensorForm dot_tensor_form(size_t npairs, size_t base2k, bool compact_supported) {
    if (!compact_supported || npairs == 0 || npairs > kDotMaxPairs || base2k < 1 || base2k > 14) return DOT_TENSOR_I64;
    return (long long)npairs * dot_term_bound(base2k) <= 32767 ? DOT_TENSOR_T16 : DOT_TENSOR_I64;
}

// 16-bit form: pair 0 is tensored straight into the accumulated tensor; every later pair into a term tensor of its own (the pairwise tails read
// the SAME pair's diagonal digits from the tensor's diagonal columns, so a pair cannot be tensored into the running sum), and one launch of
// k_t16_sum adds a group of term tensors to the accumulated one.  Per element and pair the tails write 2 B and the sum reads 2 B; a group of
// g terms also reads and rewrites the accumulated tensor, 4 B / g.  g = 4 leaves 5 B per element and pair against 8 B at g = 1 and 4.5 B
// at g = 8, for four term tensors of workspace instead of eight - and the bound above admits at most 4 later pairs at base2k 12, so one
// launch sums all of them there.
constexpr int kDotSumTerms = 4;
inline int dot_sum_group(size_t npairs) { return npairs <= 1 ? 0 : (int)(npairs - 1 < (size_t)kDotSumTerms ? npairs - 1 : (size_t)kDotSumTerms); }

}  // namespace pz
