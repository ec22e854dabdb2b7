// test_dot_form.cpp — poulpy_amd/csrc/dot_form.hpp with the host compiler, its own main (driven by tests/test_ckks_dot_host.py): the form of
// the accumulated tensor of pz_glwe_tensor_dot_relinearize_batched at every (npairs, base2k), against the bound worked out here from the
// digit ranges alone, and pinned at the boundaries.
#include <cstdio>
#include <cstdlib>

#include "../../poulpy_amd/csrc/dot_form.hpp"

using namespace pz;

static int fails = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

int main() {
    // one pair's tensor: a diagonal column holds one digit, a pairwise column pair - d_i - d_j; a digit is in [-2^(k-1), 2^(k-1)]
    for (size_t k = 1; k <= 20; ++k) {
        const long long digit = 1ll << (k - 1);
        CHECK(dot_term_bound(k) == 3 * digit);
        for (size_t npairs = 0; npairs <= kDotMaxPairs + 1; ++npairs) {
            const bool fits = npairs >= 1 && npairs <= kDotMaxPairs && k <= 14 && (long long)npairs * 3 * digit <= 32767;
            CHECK(dot_tensor_form(npairs, k, true) == (fits ? DOT_TENSOR_T16 : DOT_TENSOR_I64));
            CHECK(dot_tensor_form(npairs, k, false) == DOT_TENSOR_I64);
        }
    }
    // the boundaries in numbers
    CHECK(dot_tensor_form(5, 12, true) == DOT_TENSOR_T16 && dot_tensor_form(6, 12, true) == DOT_TENSOR_I64);    // 5 x 6144 = 30 720
    CHECK(dot_tensor_form(2, 13, true) == DOT_TENSOR_T16 && dot_tensor_form(3, 13, true) == DOT_TENSOR_I64);    // 2 x 12 288 = 24 576
    CHECK(dot_tensor_form(1, 14, true) == DOT_TENSOR_T16 && dot_tensor_form(2, 14, true) == DOT_TENSOR_I64);    // 1 x 24 576
    CHECK(dot_tensor_form(1, 15, true) == DOT_TENSOR_I64 && dot_tensor_form(1, 17, true) == DOT_TENSOR_I64);    // above 14: never
    CHECK(dot_tensor_form(10, 11, true) == DOT_TENSOR_T16 && dot_tensor_form(11, 11, true) == DOT_TENSOR_I64);  // 10 x 3072 = 30 720
    // what the diagonal columns alone would admit overflows a pairwise column: 15 pairs at base2k 12 reach 15 x 6144 = 92 160
    CHECK(15ll * (1 << 11) <= 32767 && 15ll * dot_term_bound(12) > 32767 && dot_tensor_form(15, 12, true) == DOT_TENSOR_I64);
    // the groups of the summing kernel: pair 0 goes straight into the accumulated tensor
    CHECK(dot_sum_group(1) == 0 && dot_sum_group(2) == 1 && dot_sum_group(5) == 4 && dot_sum_group(6) == 4 && dot_sum_group(64) == kDotSumTerms);
    if (fails) { printf("%d checks failed\n", fails); return 1; }
    printf("all dot-form checks passed\n");
    return 0;
}
