// znx_steps.hpp — the base-2^k carry steps of poulpy-cpu-ref (reference/znx/normalization.rs) and the same-base normalization of
// reference/vec_znx/normalize.rs, restated once for every integer kernel and for the host.  One function per reference function, on one
// coefficient: the reference's slices become the caller's loop.  Arithmetic is wrapping i64 through unsigned casts, bit for bit the
// reference's (whose + on i64 wraps in release builds).  tests/cpp/test_znx_steps.cpp runs the plan and the walk on the host against the
// oracle; test_lincomb_walk.cpp and test_sum_walk.cpp run the shifted steps.
//
// A step with lsh != 0 takes the low k - lsh bits of the limb as its digit and places them lsh bits up; the reference's
// `base2k_lsh = base2k - lsh` under `lsh != 0` and `base2k` otherwise are the same number, k - lsh, and it is derived here and nowhere else.
// The _assign forms (the limb is read and written in place) and the <OVERWRITE> / _sub forms (the digit is stored, added or subtracted)
// differ only in what the caller does with the returned digit.
#pragma once
#include <hip/hip_runtime.h>

namespace pz {

__host__ __device__ __forceinline__ long long wadd(long long a, long long b) { return (long long)((unsigned long long)a + (unsigned long long)b); }
__host__ __device__ __forceinline__ long long wsub(long long a, long long b) { return (long long)((unsigned long long)a - (unsigned long long)b); }
__host__ __device__ __forceinline__ long long wshl(long long a, int s) { return (long long)((unsigned long long)a << s); }

// get_digit_i64 / get_carry_i64 (normalization.rs:3-11)
__host__ __device__ __forceinline__ long long znx_digit(int k, long long x) { return (long long)((unsigned long long)x << (64 - k)) >> (64 - k); }
__host__ __device__ __forceinline__ long long znx_carry(int k, long long x, long long d) { return wsub(x, d) >> k; }

// znx_normalize_first_step_carry_only (normalization.rs:23-41)
__host__ __device__ __forceinline__ long long znx_first_step_carry_only(int k, int lsh, long long x) {
    return znx_carry(k - lsh, x, znx_digit(k - lsh, x));
}
// znx_normalize_middle_step<OVERWRITE>, _sub and _assign (normalization.rs:131-157, :178-251): the limb's digit; carry <- the carry out
__host__ __device__ __forceinline__ long long znx_middle_step(int k, int lsh, long long x, long long& carry) {
    const long long d = znx_digit(k - lsh, x);
    const long long cr = znx_carry(k - lsh, x, d);
    const long long dpc = wadd(wshl(d, lsh), carry);
    const long long x1 = znx_digit(k, dpc);
    carry = wadd(cr, znx_carry(k, dpc, x1));
    return x1;
}
// znx_normalize_middle_step_carry_only (normalization.rs:106-129): the middle step without its digit
__host__ __device__ __forceinline__ void znx_middle_step_carry_only(int k, int lsh, long long x, long long& carry) {
    (void)znx_middle_step(k, lsh, x, carry);
}
// znx_normalize_final_step<OVERWRITE>, _sub and _assign (normalization.rs:253-323): the carry out is dropped
__host__ __device__ __forceinline__ long long znx_final_step(int k, int lsh, long long x, long long carry) {
    return znx_digit(k, wadd(wshl(znx_digit(k - lsh, x), lsh), carry));
}

// The plan of vec_znx_normalize_inter_base2k (normalize.rs:83-99): res takes a, moved up by res_offset bits, both in base 2^base2k.
struct ZnxInterPlan {
    int lsh;                  // bits by which every digit is shifted inside its limb
    int res_end, res_start;   // res limbs [0, res_end) take only the carry, [res_end, res_start) a limb of a, [res_start, res_size) zero
    int a_end, a_start;       // a limbs [a_end, a_start) are stored, [a_start, a_size) only feed the carry
};
__host__ __device__ __forceinline__ ZnxInterPlan znx_inter_plan(int res_size, int a_size, int base2k, long long res_offset) {
    const long long k = base2k;
    long long lsh = res_offset % k, lo = res_offset / k;
    if (res_offset < 0 && lsh != 0) { lsh = (lsh + k) % k; lo -= 1; }
    auto clamp = [](long long v, long long hi) { return (int)(v < 0 ? 0 : (v > hi ? hi : v)); };
    return ZnxInterPlan{(int)lsh, clamp(-lo, res_size), clamp((long long)a_size - lo, res_size), clamp(lo, a_size), clamp((long long)res_size + lo, a_size)};
}

// The walk of vec_znx_normalize_inter_base2k on one coefficient (normalize.rs:101-143): load(l) is limb l of a, store(j, v) takes digit v
// of res limb j; every limb of res is stored once, every limb of a from a_end on is loaded once, from the last to the first.
template <class Load, class Store>
__host__ __device__ __forceinline__ void znx_normalize_inter_walk(const ZnxInterPlan& p, int k, int res_size, int a_size, Load load, Store store) {
    long long c = 0;
    for (int j = 0; j < a_size - p.a_start; ++j) {   // the limbs of a below res: their carry only
        const long long x = load(a_size - j - 1);
        if (j == 0) c = znx_first_step_carry_only(k, p.lsh, x);
        else znx_middle_step_carry_only(k, p.lsh, x, c);
    }
    for (int j = p.res_start; j < res_size; ++j) store(j, 0);
    for (int j = 0; j < p.a_start - p.a_end; ++j) store(p.res_start - j - 1, znx_middle_step(k, p.lsh, load(p.a_start - j - 1), c));
    for (int j = 0; j < p.res_end; ++j)              // the limbs of res above a: zeroed, then the _assign steps spread the carry
        store(p.res_end - j - 1, j == p.res_end - 1 ? znx_final_step(k, p.lsh, 0, c) : znx_middle_step(k, p.lsh, 0, c));
}

}  // namespace pz
