// device_sum.hpp — k_glwe_sum: the normalized signed sum of up to 64 GLWE batches in one pass over HBM (pz_glwe_sum_batched): poulpy-ckks's
// ckks_add_many (leveled/delegates/composite.rs:63-93) and the join of every dot product (accumulate_unnormalized, :478-506).
//
// The reference joins term after term into dst by one of the three branches of ckks_add_assign_unsafe / ckks_sub_assign_unsafe
// (leveled/default/add.rs:122-146) and closes with glwe_normalize_assign.  Every step of that chain keeps the value of the container,
// sum_j limb_j 2^((res_size-1-j) base2k), exact modulo 2^(res_size base2k) - vec_znx_lsh's middle step splits x << k_rem into a digit and
// a carry that add up to it, its final step and glwe_lsh_assign drop only multiples of the modulus - and the closing normalize writes
// the canonical digits of that value.  The one step that is not value-exact is the carry-only prologue of vec_znx_lsh over the operand
// limbs below the window (shift.rs:105-111: the first step drops its digit), so the result is the canonical digit string of
//
//   sum_t sign_t 2^(T_t) ( sum_{j < min_size} (a[j + steps] << k_rem) 2^((res_size-1-j) base2k) + c_t 2^((res_size-min_size) base2k) )
//
// with steps / k_rem / min_size of shift.rs:90-104 (a plain join: 0 / 0 / min(res_size, a_size), no prologue), c_t the prologue's carry
// computed by the reference's own steps (znx_steps.hpp), and T_t the bits by which later PZ_JOIN_LSH_ACC joins shift the running sum.  sum_plan folds
// T_t into the term on the host: output limb j reads operand limb j + off, shifted left by sh < base2k bits, while that limb lies in the
// term's window [lo, hi); the prologue's carry enters output limb cj shifted by csh.
//
// One thread owns two neighbouring coefficients of one column of one ciphertext (16-byte loads and stores) and walks the output limbs
// from res_size - 1 to 0: it adds every term's shifted limb into one 128-bit accumulator per coefficient, runs a term's prologue when
// the walk reaches the limb its carry enters (every operand limb is read once), takes the limb's digit, keeps the rest as the carry and
// stores the limb once.  |x << sh| < 2^(62 + base2k) and nterms <= 2^(63 - base2k) (ensure_accumulation_fits): the sum stays below
// 2^126.  No accumulator in LDS, no per-term state in registers.  Term 0 may be res itself; where a shift makes it read a limb above the
// one being stored, its limbs are staged once in the thread's LDS slice, as k_glwe_combine stages an in-place LSH operand.
//
// sum_plan and sum_walk are __host__ __device__: tests/cpp/test_sum_walk.cpp runs them on the host against the oracle chain's digits.
#pragma once
#include <hip/hip_runtime.h>

#include "znx_steps.hpp"

namespace pz {

constexpr int kSumMaxTerms = 64;
constexpr int kSumBlock = 128;
constexpr int kSumMaxStage = 32;   // limbs of an in-place, shifted term 0 staged in LDS: 32 x 16 B x 128 threads = 64 KiB
enum { SUM_JOIN_PLAIN = 0, SUM_JOIN_LSH_TERM = 1, SUM_JOIN_LSH_ACC = 2 };
enum { SUM_F_NEG = 1, SUM_F_SHARED = 2, SUM_F_STAGE = 4 };

// one term as the entry point describes it
struct SumSpec {
    const long long* a;     // column 0 of ciphertext 0
    int shared, a_size, join, neg;
    int inplace;            // the operand is res itself (term 0 only)
    unsigned long long k;   // the join's shift in bits
};
// one term as the kernel reads it from its arguments (48 bytes; 64 of them and the header stay below the 4 KiB of kernel arguments)
struct SumTerm {
    const long long* a;
    int size, flags;        // a_size; SUM_F_*
    int off, sh;            // output limb j reads operand limb j + off, shifted left by sh bits
    int lo, hi;             // the window: operand limbs [lo, hi) take part
    int k_rem;              // the prologue's digit split (shift.rs:90); it runs over operand limbs [hi, size)
    int cj, csh;            // the prologue's carry enters output limb cj shifted left by csh bits; cj < 0: no prologue
    int pad;
};
struct SumArgs {
    long long* res;
    int n, batch, cols, res_size, k, nterms;
    int stage;              // limbs of term 0 (res itself) staged in LDS, 0: none
    int pad;
    SumTerm t[kSumMaxTerms];
};

// The chain's terms folded for the walk (see the head of the file).  Terms that add nothing - the early return of shift.rs:92-100, an empty
// window, or a running sum shifted out of the container - are dropped.  Returns the number of terms kept; g.t[] holds them in reverse order.
__host__ __device__ inline int sum_plan(SumArgs& g, const SumSpec* s, int nterms, int res_size, int base2k) {
    unsigned long long T = 0;   // bits by which the joins after term u shift the running sum
    const unsigned long long b = (unsigned long long)base2k;
    int kept = 0;
    g.stage = 0;
    for (int u = nterms - 1; u >= 0; --u) {
        const SumSpec& in = s[u];
        unsigned long long steps = 0;
        int k_rem = 0, min_size = in.a_size < res_size ? in.a_size : res_size;
        bool dead = false;
        if (in.join == SUM_JOIN_LSH_TERM) {
            steps = in.k / b;
            k_rem = (int)(in.k % b);
            if (steps >= (unsigned long long)(res_size > in.a_size ? res_size : in.a_size)) dead = true;   // shift.rs:92-100
            else {
                const int left = in.a_size - (int)steps;   // shift.rs:102
                min_size = left < 0 ? 0 : (left < res_size ? left : res_size);
                dead = min_size == 0;
            }
        }
        const unsigned long long t_steps = T / b;
        const int t_rem = (int)(T % b);
        if (!dead && t_steps < (unsigned long long)res_size) {
            SumTerm& t = g.t[kept++];
            t = SumTerm{};
            t.a = in.a;
            t.size = in.a_size;
            t.flags = (in.neg ? SUM_F_NEG : 0) | (in.shared ? SUM_F_SHARED : 0);
            int sh = k_rem + t_rem, extra = 0;
            if (sh >= base2k) { sh -= base2k; extra = 1; }   // (x << (base2k + s)) at limb j is (x << s) at limb j - 1
            t.off = (int)steps + (int)t_steps + extra;
            t.sh = sh;
            t.lo = (int)steps;
            t.hi = (int)steps + min_size;
            t.k_rem = k_rem;
            // only vec_znx_lsh looks below its window; a plain join ignores the limbs past res_size
            t.cj = in.join == SUM_JOIN_LSH_TERM && t.hi < in.a_size ? min_size - 1 - (int)t_steps : -1;
            t.csh = t_rem;
            // res as an operand: limb j is read before it is stored unless a shift makes the walk read a limb above it
            if (in.inplace && t.off != 0) { t.flags |= SUM_F_STAGE; g.stage = in.a_size; }
        }
        if (in.join == SUM_JOIN_LSH_ACC) T += in.k;
    }
    g.nterms = kept;
    return kept;
}

// ---- the 128-bit accumulator: two u64, wrapping ----
struct Acc128 { unsigned long long lo, hi; };

__host__ __device__ __forceinline__ void acc_add_shl(Acc128& a, unsigned long long x, int sh, bool neg) {
    const unsigned long long lo = x << sh;
    const unsigned long long hi = (unsigned long long)(((long long)x >> 1) >> (63 - sh));   // sh in [0, 63)
    if (neg) {
        const unsigned long long br = a.lo < lo ? 1ull : 0ull;
        a.lo -= lo;
        a.hi -= hi + br;
    } else {
        a.lo += lo;
        a.hi += hi + (a.lo < lo ? 1ull : 0ull);
    }
}
// the accumulator's digit in base 2^k (znx get_digit, normalization.rs:4-7); the accumulator keeps the carry (:9-12)
__host__ __device__ __forceinline__ unsigned long long acc_take_digit(Acc128& a, int k) {
    const unsigned long long d = (unsigned long long)((long long)(a.lo << (64 - k)) >> (64 - k));
    const unsigned long long dh = (unsigned long long)((long long)d >> 63);
    const unsigned long long br = a.lo < d ? 1ull : 0ull;
    const unsigned long long lo = a.lo - d, hi = a.hi - dh - br;
    a.lo = (lo >> k) | (hi << (64 - k));
    a.hi = (unsigned long long)((long long)hi >> k);
    return d;
}

// Coefficients x, x + 1 of column c of ciphertext bt.  `stage`: this thread's slice for term 0 when g.stage (limb l at stage[l * ss]).
__host__ __device__ inline void sum_walk(const SumArgs& g, long long bt, int c, int x, ulonglong2* stage, int ss) {
    const int k = g.k, rs = g.res_size;
    const long long ls = (long long)g.cols * g.n;   // scalars between limbs, the same for every container of the call
    const long long at = (long long)c * g.n + x;
    unsigned long long* r = (unsigned long long*)g.res + bt * ls * rs + at;
    if (g.stage)   // every read of res precedes the first store
        for (int l = 0; l < g.stage; ++l) stage[l * ss] = *reinterpret_cast<const ulonglong2*>(r + (long long)l * ls);
    Acc128 a0 = {0, 0}, a1 = {0, 0};
    for (int j = rs - 1; j >= 0; --j) {
        for (int u = 0; u < g.nterms; ++u) {
            const SumTerm& t = g.t[u];
            const bool neg = (t.flags & SUM_F_NEG) != 0, staged = (t.flags & SUM_F_STAGE) != 0;
            const unsigned long long* a =
                (const unsigned long long*)t.a + ((t.flags & SUM_F_SHARED) ? 0 : bt * ls * t.size) + at;
            if (j == t.cj) {
                long long c0 = 0, c1 = 0;   // the carry of the operand limbs below the window
                for (int l = t.size - 1; l >= t.hi; --l) {
                    const ulonglong2 v = staged ? stage[l * ss] : *reinterpret_cast<const ulonglong2*>(a + (long long)l * ls);
                    if (l == t.size - 1) {
                        c0 = znx_first_step_carry_only(k, t.k_rem, (long long)v.x);
                        c1 = znx_first_step_carry_only(k, t.k_rem, (long long)v.y);
                    } else {
                        znx_middle_step_carry_only(k, t.k_rem, (long long)v.x, c0);
                        znx_middle_step_carry_only(k, t.k_rem, (long long)v.y, c1);
                    }
                }
                acc_add_shl(a0, (unsigned long long)c0, t.csh, neg);
                acc_add_shl(a1, (unsigned long long)c1, t.csh, neg);
            }
            const int l = j + t.off;
            if (l >= t.lo && l < t.hi) {
                const ulonglong2 v = staged ? stage[l * ss] : *reinterpret_cast<const ulonglong2*>(a + (long long)l * ls);
                acc_add_shl(a0, v.x, t.sh, neg);
                acc_add_shl(a1, v.y, t.sh, neg);
            }
        }
        // vec_znx_normalize_assign (normalize.rs:403-425): the digit of limb j, the rest carries into limb j - 1; the carry out of limb 0
        // is dropped as by the final step
        ulonglong2 o;
        o.x = acc_take_digit(a0, k);
        o.y = acc_take_digit(a1, k);
        *reinterpret_cast<ulonglong2*>(r + (long long)j * ls) = o;
    }
}

// grid: ceil(batch * cols * n / 2 / kSumBlock) workgroups; dynamic LDS: g.stage x kSumBlock x 16 B
__global__ void __launch_bounds__(kSumBlock) k_glwe_sum(SumArgs g) {
    extern __shared__ ulonglong2 sum_lds[];
    const int hn = g.n >> 1;
    const long long tid = (long long)blockIdx.x * kSumBlock + threadIdx.x;
    if (tid >= (long long)g.batch * g.cols * hn) return;
    const int x = 2 * (int)(tid % hn);
    const long long q = tid / hn;
    sum_walk(g, q / g.cols, (int)(q % g.cols), x, sum_lds + threadIdx.x, kSumBlock);
}

}  // namespace pz
