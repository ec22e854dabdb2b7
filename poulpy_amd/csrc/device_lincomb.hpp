// device_lincomb.hpp — k_lincomb_const: res = [res] +- sum_t c_t * a_t on GLWE batches, one pass over HBM (poulpy-ckks
// leveled/delegates/composite.rs: ckks_mul_add_pt_const_* :290-330, ckks_mul_sub_pt_const_* :423-463, ckks_dot_product_pt_const_znx :760-784).
//
// The reference forms every term's product into a scratch ciphertext (ckks_mul_pt_const_znx_into, leveled/default/mul.rs:342-374: the four
// arms of the complex constant), joins it to dst by one of the three branches of ckks_add_assign_unsafe / ckks_sub_assign_unsafe
// (leveled/default/add.rs:122-146, sub.rs:122-146) and closes with glwe_normalize_assign.  All of it is local to one coefficient (to the
// pair (x, x + N/2) once a term has an imaginary part: X^{N/2} maps x -> x + N/2 and x + N/2 -> -(x)), so one thread walks every column
// with the accumulator, the product and the term's operand limbs in its own LDS slice and stores each limb of res once.
//
// The product digits are mc_walk's (device_plain.hpp, what k_mul_const_nz stores).  A join that shifts nothing adds them straight into the
// accumulator (wrapping i64 sums commute); glwe_lsh_add / glwe_lsh_sub walk the product from the bottom limb up with the carry in a register
// (shift.rs:68-180 with equal sizes: no carry-only range; the steps are znx_steps.hpp's); glwe_lsh_assign on the running, un-normalized
// accumulator reads limb j + steps for limb j, so its result goes to the product's buffer and the two buffers trade places.
//
// lc_walk is __host__ __device__: tests/cpp/test_lincomb_walk.cpp runs it on the host against the oracle's digits.
#pragma once
#include "device_plain.hpp"

namespace pz {

constexpr int kLinMaxTerms = 64;   // entries of the module's device term table
enum { LC_JOIN_PLAIN = 0, LC_JOIN_LSH_TMP = 1, LC_JOIN_LSH_ACC = 2 };
enum { LC_RE = 0, LC_IM = 1, LC_BOTH = 2, LC_ZERO = 3 };   // LinTerm::mc.form: 0 - 2 as k_mul_const_nz, 3: neither re nor im

// one term as the kernel reads it from the device table
struct LinTerm {
    MulConstArgs mc;            // a, a_bs (0: one operand for the batch), a_size, res_size, k, lsh, form and the arms' plans; res / n / batch / cols unused
    int join, neg;              // LC_JOIN_*; neg: the product is subtracted
    int steps, k_rem, min_size; // the shift of the join: k / base2k, k % base2k, output limbs [0, min_size) (shift.rs:90, :102)
    int pad;
};
struct LinArgs {
    long long* res;
    long long res_bs;           // scalars between ciphertexts
    const LinTerm* terms;
    int n, batch, cols, res_size, k, nterms;
    int init_res;               // 1: the accumulator starts as res (mul_add / mul_sub); 0: the first product overwrites it (dot product)
    int normalize;
    int pair;                   // 1: one thread per (x, x + N/2)
    int a_max;                  // operand limbs staged per coefficient: the largest a_size of the call
    int has_tmp;                // 1: some join shifts, so the product needs a buffer of its own; 0: every product goes straight into the accumulator
};

// a term's plan from its description (host): the product as pz_glwe_mul_const_batched (PZ_MUL_CONST) plans it - (cnv_offset_hi,
// cnv_offset_lo) of operations/glwe.rs:83-87, res_big of a_size + b_size - hi limbs (:89) - and the digit split of the join's shift
inline void lc_plan_term(LinTerm& t, const LinTermSpec& s, int res_size, int base2k) {
    t = LinTerm{};
    t.mc.a = s.a; t.mc.a_bs = s.a_bs;
    if (!s.re && !s.im) {
        t.mc.a_size = s.a_size; t.mc.res_size = res_size; t.mc.k = base2k; t.mc.form = LC_ZERO;
    } else {
        int hi = 0;
        long long lo = 0;
        if (s.cnv_offset < (size_t)base2k) lo = -(long long)((size_t)base2k - s.cnv_offset % (size_t)base2k);
        else { const size_t q = s.cnv_offset / (size_t)base2k; hi = (int)(q ? q - 1 : 0); lo = (long long)(s.cnv_offset % (size_t)base2k); }
        const int big = s.a_size + s.b_size - hi;
        const MulConstArmSpec arms[2] = {{s.re ? s.re : s.im, s.b_size, big, hi}, {s.im, s.b_size, big, hi}};
        mul_const_plan(t.mc, s.a_size, res_size, base2k, lo, s.re && s.im ? LC_BOTH : (s.im ? LC_IM : LC_RE), arms);
    }
    t.join = s.join; t.neg = s.neg;
    // shift.rs:90-102 with a_size = res_size: steps >= res_size leaves nothing to shift in
    const size_t steps = s.k / (size_t)base2k;
    t.steps = steps < (size_t)res_size ? (int)steps : res_size;
    t.k_rem = (int)(s.k % (size_t)base2k);
    t.min_size = res_size - t.steps;
}

// i64 slots per coefficient slice: operand limbs + accumulator (+ product, where a join shifts), twice in the paired mapping
__host__ __device__ constexpr long long lc_slots(int a_max, int res_size, int pair, int has_tmp) {
    return (long long)(pair ? 2 : 1) * (a_max + (has_tmp ? 2 : 1) * res_size);
}

// the term's product as pz_glwe_mul_const_batched (PZ_MUL_CONST) writes it (mul.rs:354-369) into d0 (coefficient x) / d1 (x + N/2):
// op 0 overwrites, 1 adds, 2 subtracts.  Limb stride kMulConstBlock everywhere.
__host__ __device__ __forceinline__ void lc_product(const LinTerm& t, const long long* la0, const long long* la1, long long* d0, long long* d1,
                                                    bool pair, int op) {
    const MulConstArgs& g = t.mc;
    const long long S = kMulConstBlock;
    const int pos = op == 0 ? 1 : (op == 1 ? 3 : 4), ngt = op == 0 ? 2 : (op == 1 ? 4 : 3);
    if (g.form == LC_ZERO) {   // dst.data_mut().zero()
        if (op == 0)
            for (int j = 0; j < g.res_size; ++j) { d0[j * S] = 0; if (pair) d1[j * S] = 0; }
    } else if (g.form == LC_RE) {
        mc_walk(g, g.arm[0], la0, d0, S, pos);
        if (pair) mc_walk(g, g.arm[0], la1, d1, S, pos);
    } else if (g.form == LC_IM) {   // X^{N/2} * v: v[x] -> x + N/2, v[x + N/2] -> -(x)
        mc_walk(g, g.arm[0], la0, d1, S, pos);
        mc_walk(g, g.arm[0], la1, d0, S, ngt);
    } else {                        // re, then X^{N/2} * im added without renormalization
        mc_walk(g, g.arm[0], la0, d0, S, pos);
        mc_walk(g, g.arm[0], la1, d1, S, pos);
        mc_walk(g, g.arm[1], la0, d1, S, op == 2 ? 4 : 3);
        mc_walk(g, g.arm[1], la1, d0, S, op == 2 ? 3 : 4);
    }
}

// digit j of vec_znx_lsh of `src` (res_size limbs, equal sizes) and the carry into limb j - 1, as k_glwe_combine's LSH terms
__host__ __device__ __forceinline__ long long lc_lsh_digit(const LinTerm& t, int k, const long long* src, int j, long long& c) {
    const long long x = src[(long long)(j + t.steps) * kMulConstBlock];
    return j == 0 ? znx_final_step(k, t.k_rem, x, c) : znx_middle_step(k, t.k_rem, x, c);
}
// acc +- lsh(tmp, k): glwe_lsh_add / glwe_lsh_sub
__host__ __device__ __forceinline__ void lc_join_lsh_tmp(const LinTerm& t, int k, long long* acc, const long long* tmp) {
    long long c = 0;
    for (int j = t.min_size - 1; j >= 0; --j) {
        const long long x1 = lc_lsh_digit(t, k, tmp, j, c);
        long long* r = acc + (long long)j * kMulConstBlock;
        *r = t.neg ? wsub(*r, x1) : wadd(*r, x1);
    }
}
// tmp = lsh(acc, k) +- tmp: glwe_lsh_assign on the accumulator (limbs >= min_size become zero), then glwe_add_assign / glwe_sub_assign
__host__ __device__ __forceinline__ void lc_join_lsh_acc(const LinTerm& t, int k, int res_size, const long long* acc, long long* tmp) {
    long long c = 0;
    for (int j = res_size - 1; j >= 0; --j) {
        const long long x1 = j < t.min_size ? lc_lsh_digit(t, k, acc, j, c) : 0;
        long long* r = tmp + (long long)j * kMulConstBlock;
        *r = t.neg ? wsub(x1, *r) : wadd(x1, *r);
    }
}

// column `c` of ciphertext `bt` at coefficient x (and x + N/2 when g.pair); `slice`: this coefficient's lc_slots() values, element e at
// slice[e * kMulConstBlock]
__host__ __device__ inline void lc_walk(const LinArgs& g, const LinTerm* terms, long long bt, int c, int x, long long* slice) {
    const long long S = kMulConstBlock;
    const bool pair = g.pair != 0;
    const int rs = g.res_size, h = g.n / 2, k = g.k;
    const long long rls = (long long)g.cols * g.n;
    long long* la0 = slice;
    long long* la1 = la0 + (pair ? (long long)g.a_max * S : 0);
    long long* acc0 = la0 + (long long)(pair ? 2 : 1) * g.a_max * S;
    long long* acc1 = acc0 + (pair ? (long long)rs * S : 0);
    long long* tmp0 = acc0 + (long long)(pair ? 2 : 1) * rs * S;
    long long* tmp1 = tmp0 + (pair ? (long long)rs * S : 0);
    long long* r = g.res + bt * g.res_bs + (long long)c * g.n + x;
    bool have = g.init_res != 0;
    if (have)
        for (int j = 0; j < rs; ++j) {
            acc0[j * S] = __builtin_nontemporal_load(r + (long long)j * rls);
            if (pair) acc1[j * S] = __builtin_nontemporal_load(r + (long long)j * rls + h);
        }
    for (int u = 0; u < g.nterms; ++u) {
        const LinTerm& t = terms[u];
        if (t.mc.form != LC_ZERO) {
            const long long* a = t.mc.a + bt * t.mc.a_bs + (long long)c * g.n + x;
            for (int l = 0; l < t.mc.a_size; ++l) {
                la0[l * S] = __builtin_nontemporal_load(a + (long long)l * rls);
                if (pair) la1[l * S] = __builtin_nontemporal_load(a + (long long)l * rls + h);
            }
        }
        if (!have) {
            lc_product(t, la0, la1, acc0, acc1, pair, 0);
            have = true;
        } else if (t.join == LC_JOIN_PLAIN) {
            lc_product(t, la0, la1, acc0, acc1, pair, t.neg ? 2 : 1);
        } else {
            lc_product(t, la0, la1, tmp0, tmp1, pair, 0);
            if (t.join == LC_JOIN_LSH_TMP) {
                lc_join_lsh_tmp(t, k, acc0, tmp0);
                if (pair) lc_join_lsh_tmp(t, k, acc1, tmp1);
            } else {
                lc_join_lsh_acc(t, k, rs, acc0, tmp0);
                if (pair) lc_join_lsh_acc(t, k, rs, acc1, tmp1);
                long long* s0 = acc0; acc0 = tmp0; tmp0 = s0;
                long long* s1 = acc1; acc1 = tmp1; tmp1 = s1;
            }
        }
    }
    // vec_znx_normalize_assign: first / middle / final step_assign with lsh 0 (normalize.rs:403-425), as k_glwe_combine closes
    long long nc0 = 0, nc1 = 0;
    for (int j = rs - 1; j >= 0; --j) {
        long long v0 = acc0[j * S], v1 = pair ? acc1[j * S] : 0;
        if (g.normalize) {
            v0 = znx_middle_step(k, 0, v0, nc0);
            if (pair) v1 = znx_middle_step(k, 0, v1, nc1);
        }
        r[(long long)j * rls] = v0;
        if (pair) r[(long long)j * rls + h] = v1;
    }
}

// grid: ceil(batch * npts / kMulConstBlock) workgroups, npts = n (unpaired) or n / 2; dynamic LDS = lc_slots() x kMulConstBlock i64
__global__ void __launch_bounds__(kMulConstBlock) k_lincomb_const(LinArgs g) {
    extern __shared__ long long lc_lds[];
    const int npts = g.pair ? g.n / 2 : g.n;
    const long long t = (long long)blockIdx.x * kMulConstBlock + threadIdx.x;
    if (t >= (long long)g.batch * npts) return;
    const int x = (int)(t % npts);
    const long long bt = t / npts;
    for (int c = 0; c < g.cols; ++c) lc_walk(g, g.terms, bt, c, x, lc_lds + threadIdx.x);
}

}  // namespace pz
