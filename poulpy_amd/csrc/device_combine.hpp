// device_combine.hpp — k_glwe_combine: a GLWE linear combination sum_t term_t, optionally normalized, in one pass over HBM.
//
// Every term is one of poulpy's limb-walking primitives on its own operand (poulpy-cpu-ref reference/vec_znx/shift.rs, add.rs, sub.rs,
// negate.rs): RAW (the limbs as stored, vec_znx_add_into / sub / add_assign / negate), LSH (the digits vec_znx_lsh<false> / vec_znx_lsh_sub
// add / subtract, shift.rs:68-180) and RSH (vec_znx_rsh<false> / vec_znx_rsh_sub, shift.rs:245-...).  The reference applies them one after
// the other, each over all limbs; here one thread owns two neighbouring coefficients of one column of one ciphertext and walks the output
// limbs from the bottom (res_size - 1) to the top, applying every term to the limb in term order, then the final normalize chain
// (vec_znx_normalize_assign, normalize.rs:403-425), and stores the limb once.  That is the same result because every term's effect on limb j
// depends only on the running value of limb j and on the term's own carry, which flows from the limbs below:
//  * RAW / LSH / the middle range of RSH add (or subtract) a digit computed from the operand alone (normalization.rs:179-260);
//  * the low range of RSH (limbs < min(res_size, steps)) renormalizes the running value with the term's carry (shift.rs:326-340).
// An LSH term whose operand IS res reads limb j + steps after limb j + steps was stored: that operand's limbs are staged once, before the
// walk, in the thread's own LDS slice.  The steps themselves are those of znx_steps.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "znx_steps.hpp"

namespace pz {

constexpr int kCombMaxTerms = 4;
constexpr int kCombBlock = 128;
constexpr int kCombMaxStage = 32;   // limbs of an in-place LSH operand staged in LDS: 32 x 16 B x 128 threads = 64 KiB
enum { CB_NONE = 0, CB_RAW = 1, CB_LSH = 2, CB_RSH = 3 };

struct CombTerm {
    const long long* a;   // column 0 of ciphertext 0
    long long bs, ls;     // scalars between ciphertexts (0: one operand for the batch) and between limbs
    int cstep;            // 1: column c of res reads column c of a; 0: column 0 only (plaintext terms; other columns skip the term)
    int size, kind, neg, stage;
    int lsh, pad, steps;  // the digit split of the shift (shift.rs:90 / :282-293); pad keeps the layout
    int pro;              // carry-only prologue over limbs [pro, size) of a (shift.rs:108-119 / :300-309)
    int lo, hi;           // LSH: output limbs [0, lo = min_size) (shift.rs:107).  RSH: middle range [lo = res_end, hi = res_start) (:294-295)
};
struct CombArgs {
    long long* res;
    long long res_bs, res_ls;
    int n, batch, cols, res_size, k, nterms, normalize;
    CombTerm t[kCombMaxTerms];
};

__global__ void __launch_bounds__(kCombBlock) k_glwe_combine(CombArgs g) {
    extern __shared__ ulonglong2 cb_lds[];
    const int hn = g.n >> 1;
    const long long tid = (long long)blockIdx.x * kCombBlock + threadIdx.x;
    if (tid >= (long long)g.batch * g.cols * hn) return;
    const int x = 2 * (int)(tid % hn);
    const long long q = tid / hn;
    const int c = (int)(q % g.cols);
    const long long b = q / g.cols;
    const int k = g.k;
    unsigned long long* r = (unsigned long long*)g.res + b * g.res_bs + (long long)c * g.n + x;

    const ulonglong2* ap[kCombMaxTerms];
    long long cr[kCombMaxTerms][2];
    int kind[kCombMaxTerms];
#pragma unroll
    for (int u = 0; u < kCombMaxTerms; ++u) {
        const CombTerm& t = g.t[u];
        kind[u] = u < g.nterms && (t.cstep || c == 0) ? t.kind : CB_NONE;
        ap[u] = reinterpret_cast<const ulonglong2*>(t.a + b * t.bs + (long long)(c * t.cstep) * g.n + x);
        cr[u][0] = cr[u][1] = 0;
        if (kind[u] == CB_NONE) continue;
        if (t.stage) {   // every read of the operand precedes the first store (the operand is res)
            for (int l = 0; l < t.size; ++l) cb_lds[l * kCombBlock + threadIdx.x] = ap[u][(long long)l * (t.ls >> 1)];
        }
        if (kind[u] == CB_LSH || kind[u] == CB_RSH) {
            for (int l = t.size - 1; l >= t.pro; --l) {   // the limbs below the window: their carry only
                const ulonglong2 v = t.stage ? cb_lds[l * kCombBlock + threadIdx.x] : ap[u][(long long)l * (t.ls >> 1)];
                const long long xv[2] = {(long long)v.x, (long long)v.y};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if (l == t.size - 1) cr[u][e] = znx_first_step_carry_only(k, t.lsh, xv[e]);
                    else znx_middle_step_carry_only(k, t.lsh, xv[e], cr[u][e]);
                }
            }
        }
    }

    long long nc[2] = {0, 0};
    for (int j = g.res_size - 1; j >= 0; --j) {
        long long v[2] = {0, 0};
#pragma unroll
        for (int u = 0; u < kCombMaxTerms; ++u) {
            const CombTerm& t = g.t[u];
            if (kind[u] == CB_RAW) {
                if (j < t.size) {
                    const ulonglong2 a = ap[u][(long long)j * (t.ls >> 1)];
                    if (t.neg) { v[0] = wsub(v[0], (long long)a.x); v[1] = wsub(v[1], (long long)a.y); }
                    else { v[0] = wadd(v[0], (long long)a.x); v[1] = wadd(v[1], (long long)a.y); }
                }
            } else if (kind[u] == CB_LSH || (kind[u] == CB_RSH && j >= t.lo && j < t.hi)) {
                // LSH: output limb j < min_size from a[j + steps]; RSH middle range: a[j - steps]
                const bool lsh_term = kind[u] == CB_LSH;
                if (lsh_term && j >= t.lo) continue;
                const int l = lsh_term ? j + t.steps : j - t.steps;
                const ulonglong2 a = t.stage ? cb_lds[l * kCombBlock + threadIdx.x] : ap[u][(long long)l * (t.ls >> 1)];
                const long long xv[2] = {(long long)a.x, (long long)a.y};
#pragma unroll
                for (int e = 0; e < 2; ++e) {   // the top limb of an LSH term takes the final step
                    const long long x1 = lsh_term && j == 0 ? znx_final_step(k, t.lsh, xv[e], cr[u][e]) : znx_middle_step(k, t.lsh, xv[e], cr[u][e]);
                    v[e] = t.neg ? wsub(v[e], x1) : wadd(v[e], x1);
                }
            } else if (kind[u] == CB_RSH && j < t.lo) {
                // limbs below the shifted operand: the running value renormalized with the term's carry, negated first by rsh_sub
                // (shift.rs:326-340 and vec_znx_rsh_sub: the _assign steps with lsh 0)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    if (j == t.lo - 1 && t.neg) cr[u][e] = wsub(0, cr[u][e]);
                    v[e] = j == 0 ? znx_final_step(k, 0, v[e], cr[u][e]) : znx_middle_step(k, 0, v[e], cr[u][e]);
                }
            }
        }
        if (g.normalize) {   // vec_znx_normalize_assign: first / middle / final step_assign with lsh 0 (normalize.rs:403-425)
#pragma unroll
            for (int e = 0; e < 2; ++e) v[e] = znx_middle_step(k, 0, v[e], nc[e]);
        }
        *reinterpret_cast<ulonglong2*>(r + (long long)j * g.res_ls) = make_ulonglong2((unsigned long long)v[0], (unsigned long long)v[1]);
    }
}

}  // namespace pz
