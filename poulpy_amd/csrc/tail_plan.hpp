// tail_plan.hpp — which launches of the fused tail (k_inv_tail, device_fft.hpp) a call becomes: the plans that have each form, the split of the
// columns, the form of every launch and every refusal.  Plain C++ with no HIP header: launch_tail.hip runs the plan, tail_forms.hpp walks the
// same three lists to launch, tests/cpp/test_tail_plan.cpp compiles all of it with the host compiler and sweeps it (every form chosen has an
// entry; every column is written by exactly one launch; the launches are the ones tests/golden/tail_plans.txt records).
#pragma once
#include <cstddef>
#include <cstdio>

#include "../../include/poulpy_hip.h"

namespace pz {

// (f1a, f1b, cb) of the FftPlans with a tail
#define PZ_P1F_CASES(X) X(4, 1, 4) X(8, 1, 4) X(8, 1, 16) X(16, 1, 16) X(4, 4, 16) X(4, 8, 16) X(8, 8, 16) X(8, 16, 16) X(16, 16, 16) X(8, 16, 8)
// the forms beyond the plain one - digits leaving through a one-bit vec_znx_rsh (glwe_trace), the sign-only tail of a spectral automorphism,
// the tensoring tails - are instantiated for the 128-point-row plans (N = 2^13 .. 2^16)
#define PZ_RSH_CASES(X) X(4, 8, 16) X(8, 8, 16) X(8, 16, 16) X(16, 16, 16)
// the 32-bit-accumulator form (blind rotation on the pipeline): every 128-point-row plan it runs on, N = 2^12 .. 2^16
#define PZ_ACC32_CASES(X) X(4, 4, 16) PZ_RSH_CASES(X)

struct TailForm {
    // SGN: signs without an operand; SGN16: + a 16-bit operand; SGN16R: + the shifted store.  NZ1 / NZ2: the tensoring tails (diagonal / pairwise or
    // combining), NZ1W / NZ2R: with 16-bit side copies (write / read), NZ1O / NZ2O: 16-bit digits ONLY.  ACC32: 32-bit accumulator digits
    enum Kind { PLAIN, RSH, SGN, NZ1, NZ2, ACC32, NZ1W, NZ2R, NZ1O, NZ2O, SGN16, SGN16R } kind = PLAIN;
    bool rowmajor = false, has_small = false;   // PLAIN: one instantiation per (row-major, body add) combination
};

#define PZ_TAIL_PLAN_IS(A, B, C) if (f1a == A && f1b == B && cb == C) return true;
inline bool tail_plan_plain(int f1a, int f1b, int cb) { PZ_P1F_CASES(PZ_TAIL_PLAN_IS) return false; }
inline bool tail_plan_rsh(int f1a, int f1b, int cb) { PZ_RSH_CASES(PZ_TAIL_PLAN_IS) return false; }
inline bool tail_plan_acc32(int f1a, int f1b, int cb) { PZ_ACC32_CASES(PZ_TAIL_PLAN_IS) return false; }
#undef PZ_TAIL_PLAN_IS
// the two roles of k_inv_tail must be whole waves
inline bool tail_plan_whole_waves(int f1b, int cb) { return (f1b * cb) % 64 == 0; }
// the list tail_launch_form walks for a kind has this plan
inline bool tail_form_exists(const TailForm& f, int f1a, int f1b, int cb) {
    if (f.kind == TailForm::ACC32) return tail_plan_acc32(f1a, f1b, cb);
    return f.kind == TailForm::PLAIN ? tail_plan_plain(f1a, f1b, cb) : tail_plan_rsh(f1a, f1b, cb);
}

// the dispatch note of a form on a plan, worded as tests/golden/tail_plans.txt names forms (tests and the bench tools match on these); the
// rounding-margin instantiation of the same form (launch_tail_probe.hip) adds " PROBE"
inline void tail_note(const TailForm& f, int f1a, int f1b, int cb, char* buf, size_t n) {
    static const char* const kind[] = {"PLAIN", "RSH", "SGN", "NZ1", "NZ2", "ACC32", "NZ1W", "NZ2R", "NZ1O", "NZ2O", "SGN16", "SGN16R"};
    if (f.kind == TailForm::PLAIN) snprintf(buf, n, "k_inv_tail<%d,%d,%d> PLAIN(%d,%d)", f1a, f1b, cb, (int)f.rowmajor, (int)f.has_small);
    else snprintf(buf, n, "k_inv_tail<%d,%d,%d> %s", f1a, f1b, cb, kind[f.kind]);
}

// What the plan reads of a call: the scalars of a TailCall under their own names, "is set" for its pointers, the widths of its digits, the
// FftPlan, and what launch_inv_tail_nz adds (TailNz, launch_tail.hip).
struct TailFacts {
    int f1a = 0, f1b = 0, cb = 0;
    int batch = 0, ncols = 0, body_col = 0, base2k = 0;
    bool rowmajor = false;
    bool small = false, small_all = false, small_neg = false, small16 = false;
    long long small_bs = 0;
    int small_size = 0, small_bits = 64, res_bits = 64;
    bool body_src = false, body_only = false;
    long long body_bs = 0, body_ls = 0;
    bool body16 = false, body16_wide = false, other16 = false;
    int body16_limbs = 0;
    unsigned auto_mul = 0, gather_mul = 0;
    bool auto_neg = false, post_neg = false, big_neg = false, keyauto = false, gather_neg = false, post_rsh = false;
    // the normalizing store of the tensoring forms: its shift, plain (mode 1, no second result) or pairwise (NzCombine mode 5), 16-bit side copies
    bool nz = false, nz_plain = false, nz_mode5 = false;
    int nz_lsh = 0;
    bool d16 = false, d16_w = false, d16_ra = false, d16_only = false;
};

// The derivation of the caller's call that a launch runs on.
enum class TailRole {
    AS_GIVEN,
    BODY,      // the body column of a key switch: its operand and the signs that go with it
    PLAIN,     // the other columns of a key switch: no operand, no signs
    SIGNS,     // no operand, the signs stay (the f64 chain of the sign-only form)
    BODY16,    // the same with the body column's 16-bit operand
    OTHER16,   // the same with the other column's 16-bit operand (add / sub forms at rank 1)
    OPERAND,   // as given without the 16-bit operand: the columns that have their own +-a[col]
};
// C = TailCall (launch_tail.hip) or TailFacts: the members named here are called the same in both.  The only place that clears fields.
template <class C>
inline C tail_role_call(const C& c, TailRole role) {
    C r = c;
    if (role == TailRole::AS_GIVEN) return r;
    if (role == TailRole::OPERAND) { r.body16 = {}; r.body16_wide = {}; r.body16_limbs = 0; return r; }
    // the other five: nothing gathered or prepared, and an operand on BODY alone, for its one column
    r.gather_mul = 0; r.body_src = {}; r.body_bs = r.body_ls = 0; r.small_all = false;
    r.body_only = role == TailRole::SIGNS && c.keyauto && c.body_only;   // (the permuted-key form hands it on)
    if (role != TailRole::BODY) { r.small = {}; r.small_bs = 0; }
    if (role == TailRole::BODY || role == TailRole::PLAIN) r.gather_neg = r.small_neg = r.post_rsh = r.post_neg = false;
    if (role == TailRole::PLAIN) { r.auto_mul = 0; r.auto_neg = false; r.body_col = 0; }
    if (role == TailRole::SIGNS) { r.small_size = 0; r.body16 = {}; r.body16_wide = {}; r.body16_limbs = 0; }   // (BODY16: small_size = the operand's limbs)
    // add / sub forms: the sign of the body operand is the pre-pass's, the other column's 16-bit values take the operand's (small_neg)
    if ((role == TailRole::BODY16 && !c.body_only) || role == TailRole::OTHER16) { r.gather_neg = false; r.small_neg = role == TailRole::OTHER16 && c.small_neg; }
    if (role == TailRole::OTHER16) { r.body16 = c.other16; r.body16_limbs = c.small_size; }
    return r;
}

struct TailLaunch {
    int col_base = 0, col_count = 0;   // columns [col_base, col_base + col_count) of the big value
    TailRole role = TailRole::AS_GIVEN;
    TailForm form;
    bool xcd = false;                  // XCD-aware block order (launch_tail.hip)
};
struct TailPlan {
    int err = PZ_OK;
    const char* msg = nullptr;         // of the refusal
    int n = 0;
    TailLaunch launch[4];
};
inline TailPlan tail_refuse(int err, const char* msg) {
    TailPlan p;
    p.err = err; p.msg = msg;
    return p;
}

// The form of one launch, c = the call of its role: shifted store | sign-only | tensoring (pairwise / diagonal) | plain (with or without the body
// operand).  A refusal comes back as a plan without launches.
inline TailPlan tail_form(const TailFacts& c, TailForm& f) {
    const bool rsh_plan = tail_plan_rsh(c.f1a, c.f1b, c.cb);
    const bool narrow = c.small_bits != 64 || c.res_bits != 64;
    f.kind = TailForm::PLAIN; f.rowmajor = c.rowmajor; f.has_small = c.small;
    if (narrow || c.small16) {   // 32-bit accumulator digits: the plain every-column-operand form, nothing else
        if (!(tail_plan_acc32(c.f1a, c.f1b, c.cb) && c.rowmajor && c.small && c.small_all && !c.post_rsh && !c.nz && c.auto_mul == 0 && c.gather_mul == 0 &&
              !c.body_src && c.base2k <= 31 && !(narrow && c.small16)))
            return tail_refuse(PZ_ERR_UNSUPPORTED, "fused tail: no 32-bit-accumulator variant for this call");
        f.kind = TailForm::ACC32;
    } else if (c.post_rsh && c.body16 && !c.small) {   // the 16-bit-operand form with the shifted store (glwe_trace's body column)
        if (!(rsh_plan && c.rowmajor && !c.nz && c.base2k <= 29)) return tail_refuse(PZ_ERR_UNSUPPORTED, "fused tail: no shifted-store 16-bit-operand variant for this call");
        f.kind = TailForm::SGN16R;
    } else if (c.post_rsh) {
        if (!(rsh_plan && c.rowmajor && c.small)) return tail_refuse(PZ_ERR_UNSUPPORTED, "fused tail: no shifted-store variant for this plan");
        f.kind = TailForm::RSH;
    } else if (!c.small && (c.auto_mul != 0 || c.body16)) {   // signs without an operand (+ the 16-bit operand of the body column)
        if (!(c.rowmajor && !c.nz && rsh_plan)) return tail_refuse(PZ_ERR_UNSUPPORTED, "fused tail: no sign-only variant for this plan");
        if (c.body16 && c.base2k > 31) return tail_refuse(PZ_ERR_UNSUPPORTED, "fused tail: the 16-bit-operand form needs digits of at most 31 bits");
        f.kind = c.body16 ? TailForm::SGN16 : TailForm::SGN;
    } else if (c.nz) {   // the tensoring forms: their own instantiation of the row-major, operand-free tail
        if (!(c.rowmajor && !c.small && rsh_plan)) return tail_refuse(PZ_ERR_UNSUPPORTED, "fused tail: the tensoring forms need the row-major layout of a 128-point-row plan");
        // contract of the NZ = 1 instantiation (device_fft.hpp): plain normalized store (mode 1, no second result), shift below one limb;
        // NzCombine mode 5 reads diagonal columns that a mode-1 launch of the same call wrote before it
        if (!(c.nz_lsh >= 0 && c.nz_lsh < c.base2k)) return tail_refuse(PZ_ERR_INVALID, "fused tail: normalizing store needs 0 <= lsh < base2k");
        // any NzCombine mode (pairwise term: with the prefetch of the diagonal digits): NZ2; the diagonal launches: NZ1
        f.kind = c.nz_plain ? TailForm::NZ1 : TailForm::NZ2;
        // 16-bit side copies (TailD16): the diagonal launch that writes them, the pairwise launch (mode 5) that reads them
        if (f.kind == TailForm::NZ1 && c.d16_w) f.kind = TailForm::NZ1W;
        if (f.kind == TailForm::NZ2 && c.d16_ra) {
            if (!c.nz_mode5) return tail_refuse(PZ_ERR_INVALID, "fused tail: 16-bit side copies are read by the mode-5 pairwise launch only");
            f.kind = TailForm::NZ2R;
        }
        if (c.d16_only) {   // the digits leave only as 16-bit copies
            if (f.kind == TailForm::NZ1W) f.kind = TailForm::NZ1O;
            else if (f.kind == TailForm::NZ2R && c.d16_w) f.kind = TailForm::NZ2O;
            else return tail_refuse(PZ_ERR_INVALID, "fused tail: 16-bit-only digits need the side-copy forms (a diagonal launch that writes them, a pairwise launch that reads and writes them)");
        }
    }
    return TailPlan{};
}

// columns [base, base + count) on `role`; an empty range launches nothing and refuses nothing, the first refusal ends the plan
inline void tail_plan_cols(TailPlan& p, const TailFacts& c, int base, int count, TailRole role) {
    if (p.err != PZ_OK || c.batch * count == 0) return;
    const TailFacts r = tail_role_call(c, role);
    TailLaunch l;
    l.col_base = base; l.col_count = count; l.role = role;
    // XCD-aware block order: the gathers of the automorphism forms need it for L2 locality, and the row-major pipeline streams faster with it
    l.xcd = r.gather_mul != 0 || r.rowmajor;
    const TailPlan no = tail_form(r, l.form);
    if (no.err != PZ_OK) p = no;
    else p.launch[p.n++] = l;
}
// the columns before and after the body column
inline void tail_plan_around(TailPlan& p, const TailFacts& c, TailRole role) {
    tail_plan_cols(p, c, 0, c.body_col, role);
    tail_plan_cols(p, c, c.body_col + 1, c.ncols - 1 - c.body_col, role);
}

// The launches of one call, at most four.  The body operand of a key switch only exists for one column (0; `body_col` for ggsw_expand_row): that
// column runs the variant that prefetches it (more registers, one workgroup less per CU), the other columns the plain one.  A column with a 16-bit
// operand is launched twice, on the 16-bit-operand form and on the operand variant that keeps body16_wide: the first returns at once if the
// pre-pass raised the flag, the second unless it did - exactly one of them writes the column.
inline TailPlan tail_plan(const TailFacts& c) {
    TailPlan p;
    if (c.nz) {   // launch_inv_tail_nz: one column, one launch
        if (c.d16 && !(c.base2k <= 16)) return tail_refuse(PZ_ERR_INVALID, "fused tail: 16-bit side copies of the digits need base2k <= 16");
        if (c.d16 && !(!c.d16_only || c.base2k <= 14)) return tail_refuse(PZ_ERR_INVALID, "fused tail: a pairwise column kept as 16-bit values needs base2k <= 14");
        tail_plan_cols(p, c, 0, c.ncols, TailRole::AS_GIVEN);
        return p;
    }
    if (c.big_neg && !(c.small && c.small_all && c.auto_mul == 0 && !c.auto_neg && !c.post_neg && !c.small_neg && !c.post_rsh && !c.keyauto && c.gather_mul == 0 &&
                       !c.body_src && !c.body16 && !c.small16 && !c.body_only && c.small_bits == 64 && c.res_bits == 64))
        return tail_refuse(PZ_ERR_INVALID, "fused tail: the negated big value takes an i64 operand per column and nothing else");
    if (c.post_rsh && !(c.small && c.small_all)) return tail_refuse(PZ_ERR_UNSUPPORTED, "fused tail: shifted store needs an operand per column");
    const bool rsh_plan = tail_plan_rsh(c.f1a, c.f1b, c.cb);
    if (c.keyauto) {
        // key switch by a permuted key (glwe_automorphism_key_automorphism, wave_keyauto_tail in api_glwe.hip): the carry chain of every column runs
        // between the signs of X -> X^p, s .* normalize(s .* big) - the body column on the operand variant (a0 at the natural index), the others on
        // the sign-only variant of the f64 chain
        if (!(c.small && !c.small_all && c.auto_mul != 0 && c.post_neg && c.ncols > 1 && c.rowmajor && !c.post_rsh && c.gather_mul == 0 && !c.body_src && !c.body16))
            return tail_refuse(PZ_ERR_INVALID, "fused tail: the permuted-key form takes the plain key switch's operand and the signs of auto_mul, nothing else");
        // (N = 4096 has no sign-only instantiation: every column on the operand variant, which only finds an operand on the body column)
        if (!rsh_plan) { tail_plan_cols(p, c, 0, c.ncols, TailRole::AS_GIVEN); return p; }
        tail_plan_cols(p, c, c.body_col, 1, TailRole::AS_GIVEN);
        tail_plan_around(p, c, TailRole::SIGNS);
    } else if (c.small && !c.small_all && c.ncols > 1) {
        tail_plan_cols(p, c, c.body_col, 1, TailRole::BODY);
        tail_plan_around(p, c, TailRole::PLAIN);
    } else if (c.small && c.small_all && c.body_only && c.auto_mul != 0 && c.ncols > 1 && !c.post_rsh && c.rowmajor && rsh_plan) {
        // plain spectral glwe_automorphism (only the body column has an operand): that column on the operand variant (and, body16, on the
        // 16-bit-operand form), the others on the sign-only variant of the f64 chain (profiles/r04_ab_auto_sgn.txt)
        tail_plan_cols(p, c, c.body_col, 1, TailRole::AS_GIVEN);
        if (c.body16) tail_plan_cols(p, c, c.body_col, 1, TailRole::BODY16);
        tail_plan_around(p, c, TailRole::SIGNS);
    } else if (c.body16 && c.small && c.small_all && !c.body_only && c.rowmajor && rsh_plan) {
        // add / sub forms of the spectral automorphism with the body-column operand phi(body) +- a0 as 16-bit copies (TailCall::body16): that column
        // as above, every other column on the operand variant with its own +-a[col] - or, at rank 1 with other16 (pass 1 left +-a[1] as 16-bit
        // values), as a pair of launches too
        tail_plan_cols(p, c, c.body_col, 1, TailRole::AS_GIVEN);
        tail_plan_cols(p, c, c.body_col, 1, TailRole::BODY16);
        if (c.other16 && c.ncols == 2 && c.body_col == 0) {
            tail_plan_cols(p, c, 1, 1, TailRole::AS_GIVEN);
            tail_plan_cols(p, c, 1, 1, TailRole::OTHER16);
        } else tail_plan_around(p, c, TailRole::OPERAND);
    } else tail_plan_cols(p, c, 0, c.ncols, TailRole::AS_GIVEN);
    return p;
}

}  // namespace pz
