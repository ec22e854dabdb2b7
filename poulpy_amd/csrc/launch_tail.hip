// launch_tail.hip — dispatch of the fused tail (k_inv_tail, device_fft.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "internal.hpp"
#include "tail_forms.hpp"

namespace pz {

// the plan lists as the units see them (tail_plan.hpp)
bool tail_supported(const pz_module* M) { return tail_plan_whole_waves(M->plan.f1b, M->plan.cb); }
bool tail_narrow_supported(const pz_module* M) { return tail_plan_acc32(M->plan.f1a, M->plan.f1b, M->plan.cb); }
bool tail_rsh_supported(const pz_module* M) { return tail_plan_rsh(M->plan.f1a, M->plan.f1b, M->plan.cb); }
bool tail_d16_only_supported(const pz_module* M) { return tail_rsh_supported(M) && tail_narrow_supported(M); }

struct TailNz { int lsh, res_end, res_start, a_end, a_start, zero_from, col, mode, col2[2], mode2[2]; bool side16; TailD16 d16; };   // side16: the call names a TailD16
// columns [col_base, col_base + col_count) of the big value in one launch; nz: the tensoring forms (launch_inv_tail_nz)
static TailArgs tail_args(const pz_module* M, const TailCall& c, int col_base, int col_count, const TailNz* nz) {
    TailArgs g;
    g.T = c.T; g.res = c.res; g.small = c.small; g.res_bs = c.res_bs; g.small_bs = c.small_bs;
    g.nlimbs = c.nlimbs; g.ncols = c.ncols; g.res_cols = c.res_cols; g.res_size = c.res_size;
    g.small_cols = c.small_cols; g.small_size = c.small_size; g.base2k = c.base2k; g.m2 = M->plan.m2;
    g.tw1inv = M->tw1inv; g.wL1 = M->wL1; g.margin = M->probe ? M->margin : nullptr;
    g.small_all = c.small_all ? 1 : 0; g.auto_mul = c.auto_mul; g.auto_neg = c.auto_neg ? 1 : 0;
    g.col_base = col_base; g.col_count = col_count; g.body_col = c.body_col;
    g.gather_mul = c.gather_mul; g.gather_neg = c.gather_neg ? 1 : 0;
    g.pre_body = c.body_src != nullptr ? 1 : 0; g.small_neg = c.small_neg ? 1 : 0;
    g.body_src = c.body_src; g.body_bs = c.body_bs; g.body_ls = c.body_ls;
    g.body_add = 0; g.post_neg = c.post_neg ? 1 : 0; g.body_only = c.body_only ? 1 : 0; g.raw = 0;
    g.nz = nz ? 1 : 0;
    g.nz_lsh = nz ? nz->lsh : 0; g.nz_res_end = nz ? nz->res_end : 0; g.nz_res_start = nz ? nz->res_start : 0; g.nz_a_end = nz ? nz->a_end : 0;
    g.nz_a_start = nz ? nz->a_start : 0; g.nz_zero_from = nz ? nz->zero_from : 0; g.nz_col = nz ? nz->col : 0; g.nz_mode = nz ? nz->mode : 0;
    for (int u = 0; u < 2; ++u) { g.nz_col2[u] = nz ? nz->col2[u] : 0; g.nz_mode2[u] = nz ? nz->mode2[u] : 0; }
    // k_inv_tail's own mask (TailArgs, device_fft.hpp): bits 0 / 1 = 32-bit operand / result, bit 2 = the operand is a 16-bit GLWETensor,
    // bits 3 / 4 = 16-bit operand / result
    g.acc32 = (c.small_digits == Digits::I32 ? 1 : 0) | (c.res_digits == Digits::I32 ? 2 : 0) | (c.small16 ? 4 : 0) |
              (c.small_digits == Digits::I16 ? 8 : 0) | (c.res_digits == Digits::I16 ? 16 : 0);
    g.xcd_map = 0;
    g.d16w = nz ? nz->d16.w : nullptr; g.d16a = nz ? nz->d16.ra : nullptr; g.d16b = nz ? nz->d16.rb : nullptr;
    if (c.small16) { g.d16a = c.small16; g.body_bs = c.small16_cs; }
    if (c.big_neg) {
        // small - big = -(big + (-small)): every sign flipped (auto_mul = 2N gives s(n) = +1 everywhere, auto_neg flips it) on the sum with the negated
        // operand.  small_neg acts on the prepared-operand path: the body column's stream is column body_col of `small` itself, at the strides of `small`
        g.auto_mul = 2u * (unsigned)M->n; g.auto_neg = 1; g.small_neg = 1; g.pre_body = 1;
        g.body_src = c.small + (long long)c.body_col * (long long)M->n; g.body_bs = c.small_bs; g.body_ls = (long long)c.small_cols * (long long)M->n;
    }
    g.body16_wide = nullptr;
    if (c.body16) { g.d16a = c.body16; g.body_bs = (long long)c.body16_limbs * (long long)M->n; g.body16_wide = c.body16_wide; }
    return g;
}
// what tail_plan reads of a call
static TailFacts tail_facts(const pz_module* M, const TailCall& c, const TailNz* nz) {
    auto bits = [](Digits d) { return d == Digits::I64 ? 64 : d == Digits::I32 ? 32 : 16; };
    TailFacts f;
    f.f1a = M->plan.f1a; f.f1b = M->plan.f1b; f.cb = M->plan.cb;
    f.batch = c.batch; f.ncols = c.ncols; f.body_col = c.body_col; f.base2k = c.base2k; f.rowmajor = c.rowmajor;
    f.small = c.small != nullptr; f.small_all = c.small_all; f.small_neg = c.small_neg; f.small16 = c.small16 != nullptr;
    f.small_bs = c.small_bs; f.small_size = c.small_size; f.small_bits = bits(c.small_digits); f.res_bits = bits(c.res_digits);
    f.body_src = c.body_src != nullptr; f.body_only = c.body_only; f.body_bs = c.body_bs; f.body_ls = c.body_ls;
    f.body16 = c.body16 != nullptr; f.body16_wide = c.body16_wide != nullptr; f.other16 = c.other16 != nullptr; f.body16_limbs = c.body16_limbs;
    f.auto_mul = c.auto_mul; f.gather_mul = c.gather_mul; f.auto_neg = c.auto_neg; f.post_neg = c.post_neg; f.big_neg = c.big_neg;
    f.keyauto = c.keyauto; f.gather_neg = c.gather_neg; f.post_rsh = c.post_rsh;
    if (nz) {
        f.nz = true; f.nz_lsh = nz->lsh;
        f.nz_plain = nz->mode == 1 && nz->mode2[0] == 0 && nz->mode2[1] == 0; f.nz_mode5 = nz->mode2[0] == 5;
        f.d16 = nz->side16; f.d16_w = nz->d16.w != nullptr; f.d16_ra = nz->d16.ra != nullptr; f.d16_only = nz->d16.only;
    }
    return f;
}
// plan, then every launch of it on the call of its role; a refused call launches nothing
static int launch_tail_plan(pz_module* M, const TailCall& c, const TailNz* nz) {
    const FftPlan& pl = M->plan;
    const TailPlan p = tail_plan(tail_facts(M, c, nz));
    if (p.err != PZ_OK) return fail(p.err, "%s", p.msg);
    for (int i = 0; i < p.n; ++i) {
        const TailLaunch& l = p.launch[i];
        int blocks = c.batch * l.col_count * (pl.m2 / pl.cb);
        KTimer kt(M, PZ_K_FUSED_TAIL);
        TailArgs g = tail_args(M, tail_role_call(c, l.role), l.col_base, l.col_count, nz);
        // XCD-aware block order (all column blocks of one (ciphertext, column) on one XCD, back to back; see k_fwd_pass1): the grid is padded to
        // whole groups of 8 (ciphertext, column) pairs
        if (l.xcd) {
            const int nbc = c.batch * l.col_count, ncb = pl.m2 / pl.cb;
            g.xcd_map = nbc;
            blocks = ((nbc + 7) / 8) * 8 * ncb;
        }
        // the rounding-margin instantiation of the same form when the module's probe is on (pz_module_set_margin_probe): the same source with the
        // probe block compiled in, so that the margin is measured on the form the product path dispatches (launch_tail_probe.hip)
        PZ_TRY(M->probe ? tail_launch_form_probe(M, g, blocks, l.form) : tail_launch_form<false>(M, g, blocks, l.form));
        char note[64];
        tail_note(l.form, pl.f1a, pl.f1b, pl.cb, note, sizeof note);
        dispatch_note(M, M->probe ? "%s PROBE" : "%s", note);
    }
    return PZ_OK;
}
int launch_inv_tail(pz_module* M, const TailCall& c) { return launch_tail_plan(M, c, nullptr); }

// the inverse column pass on the row-major T2' with vec_znx_normalize's same-base steps (bit offset res_offset, a.size = a_size limbs of which
// the first nlimbs are transformed and the rest are zero) and NzCombine's stores into `res` (GLWE tensoring: raw inverse pass + normalize
// kernel in one; TailArgs::nz)
int launch_inv_tail_nz(pz_module* M, int batch, const NzTailCall& s) {
    const int nlimbs = s.nlimbs, res_size = s.res_size, base2k = s.base2k, a_size = s.a_size;
    const NzCombine* cb = s.cb;
    const TailD16* d16 = s.d16;
    const ZnxInterPlan p = znx_inter_plan(res_size, a_size, base2k, s.res_offset);
    TailNz nz;
    nz.lsh = p.lsh; nz.res_end = p.res_end; nz.res_start = p.res_start; nz.a_end = p.a_end; nz.a_start = p.a_start;
    nz.zero_from = nz.res_start - std::max(0, nz.a_start - std::max(nlimbs, nz.a_end));
    nz.col = s.res_col;
    nz.mode = cb ? cb->mode : 1;
    for (int u = 0; u < 2; ++u) { nz.col2[u] = cb ? cb->col2[u] : 0; nz.mode2[u] = cb ? cb->mode2[u] : 0; }
    nz.side16 = d16 != nullptr;
    if (d16) nz.d16 = *d16;
    TailCall c;
    c.batch = batch; c.T = s.T; c.rowmajor = true; c.nlimbs = nlimbs; c.ncols = 1;
    c.res = s.res; c.res_bs = s.res_bs; c.res_cols = s.res_cols; c.res_size = res_size; c.base2k = base2k;
    return launch_tail_plan(M, c, &nz);
}

}  // namespace pz
