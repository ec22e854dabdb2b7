// api_plain.hip — C ABI of GLWE x plaintext polynomial and GLWE x constant on device-resident batches (poulpy-core
// operations/glwe.rs:66-303 glwe_mul_const / glwe_mul_plain and their assign forms; poulpy-ckks leveled/default/mul.rs:342-415, the
// complex constant).  The reference composes them per ciphertext and per column from the convolution family (cnv_prepare_left/right,
// cnv_apply_dft, idft_apply_consume, big_normalize; cnv_by_const_apply + big_normalize); here every step covers the whole batch.
#include "api_common.hpp"

namespace {

inline long long mask_bottom_limb(size_t base2k, size_t k) {   // operations/glwe.rs:921-926
    const size_t r = k % base2k;
    return r == 0 ? -1ll : (long long)(~0ull << (base2k - r));
}
// (cnv_offset_hi, cnv_offset_lo), operations/glwe.rs:83-87 / :223-227
inline void offset_split(size_t cnv_offset, size_t base2k, int* hi, long long* lo) {
    if (cnv_offset < base2k) { *hi = 0; *lo = -(long long)(base2k - (cnv_offset % base2k)); }
    else { const size_t q = cnv_offset / base2k; *hi = (int)(q ? q - 1 : 0); *lo = (long long)(cnv_offset % base2k); }
}
inline size_t wave_chunk(const pz_module* M, size_t per_ct, size_t batch) {
    if (M->chunk) return std::min(M->chunk, batch);
    const size_t c = ((size_t)24 << 30) / std::max<size_t>(per_ct, 1);   // as the GLWE pipeline and the tensoring: ~24 GiB of the 288
    return std::min(std::max<size_t>(c, 1), batch);
}

// ---------------------------------------------------------------------------------------------------------------------
// GLWE x plaintext.  Two compositions, the same digits:
//  * pipeline plans (m = m1 x 128, N >= 4096) at one base2k (the default): pass 1 of the operand limbs and of the plaintext, then per column
//    one k_mid_cnv (forward row transforms, limb convolution, inverse row transform) and the normalizing inverse column pass
//    (launch_inv_tail_nz).  k_mid_cnv reads the plaintext in the operand's column layout, so the plaintext's pass 1 runs once per GLWE column
//    and ciphertext even when one plaintext serves the batch (0.28 of 5.5 ms per 256 at N = 2^16);
//  * POULPY_DBG_MULPLAIN_FUSED=1: ONE k_mid_cnv_pt for all columns (operand and plaintext rows loaded and row-transformed once per tile, the
//    plaintext in registers, its pass 1 once per call when shared), then the tail per column.  Same digits; measured 1.3 - 1.4x slower;
//  * everywhere else the batched per-op kernels: prepare (forward transforms, bottom limbs masked), per column limb convolution in the
//    DFT domain -> inverse transform -> normalize.
// ---------------------------------------------------------------------------------------------------------------------
struct PlainPlan {
    int cols, as, bs, res_size, hi, dft_size, min_size, off;
    long long lo, a_mask, b_mask;
    bool assign, mid, fused;
    size_t per_ct, once;   // workspace bytes per ciphertext / per call
};
int plain_plan(const pz_module* M, const pz_glwe_tensor_params* p, int mode, int pt_shared, PlainPlan& t) {
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(mode == PZ_MUL_PLAIN || mode == PZ_MUL_PLAIN_ASSIGN, "glwe_mul_plain: unknown mode");
    PZ_REQUIRE(p->rank >= 1 && p->a_size >= 1 && p->b_size >= 1 && p->res_size >= 1, "glwe_mul_plain: empty shape");
    PZ_REQUIRE(p->rank <= 64 && p->a_size <= 4096 && p->b_size <= 4096 && p->res_size <= 4096, "glwe_mul_plain: shape out of range");
    PZ_REQUIRE(p->ab_base2k >= 1 && p->ab_base2k <= 63 && p->res_base2k >= 1 && p->res_base2k <= 63, "glwe_mul_plain: base2k out of range");
    const size_t ab = p->ab_base2k;
    t.assign = mode == PZ_MUL_PLAIN_ASSIGN;
    if (t.assign) {   // operations/glwe.rs:270-273
        PZ_REQUIRE(p->res_base2k == ab, "glwe_mul_plain_assign: res.base2k must equal the plaintext's base2k");
        PZ_REQUIRE(p->a_size == p->res_size, "glwe_mul_plain_assign: a_size must equal res_size (res is the operand)");
    }
    PZ_REQUIRE((p->a_effective_k + ab - 1) / ab == p->a_size && (p->b_effective_k + ab - 1) / ab == p->b_size,
               "glwe_mul_plain: effective_k.div_ceil(base2k) must equal the size");                        // :208-209 / :272-273
    t.cols = (int)p->rank + 1;
    t.as = (int)p->a_size; t.bs = (int)p->b_size; t.res_size = (int)p->res_size;
    offset_split(p->cnv_offset, ab, &t.hi, &t.lo);
    PZ_REQUIRE((size_t)t.hi < p->a_size + p->b_size, "glwe_mul_plain: cnv_offset beyond the product");
    t.dft_size = t.as + t.bs - t.hi;                                                                       // :229 (no clipping)
    const int bound = t.as + t.bs - 1;
    t.min_size = std::min(t.dft_size, bound);
    t.off = std::min(t.hi, bound);
    t.a_mask = mask_bottom_limb(ab, p->a_effective_k);
    t.b_mask = mask_bottom_limb(ab, p->b_effective_k);
    t.mid = p->res_base2k == ab && mid_cnv_supported(M, t.as, t.bs, t.min_size);
    t.fused = t.mid && mid_cnv_pt_supported(M, t.cols, t.as, t.bs, t.min_size);
    const size_t n8 = (size_t)M->n * 8;   // one polynomial of i64 / f64, or one row-major T' polynomial (m complex points)
    if (t.fused) {
        t.per_ct = n8 * ((size_t)t.cols * t.as + (pt_shared ? 0 : (size_t)t.bs) + (size_t)t.cols * t.min_size);
        t.once = pt_shared ? n8 * t.bs : 0;
    } else if (t.mid) {
        t.per_ct = n8 * ((size_t)t.cols * t.as + (size_t)t.cols * t.bs + t.min_size);
        t.once = 0;
    } else {
        const size_t pb = n8 * t.bs;
        const size_t T = n8 * std::max({t.cols * t.as, t.bs, t.dft_size});
        t.per_ct = n8 * ((size_t)t.cols * t.as + t.dft_size) + T + (pt_shared ? 0 : pb);
        t.once = pt_shared ? pb : 0;
    }
    return PZ_OK;
}

int mul_plain_wave(pz_module* M, const PlainPlan& t, const pz_glwe_tensor_params* p, int nb, int64_t* res, const int64_t* a,
                   const int64_t* pt, bool shared, double* pb_once, bool pb_ready) {
    const long long n = (long long)M->n;
    const long long a_ct = n * t.cols * t.as, r_ct = n * t.cols * t.res_size, pt_ct = shared ? 0 : n * t.bs;
    char* base = (char*)M->ws;
    if (t.fused) {
        cplx *ta, *tb, *T2;
        const size_t m16 = (size_t)M->m * sizeof(cplx);
        PZ_TRY(ws_take(M, base, align256((size_t)nb * t.cols * t.as * m16), &ta));
        PZ_TRY(ws_take(M, base, align256((size_t)t.cols * nb * t.min_size * m16), &T2));
        if (shared) tb = (cplx*)pb_once;
        else PZ_TRY(ws_take(M, base, align256((size_t)nb * t.bs * m16), &tb));
        cplx* ta_last = ta + (size_t)nb * (t.as - 1) * t.cols * M->m;
        if (t.as > 1) {
            PolyMap sm{t.as - 1, t.cols, a_ct, (long long)t.cols * n, n, 0};
            PZ_TRY(launch_fwd_pass1(M, nb * (t.as - 1) * t.cols, (const long long*)a, sm, ta, true));
        }
        PolyMap sal{1, t.cols, a_ct, 0, n, (long long)(t.as - 1) * t.cols * n};
        PZ_TRY(launch_fwd_pass1(M, nb * t.cols, (const long long*)a, sal, ta_last, true, t.a_mask));
        // the plaintext's T': [pt][limb < bs - 1][m] then [pt][m]; one plaintext for the batch: once per call (the first wave)
        const int npt = shared ? 1 : nb;
        cplx* tb_last = tb + (size_t)npt * (t.bs - 1) * M->m;
        if (!shared || !pb_ready) {
            if (t.bs > 1) {
                PolyMap sm{t.bs - 1, 1, n * t.bs, n, 0, 0};
                PZ_TRY(launch_fwd_pass1(M, npt * (t.bs - 1), (const long long*)pt, sm, tb, true));
            }
            PolyMap sbl{1, 1, n * t.bs, 0, 0, (long long)(t.bs - 1) * n};
            PZ_TRY(launch_fwd_pass1(M, npt, (const long long*)pt, sbl, tb_last, true, t.b_mask));
        }
        MidCnvCall mc{ta, ta_last, tb, tb_last, T2, t.cols, t.as, t.bs, t.min_size, t.off};
        mc.b_shared = shared;
        PZ_TRY(launch_mid_cnv_pt(M, nb, mc));
        NzTailCall nz{T2, t.min_size, (long long*)res, r_ct, t.cols, t.res_size, 0, (int)p->res_base2k, t.lo, t.dft_size};
        for (int c = 0; c < t.cols; ++c, ++nz.res_col, nz.T += (size_t)nb * t.min_size * M->m) PZ_TRY(launch_inv_tail_nz(M, nb, nz));
        return PZ_OK;
    }
    if (t.mid) {
        cplx *ta, *tb, *T2;
        const size_t m16 = (size_t)M->m * sizeof(cplx);
        PZ_TRY(ws_take(M, base, align256((size_t)nb * t.cols * t.as * m16), &ta));
        PZ_TRY(ws_take(M, base, align256((size_t)nb * t.cols * t.bs * m16), &tb));
        PZ_TRY(ws_take(M, base, align256((size_t)nb * t.min_size * m16), &T2));
        // pass 1 in k_mid_cnv's layout: main limbs [ct][limb < size - 1][col][m], the masked bottom limb [ct][col][m]
        cplx* ta_last = ta + (size_t)nb * (t.as - 1) * t.cols * M->m;
        cplx* tb_last = tb + (size_t)nb * (t.bs - 1) * t.cols * M->m;
        if (t.as > 1) {
            PolyMap sm{t.as - 1, t.cols, a_ct, (long long)t.cols * n, n, 0};
            PZ_TRY(launch_fwd_pass1(M, nb * (t.as - 1) * t.cols, (const long long*)a, sm, ta, true));
        }
        PolyMap sal{1, t.cols, a_ct, 0, n, (long long)(t.as - 1) * t.cols * n};
        PZ_TRY(launch_fwd_pass1(M, nb * t.cols, (const long long*)a, sal, ta_last, true, t.a_mask));
        // the plaintext's single column read once per GLWE column (column stride 0), per ciphertext (batch stride 0 when shared)
        if (t.bs > 1) {
            PolyMap sm{t.bs - 1, t.cols, pt_ct, n, 0, 0};
            PZ_TRY(launch_fwd_pass1(M, nb * (t.bs - 1) * t.cols, (const long long*)pt, sm, tb, true));
        }
        PolyMap sbl{1, t.cols, pt_ct, 0, 0, (long long)(t.bs - 1) * n};
        PZ_TRY(launch_fwd_pass1(M, nb * t.cols, (const long long*)pt, sbl, tb_last, true, t.b_mask));
        MidCnvCall mc{ta, ta_last, tb, tb_last, T2, t.cols, t.as, t.bs, t.min_size, t.off};
        NzTailCall nz{T2, t.min_size, (long long*)res, r_ct, t.cols, t.res_size, 0, (int)p->res_base2k, t.lo, t.dft_size};
        for (int c = 0; c < t.cols; ++c) {
            mc.col_i = nz.res_col = c;
            PZ_TRY(launch_mid_cnv(M, nb, mc));
            PZ_TRY(launch_inv_tail_nz(M, nb, nz));
        }
        return PZ_OK;
    }
    double *pa, *pb, *rd;
    cplx* T;
    const long long pa_bs = n * t.cols * t.as, rd_bs = n * t.dft_size;
    PZ_TRY(ws_take(M, base, align256((size_t)nb * t.cols * t.as * n * 8), &pa));
    PZ_TRY(ws_take(M, base, align256((size_t)nb * t.dft_size * n * 8), &rd));
    PZ_TRY(ws_take(M, base, align256((size_t)nb * std::max({t.cols * t.as, t.bs, t.dft_size}) * n * 8), &T));
    if (shared) pb = pb_once;
    else PZ_TRY(ws_take(M, base, align256((size_t)nb * t.bs * n * 8), &pb));
    PZ_TRY(dev_cnv_prepare(M, nb, pa, pa_bs, t.cols, t.as, a, a_ct, t.cols, t.as, t.a_mask, T));
    if (!shared || !pb_ready) PZ_TRY(dev_cnv_prepare(M, shared ? 1 : nb, pb, n * t.bs, 1, t.bs, pt, n * t.bs, 1, t.bs, t.b_mask, T));
    const long long pb_bs = shared ? 0 : n * t.bs;
    for (int c = 0; c < t.cols; ++c) {
        PZ_TRY(launch_cnv_apply(M, nb, rd, rd_bs, 1, 0, t.min_size, t.off, pa, pa_bs, t.as, c, -1, pb, pb_bs, t.bs, 0, -1));
        if (t.dft_size > t.min_size)   // convolution.rs:256-258
            PZ_TRY(launch_ew(M, EW_ZERO, rd + (long long)t.min_size * n, rd_bs, n, nullptr, 0, 0, nullptr, 0, 0, t.dft_size - t.min_size, nb));
        DV dv{rd, rd_bs, 1, t.dft_size};
        PZ_TRY(dev_idft(M, nb, dv, 0, dv, 0, 1, t.dft_size, T));
        DV out{res, r_ct, t.cols, t.res_size};
        PZ_TRY(dev_normalize(M, nb, out, (int)p->res_base2k, t.lo, c, dv, (int)p->ab_base2k, 0));
    }
    return PZ_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// GLWE x constant.  k_mul_const_nz (launch_plain.hip) at one base2k; two bases (or constants beyond the kernel's 32 digits / operands
// beyond 64 limbs, or POULPY_DBG_MULCONST_FUSED=0) take the composition the reference runs, each step batched: cnv_by_const_apply into
// res_big (k_cnv_by_const_batched), normalize, rotate, add.
// ---------------------------------------------------------------------------------------------------------------------
struct ConstArm { const int64_t* b; int big, hi; long long lo; int in_base2k; };

// one arm into `dst` (batch stride dst_bs, the GLWE layout) through the per-op kernels
int const_arm_composed(pz_module* M, int nb, const ConstArm& w, int b_size, int64_t* dst, long long dst_bs, const int64_t* a, long long a_bs,
                       int cols, int a_size, int res_size, int res_base2k, long long* big, long long* bdev) {
    const long long n = (long long)M->n;
    PZ_HIP(hipMemcpyAsync(bdev, w.b, (size_t)b_size * 8, hipMemcpyHostToDevice, M->stream));
    const int bound = a_size + b_size - 1, min_size = std::min(w.big, bound), off = std::min(w.hi, bound);
    const long long big_bs = n * cols * w.big;
    PZ_TRY(launch_cnv_by_const_batched(M, nb, big, big_bs, w.big, min_size, off, (const long long*)a, a_bs, cols, a_size, bdev, b_size));
    DV bv{big, big_bs, cols, w.big};
    for (int c = 0; c < cols; ++c) {
        if (w.big > min_size)
            PZ_TRY(launch_ew(M, EW_ZERO, poly_ptr(M, bv, c, min_size), big_bs, limb_stride(M, bv), nullptr, 0, 0, nullptr, 0, 0, w.big - min_size, nb));
        DV out{dst, dst_bs, cols, res_size};
        PZ_TRY(dev_normalize(M, nb, out, res_base2k, w.lo, c, bv, w.in_base2k, c));
    }
    return PZ_OK;
}

}  // namespace

extern "C" {

size_t pz_glwe_mul_plain_workspace_bytes(const pz_module* M, const pz_glwe_tensor_params* p, int mode, int pt_shared, size_t batch) {
    PlainPlan t;
    if (!M || plain_plan(M, p, mode, pt_shared, t) != PZ_OK) return 0;
    return wave_chunk(M, t.per_ct, batch) * (t.per_ct + 4 * 256) + t.once + 256;
}

int pz_glwe_mul_plain_batched(pz_module* M, int64_t* res, const int64_t* a, const int64_t* pt, int pt_shared, const pz_glwe_tensor_params* p,
                              int mode, size_t batch) {
    PZ_ENTER(M);
    PlainPlan t;
    PZ_TRY(plain_plan(M, p, mode, pt_shared, t));
    if (t.assign) {
        PZ_REQUIRE(a == nullptr || a == res, "glwe_mul_plain_assign: a must be NULL or res (res is the operand)");
        a = res;
    }
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a) && is_device_ptr(pt), "batched entry points take device pointers");
    PZ_REQUIRE((const void*)res != (const void*)pt, "glwe_mul_plain: res must not alias the plaintext");
    PZ_REQUIRE(t.assign || (const void*)res != (const void*)a, "glwe_mul_plain: res must not alias a (use PZ_MUL_PLAIN_ASSIGN)");
    if (batch == 0) return PZ_OK;
    const bool shared = pt_shared != 0;
    const size_t chunk = wave_chunk(M, t.per_ct, batch);
    PZ_TRY(ws_reserve(M, chunk * (t.per_ct + 4 * 256) + t.once + 256));
    // (the plaintext prepared once per call sits at the end of the workspace, behind every wave's segments)
    double* pb_once = t.once ? (double*)((char*)M->ws + chunk * (t.per_ct + 4 * 256)) : nullptr;
    const long long n = (long long)M->n, a_ct = n * t.cols * t.as, r_ct = n * t.cols * t.res_size, pt_ct = shared ? 0 : n * t.bs;
    if (t.mid && !t.fused) dispatch_note(M, "glwe_mul_plain: pass 1 + k_mid_cnv per column + normalizing tail");
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (int)std::min(chunk, batch - b0);
        // every wave carves the workspace again, and a shorter last wave puts its segments over the guards of the waves before it: those are
        // verified now, before their bytes become someone else's segment (as ws_reserve does for a composite call)
        if (canary_mode() && b0 > 0) canary_verify(M, "a workspace segment carved by an earlier wave of this call", M->ws, (char*)M->ws + M->ws_bytes);
        PZ_TRY(mul_plain_wave(M, t, p, nb, res + (long long)b0 * r_ct, a + (long long)b0 * a_ct, pt + (long long)b0 * pt_ct, shared, pb_once,
                              b0 > 0));
    }
    return PZ_OK;
}

int pz_glwe_mul_const_batched(pz_module* M, int64_t* res, const int64_t* a, const int64_t* re, const int64_t* im, size_t b_size,
                              const pz_glwe_mul_const_params* p, int mode, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(mode == PZ_MUL_CONST || mode == PZ_MUL_CONST_ASSIGN, "glwe_mul_const: unknown mode");
    PZ_REQUIRE(p->rank >= 1 && p->rank <= 64 && p->a_size >= 1 && p->res_size >= 1 && p->a_size <= 4096 && p->res_size <= 4096,
               "glwe_mul_const: empty or out-of-range shape");
    PZ_REQUIRE(p->a_base2k >= 1 && p->a_base2k <= 63 && p->res_base2k >= 1 && p->res_base2k <= 63, "glwe_mul_const: base2k out of range");
    PZ_REQUIRE((re == nullptr && im == nullptr) || (b_size >= 1 && b_size <= 4096), "glwe_mul_const: b_size must be in 1..4096");
    const bool assign = mode == PZ_MUL_CONST_ASSIGN;
    if (assign) {
        PZ_REQUIRE(a == nullptr || a == res, "glwe_mul_const_assign: a must be NULL or res (res is the operand)");
        PZ_REQUIRE(p->a_size == p->res_size && p->a_base2k == p->res_base2k, "glwe_mul_const_assign: a_size / a_base2k must equal res_size / res_base2k");
        a = res;
    }
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a), "batched entry points take device pointers");
    PZ_REQUIRE(assign || (const void*)res != (const void*)a, "glwe_mul_const: res must not alias a (use PZ_MUL_CONST_ASSIGN)");
    const int cols = (int)p->rank + 1, as = (int)p->a_size, rs = (int)p->res_size, bsz = (int)b_size;
    const long long n = (long long)M->n, a_ct = n * cols * as, r_ct = n * cols * rs;
    int hi = 0;
    long long lo = 0;
    offset_split(p->cnv_offset, assign ? p->res_base2k : p->a_base2k, &hi, &lo);   // :83-87 (a_base2k), :113-117 (res_base2k)
    PZ_REQUIRE(re == nullptr && im == nullptr ? true : (size_t)hi < p->a_size + b_size, "glwe_mul_const: cnv_offset beyond the product");
    if (batch == 0) return PZ_OK;
    if (re == nullptr && im == nullptr)   // mul.rs:360 / :397: dst.data_mut().zero()
        return launch_ew(M, EW_ZERO, res, r_ct, n, nullptr, 0, 0, nullptr, 0, 0, cols * rs, (int)batch);
    // the arms: `re` as the call itself (the assign form's res_big has res.size() limbs, :119); `im` in the complex forms: for _into
    // glwe_mul_const from a (:367 / :374), for _assign glwe_mul_const from dst BEFORE dst is overwritten (mul.rs:408-409)
    const int big_full = as + bsz - hi;                                                                    // :89
    ConstArm w_re{re, assign ? rs : big_full, hi, lo, (int)p->a_base2k};
    ConstArm w_im{im, big_full, hi, lo, (int)p->a_base2k};
    if (assign && re == nullptr) w_im.big = rs;   // (None, Some(im)) assign: glwe_mul_const_assign with im (mul.rs:400)
    const int form = re && im ? 2 : (im ? 1 : 0);
    const ConstArm& first = re ? w_re : w_im;
    static const bool fused_env = (rt_knob("POULPY_DBG_MULCONST_FUSED", 1) != 0);
    const bool fused = fused_env && p->a_base2k == p->res_base2k && mul_const_nz_supported(M, as, bsz);
    if (fused) {
        MulConstArmSpec arms[2] = {{first.b, bsz, first.big, first.hi}, {w_im.b, bsz, w_im.big, w_im.hi}};
        const size_t chunk = M->chunk ? std::min(M->chunk, batch) : batch;
        for (size_t b0 = 0; b0 < batch; b0 += chunk) {
            const int nb = (int)std::min(chunk, batch - b0);
            PZ_TRY(launch_mul_const_nz(M, nb, (long long*)(res + (long long)b0 * r_ct), r_ct, (const long long*)(a + (long long)b0 * a_ct), a_ct, cols,
                                       as, rs, (int)p->res_base2k, lo, form, arms));
        }
        return PZ_OK;
    }
    // composition: res_big and the im product (a GLWE of res's layout, take_glwe(dst)) in the workspace
    const int big_max = std::max(w_re.big, w_im.big);
    const size_t per_ct = (size_t)n * 8 * cols * ((size_t)big_max + (form == 2 ? 2 * rs : rs)) + 3 * 256;
    const size_t chunk = wave_chunk(M, per_ct, batch);
    PZ_TRY(ws_reserve(M, chunk * per_ct + align256(b_size * 8) + 256));
    char* base = (char*)M->ws;
    long long *big, *tmp, *rot, *bdev;
    PZ_TRY(ws_take(M, base, align256(chunk * n * 8 * cols * big_max), &big));
    PZ_TRY(ws_take(M, base, align256(chunk * n * 8 * cols * rs), &tmp));
    PZ_TRY(ws_take(M, base, form == 2 ? align256(chunk * n * 8 * cols * rs) : 0, &rot));
    PZ_TRY(ws_take(M, base, align256(b_size * 8), &bdev));
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        const int nb = (int)std::min(chunk, batch - b0);
        int64_t* r0 = res + (long long)b0 * r_ct;
        const int64_t* a0 = a + (long long)b0 * a_ct;
        if (form == 0) {
            PZ_TRY(const_arm_composed(M, nb, w_re, bsz, r0, r_ct, a0, a_ct, cols, as, rs, (int)p->res_base2k, big, bdev));
            continue;
        }
        // X^{N/2} * (the im product), rotate.rs:3-27 on every column and limb
        int64_t* im_dst = (int64_t*)tmp;
        PZ_TRY(const_arm_composed(M, nb, w_im, bsz, im_dst, r_ct, a0, a_ct, cols, as, rs, (int)p->res_base2k, big, bdev));
        PZ_HIP(hipStreamSynchronize(M->stream));   // (bdev is refilled from the host by the next arm)
        int64_t* rot_dst = form == 2 ? (int64_t*)rot : r0;
        PolyMap sm{rs * cols, 1, r_ct, n, 0, 0};
        PZ_TRY(launch_rotate(M, nb * rs * cols, (const long long*)im_dst, sm, (long long*)rot_dst, sm, n / 2));
        if (form == 2) {
            PZ_TRY(const_arm_composed(M, nb, w_re, bsz, r0, r_ct, a0, a_ct, cols, as, rs, (int)p->res_base2k, big, bdev));
            PZ_TRY(launch_ew(M, EW_ADD_I64, r0, r_ct, n, r0, r_ct, n, rot, r_ct, n, cols * rs, nb));   // glwe_add_assign, no normalization
        }
        PZ_HIP(hipStreamSynchronize(M->stream));
    }
    return PZ_OK;
}

}  // extern "C"
