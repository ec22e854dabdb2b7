// api_cnv.hip — C ABI of the convolution family (HalImpl cnv_*, poulpy-hal/src/oep/hal_impl.rs:670-754; reference
// poulpy-cpu-ref/src/reference/fft64/convolution.rs) and of GLWE tensoring on device-resident batches
// (poulpy-core/src/operations/glwe.rs:609-913), SURVEY.md §8f rank 4 / BASELINE configs[4].
#include "api_common.hpp"
#include "glwe_call.hpp"
#include "dot_form.hpp"

// CnvPVecL / CnvPVecR bytes in this backend: polynomial (col, limb) = its spectrum in device order at (col*size + limb)*n doubles.
static inline size_t cnv_bytes(const pz_module* M, size_t cols, size_t size) { return (size_t)M->n * cols * size * 8; }

extern "C" {

// hal_defaults/convolution.rs:40-45, :63-68, and cnv_prepare_self_tmp_bytes: one VecZnxDft(1, min(res_size, a_size))
size_t pz_cnv_prepare_left_tmp_bytes(const pz_module* M, size_t res_size, size_t a_size) {
    return M ? (size_t)M->n * std::min(res_size, a_size) * 8 : 0;
}
size_t pz_cnv_prepare_right_tmp_bytes(const pz_module* M, size_t res_size, size_t a_size) { return pz_cnv_prepare_left_tmp_bytes(M, res_size, a_size); }
size_t pz_cnv_prepare_self_tmp_bytes(const pz_module* M, size_t res_size, size_t a_size) { return pz_cnv_prepare_left_tmp_bytes(M, res_size, a_size); }
// convolution.rs:205-208, :261-263, :142-145
size_t pz_cnv_apply_dft_tmp_bytes(const pz_module*, size_t, size_t res_size, size_t a_size, size_t b_size) {
    return 8 * 8 * std::min(res_size, a_size + b_size - 1);
}
size_t pz_cnv_pairwise_apply_dft_tmp_bytes(const pz_module* M, size_t cnv_offset, size_t res_size, size_t a_size, size_t b_size) {
    return pz_cnv_apply_dft_tmp_bytes(M, cnv_offset, res_size, a_size, b_size) + (a_size + b_size) * 8 * 8;
}
size_t pz_cnv_by_const_apply_tmp_bytes(const pz_module*, size_t, size_t res_size, size_t a_size, size_t b_size) {
    return 8 * (std::min(res_size, a_size + b_size - 1) + a_size) * 8;
}

static int cnv_prepare_one(pz_module* M, double* res, size_t res_cols, size_t res_size, const int64_t* a, size_t a_cols, size_t a_size,
                           int64_t mask, double* copy_to) {
    PZ_REQUIRE(a_cols == res_cols, "cnv_prepare: a.cols %zu != res.cols %zu", a_cols, res_cols);   // convolution.rs:46
    Stage sr, sa, sc;
    PZ_TRY(sa.in(a, vbytes(M, a_cols, a_size), true, false, M));
    PZ_TRY(sr.in(res, cnv_bytes(M, res_cols, res_size), false, true, M));
    if (copy_to) PZ_TRY(sc.in(copy_to, cnv_bytes(M, res_cols, res_size), false, true, M));
    cplx* T;
    PZ_TRY(need_T(M, res_cols * std::max<size_t>(std::min(res_size, a_size), 1), &T));
    PZ_TRY(dev_cnv_prepare(M, 1, (double*)sr.dev, 0, (int)res_cols, (int)res_size, (const int64_t*)sa.dev, 0, (int)a_cols, (int)a_size,
                           (long long)mask, T));
    if (copy_to)   // convolution.rs:134-138: right = left (identical data for FFT64)
        PZ_TRY(launch_ew(M, EW_COPY, sc.dev, 0, (long long)M->n, sr.dev, 0, (long long)M->n, nullptr, 0, 0, (int)(res_cols * res_size), 1));
    const bool host = sr.owned || sa.owned || sc.owned;
    PZ_TRY(sr.finish());
    PZ_TRY(sa.finish());
    PZ_TRY(sc.finish());
    return finish_call(M, host);
}
int pz_cnv_prepare_left(pz_module* M, double* res, size_t res_cols, size_t res_size, const int64_t* a, size_t a_cols, size_t a_size,
                        int64_t mask) {
    PZ_ENTER(M);
    return cnv_prepare_one(M, res, res_cols, res_size, a, a_cols, a_size, mask, nullptr);
}
int pz_cnv_prepare_right(pz_module* M, double* res, size_t res_cols, size_t res_size, const int64_t* a, size_t a_cols, size_t a_size,
                         int64_t mask) {
    PZ_ENTER(M);
    return cnv_prepare_one(M, res, res_cols, res_size, a, a_cols, a_size, mask, nullptr);
}
int pz_cnv_prepare_self(pz_module* M, double* left, double* right, size_t cols, size_t size, const int64_t* a, size_t a_cols, size_t a_size,
                        int64_t mask) {
    PZ_ENTER(M);
    PZ_REQUIRE((const void*)left != (const void*)right, "cnv_prepare_self: left and right must be distinct buffers");
    return cnv_prepare_one(M, left, cols, size, a, a_cols, a_size, mask, right);
}

static int cnv_apply_common(pz_module* M, size_t cnv_offset, double* res, size_t res_cols, size_t res_size, size_t res_col, const double* a,
                            size_t a_cols, size_t a_size, const double* b, size_t b_cols, size_t b_size, size_t a_i, size_t b_i, int a_j,
                            int b_j) {
    PZ_CHECK_COL(res_col, res_cols, "cnv_apply_dft(res)");
    PZ_CHECK_COL(a_i, a_cols, "cnv_apply_dft(a)");
    PZ_CHECK_COL(b_i, b_cols, "cnv_apply_dft(b)");
    PZ_REQUIRE(a_size > 0 && b_size > 0, "cnv_apply_dft: empty operand");                                // reim4/mod.rs:47-48
    PZ_REQUIRE((const void*)res != (const void*)a && (const void*)res != (const void*)b, "cnv_apply_dft: res must not alias an operand");
    Stage sr, sa, sb;
    PZ_TRY(sa.in(a, cnv_bytes(M, a_cols, a_size), true, false, M));
    if ((const void*)b == (const void*)a) { sb.M = M; sb.dev = sa.dev; }
    else PZ_TRY(sb.in(b, cnv_bytes(M, b_cols, b_size), true, false, M));
    PZ_TRY(sr.in(res, vbytes(M, res_cols, res_size), true, true, M));   // inout: other columns survive
    const size_t bound = a_size + b_size - 1;
    const int min_size = (int)std::min(res_size, bound), offset = (int)std::min(cnv_offset, bound);
    PZ_TRY(launch_cnv_apply(M, 1, (double*)sr.dev, 0, (int)res_cols, (int)res_col, min_size, offset, (const double*)sa.dev, 0, (int)a_size,
                            (int)a_i, a_j, (const double*)sb.dev, 0, (int)b_size, (int)b_i, b_j));
    DV dr{sr.dev, 0, (int)res_cols, (int)res_size};
    PZ_TRY(launch_ew(M, EW_ZERO, poly_ptr(M, dr, (int)res_col, min_size), 0, limb_stride(M, dr), nullptr, 0, 0, nullptr, 0, 0,
                     (int)res_size - min_size, 1));                                                     // convolution.rs:256-258
    const bool host = sr.owned || sa.owned || sb.owned;
    PZ_TRY(sr.finish());
    PZ_TRY(sa.finish());
    PZ_TRY(sb.finish());
    return finish_call(M, host);
}
int pz_cnv_apply_dft(pz_module* M, size_t cnv_offset, double* res, size_t res_cols, size_t res_size, size_t res_col, const double* a,
                     size_t a_cols, size_t a_size, size_t a_col, const double* b, size_t b_cols, size_t b_size, size_t b_col) {
    PZ_ENTER(M);
    return cnv_apply_common(M, cnv_offset, res, res_cols, res_size, res_col, a, a_cols, a_size, b, b_cols, b_size, a_col, b_col, -1, -1);
}
int pz_cnv_pairwise_apply_dft(pz_module* M, size_t cnv_offset, double* res, size_t res_cols, size_t res_size, size_t res_col,
                              const double* a, size_t a_cols, size_t a_size, const double* b, size_t b_cols, size_t b_size, size_t col_i,
                              size_t col_j) {
    PZ_ENTER(M);
    PZ_CHECK_COL(col_j, a_cols, "cnv_pairwise_apply_dft(a)");
    PZ_CHECK_COL(col_j, b_cols, "cnv_pairwise_apply_dft(b)");
    const int j = col_i == col_j ? -1 : (int)col_j;                                                     // convolution.rs:281-284
    return cnv_apply_common(M, cnv_offset, res, res_cols, res_size, res_col, a, a_cols, a_size, b, b_cols, b_size, col_i, col_i, j, j);
}

int pz_cnv_by_const_apply(pz_module* M, size_t cnv_offset, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                          size_t a_cols, size_t a_size, size_t a_col, const int64_t* b, size_t b_len) {
    PZ_ENTER(M);
    PZ_CHECK_COL(res_col, res_cols, "cnv_by_const_apply(res)");
    PZ_CHECK_COL(a_col, a_cols, "cnv_by_const_apply(a)");
    PZ_REQUIRE(a_size > 0 && b_len > 0, "cnv_by_const_apply: empty operand");
    PZ_REQUIRE((const void*)res != (const void*)a, "cnv_by_const_apply: res must not alias a");
    Stage sr, sa, sb;
    PZ_TRY(sa.in(a, vbytes(M, a_cols, a_size), true, false, M));
    PZ_TRY(sb.in(b, b_len * 8, true, false, M));
    PZ_TRY(sr.in(res, vbytes(M, res_cols, res_size), true, true, M));
    const size_t bound = a_size + b_len - 1;
    const int min_size = (int)std::min(res_size, bound), offset = (int)std::min(cnv_offset, bound);
    PZ_TRY(launch_cnv_by_const(M, (long long*)sr.dev, (int)res_cols, (int)res_col, min_size, offset, (const long long*)sa.dev, (int)a_cols,
                               (int)a_size, (int)a_col, (const long long*)sb.dev, (int)b_len));
    DV dr{sr.dev, 0, (int)res_cols, (int)res_size};
    PZ_TRY(launch_ew(M, EW_ZERO, poly_ptr(M, dr, (int)res_col, min_size), 0, limb_stride(M, dr), nullptr, 0, 0, nullptr, 0, 0,
                     (int)res_size - min_size, 1));
    const bool host = sr.owned || sa.owned || sb.owned;
    PZ_TRY(sr.finish());
    PZ_TRY(sa.finish());
    PZ_TRY(sb.finish());
    return finish_call(M, host);
}

// ---------------------------------------------------------------------------------------------------------------------
// GLWE tensoring on `batch` device-resident ciphertext pairs (poulpy-core/src/operations/glwe.rs:700-807 glwe_tensor_apply,
// :809-913 _add_assign, :609-698 glwe_tensor_square_apply).  res: batch GLWETensors = VecZnx((rank+1)(rank+2)/2, res_size);
// column of the pair (i, j >= i) = i cols - i (i + 1) / 2 + j.
// Composition, every step one batched launch: prepare (forward transforms of all columns x limbs, bottom limb masked) | per product
// term: limb convolution in the DFT domain -> inverse transform -> normalize with cnv_offset_lo into a one-column temporary
// -> the reference's copy / negate / add / sub into the tensor columns.
// ---------------------------------------------------------------------------------------------------------------------
static inline long long msb_mask_bottom_limb(size_t base2k, size_t k) {   // operations/glwe.rs:921-926
    const size_t r = k % base2k;
    return r == 0 ? -1ll : (long long)(~0ull << (base2k - r));
}
static inline size_t tensor_dft_size(size_t full, size_t res_size, size_t res_base2k, size_t in_base2k, long long res_offset) {   // :929-957
    long long ob = res_offset % (long long)in_base2k;
    if (res_offset < 0 && ob != 0) ob += (long long)in_base2k;
    return std::min(full, (res_size * res_base2k + (size_t)ob + in_base2k - 1) / in_base2k);
}
struct TensorPlan {
    int cols, tcols, a_size, b_size, res_size, dft_size, hi;
    long long lo;
    size_t prep_a, prep_b, res_dft, tmp, diag, T, d16, per_ct;
};
static int tensor_plan(const pz_module* M, const pz_glwe_tensor_params* p, int mode, TensorPlan& t) {
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(mode >= PZ_TENSOR_APPLY && mode <= PZ_TENSOR_SQUARE, "glwe_tensor_apply: unknown mode");
    PZ_REQUIRE(p->rank >= 1 && p->a_size >= 1 && p->res_size >= 1 && (mode == PZ_TENSOR_SQUARE || p->b_size >= 1), "glwe_tensor_apply: empty shape");
    PZ_REQUIRE(p->ab_base2k >= 1 && p->ab_base2k <= 63 && p->res_base2k >= 1 && p->res_base2k <= 63, "glwe_tensor_apply: base2k out of range");
    const size_t ab = p->ab_base2k, bsz = mode == PZ_TENSOR_SQUARE ? p->a_size : p->b_size;
    const size_t bk = mode == PZ_TENSOR_SQUARE ? p->a_effective_k : p->b_effective_k;
    PZ_REQUIRE((p->a_effective_k + ab - 1) / ab == p->a_size && (bk + ab - 1) / ab == bsz,
               "glwe_tensor_apply: effective_k.div_ceil(base2k) must equal the size");                  // :721-722
    t.cols = (int)p->rank + 1;
    t.tcols = t.cols * (t.cols + 1) / 2;
    t.a_size = (int)p->a_size; t.b_size = (int)bsz; t.res_size = (int)p->res_size;
    if (p->cnv_offset < ab) { t.hi = 0; t.lo = -(long long)(ab - (p->cnv_offset % ab)); }               // :733-737
    else { const size_t q = p->cnv_offset / ab; t.hi = (int)(q ? q - 1 : 0); t.lo = (long long)(p->cnv_offset % ab); }
    PZ_REQUIRE((size_t)t.hi < p->a_size + bsz, "glwe_tensor_apply: cnv_offset beyond the product");
    t.dft_size = (int)tensor_dft_size(p->a_size + bsz - (size_t)t.hi, p->res_size, p->res_base2k, ab, t.lo);
    const size_t n8 = (size_t)M->n * 8;
    t.prep_a = n8 * t.cols * t.a_size;
    t.prep_b = n8 * t.cols * t.b_size;
    t.res_dft = n8 * std::max(t.dft_size, 1);
    t.tmp = n8 * t.res_size;
    t.diag = mode == PZ_TENSOR_SQUARE ? n8 * t.cols * t.res_size : 0;
    // (k_mid_cnv3 leaves the three result sets of a rank-1 tensoring side by side: 3 x min(dft_size, a_size + b_size - 1) polynomials)
    t.T = (size_t)M->m * sizeof(cplx) * std::max({t.cols * t.a_size, t.cols * t.b_size, t.dft_size, 1, t.cols == 2 ? 3 * std::min(t.dft_size, t.a_size + t.b_size - 1) : 0});
    // 16-bit side copies of the diagonal terms' digits for the pairwise tails (apply / square with base2k <= 16; TailD16)
    t.d16 = (mode != PZ_TENSOR_APPLY_ADD_ASSIGN && p->res_base2k <= 16 && p->res_base2k == p->ab_base2k) ? (size_t)M->n * 2 * t.cols * t.res_size : 0;
    t.per_ct = t.prep_a + t.prep_b + t.res_dft + t.tmp + t.diag + t.T + t.d16;
    return PZ_OK;
}
static size_t tensor_chunk(const pz_module* M, const TensorPlan& t, size_t batch) {
    if (M->chunk) return std::min(M->chunk, batch);
    size_t c = ((size_t)24 << 30) / std::max<size_t>(t.per_ct, 1);   // as the GLWE pipeline: ~24 GiB of the 288 (at 16 GiB the bench's 256 pairs of 16 limbs split 222 + 34)
    return std::min(std::max<size_t>(c, 1), batch);
}
size_t pz_glwe_tensor_apply_workspace_bytes(const pz_module* M, const pz_glwe_tensor_params* p, int mode, size_t batch) {
    TensorPlan t;
    if (!M || tensor_plan(M, p, mode, t) != PZ_OK) return 0;
    return tensor_chunk(M, t, batch) * (t.per_ct + 6 * 256);
}

// One wave of a GLWE tensoring (glwe_tensor_apply / _add_assign / _square, poulpy-core operations/glwe.rs:609-913): `nb` pairs whose operands have
// been prepared, the product terms (i, j) one at a time into the tensor columns.  State shared by the steps below; the entry point owns the loop
// over waves.
struct TensorWave {
    pz_module* M;
    const pz_glwe_tensor_params* p;
    TensorPlan t;
    bool square, add;
    long long n;
    // i64 elements between consecutive ciphertexts of a / b; 0: packed (n cols a_size).  Only pass 1 reads the operands, so a container
    // with more limbs than the operand uses (a rescaled ciphertext: the used limbs are a prefix) is read in place
    long long a_cs = 0, b_cs = 0;
    // workspace of a wave
    double *pa = nullptr, *pb = nullptr, *rd = nullptr;
    int64_t *tmp = nullptr, *diag = nullptr;
    short* d16 = nullptr;   // [diagonal term i][pair][res limb][n] (TensorPlan::d16)
    // the fused multiply + relinearize (pz_glwe_tensor_mul_relinearize_batched): the GLWETensor leaves ONLY as 16-bit digits,
    // t16[tensor column][pair][res limb][n] in the tail's tile order; `rb` is not written
    short* t16 = nullptr;
    long long t16_cs = 0;   // int16 elements between tensor columns
    cplx* T = nullptr;
    long long r_ct = 0, pa_bs = 0, pb_bs = 0, rd_bs = 0, tmp_bs = 0, dg_bs = 0, rls = 0, a_mask = 0, b_mask = 0;
    // the wave
    int nb = 0;
    int64_t* rb = nullptr;
    bool fused = false, all3 = false;
    cplx *ta_main = nullptr, *ta_last = nullptr, *tb_main = nullptr, *tb_last = nullptr;
    MidCnvCall mid;   // the fused row pass of this wave: operands, the product window (prepare)

    int take_workspace(size_t chunk) {
        const size_t s_pa = align256(chunk * t.prep_a), s_pb = square ? 0 : align256(chunk * t.prep_b), s_rd = align256(chunk * t.res_dft);
        const size_t s_tmp = align256(chunk * t.tmp), s_dg = align256(chunk * t.diag), s_T = align256(chunk * t.T), s_d16 = align256(chunk * t.d16);
        PZ_TRY(ws_reserve(M, s_pa + s_pb + s_rd + s_tmp + s_dg + s_T + s_d16));
        char* base = (char*)M->ws;
        PZ_TRY(ws_take(M, base, s_pa, &pa));
        PZ_TRY(ws_take(M, base, s_pb, &pb));
        if (square) pb = pa;                                        // convolution.rs:134-138: right = left for FFT64
        PZ_TRY(ws_take(M, base, s_rd, &rd));
        PZ_TRY(ws_take(M, base, s_tmp, &tmp));
        PZ_TRY(ws_take(M, base, s_dg, &diag));
        PZ_TRY(ws_take(M, base, s_T, &T));
        PZ_TRY(ws_take(M, base, s_d16, &d16));
        if (!s_d16) d16 = nullptr;
        r_ct = n * t.tcols * t.res_size;
        pa_bs = n * t.cols * t.a_size; pb_bs = n * t.cols * t.b_size; rd_bs = n * std::max(t.dft_size, 1); tmp_bs = n * t.res_size;
        dg_bs = n * t.cols * t.res_size;
        a_mask = msb_mask_bottom_limb(p->ab_base2k, p->a_effective_k);
        b_mask = square ? a_mask : msb_mask_bottom_limb(p->ab_base2k, p->b_effective_k);
        rls = (long long)t.tcols * n;   // limb stride of the tensor
        return PZ_OK;
    }
    // pass 1 of one operand's limbs in the pipeline's row-major layout: all limbs but the last, then the last one under its mask
    int prep_T(const int64_t* src, long long ct, int size, long long mask, cplx* region, cplx** mainp, cplx** lastp) {
        *mainp = region;
        *lastp = region + (size_t)nb * (size - 1) * t.cols * (size_t)M->m;
        if (size > 1) {
            PolyMap sm{size - 1, t.cols, ct, (long long)t.cols * n, n, 0};
            PZ_TRY(launch_fwd_pass1(M, nb * (size - 1) * t.cols, (const long long*)src, sm, *mainp, true));
        }
        PolyMap sl{1, t.cols, ct, 0, n, (long long)(size - 1) * t.cols * n};
        return launch_fwd_pass1(M, nb * t.cols, (const long long*)src, sl, *lastp, true, mask);
    }
    // Operands of the wave.  Fused row pass (round 3, m = m1 x 128 plans, one base2k, rank <= 2): pass 1 of the operand limbs, then per term ONE
    // kernel for forward row transform + limb convolution + inverse row transform (k_mid_cnv), the inverse column pass with the normalization
    // and the combination in its stores - instead of forward pass 2 of both operands, k_cnv_apply, inverse pass 2 and inverse pass 1
    // (POULPY_DBG_TENSOR_FUSED=0).  Rank 1, 16 / 8 limbs (round 4): the three terms in ONE launch - operand rows loaded and forward-transformed
    // once, the limb convolution with one operand vector in registers (k_mid_cnv3; POULPY_DBG_TENSOR_ALLTERMS=0: k_mid_cnv per term)
    int prepare(const int64_t* ab, const int64_t* bb) {
        const long long a_ct = a_cs ? a_cs : n * t.cols * t.a_size, b_ct = b_cs ? b_cs : n * t.cols * t.b_size;
        static const bool fused_env = (rt_knob("POULPY_DBG_TENSOR_FUSED", 1) != 0);
        static const bool combine_ok_env = (rt_knob("POULPY_DBG_TENSOR_COMBINE", 1) != 0);
        const int bound = t.a_size + t.b_size - 1;
        fused = fused_env && combine_ok_env && p->res_base2k == p->ab_base2k && t.cols <= 3 && t.dft_size >= 1 &&
                mid_cnv_supported(M, t.a_size, t.b_size, std::min(t.dft_size, bound));
        if (fused) {
            PZ_TRY(prep_T(ab, a_ct, t.a_size, a_mask, (cplx*)pa, &ta_main, &ta_last));
            if (square) { tb_main = ta_main; tb_last = ta_last; }
            else PZ_TRY(prep_T(bb, b_ct, t.b_size, b_mask, (cplx*)pb, &tb_main, &tb_last));
        } else {
            PZ_TRY(dev_cnv_prepare(M, nb, pa, pa_bs, t.cols, t.a_size, ab, a_ct, t.cols, t.a_size, a_mask, T));
            if (!square) PZ_TRY(dev_cnv_prepare(M, nb, pb, pb_bs, t.cols, t.b_size, bb, b_ct, t.cols, t.b_size, b_mask, T));
        }
        const int ms_all = std::min(t.dft_size, bound), off_all = std::min(t.hi, bound);
        mid = MidCnvCall{ta_main, ta_last, tb_main, tb_last, T, t.cols, t.a_size, t.b_size, ms_all, off_all};
        all3 = fused && mid_cnv3_supported(M, t.cols, t.a_size, t.b_size, ms_all);
        if (all3) PZ_TRY(launch_mid_cnv3(M, nb, mid));
        return PZ_OK;
    }
    // one product term (i, j): convolution -> inverse transform in place -> normalize(res_base2k, cnv_offset_lo) into `dst` column dcol
    int term(int i, int j, int64_t* dst, long long dst_bs, int dst_cols, int dcol, const NzCombine* cb = nullptr, const TailD16* d16s = nullptr) {
        const int bound = t.a_size + t.b_size - 1;
        const int min_size = std::min(t.dft_size, bound), off = std::min(t.hi, bound);
        if (fused) {
            const cplx* Tt = T;
            if (all3) Tt = T + (size_t)(i == j ? i : 2) * nb * min_size * (size_t)M->m;
            else {
                mid.col_i = i; mid.col_j = i == j ? -1 : j;
                PZ_TRY(launch_mid_cnv(M, nb, mid));
            }
            // the inverse column pass normalizes on its way out (bit offset, combination and all: TailArgs::nz)
            return launch_inv_tail_nz(M, nb, NzTailCall{Tt, min_size, (long long*)dst, dst_bs, dst_cols, t.res_size, dcol, (int)p->res_base2k, t.lo, t.dft_size, cb, d16s});
        }
        PZ_TRY(launch_cnv_apply(M, nb, rd, rd_bs, 1, 0, min_size, off, pa, pa_bs, t.a_size, i, i == j ? -1 : j, pb, pb_bs, t.b_size, i, i == j ? -1 : j));
        if (t.dft_size > min_size)
            PZ_TRY(launch_ew(M, EW_ZERO, rd + (long long)min_size * n, rd_bs, n, nullptr, 0, 0, nullptr, 0, 0, t.dft_size - min_size, nb));
        DV dv{rd, rd_bs, 1, t.dft_size};
        PZ_TRY(dev_idft(M, nb, dv, 0, dv, 0, 1, t.dft_size, T));
        DV out{dst, dst_bs, dst_cols, t.res_size};
        return dev_normalize(M, nb, out, (int)p->res_base2k, t.lo, dcol, dv, (int)p->ab_base2k, 0, cb);
    }
    int64_t* col_ptr(int col) const { return rb + (long long)col * n; }
    int ew_res(int op, int col, const int64_t* x, long long x_bs, long long x_ls, const int64_t* y, long long y_bs, long long y_ls) {
        return launch_ew(M, op, col_ptr(col), r_ct, rls, x, x_bs, x_ls, y, y_bs, y_ls, t.res_size, nb);
    }
    int cidx(int i, int j) const { const int lo_ = std::min(i, j), hi_ = std::max(i, j); return lo_ * t.cols - (lo_ * (lo_ + 1) / 2) + hi_; }

    // One base2k, rank <= 2 (round 3): the digits of a term go straight from the normalizing store into every tensor column that takes them.
    // apply / square: the diagonal terms are stored, each pairwise term then reads the two diagonal columns it belongs to and stores
    // pair - d_i - d_j (mode 5: one write per column, no read-modify-write; wrapping i64: the same digits as the reference's order).
    // add_assign: the diagonal term goes into its column (+=) and out of the cross columns (-=), the pairwise term into its cross column (+=)
    int combine_in_stores() {
        if (!add && t16) {
            const long long ts = t16_cs;   // one tensor column
            for (int i = 0; i < t.cols; ++i) {
                NzCombine cb{1, {0, 0}, {0, 0}};
                TailD16 dw;
                dw.w = t16 + cidx(i, i) * ts; dw.only = true;
                PZ_TRY(term(i, i, rb, r_ct, t.tcols, cidx(i, i), &cb, &dw));
            }
            for (int i = 0; i < t.cols; ++i)
                for (int j = i + 1; j < t.cols; ++j) {
                    NzCombine cb{1, {cidx(i, i), cidx(j, j)}, {5, 5}};
                    TailD16 dr;
                    dr.ra = t16 + cidx(i, i) * ts; dr.rb = t16 + cidx(j, j) * ts; dr.w = t16 + cidx(i, j) * ts; dr.only = true;
                    PZ_TRY(term(i, j, rb, r_ct, t.tcols, cidx(i, j), &cb, &dr));
                }
            return PZ_OK;
        }
        if (!add) {
            // the diagonal launches leave 16-bit copies of their digits beside the tensor columns (base2k <= 16, fused tails): the pairwise
            // launches read those - 2 B per coefficient and diagonal column instead of the 8 B a line of the i64 column costs
            const bool use16 = d16 != nullptr && fused;
            const long long d16_ts = (long long)nb * t.res_size * n;   // one diagonal term's copies
            for (int i = 0; i < t.cols; ++i) {
                NzCombine cb{1, {0, 0}, {0, 0}};
                TailD16 dw;
                dw.w = use16 ? d16 + i * d16_ts : nullptr;
                PZ_TRY(term(i, i, rb, r_ct, t.tcols, cidx(i, i), &cb, use16 ? &dw : nullptr));
            }
            for (int i = 0; i < t.cols; ++i)
                for (int j = i + 1; j < t.cols; ++j) {
                    NzCombine cb{1, {cidx(i, i), cidx(j, j)}, {5, 5}};
                    TailD16 dr;
                    dr.ra = use16 ? d16 + i * d16_ts : nullptr; dr.rb = use16 ? d16 + j * d16_ts : nullptr;
                    PZ_TRY(term(i, j, rb, r_ct, t.tcols, cidx(i, j), &cb, use16 ? &dr : nullptr));
                }
            return PZ_OK;
        }
        for (int i = 0; i < t.cols; ++i) {
            NzCombine cb{3, {0, 0}, {0, 0}};
            int u = 0;
            for (int j = 0; j < t.cols; ++j) {
                if (j == i) continue;
                cb.col2[u] = cidx(i, j);
                cb.mode2[u] = 4;
                ++u;
            }
            PZ_TRY(term(i, i, rb, r_ct, t.tcols, cidx(i, i), &cb));
        }
        for (int i = 0; i < t.cols; ++i)
            for (int j = i + 1; j < t.cols; ++j) {
                NzCombine cb{3, {0, 0}, {0, 0}};
                PZ_TRY(term(i, j, rb, r_ct, t.tcols, cidx(i, j), &cb));
            }
        return PZ_OK;
    }
    // glwe_tensor_square_apply in the reference's order (:651-697): diagonal terms kept aside, each pairwise term minus its two diagonals
    int square_reference_order() {
        for (int i = 0; i < t.cols; ++i) {
            PZ_TRY(term(i, i, diag, dg_bs, t.cols, i));
            PZ_TRY(ew_res(EW_COPY, cidx(i, i), diag + (long long)i * n, dg_bs, (long long)t.cols * n, nullptr, 0, 0));
        }
        for (int i = 0; i < t.cols; ++i)
            for (int j = i + 1; j < t.cols; ++j) {
                const int c = cidx(i, j);
                PZ_TRY(term(i, j, rb, r_ct, t.tcols, c));
                PZ_TRY(ew_res(EW_SUB_I64, c, col_ptr(c), r_ct, rls, diag + (long long)i * n, dg_bs, (long long)t.cols * n));
                PZ_TRY(ew_res(EW_SUB_I64, c, col_ptr(c), r_ct, rls, diag + (long long)j * n, dg_bs, (long long)t.cols * n));
            }
        return PZ_OK;
    }
    // glwe_tensor_apply / _add_assign in the reference's order (:762-805 / :870-890): a temporary per term, element-wise passes over the tensor
    int apply_reference_order() {
        for (int i = 0; i < t.cols; ++i) {
            PZ_TRY(term(i, i, tmp, tmp_bs, 1, 0));
            if (add) PZ_TRY(ew_res(EW_ADD_I64, cidx(i, i), col_ptr(cidx(i, i)), r_ct, rls, tmp, tmp_bs, n));
            else PZ_TRY(ew_res(EW_COPY, cidx(i, i), tmp, tmp_bs, n, nullptr, 0, 0));
            for (int j = 0; j < t.cols; ++j) {
                if (j == i) continue;
                const int c = cidx(i, j);
                if (j < i || add) PZ_TRY(ew_res(EW_SUB_I64, c, col_ptr(c), r_ct, rls, tmp, tmp_bs, n));
                else PZ_TRY(ew_res(EW_NEG_I64, c, tmp, tmp_bs, n, nullptr, 0, 0));
            }
        }
        for (int i = 0; i < t.cols; ++i)
            for (int j = i + 1; j < t.cols; ++j) {
                PZ_TRY(term(i, j, tmp, tmp_bs, 1, 0));
                PZ_TRY(ew_res(EW_ADD_I64, cidx(i, j), col_ptr(cidx(i, j)), r_ct, rls, tmp, tmp_bs, n));
            }
        return PZ_OK;
    }
};

// a_cs / b_cs: i64 elements between consecutive ciphertexts of a / b, 0: packed (TensorWave::a_cs)
static int tensor_apply_nolock(pz_module* M, int64_t* res, const int64_t* a, const int64_t* b, const pz_glwe_tensor_params* p, int mode, size_t batch,
                               long long a_cs = 0, long long b_cs = 0);
int pz_glwe_tensor_apply_batched(pz_module* M, int64_t* res, const int64_t* a, const int64_t* b, const pz_glwe_tensor_params* p, int mode,
                                 size_t batch) {
    PZ_ENTER(M);
    return tensor_apply_nolock(M, res, a, b, p, mode, batch);
}
static int tensor_apply_nolock(pz_module* M, int64_t* res, const int64_t* a, const int64_t* b, const pz_glwe_tensor_params* p, int mode, size_t batch,
                               long long a_cs, long long b_cs) {
    TensorPlan t;
    PZ_TRY(tensor_plan(M, p, mode, t));
    const bool square = mode == PZ_TENSOR_SQUARE;
    if (square) b = a;
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a) && is_device_ptr(b), "batched entry points take device pointers");
    PZ_REQUIRE((const void*)res != (const void*)a && (const void*)res != (const void*)b, "glwe_tensor_apply: res must not alias an operand");
    if (batch == 0) return PZ_OK;
    TensorWave w;
    w.M = M; w.p = p; w.t = t; w.square = square; w.add = mode == PZ_TENSOR_APPLY_ADD_ASSIGN; w.n = (long long)M->n;
    const size_t chunk = tensor_chunk(M, t, batch);
    PZ_TRY(w.take_workspace(chunk));
    w.a_cs = a_cs; w.b_cs = b_cs;
    const long long a_ct = a_cs ? a_cs : w.n * t.cols * t.a_size, b_ct = b_cs ? b_cs : w.n * t.cols * t.b_size;
    for (size_t b0 = 0; b0 < batch; b0 += chunk) {
        w.nb = (int)std::min(chunk, batch - b0);
        w.rb = res + (long long)b0 * w.r_ct;
        PZ_TRY(w.prepare(a + (long long)b0 * a_ct, b + (long long)b0 * b_ct));
        // where the digits of a term can go straight from the normalizing store into every tensor column that takes them (one base2k,
        // rank <= 2; POULPY_DBG_TENSOR_COMBINE=0: the reference's own order of element-wise passes)
        static const bool combine_env = (rt_knob("POULPY_DBG_TENSOR_COMBINE", 1) != 0);
        if (combine_env && p->res_base2k == p->ab_base2k && t.cols <= 3) PZ_TRY(w.combine_in_stores());
        else if (square) PZ_TRY(w.square_reference_order());
        else PZ_TRY(w.apply_reference_order());
    }
    return PZ_OK;
}

}  // extern "C"

namespace {

// what pz_glwe_tensor_mul_relinearize_acc_batched adds to the one-call product; null: pz_glwe_tensor_mul_relinearize_batched itself
struct MulAcc {
    size_t a_stride, b_stride;   // limbs per ciphertext of the operand containers, 0: the operand's size
    int accumulate, join;
    size_t k;
    int sign, normalize;
};
// everything the one-call product derives from its shapes before it launches anything
struct MulRelinPlan {
    TensorPlan t;
    bool compact;                // the tensor as 16-bit digits in tile order
    size_t chunk;
    long long t16_cs;            // int16 elements between the tensor columns of a wave (compact)
    size_t tensor_bytes;         // ws2: the tensor of a wave ...
    size_t prod_bytes;           // ... and, behind it, the product of a wave (accumulate)
};
int mul_relin_plan(const pz_module* M, const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, int mode, bool accumulate, size_t batch, MulRelinPlan& q) {
    PZ_REQUIRE(mode == PZ_TENSOR_APPLY || mode == PZ_TENSOR_SQUARE, "glwe_tensor_mul_relinearize: mode is apply or square");
    PZ_TRY(tensor_plan(M, tp, mode, q.t));
    const TensorPlan& t = q.t;
    PZ_REQUIRE(rp != nullptr, "null params");
    PZ_REQUIRE(rp->rank == tp->rank && rp->rank_out == rp->rank, "glwe_tensor_mul_relinearize: the tensor key maps rank (rank + 1) / 2 -> rank");
    PZ_REQUIRE(rp->a_size == tp->res_size && rp->a_base2k == tp->res_base2k, "glwe_tensor_mul_relinearize: (a_size, a_base2k) of the relinearization describe the tensor");
    static const bool combine_env = (rt_knob("POULPY_DBG_TENSOR_COMBINE", 1) != 0), fused_env = (rt_knob("POULPY_DBG_TENSOR_FUSED", 1) != 0);
    q.compact = combine_env && fused_env && tp->res_base2k <= 14 && tp->res_base2k == tp->ab_base2k && t.cols <= 3 && t.dft_size >= 1 &&
                mid_cnv_supported(M, t.a_size, t.b_size, std::min(t.dft_size, t.a_size + t.b_size - 1)) && glwe_relin_t16_supported(M, rp);
    q.chunk = std::min(tensor_chunk(M, t, batch), glwe_relin_chunk(M, rp, batch));
    // the tensor of a wave: ws2 (the two halves of the call carve the main workspace one after the other).  16-bit form: the columns of a wave
    // sit a fraction of the 4 MiB channel interleave out of phase - the pairwise tail reads two columns and writes the third at the same offset,
    // the relinearization's tail reads one beside its spectrum and result streams (as T2' against the result, kT2Phase in api_glwe.hip)
    static constexpr long long t16_phase = 768 * 1024 / 2;
    q.t16_cs = (long long)q.chunk * t.res_size * (long long)M->n + t16_phase;
    const size_t tensor_ct = (size_t)M->n * t.tcols * t.res_size;
    q.tensor_bytes = q.compact ? (size_t)q.t16_cs * t.tcols * 2 : q.chunk * tensor_ct * 8;
    q.prod_bytes = accumulate ? q.chunk * (size_t)M->n * t.cols * (size_t)rp->res_size * 8 : 0;
    return PZ_OK;
}
bool ranges_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const char *a = (const char*)p, *b = (const char*)q;
    return a < b + qn && b < a + pn;
}
// the join of a wave's product (in the workspace) to res: pz_glwe_sum_batched's two-term chain - term 0 res in place, term 1 the product
// with (join, k, sign) - or, un-normalized, the same two terms through pz_glwe_combine_batched's kernel
int mul_acc_join(pz_module* M, int64_t* res, const int64_t* prod, const pz_glwe_op_params* rp, const MulAcc& ap, size_t nb, bool dry) {
    const size_t cols = rp->rank + 1, size = rp->res_size, base2k = rp->res_base2k;
    const int64_t* ops[2] = {res, prod};
    if (ap.normalize) {
        const int shared[2] = {0, 0}, join[2] = {PZ_JOIN_PLAIN, ap.join}, sign[2] = {1, ap.sign};
        const size_t a_size[2] = {size, size}, k[2] = {0, ap.k};
        return glwe_sum_nolock(M, res, cols, size, base2k, ops, shared, a_size, join, k, sign, 2, nb, dry);
    }
    const bool acc = ap.join == PZ_JOIN_LSH_ACC, term = ap.join == PZ_JOIN_LSH_TERM;
    const pz_glwe_term terms[2] = {{size, acc ? ap.k : 0, base2k, acc ? PZ_TERM_LSH : PZ_TERM_RAW, 1, 0, 0},
                                   {size, term ? ap.k : 0, base2k, term ? PZ_TERM_LSH : PZ_TERM_RAW, ap.sign, 0, 0}};
    return glwe_combine_nolock(M, res, cols, size, base2k, ops, terms, 2, 0, nb, dry);
}

// glwe_tensor_apply (or _square_apply) followed by glwe_tensor_relinearize with the GLWETensor in scratch - poulpy-ckks's multiplication
// (poulpy-ckks/src/leveled/default/mul.rs:49-85 ckks_mul_into_default, :131-170 the square: `tmp` is taken from the scratch space, filled by
// glwe_tensor_apply and consumed by glwe_tensor_relinearize; operations/glwe.rs:609-913 and :541-607).  The tensor never reaches the caller, so
// where its digits fit 16 bits (one base2k <= 14 throughout, pipeline plans) it only ever exists as int16 copies in the tails' own tile
// order: the tensoring tails write 2 B per coefficient instead of 8, the relinearization's forward pass and tail read 2 B instead of 8
// (9.6 GB less HBM traffic per 256 multiplications at N = 2^16, 16 limbs).  Everywhere else: the i64 tensor in the workspace, the two calls as they are.
// ap (pz_glwe_tensor_mul_relinearize_acc_batched): strided operands, the alias rule, the product joined to res wave by wave.
int mul_relin_run(pz_module* M, int64_t* res, const int64_t* a, const int64_t* b, const double* tsk_pmat, const pz_glwe_tensor_params* tp,
                  const pz_glwe_op_params* rp, const MulAcc* ap, int mode, size_t batch) {
    const bool accumulate = ap && ap->accumulate;
    MulRelinPlan q;
    PZ_TRY(mul_relin_plan(M, tp, rp, mode, accumulate, batch, q));
    const TensorPlan& t = q.t;
    const bool square = mode == PZ_TENSOR_SQUARE;
    if (square) b = a;
    const long long n = (long long)M->n;
    size_t a_stride = t.a_size, b_stride = t.b_size;
    if (ap) {
        PZ_REQUIRE(batch <= (size_t)1 << 24, "glwe_tensor_mul_relinearize_acc: batch out of range");
        PZ_REQUIRE(ap->accumulate == 0 || ap->accumulate == 1, "glwe_tensor_mul_relinearize_acc: accumulate must be 0 or 1");
        if (ap->a_stride) a_stride = ap->a_stride;
        if (square) b_stride = a_stride;
        else if (ap->b_stride) b_stride = ap->b_stride;
        PZ_REQUIRE(a_stride >= (size_t)t.a_size && b_stride >= (size_t)t.b_size && a_stride <= 4096 && b_stride <= 4096,
                   "glwe_tensor_mul_relinearize_acc: a stride (%zu, %zu limbs) is below the operand's size (%d, %d) or out of range", a_stride, b_stride,
                   t.a_size, t.b_size);
        if (accumulate) {
            PZ_REQUIRE(ap->join == PZ_JOIN_PLAIN || ap->join == PZ_JOIN_LSH_TERM || ap->join == PZ_JOIN_LSH_ACC, "glwe_tensor_mul_relinearize_acc: unknown join");
            PZ_REQUIRE(ap->sign == 1 || ap->sign == -1, "glwe_tensor_mul_relinearize_acc: sign must be +1 or -1");
            PZ_REQUIRE(ap->normalize == 0 || ap->normalize == 1, "glwe_tensor_mul_relinearize_acc: normalize must be 0 or 1");
            PZ_REQUIRE(ap->join == PZ_JOIN_PLAIN ? ap->k == 0 : ap->k <= ((size_t)1 << 40), "glwe_tensor_mul_relinearize_acc: shift out of range (a plain join takes k = 0)");
        }
    }
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a) && is_device_ptr(b) && is_device_ptr(tsk_pmat), "batched entry points take device pointers");
    const long long a_ct = n * t.cols * (long long)a_stride, b_ct = n * t.cols * (long long)b_stride, res_ct = n * t.cols * (long long)rp->res_size;
    if (ap) {
        // Only pass 1 of a wave reads the operands, and it is issued in front of every kernel of the wave that stores (the relinearization's
        // tail alone writes caller memory).  With res == an operand at equal strides wave w stores exactly the ciphertexts it has read and
        // later waves read other ones: no case needs staging.  At unequal strides wave w's stores would reach ciphertexts a later wave
        // still reads - refused, like every partial overlap.
        const size_t res_ext = batch * (size_t)res_ct * 8;
        const struct { const int64_t* p; size_t stride, ext; const char* name; } opnd[2] = {{a, a_stride, batch * (size_t)a_ct * 8, "a"}, {b, b_stride, batch * (size_t)b_ct * 8, "b"}};
        for (int u = 0; u < (square ? 1 : 2); ++u) {
            const bool same = (const void*)opnd[u].p == (const void*)res && opnd[u].stride == rp->res_size && !accumulate;
            if (!same && batch > 0 && ranges_overlap(opnd[u].p, opnd[u].ext, res, res_ext))
                return fail(PZ_ERR_ALIAS, "glwe_tensor_mul_relinearize_acc: res overlaps %s (accumulate = 0 takes res == %s at a stride of res_size limbs)", opnd[u].name, opnd[u].name);
        }
    }
    if (batch == 0) return PZ_OK;
    PZ_TRY(ws2_reserve(M, accumulate ? align256(q.tensor_bytes) + q.prod_bytes : q.tensor_bytes));
    void* tensor = M->ws2;
    int64_t* prod = nullptr;
    if (accumulate) {   // (the plain product keeps the tensor at the head of ws2, without a segment of its own, as before)
        char* base = (char*)M->ws2;
        PZ_TRY(ws_take(M, base, align256(q.tensor_bytes), &tensor));
        PZ_TRY(ws_take(M, base, q.prod_bytes, &prod));
        PZ_TRY(mul_acc_join(M, res, prod, rp, *ap, std::min(q.chunk, batch), true));   // what the join would refuse, before anything is launched
    }
    if (q.compact) dispatch_note(M, "glwe_tensor_mul_relinearize: 16-bit tensor in tile order");
    auto waves = [&]() -> int {
        TensorWave w;
        w.M = M; w.p = tp; w.t = t; w.square = square; w.add = false; w.n = n;
        w.a_cs = a_ct; w.b_cs = b_ct;
        for (size_t b0 = 0; b0 < batch; b0 += q.chunk) {
            const size_t nb = std::min(q.chunk, batch - b0);
            int64_t* rw = res + (long long)b0 * res_ct;
            int64_t* r0 = accumulate ? prod : rw;
            if (!q.compact) {
                // (not through the public entry points: the module lock is held)
                PZ_TRY(tensor_apply_nolock(M, (int64_t*)tensor, a + (long long)b0 * a_ct, b + (long long)b0 * b_ct, tp, mode, nb, a_ct, b_ct));
                PZ_TRY(glwe_op(M, GlweKind::TensorRelin, r0, (const int64_t*)tensor, tsk_pmat, rp, nb));
            } else {
                PZ_TRY(w.take_workspace(nb));
                w.nb = (int)nb; w.rb = nullptr; w.t16 = (short*)tensor; w.t16_cs = q.t16_cs;
                PZ_TRY(w.prepare(a + (long long)b0 * a_ct, b + (long long)b0 * b_ct));
                PZ_REQUIRE(w.fused, "glwe_tensor_mul_relinearize: the fused tensoring path was expected here");
                PZ_TRY(w.combine_in_stores());
                PZ_TRY(glwe_relin_t16(M, r0, (const short*)tensor, q.t16_cs, tsk_pmat, rp, nb));
            }
            if (accumulate) PZ_TRY(mul_acc_join(M, rw, prod, rp, *ap, nb, false));
        }
        return PZ_OK;
    };
    if (!ap) return waves();
    // kernel nodes only: a call repeated with the same arguments replays as one graph
    KeyHash key = graph_key(M, GRAPH_TENSOR_MUL_ACC, res, a, b, tsk_pmat, *tp, *rp, a_stride, b_stride, ap->accumulate, mode, batch);
    if (accumulate) { key.add(ap->join); key.add(ap->k); key.add(ap->sign); key.add(ap->normalize); }
    return with_graph(M, key.h, waves);
}

// everything pz_glwe_tensor_dot_relinearize_batched derives from its shapes before it launches anything
struct DotRelinPlan {
    MulRelinPlan q;              // the one-call product of one pair: shapes, chunk, the 16-bit column stride
    DotTensorForm form;          // of the accumulated tensor of a wave (dot_form.hpp)
    int group;                   // 16-bit form: term tensors beside the accumulated one = terms of one k_t16_sum launch
    size_t tensor_bytes;         // one tensor of a wave in its form
    size_t slot_bytes;           // 16-bit form: bytes between the tensors of a wave in ws2
    size_t ws2_bytes;
};
// 16-bit form: the accumulated tensor and the term tensors of a wave start a multiple of the 4 MiB channel interleave plus s x 832 KiB apart
// (s = 0 .. 4): k_t16_sum streams all of them at one (column, offset), five streams 832 KiB apart modulo 4 MiB.  The columns inside a tensor
// keep their own 768 KiB (mul_relin_plan: t16_phase), which is what a tail - three columns of ONE tensor at one offset - streams.  (The launches
// of a wave run one after the other on the module stream: no kernel streams two tensors at two columns.)
constexpr size_t kDotChannel = (size_t)4 << 20, kDotSlotPhase = (size_t)832 << 10;
int dot_relin_plan(const pz_module* M, const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, size_t npairs, size_t batch, DotRelinPlan& d) {
    PZ_REQUIRE(npairs >= 1 && npairs <= kDotMaxPairs, "glwe_tensor_dot_relinearize: %zu pairs (1 .. %zu per call)", npairs, kDotMaxPairs);
    PZ_TRY(mul_relin_plan(M, tp, rp, PZ_TENSOR_APPLY, false, batch, d.q));
    d.form = dot_tensor_form(npairs, tp->res_base2k, d.q.compact);
    const TensorPlan& t = d.q.t;
    if (d.form == DOT_TENSOR_T16) {
        d.group = dot_sum_group(npairs);
        d.tensor_bytes = (size_t)d.q.t16_cs * t.tcols * 2;
        d.slot_bytes = (d.tensor_bytes + kDotChannel - 1) / kDotChannel * kDotChannel + kDotSlotPhase;
        d.ws2_bytes = (size_t)d.group * d.slot_bytes + align256(d.tensor_bytes);
    } else {
        d.group = 0;
        d.tensor_bytes = d.q.chunk * (size_t)M->n * t.tcols * t.res_size * 8;
        d.slot_bytes = 0;
        d.ws2_bytes = d.tensor_bytes;
    }
    return PZ_OK;
}

// glwe_tensor_apply on pair 0, glwe_tensor_apply_add_assign on every further pair - all into ONE GLWETensor - and one
// glwe_tensor_relinearize: the fast branch of poulpy-ckks's ckks_dot_product_ct (leveled/delegates/composite.rs:671-699; poulpy-core
// operations/glwe.rs:700-917, :541-607).  The accumulated tensor of a wave lives in ws2.
//   i64 form: tensor_apply_nolock per pair (PZ_TENSOR_APPLY, then PZ_TENSOR_APPLY_ADD_ASSIGN) into the wave's i64 tensor, then the i64
//     relinearization, which reads the un-normalized limbs as they are.
//   16-bit form (dot_form.hpp: compact shapes, every accumulated value inside int16): pair 0 through the one-call product's own launches into
//     the accumulated 16-bit tensor, every later pair through the same launches into a term tensor, k_t16_sum adds up to four term tensors
//     per launch, glwe_relin_t16 reads the accumulated tensor.  glwe_relin_t16 takes any int16: its forward pass converts the value to f64, its
//     tail (k_inv_tail's ACC32 form, acc32 bit 2) sign-extends it into the 64-bit carry chain - neither uses |digit| <= 2^(base2k-1); the
//     tensoring tails, whose side-copy forms are compiled as "normalizing, never raw", run per pair exactly as in the one-call product.
int dot_relin_run(pz_module* M, int64_t* res, const int64_t* const* a, const int64_t* const* b, size_t npairs, const size_t* a_stride,
                  const size_t* b_stride, const double* tsk_pmat, const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, size_t batch) {
    DotRelinPlan d;
    PZ_TRY(dot_relin_plan(M, tp, rp, npairs, batch, d));
    const MulRelinPlan& q = d.q;
    const TensorPlan& t = q.t;
    const long long n = (long long)M->n;
    PZ_REQUIRE(a != nullptr && b != nullptr, "glwe_tensor_dot_relinearize: null operand list");
    PZ_REQUIRE(batch <= (size_t)1 << 24, "glwe_tensor_dot_relinearize: batch out of range");
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(tsk_pmat), "batched entry points take device pointers");
    long long a_ct[kDotMaxPairs], b_ct[kDotMaxPairs];
    size_t as[kDotMaxPairs], bs[kDotMaxPairs];
    const long long res_ct = n * t.cols * (long long)rp->res_size;
    for (size_t i = 0; i < npairs; ++i) {
        as[i] = a_stride && a_stride[i] ? a_stride[i] : (size_t)t.a_size;
        bs[i] = b_stride && b_stride[i] ? b_stride[i] : (size_t)t.b_size;
        PZ_REQUIRE(as[i] >= (size_t)t.a_size && bs[i] >= (size_t)t.b_size && as[i] <= 4096 && bs[i] <= 4096,
                   "glwe_tensor_dot_relinearize: pair %zu: a stride (%zu, %zu limbs) is below the operand's size (%d, %d) or out of range", i, as[i], bs[i],
                   t.a_size, t.b_size);
        PZ_REQUIRE(is_device_ptr(a[i]) && is_device_ptr(b[i]), "batched entry points take device pointers");
        a_ct[i] = n * t.cols * (long long)as[i];
        b_ct[i] = n * t.cols * (long long)bs[i];
    }
    // res is written by the relinearization of wave w while later waves still read every operand: no overlap with any of the 2 npairs ranges
    for (size_t i = 0; i < npairs && batch > 0; ++i)
        if (ranges_overlap(a[i], batch * (size_t)a_ct[i] * 8, res, batch * (size_t)res_ct * 8) ||
            ranges_overlap(b[i], batch * (size_t)b_ct[i] * 8, res, batch * (size_t)res_ct * 8))
            return fail(PZ_ERR_ALIAS, "glwe_tensor_dot_relinearize: res overlaps an operand of pair %zu", i);
    if (batch == 0) return PZ_OK;
    PZ_TRY(ws2_reserve(M, d.ws2_bytes));
    const bool t16 = d.form == DOT_TENSOR_T16;
    short *acc16 = nullptr, *term16[kDotSumTerms] = {};
    int64_t* acc64 = nullptr;
    {
        char* base = (char*)M->ws2;
        if (t16) {
            PZ_TRY(ws_take(M, base, align256(d.tensor_bytes), &acc16));
            char* slot = (char*)M->ws2;
            for (int s = 0; s < d.group; ++s) {
                slot += d.slot_bytes;
                base = std::max(base, slot);
                PZ_TRY(ws_take(M, base, align256(d.tensor_bytes), &term16[s]));
            }
        } else PZ_TRY(ws_take(M, base, d.tensor_bytes, &acc64));
    }
    dispatch_note(M, t16 ? "glwe_tensor_dot_relinearize: 16-bit accumulated tensor, term tensors summed by k_t16_sum" : "glwe_tensor_dot_relinearize: i64 accumulated tensor");
    auto waves = [&]() -> int {
        TensorWave w;
        w.M = M; w.p = tp; w.t = t; w.square = false; w.add = false; w.n = n;
        for (size_t b0 = 0; b0 < batch; b0 += q.chunk) {
            const size_t nb = std::min(q.chunk, batch - b0);
            int64_t* rw = res + (long long)b0 * res_ct;
            if (!t16) {
                // (not through the public entry points: the module lock is held)
                for (size_t i = 0; i < npairs; ++i)
                    PZ_TRY(tensor_apply_nolock(M, acc64, a[i] + (long long)b0 * a_ct[i], b[i] + (long long)b0 * b_ct[i], tp,
                                               i == 0 ? PZ_TENSOR_APPLY : PZ_TENSOR_APPLY_ADD_ASSIGN, nb, a_ct[i], b_ct[i]));
                PZ_TRY(glwe_op(M, GlweKind::TensorRelin, rw, acc64, tsk_pmat, rp, nb));
                continue;
            }
            PZ_TRY(w.take_workspace(nb));
            w.nb = (int)nb; w.rb = nullptr; w.t16_cs = q.t16_cs;
            for (size_t i = 0; i < npairs; ++i) {
                const int slot = i == 0 ? -1 : (int)((i - 1) % (size_t)d.group);
                w.t16 = slot < 0 ? acc16 : term16[slot];
                w.a_cs = a_ct[i]; w.b_cs = b_ct[i];
                PZ_TRY(w.prepare(a[i] + (long long)b0 * a_ct[i], b[i] + (long long)b0 * b_ct[i]));
                PZ_REQUIRE(w.fused, "glwe_tensor_dot_relinearize: the fused tensoring path was expected here");
                PZ_TRY(w.combine_in_stores());
                if (slot >= 0 && (slot == d.group - 1 || i == npairs - 1))
                    PZ_TRY(launch_t16_sum(M, acc16, term16, slot + 1, t.tcols, (long long)nb * t.res_size * n, q.t16_cs));
            }
            PZ_TRY(glwe_relin_t16(M, rw, acc16, q.t16_cs, tsk_pmat, rp, nb));
        }
        return PZ_OK;
    };
    // kernel nodes only: a call repeated with the same arguments replays as one graph
    KeyHash key = graph_key(M, GRAPH_TENSOR_DOT, res, npairs, tsk_pmat, *tp, *rp, batch);
    for (size_t i = 0; i < npairs; ++i) { key.add(a[i]); key.add(b[i]); key.add(as[i]); key.add(bs[i]); }
    return with_graph(M, key.h, waves);
}

}  // namespace

extern "C" {

int pz_glwe_tensor_mul_relinearize_batched(pz_module* M, int64_t* res, const int64_t* a, const int64_t* b, const double* tsk_pmat,
                                           const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, int mode, size_t batch) {
    PZ_ENTER(M);
    return mul_relin_run(M, res, a, b, tsk_pmat, tp, rp, nullptr, mode, batch);
}

// The one-call product on strided operands, in place, or joined to res wave by wave (include/poulpy_hip.h): the plans of
// poulpy-ckks's ckks_mul_* / ckks_square_* / ckks_mul_add_ct_into / ckks_mul_sub_ct_into / ckks_mul_many (poulpy_amd/ckks.py)
int pz_glwe_tensor_mul_relinearize_acc_batched(pz_module* M, int64_t* res, const int64_t* a, const int64_t* b, const double* tsk_pmat,
                                               const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, size_t a_stride, size_t b_stride,
                                               int accumulate, int join, size_t k, int sign, int normalize, int mode, size_t batch) {
    PZ_ENTER(M);
    const MulAcc ap{a_stride, b_stride, accumulate, join, k, sign, normalize};
    return mul_relin_run(M, res, a, b, tsk_pmat, tp, rp, &ap, mode, batch);
}
// the module's two workspaces as that call sizes them: the larger of the tensoring's and the relinearization's carve of the main one, and
// the tensor of a wave with (accumulate) the product of a wave behind it
size_t pz_glwe_tensor_mul_relinearize_acc_workspace_bytes(const pz_module* M, const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp,
                                                          int accumulate, int mode, size_t batch) {
    MulRelinPlan q;
    if (!M || mul_relin_plan(M, tp, rp, mode, accumulate != 0, std::max<size_t>(batch, 1), q) != PZ_OK) return 0;
    const size_t main_ws = std::max(q.chunk * (q.t.per_ct + 6 * 256), pz_glwe_op_workspace_bytes(M, rp, q.chunk, (int)GlweKind::TensorRelin));
    return main_ws + kGuardSlack + align256(q.tensor_bytes) + q.prod_bytes + kGuardSlack;
}

// Sum of npairs tensor products in ONE accumulated GLWETensor, relinearized once (include/poulpy_hip.h): the fast branch of
// poulpy-ckks's ckks_dot_product_ct (poulpy_amd/ckks.py plan_dot_product_ct)
int pz_glwe_tensor_dot_relinearize_batched(pz_module* M, int64_t* res, const int64_t* const* a, const int64_t* const* b, size_t npairs,
                                           const size_t* a_stride, const size_t* b_stride, const double* tsk_pmat, const pz_glwe_tensor_params* tp,
                                           const pz_glwe_op_params* rp, size_t batch) {
    PZ_ENTER(M);
    return dot_relin_run(M, res, a, b, npairs, a_stride, b_stride, tsk_pmat, tp, rp, batch);
}
// the module's two workspaces as that call sizes them: the larger of the tensoring's and the relinearization's carve of the main one, and
// the accumulated tensor of a wave with (16-bit form) its term tensors behind it
size_t pz_glwe_tensor_dot_relinearize_workspace_bytes(const pz_module* M, const pz_glwe_tensor_params* tp, const pz_glwe_op_params* rp, size_t npairs,
                                                      size_t batch) {
    DotRelinPlan d;
    if (!M || dot_relin_plan(M, tp, rp, npairs, std::max<size_t>(batch, 1), d) != PZ_OK) return 0;
    const size_t main_ws = std::max(d.q.chunk * (d.q.t.per_ct + 6 * 256), pz_glwe_op_workspace_bytes(M, rp, d.q.chunk, (int)GlweKind::TensorRelin));
    return main_ws + kGuardSlack + d.ws2_bytes + kGuardSlack;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// Batched i64 VecZnx family: the limb-wise operations poulpy-core runs between the
// hot-path calls (glwe_add / sub / negate / copy / rotate / normalize / lsh / rsh), on `batch` device-resident containers laid
// out back to back — one launch per limb range instead of one call per ciphertext.  Same limb-range rules as the per-container
// entry points (reference/vec_znx/{add,sub,negate,copy,rotate,shift}.rs).
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct BV {   // a batched device container
    DV v;
    int col;
};
inline DV dvb(const pz_module* M, const void* p, size_t cols, size_t size) { return DV{(void*)p, (long long)(M->n * cols * size), (int)cols, (int)size}; }
inline int ewb(pz_module* M, int op, int batch, const DV& r, int rcol, int rl0, const DV* a, int acol, int al0, const DV* b, int bcol, int bl0, int nl) {
    return launch_ew(M, op, poly_ptr(M, r, rcol, rl0), r.bs, limb_stride(M, r), a ? poly_ptr(M, *a, acol, al0) : nullptr, a ? a->bs : 0,
                     a ? limb_stride(M, *a) : 0, b ? poly_ptr(M, *b, bcol, bl0) : nullptr, b ? b->bs : 0, b ? limb_stride(M, *b) : 0, nl, batch);
}
int check_batched(const pz_module* M, const void* res, const void* a, const void* b, size_t res_col, size_t res_cols, size_t a_col,
                  size_t a_cols, size_t b_col, size_t b_cols) {
    (void)M;
    PZ_CHECK_COL(res_col, res_cols, "vec_znx_*_batched(res)");
    if (a) PZ_CHECK_COL(a_col, a_cols, "vec_znx_*_batched(a)");
    if (b) PZ_CHECK_COL(b_col, b_cols, "vec_znx_*_batched(b)");
    PZ_REQUIRE(is_device_ptr(res) && (!a || is_device_ptr(a)) && (!b || is_device_ptr(b)), "batched entry points take device pointers");
    return PZ_OK;
}
// res = a +- b  (add.rs:6-65, sub.rs:6-58)
int add_sub_batched(pz_module* M, bool sub, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                    size_t a_cols, size_t a_size, size_t a_col, const int64_t* b, size_t b_cols, size_t b_size, size_t b_col) {
    PZ_TRY(check_batched(M, res, a, b, res_col, res_cols, a_col, a_cols, b_col, b_cols));
    PZ_REQUIRE((const void*)res != (const void*)b, "vec_znx_add/sub_batched: res must not alias b (use the *_assign form)");
    const DV r = dvb(M, res, res_cols, res_size), av = dvb(M, a, a_cols, a_size), bv = dvb(M, b, b_cols, b_size);
    const bool a_le_b = a_size <= b_size;
    const int sum = (int)std::min(a_le_b ? a_size : b_size, res_size), cpy = (int)std::min(a_le_b ? b_size : a_size, res_size);
    const int B = (int)batch;
    PZ_TRY(ewb(M, sub ? EW_SUB_I64 : EW_ADD_I64, B, r, (int)res_col, 0, &av, (int)a_col, 0, &bv, (int)b_col, 0, sum));
    if (a_le_b) PZ_TRY(ewb(M, sub ? EW_NEG_I64 : EW_COPY, B, r, (int)res_col, sum, &bv, (int)b_col, sum, nullptr, 0, 0, cpy - sum));
    else PZ_TRY(ewb(M, EW_COPY, B, r, (int)res_col, sum, &av, (int)a_col, sum, nullptr, 0, 0, cpy - sum));
    return ewb(M, EW_ZERO, B, r, (int)res_col, cpy, nullptr, 0, 0, nullptr, 0, 0, (int)res_size - cpy);
}
// mode 0: res += a, 1: res -= a, 2: res = a - res (and -res beyond a.size)   (add.rs:88-109, sub.rs:60-112)
int assign_batched(pz_module* M, int mode, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                   size_t a_cols, size_t a_size, size_t a_col) {
    PZ_TRY(check_batched(M, res, a, nullptr, res_col, res_cols, a_col, a_cols, 0, 0));
    const DV r = dvb(M, res, res_cols, res_size), av = dvb(M, a, a_cols, a_size);
    const int nl = (int)std::min(a_size, res_size), B = (int)batch;
    if (mode == 2) {
        PZ_TRY(ewb(M, EW_SUB_I64, B, r, (int)res_col, 0, &av, (int)a_col, 0, &r, (int)res_col, 0, nl));
        return ewb(M, EW_NEG_I64, B, r, (int)res_col, nl, &r, (int)res_col, nl, nullptr, 0, 0, (int)res_size - nl);
    }
    return ewb(M, mode == 0 ? EW_ADD_I64 : EW_SUB_I64, B, r, (int)res_col, 0, &r, (int)res_col, 0, &av, (int)a_col, 0, nl);
}
// op = EW_NEG_I64 / EW_COPY: res = op(a) over the common limbs, zero beyond   (negate.rs:6-29, copy.rs)
int unary_batched(pz_module* M, int op, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                  size_t a_cols, size_t a_size, size_t a_col) {
    PZ_TRY(check_batched(M, res, a, nullptr, res_col, res_cols, a_col, a_cols, 0, 0));
    const DV r = dvb(M, res, res_cols, res_size), av = dvb(M, a, a_cols, a_size);
    const int mn = (int)std::min(res_size, a_size), B = (int)batch;
    PZ_TRY(ewb(M, op, B, r, (int)res_col, 0, &av, (int)a_col, 0, nullptr, 0, 0, mn));
    return ewb(M, EW_ZERO, B, r, (int)res_col, mn, nullptr, 0, 0, nullptr, 0, 0, (int)res_size - mn);
}
}  // namespace

extern "C" {

int pz_vec_znx_add_into_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                                size_t a_cols, size_t a_size, size_t a_col, const int64_t* b, size_t b_cols, size_t b_size, size_t b_col) {
    PZ_ENTER(M);
    return add_sub_batched(M, false, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col, b, b_cols, b_size, b_col);
}
int pz_vec_znx_sub_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                           size_t a_cols, size_t a_size, size_t a_col, const int64_t* b, size_t b_cols, size_t b_size, size_t b_col) {
    PZ_ENTER(M);
    return add_sub_batched(M, true, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col, b, b_cols, b_size, b_col);
}
int pz_vec_znx_add_assign_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                                  size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return assign_batched(M, 0, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_sub_assign_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                                  size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return assign_batched(M, 1, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_sub_negate_assign_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                                         const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return assign_batched(M, 2, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_negate_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                              size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return unary_batched(M, EW_NEG_I64, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_copy_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col, const int64_t* a,
                            size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    PZ_REQUIRE((const void*)res != (const void*)a, "vec_znx_copy_batched: res must not alias a");
    return unary_batched(M, EW_COPY, batch, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_zero_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_col) {
    PZ_ENTER(M);
    PZ_TRY(check_batched(M, res, nullptr, nullptr, res_col, res_cols, 0, 0, 0, 0));
    const DV r = dvb(M, res, res_cols, res_size);
    return ewb(M, EW_ZERO, (int)batch, r, (int)res_col, 0, nullptr, 0, 0, nullptr, 0, 0, (int)res_size);
}
// res = X^k * a (rotate.rs:3-27); limbs of res beyond a.size zeroed
int pz_vec_znx_rotate_batched(pz_module* M, size_t batch, int64_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                              const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    PZ_TRY(check_batched(M, res, a, nullptr, res_col, res_cols, a_col, a_cols, 0, 0));
    PZ_REQUIRE((const void*)res != (const void*)a, "vec_znx_rotate_batched: res must not alias a");
    const DV r = dvb(M, res, res_cols, res_size), av = dvb(M, a, a_cols, a_size);
    const int mn = (int)std::min(res_size, a_size);
    const long long n = (long long)M->n;
    if (mn > 0 && batch > 0) {
        PolyMap sm{mn, 1, av.bs, (long long)a_cols * n, 0, n * (long long)a_col};
        PolyMap dm{mn, 1, r.bs, (long long)res_cols * n, 0, n * (long long)res_col};
        PZ_TRY(launch_rotate(M, (int)batch * mn, (const long long*)a, sm, (long long*)res, dm, (long long)k));
    }
    return ewb(M, EW_ZERO, (int)batch, r, (int)res_col, mn, nullptr, 0, 0, nullptr, 0, 0, (int)res_size - mn);
}
// vec_znx_normalize (same / cross base, any res_offset), vec_znx_lsh / rsh (= the same limb walk with res_offset = +-k at equal bases)
int pz_vec_znx_normalize_batched(pz_module* M, size_t batch, int64_t* res, size_t res_cols, size_t res_size, size_t res_base2k, int64_t res_offset,
                                 size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_base2k, size_t a_col) {
    return pz_vec_znx_big_normalize_batched(M, batch, res, res_cols, res_size, res_base2k, res_offset, res_col, a, a_cols, a_size, a_base2k, a_col);
}
int pz_vec_znx_lsh_batched(pz_module* M, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                           const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    if (k > ((size_t)1 << 40)) return fail(PZ_ERR_INVALID, "vec_znx_lsh_batched: shift out of range");
    return pz_vec_znx_big_normalize_batched(M, batch, res, res_cols, res_size, base2k, (int64_t)k, res_col, a, a_cols, a_size, base2k, a_col);
}
int pz_vec_znx_rsh_batched(pz_module* M, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                           const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    if (k > ((size_t)1 << 40)) return fail(PZ_ERR_INVALID, "vec_znx_rsh_batched: shift out of range");
    return pz_vec_znx_big_normalize_batched(M, batch, res, res_cols, res_size, base2k, -(int64_t)k, res_col, a, a_cols, a_size, base2k, a_col);
}

}  // extern "C"
