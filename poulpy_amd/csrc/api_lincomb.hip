// api_lincomb.hip — C ABI of the weighted sum of GLWE batches by constants (pz_glwe_lincomb_const_batched): poulpy-ckks's
// ckks_mul_add_pt_const_* / ckks_mul_sub_pt_const_* / ckks_dot_product_pt_const_znx (leveled/delegates/composite.rs:290-330, :423-463, :760-784)
// as ONE launch of k_lincomb_const (device_lincomb.hpp).  Every term is planned on the host exactly as pz_glwe_mul_const_batched
// (PZ_MUL_CONST) plans its product; the plans travel through the module's page-locked staging into its device table, outside the graph
// that holds the launch (DESIGN.md 4.4f "The graph rule", 4.6d).
#include "api_glwe.hpp"

namespace {

constexpr size_t kMaxShift = (size_t)1 << 40;

// (cnv_offset_hi, cnv_offset_lo), operations/glwe.rs:83-87
inline void offset_split(size_t cnv_offset, size_t base2k, int* hi, long long* lo) {
    if (cnv_offset < base2k) { *hi = 0; *lo = -(long long)(base2k - (cnv_offset % base2k)); }
    else { const size_t q = cnv_offset / base2k; *hi = (int)(q ? q - 1 : 0); *lo = (long long)(cnv_offset % base2k); }
}
bool overlaps(const void* p, size_t pn, const void* q, size_t qn) {
    const char *a = (const char*)p, *b = (const char*)q;
    return a < b + qn && b < a + pn;
}

}  // namespace

extern "C" {

int pz_glwe_lincomb_const_batched(pz_module* M, int64_t* res, size_t rank, size_t res_size, size_t base2k, const int64_t* const* operands,
                                  const int* shared, const size_t* a_size, const size_t* cnv_offset, const int64_t* const* re,
                                  const int64_t* const* im, const size_t* b_size, const int* join, const size_t* k, const int* sign, size_t nterms,
                                  int init, int normalize, size_t batch) {
    PZ_ENTER(M);
    PZ_REQUIRE(res && operands && shared && a_size && cnv_offset && re && im && b_size && join && k && sign, "glwe_lincomb_const: null argument");
    PZ_REQUIRE(rank >= 1 && rank <= 64 && res_size >= 1 && res_size <= 4096, "glwe_lincomb_const: res shape out of range");
    PZ_REQUIRE(base2k >= 1 && base2k <= 63, "glwe_lincomb_const: base2k %zu out of range", base2k);
    PZ_REQUIRE(nterms >= 1, "glwe_lincomb_const: no term");
    // ensure_accumulation_fits (composite.rs:43-51)
    PZ_REQUIRE(nterms <= ((size_t)1 << (63 - base2k)), "glwe_lincomb_const: %zu terms risk i64 overflow at base2k %zu", nterms, base2k);
    PZ_REQUIRE(init == PZ_LINCOMB_INIT_NONE || init == PZ_LINCOMB_INIT_RES, "glwe_lincomb_const: unknown initial accumulator");
    PZ_REQUIRE(normalize == 0 || normalize == 1, "glwe_lincomb_const: normalize must be 0 or 1");
    PZ_REQUIRE(M->n >= 2, "glwe_lincomb_const: n < 2");
    const size_t cols = rank + 1, n = (size_t)M->n;
    const size_t res_extent = batch * cols * res_size * n * 8;
    std::vector<LinTermSpec> spec(nterms);
    bool pair = false, has_tmp = false;
    int a_max = 1;
    for (size_t u = 0; u < nterms; ++u) {
        LinTermSpec& s = spec[u];
        const bool none = re[u] == nullptr && im[u] == nullptr;
        PZ_REQUIRE(operands[u] != nullptr, "glwe_lincomb_const: term %zu has no operand", u);
        PZ_REQUIRE(a_size[u] >= 1 && a_size[u] <= 4096, "glwe_lincomb_const: term %zu: a_size out of range", u);
        PZ_REQUIRE(none || (b_size[u] >= 1 && b_size[u] <= 4096), "glwe_lincomb_const: term %zu: b_size must be in 1..4096", u);
        PZ_REQUIRE(shared[u] == 0 || shared[u] == 1, "glwe_lincomb_const: term %zu: shared must be 0 or 1", u);
        PZ_REQUIRE(sign[u] == 1 || sign[u] == -1, "glwe_lincomb_const: term %zu: sign must be +1 or -1", u);
        PZ_REQUIRE(join[u] == PZ_JOIN_PLAIN || join[u] == PZ_JOIN_LSH_TERM || join[u] == PZ_JOIN_LSH_ACC, "glwe_lincomb_const: term %zu: unknown join", u);
        PZ_REQUIRE(join[u] == PZ_JOIN_PLAIN ? k[u] == 0 : k[u] <= kMaxShift, "glwe_lincomb_const: term %zu: shift out of range (a plain join takes k = 0)", u);
        int hi = 0;
        long long lo = 0;
        offset_split(cnv_offset[u], base2k, &hi, &lo);
        PZ_REQUIRE(none || (size_t)hi < a_size[u] + b_size[u], "glwe_lincomb_const: term %zu: cnv_offset beyond the product", u);
        const int as = (int)a_size[u], bs = none ? 0 : (int)b_size[u];
        s.a = (const long long*)operands[u];
        s.a_bs = shared[u] ? 0 : (long long)(cols * a_size[u] * n);
        s.a_size = as; s.cnv_offset = cnv_offset[u];
        s.re = re[u]; s.im = im[u]; s.b_size = bs;
        s.join = join[u] == PZ_JOIN_PLAIN ? 0 : (join[u] == PZ_JOIN_LSH_TERM ? 1 : 2);
        s.neg = sign[u] < 0 ? 1 : 0;
        s.k = k[u];
        pair = pair || im[u] != nullptr;
        has_tmp = has_tmp || ((u > 0 || init == PZ_LINCOMB_INIT_RES) && s.join != 0);   // (term 0 of a dot product overwrites)
        if (!none) a_max = std::max(a_max, as);
        // an operand may be res itself where res is the initial accumulator (every limb of a column is read before the column is stored)
        const size_t extent = (shared[u] ? 1 : batch) * cols * a_size[u] * n * 8;
        const bool is_res = init == PZ_LINCOMB_INIT_RES && (const void*)operands[u] == (const void*)res && !shared[u] && a_size[u] == res_size;
        if (!is_res && overlaps(operands[u], extent, res, res_extent))
            return fail(PZ_ERR_ALIAS, "glwe_lincomb_const: term %zu overlaps res without being the initial accumulator", u);
    }
    // the kernel's limits: 64 terms in the device table, 32 digits per constant in a term's plan, and the LDS slice of a workgroup,
    // (a_max + res_size, + res_size again if a join shifts) x (2 if any term has an imaginary part) x 128 threads x 8 B <= 160 KiB
    if (nterms > (size_t)kLincombMaxTerms) return fail(PZ_ERR_UNSUPPORTED, "glwe_lincomb_const: %zu terms (at most %d per call)", nterms, kLincombMaxTerms);
    for (size_t u = 0; u < nterms; ++u)
        if ((spec[u].re || spec[u].im) && !mul_const_nz_supported(M, spec[u].a_size, spec[u].b_size))
            return fail(PZ_ERR_UNSUPPORTED, "glwe_lincomb_const: term %zu: at most 64 operand limbs and 32 digits (got %d, %d)", u, spec[u].a_size,
                        spec[u].b_size);
    const size_t lds = res_size <= 1024 ? lincomb_lds_bytes(a_max, (int)res_size, pair, has_tmp) : (size_t)-1;
    if (lds > kLincombMaxLds)
        return fail(PZ_ERR_UNSUPPORTED, "glwe_lincomb_const: (%d + %d x %zu) limbs%s need %zu B of LDS (limit %zu)", a_max, has_tmp ? 2 : 1, res_size, pair ? ", paired," : "",
                    lds, kLincombMaxLds);
    PZ_REQUIRE(is_device_ptr(res), "batched entry points take device pointers");
    for (size_t u = 0; u < nterms; ++u) PZ_REQUIRE(is_device_ptr(operands[u]), "batched entry points take device pointers");
    if (batch == 0) return PZ_OK;
    PZ_REQUIRE(batch <= (size_t)1 << 24, "glwe_lincomb_const: batch out of range");
    // the constants and the operands reach the kernel through the table, which is rewritten here on every call: the graph's key covers
    // only what the launch itself is made of
    PZ_TRY(lincomb_stage(M, spec.data(), (int)nterms, (int)res_size, (int)base2k));
    KeyHash kh;
    kh.add((int)31); kh.add(res); kh.add(rank); kh.add(res_size); kh.add(base2k); kh.add(nterms); kh.add(init); kh.add(normalize); kh.add(batch);
    kh.add(pair); kh.add(a_max); kh.add(has_tmp); kh.add(M->lin_tab);
    graph_key_module(M, kh);
    return with_graph(M, kh.h, [&]() {
        return launch_lincomb(M, (int)batch, (long long*)res, (long long)(cols * res_size * n), (int)cols, (int)res_size, (int)base2k, (int)nterms,
                              init == PZ_LINCOMB_INIT_RES ? 1 : 0, normalize, pair, a_max, has_tmp);
    });
}

}  // extern "C"
