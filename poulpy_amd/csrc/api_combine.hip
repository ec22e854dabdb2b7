// api_combine.hip — C ABI of the GLWE linear combination (pz_glwe_combine_batched) and of the four accumulating shifts
// (pz_vec_znx_{lsh_add_into,lsh_sub,rsh_add_into,rsh_sub}_batched) on device-resident batches.  All of them run k_glwe_combine
// (device_combine.hpp): the shifts are the combination RAW(res) + LSH / RSH(a) on one column.  The step plans below are shift.rs's
// (poulpy-cpu-ref reference/vec_znx/shift.rs:68-180 for LSH, :245-... for RSH), computed once per call on the host.
#include "api_common.hpp"
#include "glwe_call.hpp"
#include "device_combine.hpp"

namespace {

constexpr size_t kMaxShift = (size_t)1 << 40;

struct TermIn {                 // one term, as the entry points describe it
    const int64_t* a;
    long long bs, ls;           // scalars between ciphertexts (0: shared) and between limbs
    long long col_off;          // scalars from a ciphertext's start to the column that res column 0 reads
    int cstep, size, kind, neg;
    size_t k;
    size_t extent;              // bytes the term reads, from `a`
};

// shift.rs:86-107 (LSH) / :280-295 (RSH) -> the kernel's plan; `res_size` is the output's limb count
void plan_term(const TermIn& in, int res_size, int base2k, CombTerm& t) {
    t.a = (const long long*)in.a + in.col_off;
    t.bs = in.bs; t.ls = in.ls; t.cstep = in.cstep; t.size = in.size; t.neg = in.neg; t.stage = 0;
    t.kind = in.kind; t.lsh = 0; t.pad = 0; t.steps = 0; t.pro = in.size; t.lo = 0; t.hi = 0;
    const int a_size = in.size;
    if (in.kind == CB_LSH) {
        const size_t steps = in.k / (size_t)base2k;
        const int k_rem = (int)(in.k % (size_t)base2k);
        if (steps >= (size_t)std::max(res_size, a_size)) { t.kind = CB_NONE; return; }   // :92-100: nothing is added
        const int st = (int)steps;
        const int min_size = std::min(res_size, std::max(a_size - st, 0));
        t.steps = st; t.lsh = k_rem;
        t.lo = min_size;
        t.pro = std::min(st + min_size, a_size);   // carry_only_start
    } else if (in.kind == CB_RSH) {
        size_t steps = in.k / (size_t)base2k;
        const int k_rem = (int)(in.k % (size_t)base2k);
        if (k_rem != 0) steps += 1;
        const int lsh = (base2k - k_rem) % base2k;
        const int st = (int)std::min(steps, (size_t)res_size + (size_t)a_size);   // beyond that every range below is empty or full
        t.steps = st; t.lsh = lsh;
        t.lo = std::min(res_size, st);                          // res_end
        t.hi = (int)std::min((long long)res_size, (long long)a_size + st);   // res_start
        t.pro = std::min(a_size, std::max(res_size - st, 0));   // a_start
    }
}

bool overlaps(const void* p, size_t pn, const void* q, size_t qn) {
    const char *a = (const char*)p, *b = (const char*)q;
    return a < b + qn && b < a + pn;
}

// validates, plans and launches; `res_col_off` = scalars to res column 0 of the walk
int run_combine(pz_module* M, int64_t* res, long long res_bs, long long res_ls, long long res_col_off, size_t res_extent, int cols, int res_size,
                int base2k, const TermIn* in, int nterms, int normalize, size_t batch, bool dry = false) {
    CombArgs g;
    g.res = (long long*)res + res_col_off;
    g.res_bs = res_bs; g.res_ls = res_ls;
    g.n = (int)M->n; g.batch = (int)batch; g.cols = cols; g.res_size = res_size; g.k = base2k; g.nterms = nterms; g.normalize = normalize;
    int staged = -1;
    for (int u = 0; u < kCombMaxTerms; ++u) {
        CombTerm& t = g.t[u];
        if (u >= nterms) { t = g.t[0]; t.kind = CB_NONE; continue; }
        plan_term(in[u], res_size, base2k, t);
        // the operand is res itself (same bytes, same strides): RAW and RSH read limb j, resp. limbs above it, before limb j is stored;
        // an LSH term reads a[j + steps] after res[j + steps] was stored, so its limbs go to LDS first
        const bool layout = (const void*)in[u].a == (const void*)res && in[u].bs == res_bs && in[u].ls == res_ls && in[u].size == res_size;
        const bool same = layout && in[u].col_off == res_col_off && in[u].cstep == 1;
        // another column of the same containers (the per-column shifts with a = res, a_col != res_col): never written by this call
        const bool other_col = layout && cols == 1 && in[u].col_off != res_col_off;
        if (!same && !other_col && overlaps(in[u].a, in[u].extent, res, res_extent))
            return fail(PZ_ERR_ALIAS, "glwe_combine: term %d overlaps res without being res", u);
        if (same && t.kind == CB_LSH && t.steps > 0 && t.lo > 0) {
            PZ_REQUIRE(staged < 0, "glwe_combine: at most one shifted term may be res itself");
            PZ_REQUIRE(in[u].size <= kCombMaxStage, "glwe_combine: an in-place shift is limited to %d limbs (got %d)", kCombMaxStage, in[u].size);
            t.stage = 1;
            staged = u;
        }
    }
    if (batch == 0 || dry) return PZ_OK;
    const long long threads = (long long)batch * cols * (M->n / 2);
    const size_t lds = staged >= 0 ? (size_t)g.t[staged].size * kCombBlock * sizeof(ulonglong2) : 0;
    KTimer kt(M, PZ_K_NORMALIZE);
    PZ_TRY(launch_k(k_glwe_combine, dim3((unsigned)((threads + kCombBlock - 1) / kCombBlock)), dim3(kCombBlock), lds, M->stream, g));
    dispatch_note(M, "k_glwe_combine (%d terms, %d cols, %d limbs, normalize %d, lds=%zu)", nterms, cols, res_size, normalize, lds);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// the four accumulating shifts: res[res_col] = RAW(res[res_col]) +- SHIFT(a[a_col])
int shift_acc_batched(pz_module* M, int kind, bool neg, const char* what, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols,
                      size_t res_size, size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    PZ_REQUIRE(res && a, "%s: null container", what);
    PZ_CHECK_COL(res_col, res_cols, what);
    PZ_CHECK_COL(a_col, a_cols, what);
    PZ_REQUIRE(base2k >= 1 && base2k <= 63, "%s: base2k %zu out of range", what, base2k);
    PZ_REQUIRE(k <= kMaxShift, "%s: shift out of range", what);
    PZ_REQUIRE(res_size >= 1 && res_size <= 4096 && a_size >= 1 && a_size <= 4096 && res_cols <= 64 && a_cols <= 64, "%s: shape out of range", what);
    PZ_REQUIRE(M->n >= 2, "%s: n < 2", what);
    PZ_REQUIRE(aligned16(res) && aligned16(a), "%s: containers must be 16-byte aligned", what);
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a), "batched entry points take device pointers");
    const long long n = (long long)M->n;
    TermIn t[2];
    t[0] = TermIn{res, (long long)(res_cols * res_size) * n, (long long)res_cols * n, (long long)res_col * n, 1, (int)res_size, CB_RAW, 0, 0, 0};
    t[1] = TermIn{a, (long long)(a_cols * a_size) * n, (long long)a_cols * n, (long long)a_col * n, 1, (int)a_size, kind, neg ? 1 : 0, k,
                  (size_t)batch * a_cols * a_size * n * 8};
    const size_t res_extent = (size_t)batch * res_cols * res_size * n * 8;
    t[0].extent = res_extent;
    // t[0] is res by construction; only the operand is checked for a partial overlap
    return run_combine(M, res, t[0].bs, t[0].ls, t[0].col_off, res_extent, 1, (int)res_size, (int)base2k, t, 2, 0, batch);
}

}  // namespace

namespace pz {

// pz_glwe_combine_batched for a caller who holds the module lock; dry: every check and the plan, no launch
int glwe_combine_nolock(pz_module* M, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                        const pz_glwe_term* terms, size_t nterms, int normalize, size_t batch, bool dry) {
    PZ_REQUIRE(res != nullptr && operands != nullptr && terms != nullptr, "glwe_combine: null argument");
    PZ_REQUIRE(nterms >= 1 && nterms <= (size_t)kCombMaxTerms, "glwe_combine: %zu terms (1 to %d)", nterms, kCombMaxTerms);
    PZ_REQUIRE(res_cols >= 1 && res_cols <= 64 && res_size >= 1 && res_size <= 4096, "glwe_combine: res shape out of range");
    PZ_REQUIRE(base2k >= 1 && base2k <= 63, "glwe_combine: base2k %zu out of range", base2k);
    PZ_REQUIRE(normalize == 0 || normalize == 1, "glwe_combine: normalize must be 0 or 1");
    PZ_REQUIRE(M->n >= 2, "glwe_combine: n < 2");
    const long long n = (long long)M->n;
    TermIn in[kCombMaxTerms];
    for (size_t u = 0; u < nterms; ++u) {
        const pz_glwe_term& t = terms[u];
        const int64_t* a = operands[u];
        PZ_REQUIRE(a != nullptr, "glwe_combine: term %zu has no operand", u);
        PZ_REQUIRE(t.base2k == 0 || t.base2k == base2k, "glwe_combine: term %zu has base2k %zu, res has %zu (one base2k per call)", u, t.base2k, base2k);
        PZ_REQUIRE(t.kind == PZ_TERM_RAW || t.kind == PZ_TERM_LSH || t.kind == PZ_TERM_RSH, "glwe_combine: term %zu has an unknown kind", u);
        PZ_REQUIRE(t.sign == 1 || t.sign == -1, "glwe_combine: term %zu: sign must be +1 or -1", u);
        PZ_REQUIRE((t.col0_only == 0 || t.col0_only == 1) && (t.shared == 0 || t.shared == 1), "glwe_combine: term %zu: flags must be 0 or 1", u);
        PZ_REQUIRE(t.a_size >= 1 && t.a_size <= 4096, "glwe_combine: term %zu: a_size out of range", u);
        PZ_REQUIRE(t.kind != PZ_TERM_RAW ? t.k <= kMaxShift : t.k == 0, "glwe_combine: term %zu: shift out of range (RAW takes k = 0)", u);
        PZ_REQUIRE(aligned16(a), "glwe_combine: term %zu: operand must be 16-byte aligned", u);
        const size_t acols = t.col0_only ? 1 : res_cols;
        const long long bs = t.shared ? 0 : (long long)(acols * t.a_size) * n;
        const int kind = t.kind == PZ_TERM_RAW ? CB_RAW : (t.kind == PZ_TERM_LSH ? CB_LSH : CB_RSH);
        in[u] = TermIn{a, bs, (long long)acols * n, 0, t.col0_only ? 0 : 1, (int)t.a_size, kind, t.sign < 0 ? 1 : 0, t.k,
                       (size_t)(t.shared ? 1 : batch) * acols * t.a_size * (size_t)n * 8};
    }
    PZ_REQUIRE(aligned16(res), "glwe_combine: res must be 16-byte aligned");
    PZ_REQUIRE(is_device_ptr(res), "batched entry points take device pointers");
    for (size_t u = 0; u < nterms; ++u) PZ_REQUIRE(is_device_ptr(operands[u]), "batched entry points take device pointers");
    const long long res_ls = (long long)res_cols * n, res_bs = res_ls * (long long)res_size;
    return run_combine(M, res, res_bs, res_ls, 0, (size_t)batch * res_cols * res_size * (size_t)n * 8, (int)res_cols, (int)res_size, (int)base2k, in,
                       (int)nterms, normalize, batch, dry);
}

}  // namespace pz

extern "C" {

int pz_glwe_combine_batched(pz_module* M, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                            const pz_glwe_term* terms, size_t nterms, int normalize, size_t batch) {
    PZ_ENTER(M);
    return glwe_combine_nolock(M, res, res_cols, res_size, base2k, operands, terms, nterms, normalize, batch, false);
}

int pz_vec_znx_lsh_add_into_batched(pz_module* M, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                                    size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return shift_acc_batched(M, CB_LSH, false, "vec_znx_lsh_add_into_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_lsh_sub_batched(pz_module* M, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                               const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return shift_acc_batched(M, CB_LSH, true, "vec_znx_lsh_sub_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_rsh_add_into_batched(pz_module* M, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size,
                                    size_t res_col, const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return shift_acc_batched(M, CB_RSH, false, "vec_znx_rsh_add_into_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}
int pz_vec_znx_rsh_sub_batched(pz_module* M, size_t batch, size_t base2k, size_t k, int64_t* res, size_t res_cols, size_t res_size, size_t res_col,
                               const int64_t* a, size_t a_cols, size_t a_size, size_t a_col) {
    PZ_ENTER(M);
    return shift_acc_batched(M, CB_RSH, true, "vec_znx_rsh_sub_batched", batch, base2k, k, res, res_cols, res_size, res_col, a, a_cols, a_size, a_col);
}

}  // extern "C"
