// api_sum.hip — C ABI and launcher of the normalized signed sum of GLWE batches (pz_glwe_sum_batched): poulpy-ckks's ckks_add_many
// (leveled/delegates/composite.rs:63-93) and the join of its dot products (:478-506) as ONE launch of k_glwe_sum (device_sum.hpp).  The
// chain of joins is folded into per-term walk plans on the host (sum_plan); the plans travel in the kernel's arguments, so the call is a
// single kernel node (DESIGN.md 4.4f "The graph rule", 4.6e).
#include "api_common.hpp"
#include "glwe_call.hpp"
#include "device_sum.hpp"

namespace {

constexpr size_t kMaxShift = (size_t)1 << 40;

bool overlaps(const void* p, size_t pn, const void* q, size_t qn) {
    const char *a = (const char*)p, *b = (const char*)q;
    return a < b + qn && b < a + pn;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int launch_glwe_sum(pz_module* M, const SumArgs& g) {
    if (g.batch <= 0) return PZ_OK;
    if (g.n < 2 || g.nterms < 0 || g.nterms > kSumMaxTerms || g.stage > kSumMaxStage)
        return fail(PZ_ERR_INVALID, "k_glwe_sum: shape outside the kernel");
    const long long threads = (long long)g.batch * g.cols * (g.n / 2);
    if ((threads + kSumBlock - 1) / kSumBlock > 0x7fffffffLL) return fail(PZ_ERR_INVALID, "k_glwe_sum: %lld threads are more than one grid holds", threads);
    const size_t lds = (size_t)g.stage * kSumBlock * sizeof(ulonglong2);
    KTimer kt(M, PZ_K_NORMALIZE);
    PZ_TRY(launch_k(k_glwe_sum, dim3((unsigned)((threads + kSumBlock - 1) / kSumBlock)), dim3(kSumBlock), lds, M->stream, g));
    dispatch_note(M, "k_glwe_sum (%d terms, %d cols, %d limbs, lds=%zu)", g.nterms, g.cols, g.res_size, lds);
    PZ_HIP(hipGetLastError());
    return PZ_OK;
}

}  // namespace

namespace pz {

// pz_glwe_sum_batched for a caller who holds the module lock; dry: every check and the plan, no launch
int glwe_sum_nolock(pz_module* M, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                    const int* shared, const size_t* a_size, const int* join, const size_t* k, const int* sign, size_t nterms, size_t batch, bool dry) {
    PZ_REQUIRE(res && operands && shared && a_size && join && k && sign, "glwe_sum: null argument");
    PZ_REQUIRE(res_cols >= 1 && res_cols <= 64 && res_size >= 1 && res_size <= 4096, "glwe_sum: res shape out of range");
    PZ_REQUIRE(base2k >= 1 && base2k <= 63, "glwe_sum: base2k %zu out of range", base2k);
    PZ_REQUIRE(nterms >= 1, "glwe_sum: no term");
    // ensure_accumulation_fits (composite.rs:43-51)
    PZ_REQUIRE(nterms <= ((size_t)1 << (63 - base2k)), "glwe_sum: %zu terms risk i64 overflow at base2k %zu", nterms, base2k);
    if (nterms > (size_t)kSumMaxTerms) return fail(PZ_ERR_UNSUPPORTED, "glwe_sum: %zu terms (at most %d per call)", nterms, kSumMaxTerms);
    PZ_REQUIRE(M->n >= 2 && M->n % 2 == 0, "glwe_sum: n must be even");
    PZ_REQUIRE(batch <= (size_t)1 << 24, "glwe_sum: batch out of range");
    const size_t n = (size_t)M->n;
    const size_t res_extent = batch * res_cols * res_size * n * 8;
    SumSpec spec[kSumMaxTerms];
    for (size_t u = 0; u < nterms; ++u) {
        PZ_REQUIRE(operands[u] != nullptr, "glwe_sum: term %zu has no operand", u);
        PZ_REQUIRE(a_size[u] >= 1 && a_size[u] <= 4096, "glwe_sum: term %zu: a_size out of range", u);
        PZ_REQUIRE(shared[u] == 0 || shared[u] == 1, "glwe_sum: term %zu: shared must be 0 or 1", u);
        PZ_REQUIRE(sign[u] == 1 || sign[u] == -1, "glwe_sum: term %zu: sign must be +1 or -1", u);
        PZ_REQUIRE(join[u] == PZ_JOIN_PLAIN || join[u] == PZ_JOIN_LSH_TERM || join[u] == PZ_JOIN_LSH_ACC, "glwe_sum: term %zu: unknown join", u);
        PZ_REQUIRE(join[u] == PZ_JOIN_PLAIN ? k[u] == 0 : k[u] <= kMaxShift, "glwe_sum: term %zu: shift out of range (a plain join takes k = 0)", u);
        PZ_REQUIRE(aligned16(operands[u]), "glwe_sum: term %zu: operand must be 16-byte aligned", u);
        SumSpec& s = spec[u];
        s.a = (const long long*)operands[u];
        s.shared = shared[u]; s.a_size = (int)a_size[u]; s.neg = sign[u] < 0 ? 1 : 0; s.k = k[u];
        s.join = join[u] == PZ_JOIN_PLAIN ? SUM_JOIN_PLAIN : (join[u] == PZ_JOIN_LSH_TERM ? SUM_JOIN_LSH_TERM : SUM_JOIN_LSH_ACC);
        // term 0 may be res itself: the partial sum a chunked dot product continues from
        s.inplace = u == 0 && (const void*)operands[u] == (const void*)res && !shared[u] && a_size[u] == res_size;
        const size_t extent = (shared[u] ? 1 : batch) * res_cols * a_size[u] * n * 8;
        if (!s.inplace && overlaps(operands[u], extent, res, res_extent))
            return fail(PZ_ERR_ALIAS, "glwe_sum: term %zu overlaps res without being term 0 = res", u);
    }
    PZ_REQUIRE(aligned16(res), "glwe_sum: res must be 16-byte aligned");
    SumArgs g;
    g.res = (long long*)res;
    g.n = (int)n; g.batch = (int)batch; g.cols = (int)res_cols; g.res_size = (int)res_size; g.k = (int)base2k; g.pad = 0;
    sum_plan(g, spec, (int)nterms, (int)res_size, (int)base2k);
    for (int u = g.nterms; u < kSumMaxTerms; ++u) g.t[u] = SumTerm{};
    // an in-place term 0 that later joins shift is staged in LDS, 32 limbs at the most
    if (g.stage > kSumMaxStage)
        return fail(PZ_ERR_ALIAS, "glwe_sum: term 0 is res and is shifted: at most %d limbs can be staged (got %d)", kSumMaxStage, g.stage);
    PZ_REQUIRE(is_device_ptr(res), "batched entry points take device pointers");
    for (size_t u = 0; u < nterms; ++u) PZ_REQUIRE(is_device_ptr(operands[u]), "batched entry points take device pointers");
    if (batch == 0 || dry) return PZ_OK;
    return launch_glwe_sum(M, g);
}

}  // namespace pz

extern "C" {

int pz_glwe_sum_batched(pz_module* M, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                        const int* shared, const size_t* a_size, const int* join, const size_t* k, const int* sign, size_t nterms, size_t batch) {
    PZ_ENTER(M);
    return glwe_sum_nolock(M, res, res_cols, res_size, base2k, operands, shared, a_size, join, k, sign, nterms, batch, false);
}

}  // extern "C"
