// api_gates.hip — the gates of poulpy-bin-fhe's bdd_arithmetic behind the C ABI, each one external product of the engine (api_glwe.hip) with its
// operands folded into the pipeline's stages: CMUX (eval.rs:524-626), GLWEBlindRotation by encrypted bits (blind_rotation.rs:196-264), the
// conditional swap (eval.rs:417-461) and GLWEBlindRetrieval (blind_retrieval.rs:195-266).  DESIGN.md 4.4d, 4.4e.
#include <algorithm>
#include <vector>

#include "api_common.hpp"
#include "glwe_call.hpp"

using namespace pz;

// ------------------------------------------------------------------------------
// CMUX, the gate of poulpy-bin-fhe's bdd_arithmetic (eval.rs:524-626): res = normalize((t - f) (x) GGSW + f), f added to the big
// value on every column BEFORE the carry chain - which is why the gate is not an external product followed by an addition.  Routes:
//   fused         N = 1024 / 2048 / 4096 on the small-ring kernels: the forward stage reads t and f (or f twice through the monomial map of
//                 X^rot) and forms the difference in registers; the inverse stage adds f as its every-column operand
//   materialised  every other shape the external product serves: D = t - f written to the second workspace by the element-wise / rotate kernels,
//                 then the shape's pipeline on D with f as the tail's every-column operand.  POULPY_DBG_CMUX_FUSED=0 sends every shape here.
// In place (res == t, res == f): every kernel that reads t or f of a ciphertext runs before the one that writes its result, and the inverse
// stages read f at the positions they then write - as for the automorphism family's add forms.
// ------------------------------------------------------------------------------
// (CmuxOperands, limbs of t and of f; t null: t = X^t_rot f: glwe_call.hpp)
struct CmuxShape {
    long long cols, t_ct, f_ct, d_ct, res_ct;   // i64 elements of one ciphertext of t / f / D / res
    size_t t_bytes, f_bytes, res_bytes;         // bytes of the whole batch
};
static CmuxShape cmux_shape(const pz_module* M, const pz_glwe_op_params* p, const CmuxOperands* o, size_t batch) {
    CmuxShape s;
    const long long n = (long long)M->n;
    s.cols = (long long)p->rank + 1;
    s.t_ct = n * s.cols * (long long)o->t_size; s.f_ct = n * s.cols * (long long)o->f_size;
    s.d_ct = n * s.cols * (long long)p->a_size; s.res_ct = n * s.cols * (long long)p->res_size;
    s.t_bytes = batch * (size_t)s.t_ct * 8; s.f_bytes = batch * (size_t)s.f_ct * 8; s.res_bytes = batch * (size_t)s.res_ct * 8;
    return s;
}
// the argument checks that need no module (nothing is launched when one fails)
static int cmux_check_args(const int64_t* res, const int64_t* t, const int64_t* f, const double* pmat, const pz_glwe_op_params* p,
                           const CmuxOperands* o) {
    PZ_REQUIRE(p != nullptr, "glwe_cmux: null params");
    PZ_REQUIRE(res != nullptr && f != nullptr && pmat != nullptr, "glwe_cmux: null argument");
    PZ_REQUIRE(p->dsize >= 1 && p->dnum >= 1 && p->key_size >= 1 && p->a_size >= 1 && p->res_size >= 1 && o->f_size >= 1, "glwe_cmux: empty shape");
    // external_product/glwe.rs:213 (and glwe_sub, operations.rs:343-344): t, f, res and the GGSW share one base2k
    PZ_REQUIRE(p->a_base2k == p->key_base2k && p->res_base2k == p->key_base2k, "glwe_cmux: t, f, res and the GGSW share one base2k (%llu / %llu / %llu)",
               (unsigned long long)p->a_base2k, (unsigned long long)p->res_base2k, (unsigned long long)p->key_base2k);
    if (t == nullptr) {
        PZ_REQUIRE(o->t_size == o->f_size, "glwe_cmux: the rotated source t = X^t_rot f has the layout of f (t_size == f_size)");
        if ((const void*)res == (const void*)f) return fail(PZ_ERR_ALIAS, "glwe_cmux: with the rotated source res must not overlap f");
    } else {
        PZ_REQUIRE(o->t_size >= 1, "glwe_cmux: empty shape");
        if ((const void*)res == (const void*)t) PZ_REQUIRE(p->res_size == o->t_size, "in-place call with different layouts for t and res");
    }
    if ((const void*)res == (const void*)f && t != nullptr) PZ_REQUIRE(p->res_size == o->f_size, "in-place call with different layouts for f and res");
    return PZ_OK;
}
// the checks that need the ring degree: res may BE t or f (the assign forms), any other overlap is refused
static int cmux_check_overlap(const CmuxShape& s, const int64_t* res, const int64_t* t, const int64_t* f) {
    if (t != nullptr && (const void*)res != (const void*)t && ranges_overlap(res, s.res_bytes, t, s.t_bytes))
        return fail(PZ_ERR_ALIAS, "glwe_cmux: res overlaps t without being t");
    if (((const void*)res != (const void*)f || t == nullptr) && ranges_overlap(res, s.res_bytes, f, s.f_bytes))
        return fail(PZ_ERR_ALIAS, t ? "glwe_cmux: res overlaps f without being f" : "glwe_cmux: with the rotated source res must not overlap f");
    return PZ_OK;
}
// D = t - f (t null: X^rot f - f) on the limbs of D, missing limbs of either side zero (vec_znx_sub, sub.rs:6-58; vec_znx_sub_assign :60-84)
static int cmux_materialise(pz_module* M, int64_t* D, const CmuxShape& s, const int64_t* t, const int64_t* f, const pz_glwe_op_params* p,
                            const CmuxOperands* o, size_t batch) {
    const long long n = (long long)M->n;
    const int cols = (int)s.cols, B = (int)batch, d_size = (int)p->a_size;
    const int f_sz = std::min((int)o->f_size, d_size), t_sz = t ? std::min((int)o->t_size, d_size) : f_sz;
    const int common = std::min(t_sz, f_sz), top = std::max(t_sz, f_sz);
    auto limb = [&](const int64_t* v, int l) { return v + (long long)l * cols * n; };
    if (t == nullptr) {   // glwe_rotate + glwe_sub_assign in one pass (k_rotate mode 1)
        PolyMap sm{common * cols, 1, s.f_ct, n, 0, 0}, dm{common * cols, 1, s.d_ct, n, 0, 0};
        PZ_TRY(launch_rotate(M, B * common * cols, (const long long*)f, sm, (long long*)D, dm, 1, B * common * cols, nullptr, 0, 0, (long long)o->t_rot));
    } else {
        PZ_TRY(launch_ew(M, EW_SUB_I64, D, s.d_ct, n, t, s.t_ct, n, f, s.f_ct, n, common * cols, B));
        if (t_sz > common) PZ_TRY(launch_ew(M, EW_COPY, (void*)limb(D, common), s.d_ct, n, limb(t, common), s.t_ct, n, nullptr, 0, 0, (t_sz - common) * cols, B));
        else if (f_sz > common) PZ_TRY(launch_ew(M, EW_NEG_I64, (void*)limb(D, common), s.d_ct, n, limb(f, common), s.f_ct, n, nullptr, 0, 0, (f_sz - common) * cols, B));
    }
    return launch_ew(M, EW_ZERO, (void*)limb(D, top), s.d_ct, n, nullptr, 0, 0, nullptr, 0, 0, (d_size - top) * cols, B);
}
// device pointers, the key resolved, the module lock held (pz_glwe_cmux_batched and the ladder of pz_glwe_blind_rotation_batched).
// res2 != null: the conditional swap (glwe_cswap below) - res == f, res2 == t, and t takes the second result normalize(t - big) in place
namespace pz {
int glwe_cmux(pz_module* M, int64_t* res, const int64_t* t, const int64_t* f, const double* key, const pz_glwe_op_params* p,
              const CmuxOperands* o, size_t batch, int64_t* res2) {
    GlweCall c;
    PZ_TRY(glwe_call_init(c, M, GlweKind::ExternalProduct, res, f, key, p, batch, nullptr, nullptr, nullptr));   // (`a` is set below: D, or nothing)
    if (batch == 0) return PZ_OK;
    const CmuxShape s = cmux_shape(M, p, o, batch);
    c.add = f; c.add_bs = s.f_ct; c.add_size = (int)o->f_size;
    c.res2 = res2; c.res2_bs = s.t_ct; c.res2_size = (int)o->t_size;
    const bool pipeline = fused_applies(M, p, c.s, c.kind), small_ring = !pipeline && small_ring_applies(M, p, c.s, c.kind, true);
    const int knob = rt_knob("POULPY_DBG_CMUX_FUSED", 1);   // (read per call: tests flip it)
    SmallDiff d;
    if (knob != 0 && cmux_fused_route(c)) {
        const long long n = c.n;
        const int d_size = (int)p->a_size, cols = (int)s.cols;
        d.t = (const long long*)t; d.f = (const long long*)f;
        d.tmap = PolyMap{d_size, cols, s.t_ct, (long long)cols * n, n, 0};
        d.fmap = PolyMap{d_size, cols, s.f_ct, (long long)cols * n, n, 0};
        d.t_size = t ? (int)o->t_size : (int)o->f_size; d.f_size = (int)o->f_size;
        d.rot = (unsigned)((unsigned long long)o->t_rot & (2ull * (unsigned long long)n - 1ull));
        c.diff = &d; c.a = nullptr;
        return pipeline ? glwe_fused(c) : glwe_small_ring(c);
    }
    dispatch_note(M, "%s: materialised difference (%s)", gate_name(c), knob == 0 ? "POULPY_DBG_CMUX_FUSED=0" : (pipeline ? "three-kernel pipeline" : (small_ring ? "small ring" : "five-kernel path")));
    PZ_TRY(ws2_reserve(M, batch * (size_t)s.d_ct * 8));
    int64_t* D = (int64_t*)M->ws2;
    PZ_TRY(cmux_materialise(M, D, s, t, f, p, o, batch));
    c.a = D;
    if (pipeline) return glwe_fused(c);
    if (small_ring) return glwe_small_ring(c);
    return glwe_unfused(c);
}
}  // namespace pz

extern "C" {
size_t pz_glwe_cmux_workspace_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t batch) {
    // the external product's reservation (D has a_size limbs); the materialised route keeps D in the module's second workspace on top of it
    return pz_glwe_op_workspace_bytes(M, p, batch, (int)GlweKind::ExternalProduct);
}
int pz_glwe_cmux_batched(pz_module* M, int64_t* res, const int64_t* t, size_t t_size, int64_t t_rot, const int64_t* f, size_t f_size,
                         const double* ggsw_pmat, const pz_glwe_op_params* p, size_t batch) {
    const CmuxOperands ops{t_size, f_size, t ? 0 : t_rot};
    const CmuxOperands* o = &ops;
    PZ_TRY(cmux_check_args(res, t, f, ggsw_pmat, p, o));
    PZ_ENTER(M);
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(f) && (t == nullptr || is_device_ptr(t)), "batched entry points take device pointers");
    PZ_TRY(cmux_check_overlap(cmux_shape(M, p, o, batch), res, t, f));
    const double* key = nullptr;
    PZ_TRY(resolve_key(M, ggsw_pmat, ggsw_key_bytes(M, p), &key));
    PZ_TRY(glwe_cmux(M, res, t, f, key, p, o, batch));
    return finish_call(M, false);
}

// GLWEBlindRotation::glwe_blind_rotation / _assign (bdd_arithmetic/blind_rotation.rs:196-264) on `batch` ciphertexts: nbits rotated-source CMUX
// steps that ping-pong between res and tmp (:218-236), the final copy when the step count is odd (:238-241)
size_t pz_glwe_blind_rotation_tmp_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t batch) {
    if (!M || !p) return 0;
    return batch * (size_t)M->n * 8 * (p->rank + 1) * p->res_size;
}
static int glwe_blind_rotation_steps(pz_module* M, int64_t* res, const int64_t* a, size_t nbits, const double* const* keys, int sign, size_t bit_lsh,
                                     const pz_glwe_op_params* p, int64_t* tmp, size_t batch) {
    const long long n = (long long)M->n;
    const int cols = (int)p->rank + 1, B = (int)batch;
    const long long res_ct = n * cols * (long long)p->res_size, a_ct = n * cols * (long long)p->a_size;
    // glwe_copy (:262): the common limbs, zero beyond.  With one layout for a and res the copy only feeds step 0, which then reads `a` itself:
    // the same digits, one pass over the batch less (res is first written by step 1, or by the final copy)
    const int64_t* first = (p->a_size == p->res_size && nbits > 0) ? a : res;
    if ((const void*)res != (const void*)a && first == res) {
        const int mn = (int)std::min(p->a_size, p->res_size);
        PZ_TRY(launch_ew(M, EW_COPY, res, res_ct, n, a, a_ct, n, nullptr, 0, 0, mn * cols, B));
        PZ_TRY(launch_ew(M, EW_ZERO, res + (long long)mn * cols * n, res_ct, n, nullptr, 0, 0, nullptr, 0, 0, ((int)p->res_size - mn) * cols, B));
    }
    pz_glwe_op_params q = *p;
    q.a_size = p->res_size;   // every step works on the layout of res (:212)
    CmuxOperands o;
    o.t_size = o.f_size = p->res_size;
    int64_t *cur = res, *other = tmp;
    if (first != res && (nbits & 1)) std::swap(cur, other);   // step 0 does not read res: an odd count starts INTO res and ends there, no final copy
    for (size_t i = 0; i < nbits; ++i) {
        const int64_t* src = i == 0 ? first : cur;
        const size_t sh = i + bit_lsh;
        const long long pw = sh < 62 ? (1ll << sh) : 0;   // (X^(2^sh) = 1 once 2^sh is a multiple of 2n)
        o.t_rot = sign ? pw : -pw;   // :226-229
        PZ_TRY(glwe_cmux(M, other, nullptr, src, keys[i], &q, &o, batch));   // :232, b <- (X^rot a - a) GGSW(bit) + a
        std::swap(cur, other);
    }
    if (cur != res) PZ_TRY(launch_ew(M, EW_COPY, res, res_ct, n, tmp, res_ct, n, nullptr, 0, 0, (int)p->res_size * cols, B));   // :238-241
    return PZ_OK;
}
int pz_glwe_blind_rotation_batched(pz_module* M, int64_t* res, const int64_t* a, size_t nbits, const double* const* bits, int sign, size_t bit_lsh,
                                   const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch) {
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(res != nullptr && a != nullptr && (nbits == 0 || bits != nullptr), "glwe_blind_rotation: null argument");
    PZ_TRY(require_op_shape(p, "glwe op"));
    PZ_REQUIRE(p->a_base2k == p->key_base2k && p->res_base2k == p->key_base2k, "glwe_blind_rotation: a, res and the GGSWs share one base2k");
    for (size_t i = 0; i < nbits; ++i) PZ_REQUIRE(bits[i] != nullptr, "glwe_blind_rotation: GGSW %zu is null", i);
    if ((const void*)res == (const void*)a) PZ_REQUIRE(p->res_size == p->a_size, "in-place call with different layouts for a and res");
    PZ_ENTER(M);
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a), "batched entry points take device pointers");
    const size_t cols = p->rank + 1, n8 = (size_t)M->n * 8;
    const size_t res_bytes = batch * n8 * cols * p->res_size, a_bytes = batch * n8 * cols * p->a_size;
    if ((const void*)res != (const void*)a && ranges_overlap(res, res_bytes, a, a_bytes)) return fail(PZ_ERR_ALIAS, "glwe_blind_rotation: res overlaps a without being a");
    if (nbits > 0 && batch > 0) {
        PZ_REQUIRE(tmp != nullptr && is_device_ptr(tmp) && tmp_bytes >= pz_glwe_blind_rotation_tmp_bytes(M, p, batch), "glwe_blind_rotation: tmp too small (%zu bytes)", tmp_bytes);
        if (ranges_overlap(tmp, res_bytes, res, res_bytes) || ranges_overlap(tmp, res_bytes, a, a_bytes)) return fail(PZ_ERR_ALIAS, "glwe_blind_rotation: tmp overlaps res or a");
    }
    std::vector<const double*> keys(nbits);
    for (size_t i = 0; i < nbits; ++i) PZ_TRY(resolve_key(M, bits[i], ggsw_key_bytes(M, p), &keys[i]));
    if (batch == 0) return PZ_OK;
    KeyHash k = graph_key(M, GRAPH_GLWE_BLIND_ROTATION, res, a, tmp, nbits, sign != 0, bit_lsh, batch, *p, rt_knob("POULPY_DBG_CMUX_FUSED", 1));
    for (size_t i = 0; i < nbits; ++i) k.add(keys[i]);
    PZ_TRY(with_graph(M, k.h, [&]() { return glwe_blind_rotation_steps(M, res, a, nbits, keys.data(), sign, bit_lsh, p, (int64_t*)tmp, batch); }));
    return finish_call(M, false);
}
}  // extern "C"

// ------------------------------------------------------------------------------
// Conditional swap, the other gate of bdd_arithmetic (Cswap::cswap, eval.rs:417-461, the equal-base branch), IN PLACE on a and b:
//   D = b - a (glwe_sub into tmp_c of max(a, b) limbs, not normalized);  big = D (x) GGSW - ONE external product;
//   a' = normalize(big + a) (vec_znx_big_add_small_into),  b' = normalize(b - big) (vec_znx_big_sub_small_a) on every column.
// The forward half is the CMUX's with t = b, f = a (fused: SmallDiff; materialised: cmux_materialise into the second workspace).  The inverse half leaves
// two results from the one big value:
//   small-ring kernels  the dual forms k_small_inv<.., DUAL> / k_small_one<.., DUAL>: two carry chains behind one inverse transform
//   pipeline            two tails over the same T2' (the tail only reads it), the second with the big value negated (TailCall::big_neg)
//   five-kernel path    the i64 big value in the workspace feeds both normalizations
// In place: every kernel that reads a or b of a ciphertext as a SOURCE runs before the one that writes its results (or, in the one-kernel form, four
// barriers earlier in the same workgroup), and the chains read their operands at the positions they then write.
// ------------------------------------------------------------------------------
static int cswap_check_args(const int64_t* a, size_t a_size, const int64_t* b, size_t b_size, const double* pmat, const pz_glwe_op_params* p, size_t batch) {
    PZ_REQUIRE(p != nullptr, "glwe_cswap: null params");
    PZ_REQUIRE(a != nullptr && b != nullptr && pmat != nullptr, "glwe_cswap: null argument");
    PZ_REQUIRE(p->dsize >= 1 && p->dnum >= 1 && p->key_size >= 1 && p->a_size >= 1 && p->res_size >= 1 && a_size >= 1 && b_size >= 1, "glwe_cswap: empty shape");
    // eval.rs:427 (this branch) and external_product/glwe.rs:213
    PZ_REQUIRE(p->a_base2k == p->key_base2k && p->res_base2k == p->key_base2k, "glwe_cswap: a, b and the GGSW share one base2k (%llu / %llu / %llu)",
               (unsigned long long)p->a_base2k, (unsigned long long)p->res_base2k, (unsigned long long)p->key_base2k);
    PZ_REQUIRE(p->a_size == std::max(a_size, b_size), "glwe_cswap: p->a_size is the limb count of the difference, max(a_size, b_size) = %zu, not %llu",
               std::max(a_size, b_size), (unsigned long long)p->a_size);   // tmp_c: k = max(res_a.max_k, res_b.max_k), eval.rs:437-442
    PZ_REQUIRE(p->res_size == a_size, "glwe_cswap: p->res_size is a_size = %zu, not %llu", a_size, (unsigned long long)p->res_size);
    // what the pointers alone tell: the same buffer, or two ranges that overlap at the smallest ring degree a module can have (n = 2)
    const size_t cols = p->rank + 1;
    if ((const void*)a == (const void*)b || (batch > 0 && ranges_overlap(a, batch * cols * a_size * 16, b, batch * cols * b_size * 16)))
        return fail(PZ_ERR_ALIAS, "glwe_cswap: a and b overlap");
    return PZ_OK;
}
// device pointers, the key resolved, the module lock held (pz_glwe_cswap_batched and the levels of pz_glwe_blind_retrieval_batched): the CMUX with
// t = b, f = a, res = a, and b taking the second result
static int glwe_cswap(pz_module* M, int64_t* a, size_t a_size, int64_t* b, size_t b_size, const double* key, const pz_glwe_op_params* p, size_t batch) {
    const CmuxOperands ops{b_size, a_size, 0};
    return glwe_cmux(M, a, b, a, key, p, &ops, batch, b);
}
// the levels of the retrieval network in its dense form: level i pairs slot j with slot j + t, t = 2^(nbits - 1 - i), for j < cnt (blind_retrieval.rs:222-233)
static size_t retrieval_cnt(size_t nslots, size_t t) { return t < nslots ? std::min(t, nslots - t) : 0; }
static int glwe_blind_retrieval_levels(pz_module* M, int64_t* slots, size_t nslots, size_t nbits, const double* const* keys, int reverse,
                                       const pz_glwe_op_params* p, size_t batch) {
    const size_t slot_elems = batch * (size_t)M->n * (p->rank + 1) * p->res_size;
    for (size_t s = 0; s < nbits; ++s) {
        const size_t i = reverse ? nbits - 1 - s : s;
        if (nbits - 1 - i >= 63) continue;   // (t beyond any slot count)
        const size_t t = (size_t)1 << (nbits - 1 - i), cnt = retrieval_cnt(nslots, t);
        if (cnt == 0) continue;
        PZ_TRY(glwe_cswap(M, slots, p->res_size, slots + t * slot_elems, p->res_size, keys[nbits - 1 - i], p, cnt * batch));
    }
    return PZ_OK;
}

extern "C" {
size_t pz_glwe_cswap_workspace_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t batch) {
    // the external product's reservation (D has p->a_size limbs); the materialised route keeps D in the module's second workspace on top of it
    return pz_glwe_op_workspace_bytes(M, p, batch, (int)GlweKind::ExternalProduct);
}
int pz_glwe_cswap_batched(pz_module* M, int64_t* a, size_t a_size, int64_t* b, size_t b_size, const double* ggsw_pmat, const pz_glwe_op_params* p,
                          size_t batch) {
    PZ_TRY(cswap_check_args(a, a_size, b, b_size, ggsw_pmat, p, batch));
    PZ_ENTER(M);
    PZ_REQUIRE(is_device_ptr(a) && is_device_ptr(b), "batched entry points take device pointers");
    const size_t cols = p->rank + 1, n8 = (size_t)M->n * 8;
    if (ranges_overlap(a, batch * n8 * cols * a_size, b, batch * n8 * cols * b_size)) return fail(PZ_ERR_ALIAS, "glwe_cswap: a and b overlap");
    const double* key = nullptr;
    PZ_TRY(resolve_key(M, ggsw_pmat, ggsw_key_bytes(M, p), &key));
    PZ_TRY(glwe_cswap(M, a, a_size, b, b_size, key, p, batch));
    return finish_call(M, false);
}

// GLWEBlindRetrieval::glwe_blind_retrieval_statefull / _rev (bdd_arithmetic/blind_retrieval.rs:195-266) on `batch` vectors of nslots ciphertexts in
// a dense slot-major buffer: every level of the butterfly network is one conditional swap on cnt * batch contiguous pairs
size_t pz_glwe_blind_retrieval_workspace_bytes(const pz_module* M, const pz_glwe_op_params* p, size_t nslots, size_t nbits, size_t batch) {
    if (!M || !p) return 0;
    size_t most = 0;   // the swap's figure at the largest level
    for (size_t i = 0; i < nbits && i < 63; ++i) most = std::max(most, retrieval_cnt(nslots, (size_t)1 << i));
    return most == 0 ? 0 : pz_glwe_cswap_workspace_bytes(M, p, most * batch);
}
int pz_glwe_blind_retrieval_batched(pz_module* M, int64_t* slots, size_t nslots, size_t nbits, const double* const* bits, int reverse,
                                    const pz_glwe_op_params* p, size_t batch) {
    PZ_REQUIRE(p != nullptr, "glwe_blind_retrieval: null params");
    if (nslots == 0 || nbits == 0) return PZ_OK;
    PZ_REQUIRE(slots != nullptr && bits != nullptr, "glwe_blind_retrieval: null argument");
    PZ_TRY(require_op_shape(p, "glwe_blind_retrieval"));
    PZ_REQUIRE(p->a_base2k == p->key_base2k && p->res_base2k == p->key_base2k, "glwe_blind_retrieval: the slots and the GGSWs share one base2k");
    PZ_REQUIRE(p->a_size == p->res_size, "glwe_blind_retrieval: all slots share one layout (p->a_size == p->res_size)");
    for (size_t i = 0; i < nbits; ++i) PZ_REQUIRE(bits[i] != nullptr, "glwe_blind_retrieval: GGSW %zu is null", i);
    PZ_ENTER(M);
    PZ_REQUIRE(is_device_ptr(slots), "batched entry points take device pointers");
    std::vector<const double*> keys(nbits);
    for (size_t i = 0; i < nbits; ++i) PZ_TRY(resolve_key(M, bits[i], ggsw_key_bytes(M, p), &keys[i]));
    if (batch == 0) return PZ_OK;
    KeyHash k = graph_key(M, GRAPH_BLIND_RETRIEVAL, slots, nslots, nbits, reverse != 0, batch, *p, rt_knob("POULPY_DBG_CMUX_FUSED", 1));
    for (size_t i = 0; i < nbits; ++i) k.add(keys[i]);
    PZ_TRY(with_graph(M, k.h, [&]() { return glwe_blind_retrieval_levels(M, slots, nslots, nbits, keys.data(), reverse, p, batch); }));
    return finish_call(M, false);
}
}  // extern "C"
