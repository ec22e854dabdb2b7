// api_ggsw.hip — the GGSW and automorphism-key composites behind the C ABI, each a loop of glwe_op (api_glwe.hip) over the entries of a matrix of
// GLWEs: ggsw_external_product (poulpy-core external_product/ggsw.rs:54-58), ggsw_expand_row / ggsw_from_gglwe (conversion/gglwe_to_ggsw.rs:32-268),
// ggsw_keyswitch (keyswitching/ggsw.rs:37-85), ggsw_automorphism (automorphism/ggsw_ct.rs:32-82) and glwe_automorphism_key_automorphism
// (automorphism/gglwe_atk.rs:42-155).  DESIGN.md 4.4b.
#include <algorithm>

#include "api_common.hpp"
#include "glwe_call.hpp"

using namespace pz;

namespace pz {
// ggsw_expand_row (conversion/gglwe_to_ggsw.rs:116-268): column `col` >= 1 of every row is the key switch of the mask of
// res.at(row, 0) by tsk.at(col - 1), with the body of res.at(row, 0) added to column `col` of the big value before the
// normalization.  The entries (row, 0) of `count` contiguous GGSWs are `count * dnum` ciphertexts at a fixed stride, so
// each column is one batched key switch; column 0 is left untouched.
int ggsw_expand_row(pz_module* M, int64_t* ggsw, size_t dnum, const double* const* tsk_pmat, const pz_glwe_op_params* p, size_t count) {
    PZ_REQUIRE(p != nullptr && tsk_pmat != nullptr, "null params");
    PZ_REQUIRE(p->a_size == p->res_size && p->a_base2k == p->res_base2k, "ggsw_expand_row: a and res describe the same GGSW");
    PZ_REQUIRE(dnum >= 1, "ggsw_expand_row: empty GGSW");
    const size_t cols = p->rank + 1;
    const long long ct = (long long)M->n * (long long)cols * (long long)p->res_size;
    for (size_t col = 1; col < cols; ++col) {
        PZ_REQUIRE(tsk_pmat[col - 1] != nullptr, "ggsw_expand_row: null tensor key");
        OpLayout lay{ct * (long long)cols, ct * (long long)cols, (int)col};
        PZ_TRY(glwe_op(M, GlweKind::KeySwitch, ggsw + (long long)col * ct, ggsw, tsk_pmat[col - 1], p, count * dnum, nullptr, &lay));
    }
    return PZ_OK;
}
}  // namespace pz

extern "C" {
// ggsw_external_product (external_product/ggsw.rs:54-58): every (row, column) entry of the GGSW `a` is a GLWE and the entries
// are contiguous in the MatZnx layout, so the operation is one batched external product over dnum_a * (rank+1) ciphertexts
int pz_ggsw_external_product(pz_module* M, int64_t* res, const int64_t* a, size_t a_dnum, const double* ggsw_pmat,
                             const pz_glwe_op_params* p) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    return glwe_op(M, GlweKind::ExternalProduct, res, a, ggsw_pmat, p, a_dnum * (p->rank + 1));
}
int pz_ggsw_expand_row_batched(pz_module* M, int64_t* ggsw, size_t dnum, const double* const* tsk_pmat, const pz_glwe_op_params* p,
                               size_t count) {
    PZ_ENTER(M);
    return ggsw_expand_row(M, ggsw, dnum, tsk_pmat, p, count);
}

// ggsw_from_gglwe (conversion/gglwe_to_ggsw.rs:32-61): entries (row, 0) of the GGSW are copies of the entries (row, 0) of
// the GGLWE `a` (glwe_copy), then ggsw_expand_row.  `count` contiguous GGLWEs -> `count` contiguous GGSWs, one strided copy.
int pz_ggsw_from_gglwe_batched(pz_module* M, int64_t* ggsw, const int64_t* a, size_t a_cols_in, size_t dnum,
                               const double* const* tsk_pmat, const pz_glwe_op_params* p, size_t count) {
    PZ_ENTER(M);
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE(is_device_ptr(ggsw) && is_device_ptr(a), "batched entry points take device pointers");
    PZ_REQUIRE(a_cols_in >= 1 && dnum >= 1, "ggsw_from_gglwe: empty GGLWE");
    PZ_REQUIRE((const void*)ggsw != (const void*)a, "ggsw_from_gglwe: res must not alias a");
    const size_t cols = p->rank + 1;
    const long long n = (long long)M->n, ct = n * (long long)cols * (long long)p->res_size;
    PZ_TRY(launch_ew(M, EW_COPY, ggsw, (long long)cols * ct, n, a, (long long)a_cols_in * ct, n, nullptr, 0, 0, (int)(cols * p->res_size),
                     (int)(count * dnum)));
    return ggsw_expand_row(M, ggsw, dnum, tsk_pmat, p, count);  // (the module lock is not recursive)
}
}  // extern "C"

// ------------------------------------------------------------------------------
// glwe_automorphism_key_automorphism (automorphism/gglwe_atk.rs:42-155), ggsw_keyswitch (keyswitching/ggsw.rs:37-85), ggsw_automorphism
// (automorphism/ggsw_ct.rs:32-82)
// ------------------------------------------------------------------------------
// the spectrum of phi_g(K) read from the spectrum of K (evaluation points w^(4q+1)): index q' holds K[g q' + (g-1)/4] for g = 1 mod 4,
// the conjugate of K[-g q' - (g+1)/4] for g = 3 mod 4 - the map spectral_perm (api_glwe.hip) applies on the middle kernel's stores, here on the key
static KeyPerm key_perm(unsigned g, unsigned mm) {
    KeyPerm kp;
    if ((g & 3u) == 1u) {
        kp.mul = g & (mm - 1u);
        kp.add = ((g - 1u) >> 2) & (mm - 1u);
    } else {
        kp.conj = true;
        kp.mul = (mm - (g & (mm - 1u))) & (mm - 1u);
        kp.add = (mm - (((g + 1u) >> 2) & (mm - 1u))) & (mm - 1u);
    }
    return kp;
}
// Route table: the fast form where the limbs of `a` reach the forward transform as they are and the three-kernel pipeline of
// a 128-point-row plan runs the key switch - dsize 1, one base2k, not the N = 4096 two-kernel path, every stage on
// Off by default: no rate of the fast form against the composition has been measured yet - POULPY_DBG_KEYAUTO_SPECTRAL=1 selects it
constexpr int kKeyautoSpectralDefault = 0;
static bool keyauto_fast_applies(const GlweCall& c) {
    const bool env_on = (rt_knob("POULPY_DBG_KEYAUTO_SPECTRAL", kKeyautoSpectralDefault) != 0);   // (read per call: once per GGLWE batch, and tests flip it)
    const pz_module* M = c.M;
    return env_on && M->plan.m2 == 128 && M->dbg_stages == 7 && !c.digits && !c.cross_out && !c.s.convert &&
           fused_applies(M, c.p, c.s, GlweKind::KeySwitch) && !n4096_two_kernel(c);
}
// `batch` packed entries: res[e] = phi_g(glwe_keyswitch(phi_p(a[e]), key)), p = a_gal, g = p^-1 mod 2N
static int keyauto_entries(pz_module* M, int64_t* res, const int64_t* a, const double* key, const pz_glwe_op_params* p, size_t batch, int64_t a_gal) {
    GlweCall c;
    PZ_TRY(glwe_call_init(c, M, GlweKind::KeySwitch, res, a, key, p, batch, nullptr, nullptr, nullptr));
    if (batch == 0) return PZ_OK;
    const unsigned g = inv_mod_2n((long long)a_gal, c.n);
    if (keyauto_fast_applies(c)) {
        c.keyauto = true;
        c.ka_p = (unsigned)((unsigned long long)a_gal & (2ull * (unsigned long long)c.n - 1ull));
        c.ka_perm = key_perm(g, (unsigned)M->m);
        dispatch_note(M, "key composition: key switch by the permuted key (spectral form)");
        return glwe_fused(c);
    }
    // composition: phi_p of every entry into the second workspace (before anything is written: in-place calls included), then the
    // automorphism family in mode 0 with the inverse element
    dispatch_note(M, "key composition: automorphism + glwe_automorphism (composition)");
    PZ_TRY(ws2_reserve(M, batch * (size_t)c.a_ct * 8));
    int64_t* tmp = (int64_t*)M->ws2;
    const int polys = c.s.cols_a * (int)p->a_size;
    PolyMap pm{1, polys, c.a_ct, 0, c.n, 0};
    PZ_TRY(launch_automorphism(M, (int)batch * polys, (const long long*)a, pm, (long long*)tmp, pm, g, AUTO_SIGN));
    AutoSpec au{(long long)g, 0};
    return glwe_op(M, GlweKind::Automorphism, res, tmp, key, p, batch, &au);
}

extern "C" {
int pz_glwe_automorphism_key_automorphism_batched(pz_module* M, int64_t* res, size_t res_dnum, const int64_t* a, size_t a_dnum, int64_t a_gal,
                                                  const double* key_pmat, const pz_glwe_op_params* p, size_t count) {
    // (the argument checks that need no module come first)
    PZ_REQUIRE(p != nullptr, "null params");
    PZ_REQUIRE((a_gal & 1) != 0, "glwe_automorphism_key_automorphism: the Galois element of the input key must be odd");
    PZ_REQUIRE(res_dnum >= 1 && res_dnum <= a_dnum, "glwe_automorphism_key_automorphism: res has more rows than a (or none)");
    PZ_REQUIRE(p->res_base2k == p->a_base2k, "glwe_automorphism_key_automorphism: res and a share one base2k");
    PZ_REQUIRE(p->rank >= 1 && p->rank_out == p->rank, "glwe_automorphism_key_automorphism: the keys map rank -> rank");
    PZ_ENTER(M);
    PZ_TRY(require_op_shape(p, "glwe op"));
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a) && key_pmat != nullptr, "batched entry points take device pointers");
    if ((const void*)res == (const void*)a)
        PZ_REQUIRE(res_dnum == a_dnum && p->res_size == p->a_size, "in-place call with different layouts for a and res");
    const size_t rank = p->rank, cols = rank + 1;
    const double* key = nullptr;
    PZ_TRY(resolve_key(M, key_pmat, glwe_key_bytes(M, p), &key));
    const long long a_ct = (long long)M->n * (long long)cols * (long long)p->a_size, res_ct = (long long)M->n * (long long)cols * (long long)p->res_size;
    // rows of `a` beyond res_dnum are not computed: one call over everything when the row counts agree, else one per GGLWE
    if (res_dnum == a_dnum || count <= 1) PZ_TRY(keyauto_entries(M, res, a, key, p, count * res_dnum * rank, a_gal));
    else
        for (size_t i = 0; i < count; ++i)
            PZ_TRY(keyauto_entries(M, res + (long long)(i * res_dnum * rank) * res_ct, a + (long long)(i * a_dnum * rank) * a_ct, key, p,
                                   res_dnum * rank, a_gal));
    return finish_call(M, false);
}

// entries (row, 0) of `count` GGSWs through glwe_keyswitch (ggsw.rs:52-54, :80-82), then ggsw_expand_row on res
int pz_ggsw_keyswitch_batched(pz_module* M, int64_t* res, const int64_t* a, size_t dnum, const double* key_pmat, const double* const* tsk_pmat,
                              const pz_glwe_op_params* kp, const pz_glwe_op_params* tp, size_t count) {
    PZ_REQUIRE(kp != nullptr && tp != nullptr && tsk_pmat != nullptr, "null params");
    PZ_REQUIRE(dnum >= 1, "ggsw_keyswitch: empty GGSW");
    PZ_REQUIRE(tp->rank == kp->rank_out && tp->res_size == kp->res_size && tp->res_base2k == kp->res_base2k,
               "ggsw_keyswitch: the expansion's parameters describe res");
    PZ_ENTER(M);
    PZ_REQUIRE(kp->a_size >= 1 && kp->res_size >= 1 && kp->key_size >= 1 && kp->dnum >= 1, "glwe op: empty shape");
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a) && key_pmat != nullptr, "batched entry points take device pointers");
    const long long n = (long long)M->n;
    const long long a_row = n * (long long)(kp->rank + 1) * (long long)(kp->rank + 1) * (long long)kp->a_size;
    const long long res_row = n * (long long)(kp->rank_out + 1) * (long long)(kp->rank_out + 1) * (long long)kp->res_size;
    if ((const void*)res == (const void*)a) PZ_REQUIRE(a_row == res_row, "in-place call with different layouts for a and res");
    const double* key = nullptr;
    PZ_TRY(resolve_key(M, key_pmat, glwe_key_bytes(M, kp), &key));
    OpLayout lay{a_row, res_row, 0};
    PZ_TRY(glwe_op(M, GlweKind::KeySwitch, res, a, key, kp, count * dnum, nullptr, &lay));
    PZ_TRY(ggsw_expand_row(M, res, dnum, tsk_pmat, tp, count));   // (the module lock is not recursive)
    return finish_call(M, false);
}

// entries (row, 0), row < res_dnum, of `count` GGSWs through glwe_automorphism (ggsw_ct.rs:54-56, :77-79), then ggsw_expand_row on res.  The
// automorphism family takes packed ciphertexts: the entries are staged through a packed copy in the second workspace.
int pz_ggsw_automorphism_batched(pz_module* M, int64_t* res, size_t res_dnum, const int64_t* a, size_t a_dnum, const double* key_pmat, int64_t gal,
                                 const double* const* tsk_pmat, const pz_glwe_op_params* kp, const pz_glwe_op_params* tp, size_t count) {
    PZ_REQUIRE(kp != nullptr && tp != nullptr && tsk_pmat != nullptr, "null params");
    PZ_REQUIRE((gal & 1) != 0, "ggsw_automorphism: the Galois element must be odd");
    PZ_REQUIRE(res_dnum >= 1 && res_dnum <= a_dnum, "ggsw_automorphism: res has more rows than a (or none)");
    PZ_REQUIRE(kp->rank_out == kp->rank && tp->rank == kp->rank && tp->res_size == kp->res_size && tp->res_base2k == kp->res_base2k,
               "ggsw_automorphism: rank -> rank, and the expansion's parameters describe res");
    PZ_ENTER(M);
    PZ_REQUIRE(kp->a_size >= 1 && kp->res_size >= 1 && kp->key_size >= 1 && kp->dnum >= 1, "glwe op: empty shape");
    PZ_REQUIRE(is_device_ptr(res) && is_device_ptr(a) && key_pmat != nullptr, "batched entry points take device pointers");
    if ((const void*)res == (const void*)a)
        PZ_REQUIRE(res_dnum == a_dnum && kp->res_size == kp->a_size, "in-place call with different layouts for a and res");
    if (count == 0) return finish_call(M, false);
    const long long n = (long long)M->n;
    const size_t cols = kp->rank + 1;
    const long long a_ct = n * (long long)cols * (long long)kp->a_size, res_ct = n * (long long)cols * (long long)kp->res_size;
    const double* key = nullptr;
    PZ_TRY(resolve_key(M, key_pmat, glwe_key_bytes(M, kp), &key));
    const size_t ent = count * res_dnum;
    PZ_TRY(ws2_reserve(M, align256(ent * (size_t)a_ct * 8) + ent * (size_t)res_ct * 8));
    int64_t* pa = (int64_t*)M->ws2;
    int64_t* pr = (int64_t*)((char*)M->ws2 + align256(ent * (size_t)a_ct * 8));
    for (size_t i = 0; i < count; ++i)
        PZ_TRY(launch_ew(M, EW_COPY, pa + (long long)(i * res_dnum) * a_ct, a_ct, n, a + (long long)(i * a_dnum) * (long long)cols * a_ct,
                         (long long)cols * a_ct, n, nullptr, 0, 0, (int)(cols * kp->a_size), (int)res_dnum));
    AutoSpec au{(long long)gal, 0};
    PZ_TRY(glwe_op(M, GlweKind::Automorphism, pr, pa, key, kp, ent, &au));
    PZ_TRY(launch_ew(M, EW_COPY, res, (long long)cols * res_ct, n, pr, res_ct, n, nullptr, 0, 0, (int)(cols * kp->res_size), (int)ent));
    PZ_TRY(ggsw_expand_row(M, res, res_dnum, tsk_pmat, tp, count));
    return finish_call(M, false);
}
}  // extern "C"
