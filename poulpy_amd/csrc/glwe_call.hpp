// glwe_call.hpp — what the composite units (api_ggsw.hip, api_gates.hip, api_bdd.hip, api_trace.hip, api_br.hip, api_fhe_uint.hip, api_cnv.hip)
// need from the product engine in api_glwe.hip, and the internal calls those units make into each other.  Declarations only: the shapes and
// route predicates, GlweCall and the three pipelines, then the namespace pz functions that run for a caller who holds the module lock.
#pragma once
#include "api_glwe.hpp"

// Automorphism family on top of the key switch / strided ciphertexts: see glwe_op in api_glwe.hip
struct AutoSpec {
    long long p;
    int mode;
};
// ciphertexts that are not tightly packed (the entries of one column of a GGSW) and a body that lands in another column
struct OpLayout {
    long long a_stride, res_stride;  // in i64 elements between consecutive ciphertexts
    int body_col;
};
// what a call of glwe_op computes; the values are the `keyswitch` argument of pz_glwe_op_workspace_bytes
enum class GlweKind : int { ExternalProduct = 0, KeySwitch = 1, Automorphism = 2, TensorRelin = 3 };

// ------------------------------------------------------------------------------
// shapes, pipeline choice (api_glwe.hip)
// ------------------------------------------------------------------------------
struct OpShape {
    int cols_a, cols_in, cols_out;  // columns of `a`, VMP input columns, output columns
    int a_col0;                     // first column of `a` that enters the product
    int a_size_eff;                 // limbs of `a` in the key's base (after optional conversion)
    bool convert;
};
OpShape op_shape(const pz_glwe_op_params* p, GlweKind kind);
size_t pick_chunk(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, size_t batch);
bool fused_applies(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, GlweKind kind);
bool small_ring_applies(const pz_module* M, const pz_glwe_op_params* p, const OpShape& s, GlweKind kind, bool packed);

// everything a call of glwe_op derives from its arguments before it launches anything
struct GlweCall {
    pz_module* M;
    const pz_glwe_op_params* p;
    OpShape s;
    GlweKind kind;
    bool ks, tensor;       // kind != ExternalProduct, kind == TensorRelin
    const AutoSpec* au;
    const OpLayout* lay;
    int64_t* res; const int64_t* a; const double* pmat;
    size_t batch, chunk;
    long long n;
    int dsize, dnum, ksz;
    int npi, npo;          // polynomials per ciphertext entering / leaving the product
    int nrows, ncols;      // the key matrix: dnum * cols_in rows, cols_out * key_size columns
    long long a_ct, res_ct, a_bs, res_bs;   // packed sizes and actual strides of one ciphertext (i64 elements)
    int body_col;
    bool au_big;           // add / sub / sub_negate: phi acts on the big value
    unsigned au_p, au_g;   // Galois element mod 2n and its inverse
    bool digits, cross_out;
    bool want_rsh;         // glwe_trace asked for the one-bit shift on the way out
    bool* post_rsh;        // ... and is told here whether it happened
    // relinearization of a GLWETensor that exists only as 16-bit digits in the fused tail's tile order (glwe_relin_t16, api_glwe.hip):
    // a16[column][ciphertext of this call][limb][n], a16_cs int16 elements between columns; `a` is not read
    const short* a16 = nullptr;
    long long a16_cs = 0;
    // glwe_automorphism_key_automorphism, fast form (keyauto_entries, api_ggsw.hip): a plain key switch by phi_g(key) - the row-sliced copy is read
    // through ka_perm - whose carry chains run between the signs of X -> X^ka_p
    bool keyauto = false;
    unsigned ka_p = 0;
    KeyPerm ka_perm;
    // CMUX (glwe_cmux, api_gates.hip; eval.rs:565-571): every column of `add` - add_size limbs, add_bs elements between ciphertexts - joins the big value in
    // front of the carry chain (vec_znx_big_add_small_assign on every column).  diff != null, the fused routes: `a` = t - f is not in memory, the
    // small-ring forward stage forms it from the two sources (SmallDiff; its maps address the whole call, wave_diff moves them to a wave)
    const int64_t* add = nullptr;
    long long add_bs = 0;
    int add_size = 0;
    const SmallDiff* diff = nullptr;
    // conditional swap (glwe_cswap, api_gates.hip; eval.rs:444-461): a SECOND result from the same big value, res2 = normalize(res2 - big) on every column
    // (vec_znx_big_sub_small_a), in place on its own operand; res2_size limbs, res2_bs elements between ciphertexts.  `add` is the first one's operand
    int64_t* res2 = nullptr;
    long long res2_bs = 0;
    int res2_size = 0;
    // rotated-source key switch (glwe_keyswitch_rot_nolock, api_glwe.hip): ciphertext b of the call is X^rot of ciphertext `word` of `a`, (word, rot) =
    // rot_tab[b] on the device; the one-kernel small-ring form applies the rotation where it reads the mask columns and the body operand
    const RotSrc* rot_tab = nullptr;
    int64_t* res2_at(size_t b0) const { return res2 + (long long)b0 * res2_bs; }
    int cols_in() const { return s.cols_in; }
    int64_t* res_at(size_t b0) const { return res + (long long)b0 * res_bs; }
};
static inline const char* gate_name(const GlweCall& c) { return c.res2 ? "cswap" : "cmux"; }   // (for the dispatch notes)
int glwe_call_init(GlweCall& c, pz_module* M, GlweKind kind, int64_t* res, const int64_t* a, const double* pmat, const pz_glwe_op_params* p,
                   size_t batch, const AutoSpec* au, const OpLayout* lay, bool* post_rsh);
bool n4096_two_kernel(const GlweCall& c);
bool cmux_fused_route(const GlweCall& c);
// the three pipelines on an initialised call (glwe_op picks one; the gates and the key composition enter them with their own fields set)
int glwe_fused(const GlweCall& c);
int glwe_small_ring(const GlweCall& c);
int glwe_unfused(const GlweCall& c);

// the trace in the keys' base (api_trace.hip): src -> tmp (tmp_size limbs, key_base2k), glwe_trace there, tmp -> res.  src and res have the
// layout (res_size, res_base2k) of p and may be the same buffer
int trace_in_key_base(pz_module* M, int64_t* res, const int64_t* src, int64_t* tmp, size_t tmp_size, size_t nsteps, const int64_t* gals,
                      const double* const* key_pmats, const pz_glwe_op_params* p, size_t batch);

// limbs of t and of f of a CMUX; t null: t = X^t_rot f
struct CmuxOperands { uint64_t t_size, f_size; int64_t t_rot; };

// The caller holds the module lock:
namespace pz {
// the batched GLWE product on device-resident data: external product, key switch, automorphism family (kind Automorphism, with au), strided
// ciphertexts with the body landing in another column (lay), tensor relinearization
int glwe_op(pz_module* M, GlweKind kind, int64_t* res, const int64_t* a, const double* pmat, const pz_glwe_op_params* p, size_t batch,
            const AutoSpec* au = nullptr, const OpLayout* lay = nullptr, bool* post_rsh = nullptr);
// post_rsh (glwe_trace): in: the caller would like the result shifted right by one bit (vec_znx_rsh_assign on every column) as it is
// stored; out: whether the path taken did that (spectral automorphism forms on the 256 x 128 plan) - otherwise the caller shifts itself
// glwe_trace_assign on a batch (poulpy-core glwe_trace.rs:129-176): one prepared key per step.  first_shifted (res in the keys' base,
// nsteps >= 1): the caller has already applied the one-bit vec_znx_rsh_assign the first step opens with (k_word_pre)
int glwe_trace(pz_module* M, int64_t* res, size_t nsteps, const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p,
               size_t batch, bool first_shifted = false);
// tensor relinearization of GLWETensors held as 16-bit digits in the fused tail's tile order (api_cnv.hip's fused multiply + relinearize)
bool glwe_relin_t16_supported(const pz_module* M, const pz_glwe_op_params* p);
size_t glwe_relin_chunk(const pz_module* M, const pz_glwe_op_params* p, size_t batch);
int glwe_relin_t16(pz_module* M, int64_t* res, const short* a16, long long a16_cs, const double* pmat, const pz_glwe_op_params* p, size_t batch);
// pz_glwe_sum_batched / pz_glwe_combine_batched (api_sum.hip, api_combine.hip); dry: every check and the plan, nothing launched
int glwe_sum_nolock(pz_module* M, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                    const int* shared, const size_t* a_size, const int* join, const size_t* k, const int* sign, size_t nterms, size_t batch, bool dry);
int glwe_combine_nolock(pz_module* M, int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands,
                        const pz_glwe_term* terms, size_t nterms, int normalize, size_t batch, bool dry);
// pz_bdd_circuit_execute_batched without the module lock and the closing finish_call: the argument checks that need no module (precheck; *nothing:
// the call has no ciphertext to write), then the call itself (pz_fhe_uint_execute_batched runs both halves under one lock)
int bdd_circuit_execute_precheck(const pz_module* M, const pz_bdd_circuit* c, const int64_t* out, size_t n_out, const double* const* bits, size_t nbits,
                                 const pz_glwe_op_params* p, size_t batch, bool* nothing);
int bdd_circuit_execute(pz_module* M, const pz_bdd_circuit* c, int64_t* out, size_t n_out, const double* const* bits, size_t nbits,
                        const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes, size_t batch);
// ggsw_expand_row on `count` GGSWs (conversion/gglwe_to_ggsw.rs:116-268)
int ggsw_expand_row(pz_module* M, int64_t* ggsw, size_t dnum, const double* const* tsk_pmat, const pz_glwe_op_params* p, size_t count);
// CMUX on device pointers with the key resolved (api_gates.hip); res2 != null: the conditional swap
int glwe_cmux(pz_module* M, int64_t* res, const int64_t* t, const int64_t* f, const double* key, const pz_glwe_op_params* p,
              const CmuxOperands* o, size_t batch, int64_t* res2 = nullptr);
// glwe_pack on `batch` packing problems (api_trace.hip); trace_size = 0: one base2k for ciphertexts, keys and result
int glwe_pack(pz_module* M, int64_t* res, size_t nslots, const uint64_t* indices, int64_t* const* cts, size_t log_gap_out,
              const int64_t* gals, const double* const* key_pmats, const pz_glwe_op_params* p, void* tmp, size_t tmp_bytes,
              size_t batch, size_t trace_size);
}  // namespace pz
