// poulpy_hip.hpp — header-only C++ mirror of the reference's operator interface for the FFT64 hot
// path, on top of the C ABI (poulpy_hip.h).  Same method names, argument order and error behaviour
// as poulpy-hal's api traits (poulpy-hal/src/api/{vec_znx_dft,svp_ppol,vmp_pmat,vec_znx_big}.rs):
// shape violations and runtime failures throw pz::Error where the reference panics.
// Containers are non-owning views with the reference's layout (znx_base.rs:52-82).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "poulpy_hip.h"

namespace pz {

struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string& what) : std::runtime_error(what), status(st) {}
};
inline void check(int st, const char* what) {
    if (st != 0) throw Error(st, std::string(what) + ": " + pz_last_error());
}

template <typename T>
struct Znx {  // VecZnx (T = int64_t), VecZnxBig (int64_t), VecZnxDft (double)
    T* data;
    size_t n, cols, size;
    T* at(size_t col, size_t limb) const { return data + n * (limb * cols + col); }
};
using VecZnx = Znx<int64_t>;
using VecZnxBig = Znx<int64_t>;
using VecZnxDft = Znx<double>;
struct ScalarZnx { int64_t* data; size_t n, cols; };
struct SvpPPol { double* data; size_t n, cols; };
struct MatZnx { int64_t* data; size_t n, rows, cols_in, cols_out, size; };
struct VmpPMat { double* data; size_t n, rows, cols_in, cols_out, size; };

class Module {  // Module<FFT64Hip>, poulpy-hal/src/layouts/module.rs:97-189
  public:
    explicit Module(uint64_t n) { check_abi(); check(pz_module_new(n, &m_), "Module::new"); }
    Module(uint64_t n, int device) { check_abi(); check(pz_module_new_on_device(n, device, &m_), "Module::new"); }
    // a library built from another revision of poulpy_hip.h would read mismatched struct layouts: refuse it before the first call
    static void check_abi() {
        if (pz_abi_version() != PZ_ABI_VERSION)
            throw Error(PZ_ERR_INVALID, "libpoulpy_hip ABI version " + std::to_string(pz_abi_version()) + ", header expects " + std::to_string(PZ_ABI_VERSION));
    }
    ~Module() { pz_module_free(m_); }
    Module(const Module&) = delete;
    Module& operator=(const Module&) = delete;
    uint64_t n() const { return pz_module_n(m_); }
    pz_module* raw() const { return m_; }
    void sync() { check(pz_module_sync(m_), "sync"); }

    // VecZnxDft
    void vec_znx_dft_apply(size_t step, size_t offset, VecZnxDft& res, size_t res_col, const VecZnx& a, size_t a_col) {
        check(pz_vec_znx_dft_apply(m_, step, offset, res.data, res.cols, res.size, res_col, a.data, a.cols, a.size, a_col), "vec_znx_dft_apply");
    }
    size_t vec_znx_idft_apply_tmp_bytes() const { return pz_vec_znx_idft_apply_tmp_bytes(m_); }
    void vec_znx_idft_apply(VecZnxBig& res, size_t res_col, const VecZnxDft& a, size_t a_col) {
        check(pz_vec_znx_idft_apply(m_, res.data, res.cols, res.size, res_col, a.data, a.cols, a.size, a_col), "vec_znx_idft_apply");
    }
    void vec_znx_idft_apply_tmpa(VecZnxBig& res, size_t res_col, VecZnxDft& a, size_t a_col) {
        check(pz_vec_znx_idft_apply_tmpa(m_, res.data, res.cols, res.size, res_col, a.data, a.cols, a.size, a_col), "vec_znx_idft_apply_tmpa");
    }
    VecZnxBig vec_znx_idft_apply_consume(VecZnxDft a) {
        check(pz_vec_znx_idft_apply_consume(m_, a.data, a.cols, a.size), "vec_znx_idft_apply_consume");
        return VecZnxBig{reinterpret_cast<int64_t*>(a.data), a.n, a.cols, a.size};
    }
    void vec_znx_dft_add_into(VecZnxDft& r, size_t rc, const VecZnxDft& a, size_t ac, const VecZnxDft& b, size_t bc) {
        check(pz_vec_znx_dft_add_into(m_, r.data, r.cols, r.size, rc, a.data, a.cols, a.size, ac, b.data, b.cols, b.size, bc), "vec_znx_dft_add_into");
    }
    void vec_znx_dft_sub(VecZnxDft& r, size_t rc, const VecZnxDft& a, size_t ac, const VecZnxDft& b, size_t bc) {
        check(pz_vec_znx_dft_sub(m_, r.data, r.cols, r.size, rc, a.data, a.cols, a.size, ac, b.data, b.cols, b.size, bc), "vec_znx_dft_sub");
    }
    void vec_znx_dft_add_assign(VecZnxDft& r, size_t rc, const VecZnxDft& a, size_t ac) {
        check(pz_vec_znx_dft_add_assign(m_, r.data, r.cols, r.size, rc, a.data, a.cols, a.size, ac), "vec_znx_dft_add_assign");
    }
    void vec_znx_dft_add_scaled_assign(VecZnxDft& r, size_t rc, const VecZnxDft& a, size_t ac, int64_t a_scale) {
        check(pz_vec_znx_dft_add_scaled_assign(m_, r.data, r.cols, r.size, rc, a.data, a.cols, a.size, ac, a_scale), "vec_znx_dft_add_scaled_assign");
    }
    void vec_znx_dft_sub_assign(VecZnxDft& r, size_t rc, const VecZnxDft& a, size_t ac) {
        check(pz_vec_znx_dft_sub_assign(m_, r.data, r.cols, r.size, rc, a.data, a.cols, a.size, ac), "vec_znx_dft_sub_assign");
    }
    void vec_znx_dft_sub_negate_assign(VecZnxDft& r, size_t rc, const VecZnxDft& a, size_t ac) {
        check(pz_vec_znx_dft_sub_negate_assign(m_, r.data, r.cols, r.size, rc, a.data, a.cols, a.size, ac), "vec_znx_dft_sub_negate_assign");
    }
    void vec_znx_dft_copy(size_t step, size_t offset, VecZnxDft& r, size_t rc, const VecZnxDft& a, size_t ac) {
        check(pz_vec_znx_dft_copy(m_, step, offset, r.data, r.cols, r.size, rc, a.data, a.cols, a.size, ac), "vec_znx_dft_copy");
    }
    void vec_znx_dft_zero(VecZnxDft& r, size_t rc) { check(pz_vec_znx_dft_zero(m_, r.data, r.cols, r.size, rc), "vec_znx_dft_zero"); }

    // SVP
    void svp_prepare(SvpPPol& res, size_t res_col, const ScalarZnx& a, size_t a_col) {
        check(pz_svp_prepare(m_, res.data, res.cols, res_col, a.data, a.cols, a_col), "svp_prepare");
    }
    void svp_apply_dft(VecZnxDft& res, size_t res_col, const SvpPPol& a, size_t a_col, const VecZnx& b, size_t b_col) {
        check(pz_svp_apply_dft(m_, res.data, res.cols, res.size, res_col, a.data, a.cols, a_col, b.data, b.cols, b.size, b_col), "svp_apply_dft");
    }
    void svp_apply_dft_to_dft(VecZnxDft& res, size_t res_col, const SvpPPol& a, size_t a_col, const VecZnxDft& b, size_t b_col) {
        check(pz_svp_apply_dft_to_dft(m_, res.data, res.cols, res.size, res_col, a.data, a.cols, a_col, b.data, b.cols, b.size, b_col), "svp_apply_dft_to_dft");
    }
    void svp_apply_dft_to_dft_assign(VecZnxDft& res, size_t res_col, const SvpPPol& a, size_t a_col) {
        check(pz_svp_apply_dft_to_dft_assign(m_, res.data, res.cols, res.size, res_col, a.data, a.cols, a_col), "svp_apply_dft_to_dft_assign");
    }

    // VMP
    size_t vmp_prepare_tmp_bytes(size_t rows, size_t ci, size_t co, size_t size) const { return pz_vmp_prepare_tmp_bytes(m_, rows, ci, co, size); }
    void vmp_prepare(VmpPMat& res, const MatZnx& a) {
        if (res.rows != a.rows || res.cols_in != a.cols_in || res.cols_out != a.cols_out || res.size != a.size)
            throw Error(PZ_ERR_INVALID, "vmp_prepare: shape mismatch");
        check(pz_vmp_prepare(m_, res.data, a.data, a.rows, a.cols_in, a.cols_out, a.size), "vmp_prepare");
    }
    void vmp_apply_dft(VecZnxDft& res, const VecZnx& a, const VmpPMat& b) {
        check(pz_vmp_apply_dft(m_, res.data, res.cols, res.size, a.data, a.cols, a.size, b.data, b.rows, b.cols_in, b.cols_out, b.size), "vmp_apply_dft");
    }
    void vmp_apply_dft_to_dft(VecZnxDft& res, const VecZnxDft& a, const VmpPMat& b, size_t limb_offset) {
        check(pz_vmp_apply_dft_to_dft(m_, res.data, res.cols, res.size, a.data, a.cols, a.size, b.data, b.rows, b.cols_in, b.cols_out, b.size, limb_offset), "vmp_apply_dft_to_dft");
    }
    void vmp_zero(VmpPMat& r) { check(pz_vmp_zero(m_, r.data, r.rows, r.cols_in, r.cols_out, r.size), "vmp_zero"); }

    // VecZnxBig
    size_t vec_znx_big_normalize_tmp_bytes() const { return pz_vec_znx_big_normalize_tmp_bytes(m_); }
    void vec_znx_big_normalize(VecZnx& res, size_t res_base2k, int64_t res_offset, size_t res_col, const VecZnxBig& a, size_t a_base2k, size_t a_col) {
        check(pz_vec_znx_big_normalize(m_, res.data, res.cols, res.size, res_base2k, res_offset, res_col, a.data, a.cols, a.size, a_base2k, a_col), "vec_znx_big_normalize");
    }
    void vec_znx_big_add_small_assign(VecZnxBig& res, size_t res_col, const VecZnx& a, size_t a_col) {
        check(pz_vec_znx_big_add_small_assign(m_, res.data, res.cols, res.size, res_col, a.data, a.cols, a.size, a_col), "vec_znx_big_add_small_assign");
    }
    // X -> X^p on i64 containers (hal_impl.rs:236-243, :517-524)
    void vec_znx_automorphism(int64_t p, VecZnx& res, size_t res_col, const VecZnx& a, size_t a_col) {
        check(pz_vec_znx_automorphism(m_, p, res.data, res.cols, res.size, res_col, a.data, a.cols, a.size, a_col), "vec_znx_automorphism");
    }
    void vec_znx_automorphism_assign(int64_t p, VecZnx& res, size_t res_col) {
        check(pz_vec_znx_automorphism_assign(m_, p, res.data, res.cols, res.size, res_col), "vec_znx_automorphism_assign");
    }
    void vec_znx_big_automorphism(int64_t p, VecZnxBig& res, size_t res_col, const VecZnxBig& a, size_t a_col) {
        check(pz_vec_znx_big_automorphism(m_, p, res.data, res.cols, res.size, res_col, a.data, a.cols, a.size, a_col), "vec_znx_big_automorphism");
    }
    void vec_znx_big_automorphism_assign(int64_t p, VecZnxBig& res, size_t res_col) {
        check(pz_vec_znx_big_automorphism_assign(m_, p, res.data, res.cols, res.size, res_col), "vec_znx_big_automorphism_assign");
    }

    // batched device-resident GLWE operations (CoreImpl level)
    void glwe_external_product_batched(int64_t* res, const int64_t* a, const double* ggsw, const pz_glwe_op_params& p, size_t batch) {
        check(pz_glwe_external_product_batched(m_, res, a, ggsw, &p, batch), "glwe_external_product_batched");
    }
    void glwe_keyswitch_batched(int64_t* res, const int64_t* a, const double* key, const pz_glwe_op_params& p, size_t batch) {
        check(pz_glwe_keyswitch_batched(m_, res, a, key, &p, batch), "glwe_keyswitch_batched");
    }
    // mode: PZ_AUTO | PZ_AUTO_ADD | PZ_AUTO_SUB | PZ_AUTO_SUB_NEGATE (poulpy-core automorphism/glwe_ct.rs:51-275)
    void glwe_automorphism_batched(int64_t* res, const int64_t* a, const double* key, const pz_glwe_op_params& p, int64_t gal, int mode, size_t batch) {
        check(pz_glwe_automorphism_batched(m_, res, a, key, &p, gal, mode, batch), "glwe_automorphism_batched");
    }
    // one batch rotated by nrot Galois elements (PZ_AUTO per element): gals / keys are nrot host arrays, rotation r of ciphertext b is
    // ciphertext r * batch + b of res; res must not overlap a
    void glwe_automorphism_many_batched(int64_t* res, const int64_t* a, size_t nrot, const int64_t* gals, const double* const* keys,
                                        const pz_glwe_op_params& p, size_t batch) {
        check(pz_glwe_automorphism_many_batched(m_, res, a, nrot, gals, keys, &p, batch), "glwe_automorphism_many_batched");
    }
    size_t glwe_automorphism_many_workspace_bytes(const pz_glwe_op_params& p, size_t nrot, size_t batch) const {
        return pz_glwe_automorphism_many_workspace_bytes(m_, &p, nrot, batch);
    }
    // CMUX (bdd_arithmetic/eval.rs:524-626): res = normalize((t - f) (x) ggsw + f); p.a_size = limbs of the difference; res may be t or f.
    // t == nullptr: t = X^t_rot f (one step of glwe_blind_rotation_assign), t_size == f_size
    void glwe_cmux_batched(int64_t* res, const int64_t* t, size_t t_size, int64_t t_rot, const int64_t* f, size_t f_size, const double* ggsw,
                           const pz_glwe_op_params& p, size_t batch) {
        check(pz_glwe_cmux_batched(m_, res, t, t_size, t_rot, f, f_size, ggsw, &p, batch), "glwe_cmux_batched");
    }
    size_t glwe_cmux_workspace_bytes(const pz_glwe_op_params& p, size_t batch) const { return pz_glwe_cmux_workspace_bytes(m_, &p, batch); }
    // glwe_blind_rotation / _assign (bdd_arithmetic/blind_rotation.rs:196-264): bits = nbits host entries, the prepared GGSW of bit i + bit_rsh each
    size_t glwe_blind_rotation_tmp_bytes(const pz_glwe_op_params& p, size_t batch) const { return pz_glwe_blind_rotation_tmp_bytes(m_, &p, batch); }
    void glwe_blind_rotation_batched(int64_t* res, const int64_t* a, size_t nbits, const double* const* bits, bool sign, size_t bit_lsh,
                                     const pz_glwe_op_params& p, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_glwe_blind_rotation_batched(m_, res, a, nbits, bits, sign ? 1 : 0, bit_lsh, &p, tmp, tmp_bytes, batch), "glwe_blind_rotation_batched");
    }
    // Cswap::cswap (bdd_arithmetic/eval.rs:417-461, one base2k) in place on a and b: one external product of b - a, both results from its big value;
    // p.a_size = max(a_size, b_size), p.res_size = a_size; a and b must not overlap
    void glwe_cswap_batched(int64_t* a, size_t a_size, int64_t* b, size_t b_size, const double* ggsw, const pz_glwe_op_params& p, size_t batch) {
        check(pz_glwe_cswap_batched(m_, a, a_size, b, b_size, ggsw, &p, batch), "glwe_cswap_batched");
    }
    size_t glwe_cswap_workspace_bytes(const pz_glwe_op_params& p, size_t batch) const { return pz_glwe_cswap_workspace_bytes(m_, &p, batch); }
    // glwe_blind_retrieval_statefull / _rev (bdd_arithmetic/blind_retrieval.rs:195-266): slots = dense [nslots][batch], bits = nbits host entries
    void glwe_blind_retrieval_batched(int64_t* slots, size_t nslots, size_t nbits, const double* const* bits, bool reverse, const pz_glwe_op_params& p,
                                      size_t batch) {
        check(pz_glwe_blind_retrieval_batched(m_, slots, nslots, nbits, bits, reverse ? 1 : 0, &p, batch), "glwe_blind_retrieval_batched");
    }
    size_t glwe_blind_retrieval_workspace_bytes(const pz_glwe_op_params& p, size_t nslots, size_t nbits, size_t batch) const {
        return pz_glwe_blind_retrieval_workspace_bytes(m_, &p, nslots, nbits, batch);
    }
    // ExecuteBDDCircuit::execute_bdd_circuit (bdd_arithmetic/eval.rs:123-239) on `batch` inputs: c = a compiled circuit (BddCircuit below), out = dense
    // [n_out][batch], bits = HOST array [batch][nbits] of prepared GGSWs (null where the circuit never selects the bit), tmp = device scratch
    size_t bdd_circuit_execute_tmp_bytes(const pz_bdd_circuit* c, const pz_glwe_op_params& p, size_t batch) const {
        return pz_bdd_circuit_execute_tmp_bytes(m_, c, &p, batch);
    }
    void bdd_circuit_execute_batched(const pz_bdd_circuit* c, int64_t* out, size_t n_out, const double* const* bits, size_t nbits,
                                     const pz_glwe_op_params& p, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_bdd_circuit_execute_batched(m_, c, out, n_out, bits, nbits, &p, tmp, tmp_bytes, batch), "bdd_circuit_execute_batched");
    }
    void blind_rotation_execute_batched(int64_t* res, const int64_t* lwe_2n, const int64_t* lut, const double* brk, const pz_blind_rotation_params& p, size_t batch) {
        check(pz_blind_rotation_execute_batched(m_, res, lwe_2n, lut, brk, &p, batch), "blind_rotation_execute_batched");
    }
    void pin_key(const double* pmat, size_t rows, size_t cols_in, size_t cols_out, size_t size) {
        check(pz_module_pin_key(m_, pmat, rows, cols_in, cols_out, size), "module_pin_key");
    }
    void unpin_key(const double* pmat) { check(pz_module_unpin_key(m_, pmat), "module_unpin_key"); }
    void vec_znx_rotate(int64_t k, VecZnx& res, size_t res_col, const VecZnx& a, size_t a_col) {
        check(pz_vec_znx_rotate(m_, k, res.data, res.cols, res.size, res_col, a.data, a.cols, a.size, a_col), "vec_znx_rotate");
    }
    void vec_znx_rotate_assign(int64_t k, VecZnx& res, size_t res_col) {
        check(pz_vec_znx_rotate_assign(m_, k, res.data, res.cols, res.size, res_col), "vec_znx_rotate_assign");
    }
    void vec_znx_rsh_assign(size_t base2k, size_t k, VecZnx& res, size_t res_col) {
        check(pz_vec_znx_rsh_assign(m_, base2k, k, res.data, res.cols, res.size, res_col), "vec_znx_rsh_assign");
    }
    // gals / keys: nsteps host arrays (Galois element and device pointer of the prepared key of every step)
    void glwe_trace_batched(int64_t* res, size_t nsteps, const int64_t* gals, const double* const* keys, const pz_glwe_op_params& p, size_t batch) {
        check(pz_glwe_trace_batched(m_, res, nsteps, gals, keys, &p, batch), "glwe_trace_batched");
    }
    void ggsw_external_product(int64_t* res, const int64_t* a, size_t a_dnum, const double* ggsw, const pz_glwe_op_params& p) {
        check(pz_ggsw_external_product(m_, res, a, a_dnum, ggsw, &p), "ggsw_external_product");
    }
    void circuit_bootstrapping_execute_to_constant_batched(int64_t* ggsw, const int64_t* lwe_2n, const int64_t* lut, const double* brk,
                                                           size_t nsteps, const int64_t* gals, const double* const* atk,
                                                           const double* const* tsk, const pz_circuit_bootstrapping_params& p, void* tmp,
                                                           size_t tmp_bytes, size_t batch) {
        check(pz_circuit_bootstrapping_execute_to_constant_batched(m_, ggsw, lwe_2n, lut, brk, nsteps, gals, atk, tsk, &p, tmp, tmp_bytes, batch),
              "circuit_bootstrapping_execute_to_constant_batched");
    }
    size_t lwe_from_glwe_many_tmp_bytes(const pz_glwe_op_params& p, size_t nidx, size_t batch) const {
        return pz_lwe_from_glwe_many_tmp_bytes(m_, &p, nidx, batch);
    }
    void lwe_from_glwe_many_batched(int64_t* res, size_t res_n_lwe, const int64_t* a, size_t nidx, const size_t* idx, const double* ksk,
                                    const pz_glwe_op_params& p, int64_t* lwe_2n, size_t n2, bool negate, void* tmp, size_t tmp_bytes,
                                    size_t batch) {
        check(pz_lwe_from_glwe_many_batched(m_, res, res_n_lwe, a, nidx, idx, ksk, &p, lwe_2n, n2, negate ? 1 : 0, tmp, tmp_bytes, batch),
              "lwe_from_glwe_many_batched");
    }
    void ggsw_prepare_batched(double* pmat, const int64_t* ggsw, size_t count, size_t dnum, size_t rank, size_t size) {
        check(pz_ggsw_prepare_batched(m_, pmat, ggsw, count, dnum, rank, size), "ggsw_prepare_batched");
    }
    size_t fhe_uint_prepare_tmp_bytes(const pz_fhe_uint_prepare_params& p, size_t batch, size_t chunk_bits = 0) const {
        return pz_fhe_uint_prepare_tmp_bytes(m_, &p, batch, chunk_bits);
    }
    void fhe_uint_prepare_batched(double* res_pmat, int64_t* ggsw_out, int64_t* lwe_out, const int64_t* words, const double* ks_glwe,
                                  const double* ks_lwe, const int64_t* lut, const double* brk, size_t nsteps, const int64_t* gals,
                                  const double* const* atk, const double* const* tsk, const pz_fhe_uint_prepare_params& p, void* tmp,
                                  size_t tmp_bytes, size_t batch) {
        check(pz_fhe_uint_prepare_batched(m_, res_pmat, ggsw_out, lwe_out, words, ks_glwe, ks_lwe, lut, brk, nsteps, gals, atk, tsk, &p, tmp,
                                          tmp_bytes, batch),
              "fhe_uint_prepare_batched");
    }
    size_t fhe_uint_pack_tmp_bytes(const pz_glwe_op_params& p, size_t word_bits, size_t trace_size, size_t batch) const {
        return pz_fhe_uint_pack_tmp_bytes(m_, &p, word_bits, trace_size, batch);
    }
    void fhe_uint_pack_batched(int64_t* res, int64_t* bits, size_t word_bits, const int64_t* gals, const double* const* keys,
                               const pz_glwe_op_params& p, size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_fhe_uint_pack_batched(m_, res, bits, word_bits, gals, keys, &p, trace_size, tmp, tmp_bytes, batch), "fhe_uint_pack_batched");
    }
    size_t fhe_uint_execute_tmp_bytes(const pz_bdd_circuit* c, const pz_glwe_op_params& gate_p, const pz_glwe_op_params& pack_p, size_t word_bits,
                                      size_t trace_size, size_t batch) const {
        return pz_fhe_uint_execute_tmp_bytes(m_, c, &gate_p, &pack_p, word_bits, trace_size, batch);
    }
    void fhe_uint_execute_batched(const pz_bdd_circuit* c, int64_t* res, size_t word_bits, const double* const* bits, size_t nbits,
                                  const pz_glwe_op_params& gate_p, const int64_t* gals, const double* const* atk, const pz_glwe_op_params& pack_p,
                                  size_t trace_size, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_fhe_uint_execute_batched(m_, c, res, word_bits, bits, nbits, &gate_p, gals, atk, &pack_p, trace_size, tmp, tmp_bytes, batch),
              "fhe_uint_execute_batched");
    }
    size_t fhe_uint_word_op_tmp_bytes(const pz_glwe_op_params& p, size_t word_bits, size_t max_items, size_t batch) const {
        return pz_fhe_uint_word_op_tmp_bytes(m_, &p, word_bits, max_items, batch);
    }
    void fhe_uint_get_batched(int64_t* res, const int64_t* words, size_t word_bits, int unit, size_t nidx, const uint32_t* idx, const int64_t* gals,
                              const double* const* keys, const pz_glwe_op_params& p, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_fhe_uint_get_batched(m_, res, words, word_bits, unit, nidx, idx, gals, keys, &p, tmp, tmp_bytes, batch), "fhe_uint_get_batched");
    }
    void fhe_uint_zero_byte_batched(int64_t* res, const int64_t* a, size_t word_bits, size_t byte, const int64_t* gals, const double* const* keys,
                                    const pz_glwe_op_params& p, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_fhe_uint_zero_byte_batched(m_, res, a, word_bits, byte, gals, keys, &p, tmp, tmp_bytes, batch), "fhe_uint_zero_byte_batched");
    }
    void fhe_uint_splice_batched(int64_t* res, const int64_t* a, const int64_t* b, size_t word_bits, size_t width, size_t dst, size_t src,
                                 const int64_t* gals, const double* const* keys, const pz_glwe_op_params& p, void* tmp, size_t tmp_bytes,
                                 size_t batch) {
        check(pz_fhe_uint_splice_batched(m_, res, a, b, word_bits, width, dst, src, gals, keys, &p, tmp, tmp_bytes, batch), "fhe_uint_splice_batched");
    }
    void fhe_uint_sext_batched(int64_t* word, size_t word_bits, size_t byte, const int64_t* gals, const double* const* keys,
                               const pz_glwe_op_params& p, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_fhe_uint_sext_batched(m_, word, word_bits, byte, gals, keys, &p, tmp, tmp_bytes, batch), "fhe_uint_sext_batched");
    }
    void circuit_bootstrapping_execute_to_exponent_batched(int64_t* ggsw, const int64_t* lwe_2n, const int64_t* lut, const double* brk,
                                                           const int64_t* gals, const double* const* atk, const double* const* tsk,
                                                           const pz_circuit_bootstrapping_params& p, size_t log_gap_in, size_t log_gap_out,
                                                           size_t log_domain, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_circuit_bootstrapping_execute_to_exponent_batched(m_, ggsw, lwe_2n, lut, brk, gals, atk, tsk, &p, log_gap_in, log_gap_out,
                                                                   log_domain, tmp, tmp_bytes, batch),
              "circuit_bootstrapping_execute_to_exponent_batched");
    }
    size_t circuit_bootstrapping_to_exponent_tmp_bytes(const pz_circuit_bootstrapping_params& p, size_t log_domain, size_t batch) const {
        return pz_circuit_bootstrapping_to_exponent_tmp_bytes(m_, &p, log_domain, batch);
    }
    size_t circuit_bootstrapping_tmp_bytes(const pz_circuit_bootstrapping_params& p, size_t batch) const {
        return pz_circuit_bootstrapping_tmp_bytes(m_, &p, batch);
    }
    // i64 VecZnx limb-wise family (hal_impl.rs:34-131, :289)
    void vec_znx_add_into(int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol, const int64_t* b,
                          size_t bc, size_t bs, size_t bcol) {
        check(pz_vec_znx_add_into(m_, res, rc, rs, rcol, a, ac, as, acol, b, bc, bs, bcol), "vec_znx_add_into");
    }
    void vec_znx_sub(int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol, const int64_t* b,
                     size_t bc, size_t bs, size_t bcol) {
        check(pz_vec_znx_sub(m_, res, rc, rs, rcol, a, ac, as, acol, b, bc, bs, bcol), "vec_znx_sub");
    }
    void vec_znx_add_assign(int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol) {
        check(pz_vec_znx_add_assign(m_, res, rc, rs, rcol, a, ac, as, acol), "vec_znx_add_assign");
    }
    void vec_znx_sub_assign(int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol) {
        check(pz_vec_znx_sub_assign(m_, res, rc, rs, rcol, a, ac, as, acol), "vec_znx_sub_assign");
    }
    void vec_znx_sub_negate_assign(int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol) {
        check(pz_vec_znx_sub_negate_assign(m_, res, rc, rs, rcol, a, ac, as, acol), "vec_znx_sub_negate_assign");
    }
    void vec_znx_negate(int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol) {
        check(pz_vec_znx_negate(m_, res, rc, rs, rcol, a, ac, as, acol), "vec_znx_negate");
    }
    void vec_znx_negate_assign(int64_t* res, size_t rc, size_t rs, size_t rcol) { check(pz_vec_znx_negate_assign(m_, res, rc, rs, rcol), "vec_znx_negate_assign"); }
    void vec_znx_copy(int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol) {
        check(pz_vec_znx_copy(m_, res, rc, rs, rcol, a, ac, as, acol), "vec_znx_copy");
    }
    void vec_znx_zero(int64_t* res, size_t rc, size_t rs, size_t rcol) { check(pz_vec_znx_zero(m_, res, rc, rs, rcol), "vec_znx_zero"); }
    void vec_znx_normalize(int64_t* res, size_t rc, size_t rs, size_t res_base2k, int64_t res_offset, size_t rcol, const int64_t* a, size_t ac,
                           size_t as, size_t a_base2k, size_t acol) {
        check(pz_vec_znx_normalize(m_, res, rc, rs, res_base2k, res_offset, rcol, a, ac, as, a_base2k, acol), "vec_znx_normalize");
    }
    void vec_znx_normalize_assign(size_t base2k, int64_t* res, size_t rc, size_t rs, size_t rcol) {
        check(pz_vec_znx_normalize_assign(m_, base2k, res, rc, rs, rcol), "vec_znx_normalize_assign");
    }
    void vec_znx_lsh(size_t base2k, size_t k, int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol) {
        check(pz_vec_znx_lsh(m_, base2k, k, res, rc, rs, rcol, a, ac, as, acol), "vec_znx_lsh");
    }
    void vec_znx_rsh(size_t base2k, size_t k, int64_t* res, size_t rc, size_t rs, size_t rcol, const int64_t* a, size_t ac, size_t as, size_t acol) {
        check(pz_vec_znx_rsh(m_, base2k, k, res, rc, rs, rcol, a, ac, as, acol), "vec_znx_rsh");
    }
    void vec_znx_lsh_assign(size_t base2k, size_t k, int64_t* res, size_t rc, size_t rs, size_t rcol) {
        check(pz_vec_znx_lsh_assign(m_, base2k, k, res, rc, rs, rcol), "vec_znx_lsh_assign");
    }
    size_t glwe_pack_tmp_bytes(const pz_glwe_op_params& p, size_t batch) const { return pz_glwe_pack_tmp_bytes(m_, &p, batch); }
    void glwe_pack_batched(int64_t* res, size_t nslots, const uint64_t* indices, int64_t* const* cts, size_t log_gap_out, const int64_t* gals,
                           const double* const* keys, const pz_glwe_op_params& p, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_glwe_pack_batched(m_, res, nslots, indices, cts, log_gap_out, gals, keys, &p, tmp, tmp_bytes, batch), "glwe_pack_batched");
    }
    size_t blind_rotation_extended_tmp_bytes(const pz_blind_rotation_params& p, size_t ext, size_t batch) const {
        return pz_blind_rotation_extended_tmp_bytes(m_, &p, ext, batch);
    }
    void blind_rotation_execute_extended_batched(int64_t* res, const int64_t* lwe_2n, const int64_t* lut, const double* brk,
                                                 const pz_blind_rotation_params& p, size_t ext, void* tmp, size_t tmp_bytes, size_t batch) {
        check(pz_blind_rotation_execute_extended_batched(m_, res, lwe_2n, lut, brk, &p, ext, tmp, tmp_bytes, batch),
              "blind_rotation_execute_extended_batched");
    }
    void set_graphs(bool enable) { check(pz_module_set_graphs(m_, enable ? 1 : 0), "set_graphs"); }
    uint64_t graph_launches() const { return pz_module_graph_launches(m_); }
    void ggsw_from_gglwe_batched(int64_t* ggsw, const int64_t* a, size_t a_cols_in, size_t dnum, const double* const* tsk,
                                 const pz_glwe_op_params& p, size_t count) {
        check(pz_ggsw_from_gglwe_batched(m_, ggsw, a, a_cols_in, dnum, tsk, &p, count), "ggsw_from_gglwe_batched");
    }
    void ggsw_expand_row_batched(int64_t* ggsw, size_t dnum, const double* const* tsk, const pz_glwe_op_params& p, size_t count) {
        check(pz_ggsw_expand_row_batched(m_, ggsw, dnum, tsk, &p, count), "ggsw_expand_row_batched");
    }
    // glwe_automorphism_key_automorphism (automorphism/gglwe_atk.rs:42-155) on `count` GGLWEs of Galois element a_gal; returns the Galois
    // element of the result, a_gal * key_gal mod 2N (res.set_p, :110)
    int64_t glwe_automorphism_key_automorphism_batched(int64_t* res, size_t res_dnum, const int64_t* a, size_t a_dnum, int64_t a_gal,
                                                       const double* key, int64_t key_gal, const pz_glwe_op_params& p, size_t count) {
        check(pz_glwe_automorphism_key_automorphism_batched(m_, res, res_dnum, a, a_dnum, a_gal, key, &p, count),
              "glwe_automorphism_key_automorphism_batched");
        const uint64_t mask = 2 * n() - 1;
        return (int64_t)((((uint64_t)a_gal & mask) * ((uint64_t)key_gal & mask)) & mask);
    }
    // ggsw_keyswitch (keyswitching/ggsw.rs:37-85) / ggsw_automorphism (automorphism/ggsw_ct.rs:32-82) on `count` GGSWs: kp the key switch of
    // the entries (row, 0), tsk / tp the arguments of ggsw_expand_row_batched
    void ggsw_keyswitch_batched(int64_t* res, const int64_t* a, size_t dnum, const double* key, const double* const* tsk,
                                const pz_glwe_op_params& kp, const pz_glwe_op_params& tp, size_t count) {
        check(pz_ggsw_keyswitch_batched(m_, res, a, dnum, key, tsk, &kp, &tp, count), "ggsw_keyswitch_batched");
    }
    void ggsw_automorphism_batched(int64_t* res, size_t res_dnum, const int64_t* a, size_t a_dnum, const double* key, int64_t gal,
                                   const double* const* tsk, const pz_glwe_op_params& kp, const pz_glwe_op_params& tp, size_t count) {
        check(pz_ggsw_automorphism_batched(m_, res, res_dnum, a, a_dnum, key, gal, tsk, &kp, &tp, count), "ggsw_automorphism_batched");
    }
    // GLWE x plaintext (mode PZ_MUL_PLAIN / PZ_MUL_PLAIN_ASSIGN) and GLWE x constant (PZ_MUL_CONST / PZ_MUL_CONST_ASSIGN; re / im on the host)
    size_t glwe_mul_plain_workspace_bytes(const pz_glwe_tensor_params& p, int mode, bool pt_shared, size_t batch) const {
        return pz_glwe_mul_plain_workspace_bytes(m_, &p, mode, pt_shared ? 1 : 0, batch);
    }
    void glwe_mul_plain_batched(int64_t* res, const int64_t* a, const int64_t* pt, bool pt_shared, const pz_glwe_tensor_params& p, int mode,
                                size_t batch) {
        check(pz_glwe_mul_plain_batched(m_, res, a, pt, pt_shared ? 1 : 0, &p, mode, batch), "glwe_mul_plain_batched");
    }
    void glwe_mul_const_batched(int64_t* res, const int64_t* a, const int64_t* re, const int64_t* im, size_t b_size,
                                const pz_glwe_mul_const_params& p, int mode, size_t batch) {
        check(pz_glwe_mul_const_batched(m_, res, a, re, im, b_size, &p, mode, batch), "glwe_mul_const_batched");
    }
    // res = [res] +- sum_t constant_t x operands[t] in one pass; every array has nterms entries (poulpy_hip.h)
    void glwe_lincomb_const_batched(int64_t* res, size_t rank, size_t res_size, size_t base2k, const int64_t* const* operands, const int* shared,
                                    const size_t* a_size, const size_t* cnv_offset, const int64_t* const* re, const int64_t* const* im,
                                    const size_t* b_size, const int* join, const size_t* k, const int* sign, size_t nterms, int init, bool normalize,
                                    size_t batch) {
        check(pz_glwe_lincomb_const_batched(m_, res, rank, res_size, base2k, operands, shared, a_size, cnv_offset, re, im, b_size, join, k, sign,
                                            nterms, init, normalize ? 1 : 0, batch),
              "glwe_lincomb_const_batched");
    }
    // res = normalize(sum_t +- join_t(operands[t])) in one pass, up to 64 terms; every array has nterms entries (poulpy_hip.h)
    void glwe_sum_batched(int64_t* res, size_t res_cols, size_t res_size, size_t base2k, const int64_t* const* operands, const int* shared,
                          const size_t* a_size, const int* join, const size_t* k, const int* sign, size_t nterms, size_t batch) {
        check(pz_glwe_sum_batched(m_, res, res_cols, res_size, base2k, operands, shared, a_size, join, k, sign, nterms, batch), "glwe_sum_batched");
    }
    // tensoring + relinearization in one call on strided operands: res = a b (accumulate = false; res may be a and / or b at equal strides)
    // or res = join(res, a b) with the product of a wave kept in the module's workspace (poulpy_hip.h)
    void glwe_tensor_mul_relinearize_acc_batched(int64_t* res, const int64_t* a, const int64_t* b, const double* tsk_pmat,
                                                 const pz_glwe_tensor_params& tp, const pz_glwe_op_params& rp, size_t a_stride, size_t b_stride,
                                                 bool accumulate, int join, size_t k, int sign, bool normalize, int mode, size_t batch) {
        check(pz_glwe_tensor_mul_relinearize_acc_batched(m_, res, a, b, tsk_pmat, &tp, &rp, a_stride, b_stride, accumulate ? 1 : 0, join, k, sign,
                                                         normalize ? 1 : 0, mode, batch),
              "glwe_tensor_mul_relinearize_acc_batched");
    }
    size_t glwe_tensor_mul_relinearize_acc_workspace_bytes(const pz_glwe_tensor_params& tp, const pz_glwe_op_params& rp, bool accumulate, int mode,
                                                           size_t batch) const {
        return pz_glwe_tensor_mul_relinearize_acc_workspace_bytes(m_, &tp, &rp, accumulate ? 1 : 0, mode, batch);
    }
    // res = relinearize(sum_i a[i] (x) b[i]): npairs products in one accumulated tensor, one relinearization; a / b: host arrays of npairs
    // device pointers, a_stride / b_stride: limbs of the containers per pair or nullptr (poulpy_hip.h)
    void glwe_tensor_dot_relinearize_batched(int64_t* res, const int64_t* const* a, const int64_t* const* b, size_t npairs, const size_t* a_stride,
                                             const size_t* b_stride, const double* tsk_pmat, const pz_glwe_tensor_params& tp,
                                             const pz_glwe_op_params& rp, size_t batch) {
        check(pz_glwe_tensor_dot_relinearize_batched(m_, res, a, b, npairs, a_stride, b_stride, tsk_pmat, &tp, &rp, batch),
              "glwe_tensor_dot_relinearize_batched");
    }
    size_t glwe_tensor_dot_relinearize_workspace_bytes(const pz_glwe_tensor_params& tp, const pz_glwe_op_params& rp, size_t npairs, size_t batch) const {
        return pz_glwe_tensor_dot_relinearize_workspace_bytes(m_, &tp, &rp, npairs, batch);
    }

  private:
    pz_module* m_ = nullptr;
};

// A BDD circuit in the evaluator's node format (bdd_arithmetic/eval.rs:22-63, 318-332), validated and compiled on the host: outputs[o] = the node list
// of output bit o, state_size[o] its state size.  Throws pz::Error with a message naming the output bit and the node when the circuit is malformed.
class BddCircuit {
  public:
    BddCircuit(const std::vector<std::vector<pz_bdd_node>>& outputs, const std::vector<size_t>& state_size, size_t input_size) {
        if (outputs.size() != state_size.size()) throw Error(PZ_ERR_INVALID, "BddCircuit: one state size per output");
        std::vector<const pz_bdd_node*> ptrs;
        std::vector<size_t> counts;
        for (const auto& o : outputs) { ptrs.push_back(o.data()); counts.push_back(o.size()); }
        c_ = pz_bdd_circuit_new(ptrs.data(), counts.data(), state_size.data(), outputs.size(), input_size);
        if (!c_) throw Error(PZ_ERR_INVALID, std::string("BddCircuit: ") + pz_last_error());
    }
    ~BddCircuit() { pz_bdd_circuit_free(c_); }
    BddCircuit(const BddCircuit&) = delete;
    BddCircuit& operator=(const BddCircuit&) = delete;
    const pz_bdd_circuit* raw() const { return c_; }
    size_t input_size() const { return pz_bdd_circuit_input_size(c_); }
    size_t output_size() const { return pz_bdd_circuit_output_size(c_); }
    size_t levels() const { return pz_bdd_circuit_levels(c_); }
    size_t gates() const { return pz_bdd_circuit_gates(c_); }

  private:
    pz_bdd_circuit* c_ = nullptr;
};

}  // namespace pz
